"""rth_fc_bwd's host side (r07): the shapes it builds, a workspace size that is a fixed function
of the shape, and the opt-in switch left off.  No GPU, no compute calls."""
import pytest


@pytest.mark.parametrize("shape", [(64, 128, 64), (512, 512, 3136), (64, 512, 3136)])
def test_fc_bwd_supported(shape):
    from reth_amd import _lib

    assert _lib.lib().rth_fc_bwd_supported(*shape) == 1


@pytest.mark.parametrize("shape", [(63, 128, 64), (64, 96, 64), (64, 128, 48)])
def test_fc_bwd_unsupported(shape):
    from reth_amd import _lib

    assert _lib.lib().rth_fc_bwd_supported(*shape) == 0
    assert _lib.lib().rth_fc_bwd_workspace(*shape) == 0


@pytest.mark.parametrize("shape", [(64, 128, 64), (128, 256, 64), (192, 128, 128), (64, 512, 3136), (512, 512, 3136)])
def test_fc_bwd_workspace_fixed(shape):
    from reth_amd import _lib

    size = _lib.lib().rth_fc_bwd_workspace(*shape)
    assert size >= 0 and size % 16 == 0
    assert _lib.lib().rth_fc_bwd_workspace(*shape) == size


def test_fc_bwd_workspace_plan():
    """the plan the GPU tests rely on: the loop's shape is not split (one launch, no workspace),
    the 64-row batch splits the data gradient's 49 tiles in 4 (B x K partials) and the weight
    gradient's two chunks not at all"""
    from reth_amd import _lib

    assert _lib.lib().rth_fc_bwd_workspace(512, 512, 3136) == 0
    assert _lib.lib().rth_fc_bwd_workspace(64, 512, 3136) == 4 * 64 * 3136 * 4


def test_fc1_bwd_switch_defaults_off():
    from reth_amd import model

    assert model.FC1_BWD is None
