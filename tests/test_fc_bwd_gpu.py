"""rth_fc_bwd (r07): FC1's backward -- gx [B, K] = gy w and gw [N, K] = gy^T x, the backward of
dqn_model.py:38-47 under dqn_solver.py:116-117 -- on the exact-split bf16 MFMA, both gradients
in one launch, against a float64 CPU product: within fp32 summation error (the project's FC
bound: 4x the error of the same product in fp32 on the CPU, floor 2e-6), every output element
written with nothing expected of the workspace, run-to-run bit-identical, each gradient's bits
independent of whether the other is asked for, strided gy / x, and an unsupported shape refused
without a write.  Shapes: one tile of each role, an odd count of 64-wide column tiles, the 128-
and 64-row tile forms, the split-K + reduce path, the BeamRider / 8-rank batch and the loop's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

NAN = float("nan")


def _inputs(dev, B, N, K, ldg=None, ldx=None):
    """gy ReLU-masked (a random half exactly 0), w ~ 1 / sqrt(N), x ~ 3 / sqrt(B): O(1) outputs"""
    ldg, ldx = ldg or N, ldx or K
    g = torch.Generator(device=dev).manual_seed(B * 7 + N * 3 + K)
    gyb = torch.rand((B, ldg), device=dev, generator=g) * 2 - 1
    gyb = gyb * (torch.rand((B, ldg), device=dev, generator=g) < 0.5)
    xb = torch.rand((B, ldx), device=dev, generator=g) * 3 / np.sqrt(B)
    w = (torch.rand((N, K), device=dev, generator=g) * 2 - 1) / np.sqrt(N)
    return gyb[:, :N], xb[:, :K], w


def _call(dev, gy, x, w, want_gx=True, want_gw=True):
    from reth_amd import _lib

    (B, N), K = gy.shape, w.shape[1]
    ws = torch.full((max(_lib.lib().rth_fc_bwd_workspace(B, N, K), 16) // 4,), NAN, device=dev)
    gx = torch.full((B, K), NAN, device=dev) if want_gx else None
    gw = torch.full((N, K), NAN, device=dev) if want_gw else None
    _lib.call("rth_fc_bwd", gy.data_ptr(), gy.stride(0), x.data_ptr() if want_gw else None, x.stride(0),
              w.data_ptr() if want_gx else None, B, N, K, _lib.ptr(gx), _lib.ptr(gw), ws.data_ptr(), _lib.stream_ptr())
    return gx, gw


def _bound(ours, a, b):
    """|ours - a b| (float64 on the CPU) and the same product's fp32 CPU error"""
    a, b = a.cpu(), b.cpu()
    want = a.double() @ b.double()
    err = (ours.double().cpu() - want).abs().max().item()
    err32 = ((a @ b).double() - want).abs().max().item()
    return err, err32


def _check(dev, B, N, K, ldg=None, ldx=None):
    from reth_amd import _lib

    assert _lib.lib().rth_fc_bwd_supported(B, N, K) == 1
    gy, x, w = _inputs(dev, B, N, K, ldg, ldx)
    gx, gw = _call(dev, gy, x, w)
    assert not torch.isnan(gx).any() and not torch.isnan(gw).any()
    gx2, gw2 = _call(dev, gy, x, w)
    assert torch.equal(gx, gx2) and torch.equal(gw, gw2)
    gx1, none = _call(dev, gy, x, w, want_gw=False)
    assert none is None and torch.equal(gx1, gx)
    none, gw1 = _call(dev, gy, x, w, want_gx=False)
    assert none is None and torch.equal(gw1, gw)
    for name, ours, a, b in (("gx", gx, gy, w), ("gw", gw, gy.t(), x)):
        err, err32 = _bound(ours, a.contiguous(), b.contiguous())
        print(f"rth_fc_bwd {(B, N, K)} {name}: |ours - fp64| {err:.3e}, |cpu fp32 - fp64| {err32:.3e}")
        assert err <= max(4 * err32, 2e-6), (name, err, err32)


@pytest.mark.parametrize("shape", [(64, 128, 64), (64, 128, 192), (128, 256, 64), (192, 128, 128), (64, 512, 3136),
                                   (512, 512, 3136)])
def test_fc_bwd_vs_fp64(dev, shape):
    _check(dev, *shape)


def test_fc_bwd_strided(dev):
    B, N, K = 128, 128, 128
    _check(dev, B, N, K, ldg=N + 128, ldx=K + 64)


def test_fc_bwd_unsupported(dev):
    from reth_amd import _lib

    B, N, K = 64, 96, 64
    assert _lib.lib().rth_fc_bwd_supported(B, N, K) == 0
    gy, x, w = _inputs(dev, B, N, K)
    gx, gw = torch.full((B, K), NAN, device=dev), torch.full((N, K), NAN, device=dev)
    ws = torch.full((1024,), NAN, device=dev)
    rc = _lib.lib().rth_fc_bwd(gy.data_ptr(), N, x.data_ptr(), K, w.data_ptr(), B, N, K, gx.data_ptr(), gw.data_ptr(),
                               ws.data_ptr(), _lib.stream_ptr())
    assert rc != 0 and _lib.lib().rth_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(gx).all() and torch.isnan(gw).all()
    # neither gradient asked for: an error too
    rc = _lib.lib().rth_fc_bwd(gy.data_ptr(), N, x.data_ptr(), K, w.data_ptr(), 64, 128, 64, None, None,
                               ws.data_ptr(), _lib.stream_ptr())
    assert rc != 0 and _lib.lib().rth_last_error()
