"""The argument checks of rth_clip_adam / rth_adam_prenormed and of ClipAdam's constructor.  Every
check returns before the first HIP call, so they run without a device: the pointers handed over
are small host dummies that are never followed.  (Argument sets that pass the checks would launch
and are not called here; test_optim_gpu.py and test_optim_edges_gpu.py run them.)"""
import ctypes

import pytest
import torch

from reth_amd import _lib
from reth_amd._lib import RethHipError, call
from reth_amd.optim import ClipAdam, ParamTensor

CHUNK, MAX_PARTS = 2048, 32768  # optim.hpp: kOptChunk, kMaxPartials
_dummy = (ctypes.c_double * 8)()
PTR = ctypes.addressof(_dummy)


def _tensors(ns, null_field=None):
    ts = [ParamTensor(PTR, PTR, PTR, PTR, n) for n in ns]
    if null_field is not None:
        setattr(ts[-1], null_field, None)
    return ctypes.cast((ParamTensor * max(len(ts), 1))(*ts), _lib.c_vp), len(ts)


def clip_adam(ns, null_field=None, tensors=True, step=PTR, ws=PTR):
    arr, n = _tensors(ns, null_field)
    call("rth_clip_adam", arr if tensors else None, n, 1e-3, 0.9, 0.999, 1e-8, 1.0, step, ws, None, None)


def prenormed(ns, nparts, null_field=None, tensors=True, step=PTR, ws=PTR):
    arr, n = _tensors(ns, null_field)
    call("rth_adam_prenormed", arr if tensors else None, n, 1e-3, 0.9, 0.999, 1e-8, 1.0, nparts, step, ws, None, None)


ENTRY = {"rth_clip_adam": clip_adam, "rth_adam_prenormed": lambda ns, **kw: prenormed(ns, 1, **kw)}


@pytest.mark.parametrize("name", list(ENTRY))
def test_tensor_count(name):
    for ns in ([], [4] * 33):
        with pytest.raises(RethHipError, match=rf"{name}: {len(ns)} tensors not in \[1, 32\]"):
            ENTRY[name](ns)


@pytest.mark.parametrize("name", list(ENTRY))
def test_incomplete_tensor(name):
    with pytest.raises(RethHipError, match=rf"{name}: tensor 1 incomplete"):
        ENTRY[name]([4, 0])
    with pytest.raises(RethHipError, match=rf"{name}: tensor 0 incomplete"):
        ENTRY[name]([-1])
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        with pytest.raises(RethHipError, match=rf"{name}: tensor 2 incomplete"):
            ENTRY[name]([4, 4, 4], null_field=field)


@pytest.mark.parametrize("name", list(ENTRY))
def test_null_arguments(name):
    for kw in (dict(tensors=False), dict(step=None), dict(ws=None)):
        with pytest.raises(RethHipError, match=rf"{name}: NULL argument"):
            ENTRY[name]([4], **kw)


def test_clip_adam_partial_count():
    """one partial per 2,048 elements of every tensor, at most 32,768 ([2048 x 32767, 1] has
    exactly 32,768 and would launch)"""
    for ns in ([CHUNK * MAX_PARTS + 1], [CHUNK * (MAX_PARTS - 1), 1, 1]):
        with pytest.raises(RethHipError, match=r"rth_clip_adam: 32769 norm partials \(at most 32768\)"):
            clip_adam(ns)


@pytest.mark.parametrize("nparts", [0, -1, MAX_PARTS + 1])
def test_prenormed_partial_count(nparts):
    with pytest.raises(RethHipError, match=rf"rth_adam_prenormed: {nparts} norm partials \(at most 32768\)"):
        prenormed([5, 2049], nparts)


@pytest.mark.parametrize("name", list(ENTRY))
@pytest.mark.parametrize("n", [2 ** 29, 2 ** 31, 2 ** 40])
def test_tensor_size_bound(name, n):
    """n * 4 bytes must fit the buffer resource's 32-bit record count: n < 2^29 (2^29 - 1 is valid
    and would launch)"""
    with pytest.raises(RethHipError, match=rf"{name}: tensor 1 has {n} elements \(fewer than 2\^29 = 536870912\)"):
        ENTRY[name]([4, n])


def test_workspace_size():
    assert _lib.lib().rth_clip_adam_workspace() == MAX_PARTS * 8 + 64


def _p(*shape, dtype=torch.float32):
    return torch.nn.Parameter(torch.ones(*shape, dtype=dtype))


def test_constructor_refuses():
    opt = ClipAdam([_p(4, 4), _p(3)])  # a valid set constructs without a device
    assert opt._ws.numel() == MAX_PARTS * 8 + 64 and int(opt._step) == 0
    ClipAdam([_p(2) for _ in range(32)])
    with pytest.raises(ValueError, match=r"33 parameter tensors \(1\.\.32\)"):
        ClipAdam([_p(2) for _ in range(33)])
    with pytest.raises(ValueError, match="one parameter group"):
        ClipAdam([{"params": [_p(2)]}, {"params": [_p(3)]}])
    with pytest.raises(ValueError, match="dense float32"):
        ClipAdam([_p(2), _p(2, dtype=torch.float64)])
    with pytest.raises(ValueError, match="dense float32"):
        ClipAdam([torch.nn.Parameter(torch.ones(4, 6).t())])
    with pytest.raises(ValueError, match="dense float32"):
        ClipAdam([torch.nn.Parameter(torch.ones(4, 8)[:, ::2])])
