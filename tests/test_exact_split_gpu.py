"""The exact-split kernels on order-free inputs: bit equality with fp64 rounded once.

common.hpp, fc.hip and conv.hip claim that the three-term bf16 split makes every partial product
exact in the fp32 accumulator, so the bf16-MFMA kernels add the products of an fp32 GEMM in another
fixed order.  The accuracy tests (test_fc_gpu.py, test_fc_bwd_gpu.py, test_conv_gpu.py) bound a
summation error that would hide a lost third term; here the inputs (_exact_inputs.py, proven on the
CPU in test_exact_inputs_cpu.py) have a result that no summation order can change, so a correct
kernel returns the expectation bit for bit -- whatever its tile form, k split or reduce launch --
and no tolerance enters.  Outputs are NaN-filled first; zeros must come back +0; where a dot
product meets the inf or the NaN of class E the output must be non-finite (the split turns inf
into inf - inf: the x9 kernels return NaN) and every other output keeps its finite expectation.
The fp32-MFMA kernels (rth_fc_f32, conv2 at the learner's sizes, rth_conv_wgrad_f32) run the same
inputs as the control."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import _exact_inputs as X

pytestmark = pytest.mark.gpu

NAN = float("nan")
U32 = np.uint32


def assert_bits(got, want, what, pre=None, relu=False):
    """got (a tensor) == want (numpy fp32) bit for bit where the dot product `pre` (default: want)
    is finite; non-finite where it is not (under a ReLU, 0 for a dot product of -inf as well)"""
    got = np.ascontiguousarray(got.detach().cpu().numpy(), dtype=np.float32)
    want = np.ascontiguousarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    meets = ~np.isfinite(want if pre is None else pre)
    gb, wb = got.view(U32), want.view(U32)
    bad = (gb != wb) & ~meets
    if bad.any():
        i = tuple(int(v[0]) for v in np.nonzero(bad))
        ulps = np.abs(gb[bad].astype(np.int64) - wb[bad].astype(np.int64))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs differ (largest bit-pattern distance "
                             f"{int(ulps.max())}); first at {i}: got {got[i]!r} ({gb[i]:#010x}), want {want[i]!r} ({wb[i]:#010x})")
    if meets.any():
        ok = ~np.isfinite(got[meets])
        if relu:
            ok |= (got[meets] == 0) & (np.asarray(pre)[meets] == -np.inf)
        assert ok.all(), f"{what}: a finite output where the dot product meets an inf / NaN"


def dv(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------ FC
@functools.lru_cache(maxsize=8)
def fc_cases(M, N, K, classes="ABCE"):
    return X.product_cases(M + N + K, M, N, K, classes=classes)


def run_fc(dev, kind, x, w, b, relu):
    from reth_amd import _lib

    (M, K), N = x.shape, w.shape[0]
    fn = "rth_fc_" + kind
    assert getattr(_lib.lib(), fn + "_supported")(M, N, K) == 1
    ws = torch.full((max(getattr(_lib.lib(), fn + "_workspace")(M, N, K), 16) // 4,), NAN, device=dev)
    y = torch.full((M, N), NAN, device=dev)
    _lib.call(fn, x.data_ptr(), K, M, w.data_ptr(), N, K, None if b is None else b.data_ptr(), int(relu), y.data_ptr(),
              ws.data_ptr(), _lib.stream_ptr())
    return y


def check_fc(dev, kind, shape, classes="ABCE"):
    failures = []
    for c in fc_cases(*shape, classes):
        x, w = dv(c.ops["a"], dev), dv(c.ops["b"], dev)
        b = None if c.ops["bias"] is None else dv(c.ops["bias"], dev)
        y = run_fc(dev, kind, x, w, b, c.meta["relu"])
        try:
            assert_bits(y, c.want, f"rth_fc_{kind} {shape} {c.name}", pre=c.pre, relu=c.meta["relu"])
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("shape", X.FC_X9_64)
def test_fc_x9_64_row_tile(dev, shape):
    """k_fc_x9 (M % 128 != 0): one chunk and one split; one chunk per split, fewer chunks than the
    register ring; 98 chunks over 32 uneven splits and the reduce launch"""
    check_fc(dev, "x9", shape)


@pytest.mark.parametrize("shape", X.FC_X9_128)
def test_fc_x9_128_row_tile(dev, shape):
    """k_fc_x9t; (512, 512, 3136) is the loop's shape, 16 splits"""
    check_fc(dev, "x9", shape)


@pytest.mark.parametrize("shape", X.FC_F32)
def test_fc_f32_control(dev, shape):
    """the fp32 MFMA on the same inputs: one row, a ragged row count, the loop's shape"""
    check_fc(dev, "f32", shape)


def test_fc_x9_every_pattern_value(dev):
    """class A at (1024, 128, 128): N = K, so the selection reaches every k and each of the 131,072
    pattern values of x is one output; then the patterns in w with x as the selection"""
    check_fc(dev, "x9", X.FC_ALL_PATTERNS, "A")


def test_fc_x9_exponent_domain(dev):
    """class A over every fp32 exponent (and a few subnormals) at (64, 128, 128): exponents in
    [-60, 60] are exact and nothing outside disturbs another output (every output is its own
    value or wrong by itself: a zero product of a far-out value stays zero).  Prints the first
    exponent on each side where the result stops being exact (DESIGN.md records them).  The values
    at exponent 127 stay below (2 - 2^-8) 2^127, where the first term rounds to infinity and, as in
    class E, the whole row would be NaN."""
    x, w, want, exps = X.exponent_sweep()
    top = exps == 127
    assert (np.abs(want[top]) < (2 - 2.0 ** -8) * 2.0 ** 127).all()
    y = run_fc(dev, "x9", dv(x, dev), dv(w, dev), None, False).cpu().numpy()
    exact = y.view(U32) == want.view(U32)
    per_e = {int(e): bool(exact[exps == e].all()) for e in np.unique(exps)}
    lo = next((e for e in range(-61, -128, -1) if not per_e[e]), None)
    hi = next((e for e in range(61, 128) if not per_e[e]), None)
    wrong = sorted(e for e, ok in per_e.items() if not ok)
    print(f"\nrth_fc_x9 exponent sweep: first inexact exponent below -60: {lo}, above 60: {hi} "
          f"(-127 = fp32 subnormals); all inexact exponents: {wrong}")
    for e in wrong[:8]:
        i = tuple(int(v[0]) for v in np.nonzero(~exact & (exps == e)))
        print(f"  e = {e}: got {y[i]!r} ({y.view(U32)[i]:#010x}), want {want[i]!r} ({want.view(U32)[i]:#010x})")
    inside = (exps >= -60) & (exps <= 60)
    assert exact[inside].all(), [e for e in wrong if -60 <= e <= 60]
    assert np.isfinite(y).all()  # no output was disturbed into a NaN / inf by a neighbour's terms


# ------------------------------------------------------------------------------------ FC backward
def run_fc_bwd(dev, gy, x, w, want_gx=True, want_gw=True):
    from reth_amd import _lib

    B, N = gy.shape
    K = (w if w is not None else x).shape[1]
    assert _lib.lib().rth_fc_bwd_supported(B, N, K) == 1
    ws = torch.full((max(_lib.lib().rth_fc_bwd_workspace(B, N, K), 16) // 4,), NAN, device=dev)
    gx = torch.full((B, K), NAN, device=dev) if want_gx else None
    gw = torch.full((N, K), NAN, device=dev) if want_gw else None
    _lib.call("rth_fc_bwd", gy.data_ptr(), gy.stride(0), x.data_ptr() if want_gw else None, K,
              w.data_ptr() if want_gx else None, B, N, K, _lib.ptr(gx), _lib.ptr(gw), ws.data_ptr(), _lib.stream_ptr())
    return gx, gw


@pytest.mark.parametrize("B,N,K", X.FC_BWD)
def test_fc_bwd(dev, B, N, K):
    """gx [B, K] = gy w (32-deep chunks over n) and gw [N, K] = gy^T x (over the batch row): one tile
    of each role, the 128-row form, split-K + reduce, an odd count of column tiles"""
    rng = np.random.default_rng(B + N + K)
    failures = []

    def check(got, c, what):
        try:
            assert_bits(got, c.want, f"rth_fc_bwd {(B, N, K)} {what} {c.name}", pre=c.pre)
        except AssertionError as e:
            failures.append(str(e))

    # class A, both gradients from one gy: patterns in gy against a selection w and one-hot rows of x
    cd = X.product_select(rng, B, K, N, "a", name="A/patterns-in-gy")
    gy_np = cd.ops["a"]
    cw = X.product_select(rng, N, K, B, "a", given=np.ascontiguousarray(gy_np.T), name="A/patterns-in-gy")
    gy, w, x = dv(gy_np, dev), dv(cd.ops["b"].T, dev), dv(cw.ops["b"].T, dev)
    gx, gw = run_fc_bwd(dev, gy, x, w)
    check(gx, cd, "gx (both)")
    check(gw, cw, "gw (both)")
    gx1, _ = run_fc_bwd(dev, gy, x, w, want_gw=False)
    _, gw1 = run_fc_bwd(dev, gy, x, w, want_gx=False)
    check(gx1, cd, "gx (alone)")
    check(gw1, cw, "gw (alone)")
    # every class of each product alone (the reverse roles of class A among them)
    for c in X.product_cases(B + N + K + 1, B, K, N, bias=False, classes="ABC"):  # gx = gy w: a = gy, b = w^T
        gx, _ = run_fc_bwd(dev, dv(c.ops["a"], dev), None, dv(c.ops["b"].T, dev), want_gw=False)
        check(gx, c, "gx")
    for c in X.product_cases(B + N + K + 2, N, K, B, bias=False, classes="ABC"):  # gw = gy^T x: a = gy^T, b = x^T
        _, gw = run_fc_bwd(dev, dv(c.ops["a"].T, dev), dv(c.ops["b"].T, dev), None, want_gx=False)
        check(gw, c, "gw")
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------- conv
def conv_shape(inp, geom):
    from reth_amd import _lib

    cin, h, w, cout, k, s = geom
    return _lib.ConvShape(inp, cin, h, w, cout, k, k, s)


def conv_impl(shape, n):
    from reth_amd import _lib

    ns = ctypes.c_int32(-1)
    return _lib.lib().rth_conv_impl(ctypes.byref(shape), n, ctypes.byref(ns))


def cl(a, dev):
    """an NCHW array as a channels-last device tensor (the kernels' NHWC / OHWI)"""
    return dv(a, dev).contiguous(memory_format=torch.channels_last)


def run_conv(dev, geom, x, rows, n, w, b, u8=False, nchw=False):
    """rth_conv_bias_relu; returns [n, cout, ho, wo]"""
    from reth_amd import _lib

    cin, h, wd, cout, k, s = geom
    inp = _lib.CONV_U8_CHW if u8 else _lib.CONV_F32_NHWC
    shape = conv_shape(inp, geom)
    ho, wo = (h - k) // s + 1, (wd - k) // s + 1
    pk = torch.full((_lib.lib().rth_conv_packed_bytes(ctypes.byref(shape)) // 4,), NAN, device=dev)
    wt = cl(w, dev)
    _lib.call("rth_conv_pack", ctypes.byref(shape), wt.data_ptr(), pk.data_ptr(), _lib.stream_ptr())
    run = conv_shape(inp | _lib.CONV_OUT_NCHW, geom) if nchw else shape
    assert _lib.lib().rth_conv_supported(ctypes.byref(run)) == 1
    y = torch.full((n, cout, ho, wo) if nchw else (n, ho, wo, cout), NAN, device=dev)
    bd = dv(b, dev)
    _lib.call("rth_conv_bias_relu", ctypes.byref(run), x.data_ptr(), None if rows is None else rows.data_ptr(), n,
              pk.data_ptr(), bd.data_ptr(), y.data_ptr(), _lib.stream_ptr())
    return y if nchw else y.permute(0, 3, 1, 2)


def check_conv_fwd(dev, gi, n, nchw=False, via_rows=False):
    geom = X.GEOMS[gi]
    ns, kinds, ekinds = X.CONV_FWD[gi]
    failures = []
    for kind, nf in [(k, False) for k in kinds] + [(k, True) for k in ekinds]:
        for neg in (False, True):  # w and -w: the ReLU hides the negative half of either run
            c = X.conv_fwd(100 * gi + n, geom, n, kind, negate=neg, nonfinite=nf)
            rows = None
            if gi == 0:
                stacks = c.ops["x"]
                if via_rows:  # the samples scattered in a larger store, addressed through a row index
                    rng = np.random.default_rng(n)
                    store = rng.integers(0, 256, (n + 6, 4, 84, 84)).astype(np.uint8)
                    r = rng.permutation(n + 6)[:n]
                    store[r] = stacks
                    stacks, rows = store, dv(r.astype(np.int64), dev)
                x = dv(stacks, dev)
            else:
                x = cl(c.ops["x"], dev)
            y = run_conv(dev, geom, x, rows, n, c.ops["w"], c.ops["bias"], u8=gi == 0, nchw=nchw)
            try:
                assert_bits(y, c.want, f"conv{gi + 1} n={n} {kind}{' E' if nf else ''}{' -w' if neg else ''}"
                            f"{' NCHW' if nchw else ''}{' rows' if via_rows else ''}", pre=c.pre, relu=True)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("nchw", [False, True])
@pytest.mark.parametrize("n", X.CONV_FWD[2][0])
def test_conv3_x9_forward(dev, n, nchw):
    from reth_amd import _lib

    assert conv_impl(conv_shape(_lib.CONV_F32_NHWC | (_lib.CONV_OUT_NCHW if nchw else 0), X.GEOMS[2]), n) == _lib.CONV_IMPL_X9
    check_conv_fwd(dev, 2, n, nchw=nchw)


@pytest.mark.parametrize("n", X.CONV_FWD[1][0])
def test_conv2_forward_control(dev, n):
    """conv2: the fp32-MFMA kernel at the learner's sizes (rth_conv_impl says which one runs here)"""
    from reth_amd import _lib

    print(f"\nconv2 n={n}: rth_conv_impl = {conv_impl(conv_shape(_lib.CONV_F32_NHWC, X.GEOMS[1]), n)}")
    check_conv_fwd(dev, 1, n)


@pytest.mark.parametrize("n,via_rows", [(1, False), (5, False), (5, True)])
def test_conv1_u8_forward(dev, n, via_rows):
    """conv1 on uint8 stacks (bf16x3: the weights split, the bytes exact), classes D and E"""
    from reth_amd import _lib

    assert conv_impl(conv_shape(_lib.CONV_U8_CHW, X.GEOMS[0]), n) == _lib.CONV_IMPL_BF16X3
    check_conv_fwd(dev, 0, n, via_rows=via_rows)


@pytest.mark.parametrize("gi", [1, 2])
@pytest.mark.parametrize("n", [1, 3, 37])
def test_conv_dgrad(dev, gi, n):
    """rth_conv_dgrad: lattice classes A / B (uncovered input pixels come back +0) and class C"""
    from reth_amd import _lib

    geom = X.GEOMS[gi]
    cin, h, wd, cout, k, s = geom
    shape = conv_shape(_lib.CONV_F32_NHWC, geom)
    assert _lib.lib().rth_conv_dgrad_supported(ctypes.byref(shape)) == 1
    failures = []
    for kind in X.CONV_DGRAD_KINDS:
        c = X.conv_dgrad(10 * gi + n, geom, n, kind)
        gy, w = cl(c.ops["gy"], dev), cl(c.ops["w"], dev)
        gx = torch.full((n, cin, h, wd), NAN, device=dev).contiguous(memory_format=torch.channels_last)
        _lib.call("rth_conv_dgrad", ctypes.byref(shape), gy.data_ptr(), n, w.data_ptr(), gx.data_ptr(), _lib.stream_ptr())
        try:
            assert_bits(gx, c.want, f"dgrad conv{gi + 1} n={n} {kind}")
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("kind", ["x9", "f32"])
@pytest.mark.parametrize("gi", [1, 2])
@pytest.mark.parametrize("n", [1, 3])
def test_conv_wgrad(dev, gi, n, kind):
    """rth_conv_wgrad_x9 and the fp32-MFMA control: one output pixel of one sample carries the
    gradient (the last pixel of the last sample, then pixel 0 of sample 0) while every other
    sample's x is random; and class C within its bound"""
    from reth_amd import _lib

    geom = X.GEOMS[gi]
    cin, h, wd, cout, k, s = geom
    shape = conv_shape(_lib.CONV_F32_NHWC, geom)
    assert getattr(_lib.lib(), f"rth_conv_wgrad_{kind}_supported")(ctypes.byref(shape)) == 1
    ws = torch.full((getattr(_lib.lib(), f"rth_conv_wgrad_{kind}_workspace")(ctypes.byref(shape)) // 4,), NAN, device=dev)
    failures = []
    for wk in X.CONV_WGRAD_KINDS:
        for first in (False, True):
            c = X.conv_wgrad(10 * gi + n, geom, n, wk, first=first)
            x, gy = cl(c.ops["x"], dev), cl(c.ops["gy"], dev)
            gw = torch.full((cout, cin, k, k), NAN, device=dev).contiguous(memory_format=torch.channels_last)
            _lib.call(f"rth_conv_wgrad_{kind}", ctypes.byref(shape), x.data_ptr(), n, gy.data_ptr(), gw.data_ptr(),
                      ws.data_ptr(), _lib.stream_ptr())
            try:
                assert_bits(gw, c.want, f"wgrad_{kind} conv{gi + 1} n={n} {wk}{' first' if first else ' last'}")
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("n", [1, 7])
def test_conv1_wgrad_u8(dev, n):
    """k_conv1_wgrad_bf16x3 (the upstream gradient split by truncation, the bytes exact) through
    rth_conv_relu_wgrad: class D, the ReLU mask y positive exactly where the gradient is nonzero;
    the bias gradient (a sum of the same exact values) is pinned as well"""
    from reth_amd import _lib

    shape = conv_shape(_lib.CONV_U8_CHW, X.GEOMS[0])
    ws = torch.full((_lib.lib().rth_conv_wgrad_workspace(ctypes.byref(shape)) // 4,), NAN, device=dev)
    failures = []
    for kind in ("D/sel", "D/16", "D/C"):
        for first in (False, True):
            c = X.conv_wgrad(n, X.GEOMS[0], n, kind, first=first, u8=True)
            rng = np.random.default_rng(n)
            store = rng.integers(0, 256, (n + 5, 4, 84, 84)).astype(np.uint8)
            r = rng.permutation(n + 5)[:n]
            store[r] = c.ops["x"]
            g = np.ascontiguousarray(c.ops["gy"].transpose(0, 2, 3, 1))  # NHWC
            gd, yd = dv(g, dev), dv((g != 0).astype(np.float32), dev)
            gw = torch.full((32, 8, 8, 4), NAN, device=dev)  # OHWI
            gb = torch.full((32,), NAN, device=dev)
            stacks, rows = dv(store, dev), dv(r.astype(np.int64), dev)
            _lib.call("rth_conv_relu_wgrad", ctypes.byref(shape), stacks.data_ptr(), rows.data_ptr(), n, gd.data_ptr(), yd.data_ptr(), gw.data_ptr(), gb.data_ptr(), ws.data_ptr(), _lib.stream_ptr())
            try:
                what = f"conv1 wgrad u8 n={n} {kind}{' first' if first else ' last'}"
                assert_bits(gw.permute(0, 3, 1, 2), c.want, what)
                assert_bits(gb, c.meta["gb"], what + " (bias gradient)")
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, "\n".join(failures)
