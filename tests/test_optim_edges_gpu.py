"""rth_clip_adam / rth_adam_prenormed (ClipAdam) against the op-by-op fp32 model of
_adam_model.py, bit for bit, at the chunk, float4 and workgroup edges of k_adam / k_grad_sqsum.

The kernels' comments state their arithmetic exactly (every fp32 operation rounded on its own,
correctly rounded fp32 divide and sqrtf, an fp64 norm rounded once), and _adam_model.step32 is that
statement in numpy (checked on the CPU by test_adam_model_cpu.py).  The norm, the one part that
depends on a summation order, is made order-free by the inputs (_adam_model.order_free_grads), so
every comparison below is an equality of bits unless it says otherwise:

a  16 (and 32) tensors of _adam_model.SIZES in one call, 6 steps, nonzero state: total_norm, the
   scalars read back from the workspace, and p / m / v of every tensor after every step
b  the same runs against fp64 (_adam_model.step64), the project's bound per tensor with step32 as
   the fp32 yardstick: |ours - fp64| <= max(1.5 |model - fp64|, 1e-6 max|fp64|)
c  randn gradients (not order-free): total_norm within one fp32 ulp of the exact norm (the fp64
   sum's relative error is below 2^-38 at these sizes), p / m / v equal to the model fed that norm
d  each of the four arrays alone 4, 8 and 12 bytes past a 16-byte boundary (the scalar ld4 / st4
   path): equal to the aligned run
e  NaN and sentinel guard bands of 64 elements around every array: nothing past n is read into the
   norm or the update, nothing past n is written, .grad is unchanged
f  partial counts around kPartLoads x kOptThreads = 1,280 through rth_adam_prenormed
g  the clip coefficient where max_norm / (total + 1e-6) meets 1, and a zero gradient
h  gradients whose square leaves fp32's range (_adam_model.EDGE_VALUES)
i  the device step count and its bias corrections at t = 1, 10, 1000, 10^6; repeatability

Every array of every test lives inside a flat buffer with 64 elements of margin on both sides --
NaN beside .grad, a sentinel beside the others, unless the test says otherwise -- and every step
checks that the margins and .grad are unchanged (Chain.step).

On the MI355X p, m and v are bit-equal to the model in every test: the fallback to the fp64 bound
that a not correctly rounded sqrtf or divide would have called for is not used."""
import math

import numpy as np
import pytest
import torch

import _adam_model as A

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
KINDS = ("param", "grad", "exp_avg", "exp_avg_sq")
MARGIN = 64
MAX_PARTS = 32768
SC_OFF = MAX_PARTS * 8  # include/reth_hip.h: [32,768 doubles][OptScalars 16 B][BiasCorr 8 B]
B1, B2 = 0.9, 0.999
SENTINEL, NAN = F32(-12345.678), F32(np.nan)
# the margins of every test unless it says otherwise: NaN beside .grad (a read past n poisons the
# norm and the update), a sentinel beside the arrays that are written
GUARD = dict(param=SENTINEL, grad=NAN, exp_avg=SENTINEL, exp_avg_sq=SENTINEL)
ALL_NAN = dict(param=NAN, grad=NAN, exp_avg=NAN, exp_avg_sq=NAN)
ZEROS = dict(param=F32(0), grad=F32(0), exp_avg=F32(0), exp_avg_sq=F32(0))


class Rig:
    """the four arrays of every tensor as views into one flat device buffer per kind: tensor i of
    kind k starts `offsets[k]` bytes past a 16-byte boundary, with at least MARGIN elements holding
    `fills[k]` (default GUARD) on both sides"""

    def __init__(self, dev, sizes, offsets=None, fills=None):
        self.sizes = [int(n) for n in sizes]
        self.off = {k: (offsets or {}).get(k, 0) for k in KINDS}
        self.start, self.host, self.buf, self.inside = {}, {}, {}, {}
        for k in KINDS:
            assert self.off[k] in (0, 4, 8, 12)
            cur, st = 0, []
            for n in self.sizes:
                cur += MARGIN
                st.append(cur + self.off[k] // 4)
                cur = (st[-1] + n + 3) // 4 * 4
            total = cur + MARGIN + 4
            self.start[k] = st
            self.host[k] = np.full(total, (fills or GUARD)[k], dtype=F32)
            self.inside[k] = np.zeros(total, dtype=bool)
            for s, n in zip(st, self.sizes):
                self.inside[k][s:s + n] = True
            self.buf[k] = torch.empty(total, dtype=torch.float32, device=dev)
            assert self.buf[k].data_ptr() % 16 == 0
            self.buf[k].copy_(torch.from_numpy(self.host[k]))

    def put(self, kind, arrays):
        for s, n, a in zip(self.start[kind], self.sizes, arrays):
            assert a.dtype == F32 and a.shape == (n,)
            self.host[kind][s:s + n] = a
        self.buf[kind].copy_(torch.from_numpy(self.host[kind]))

    def get(self, kind):
        """(the tensors, margins unchanged) as the device holds them now"""
        d = self.buf[kind].cpu().numpy()
        out = [d[s:s + n].copy() for s, n in zip(self.start[kind], self.sizes)]
        m = ~self.inside[kind]
        return out, A.same_bits(d[m], self.host[kind][m])

    def views(self, kind):
        vs = [self.buf[kind][s:s + n] for s, n in zip(self.start[kind], self.sizes)]
        for v in vs:
            assert v.data_ptr() % 16 == self.off[kind]
        return vs

    def make_opt(self, **kw):
        from reth_amd.optim import ClipAdam

        ps = [torch.nn.Parameter(v) for v in self.views("param")]
        opt = ClipAdam(ps, **kw)
        for p, g, m, v in zip(ps, self.views("grad"), self.views("exp_avg"), self.views("exp_avg_sq")):
            p.grad = g
            opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"] = m, v
        for k, ts in (("param", ps), ("grad", [p.grad for p in ps]), ("exp_avg", [opt.state[p]["exp_avg"] for p in ps]),
                      ("exp_avg_sq", [opt.state[p]["exp_avg_sq"] for p in ps])):
            for t, s in zip(ts, self.start[k]):  # the optimizer sees the views themselves
                assert t.data_ptr() == self.buf[k].data_ptr() + 4 * s and t.data_ptr() % 16 == self.off[k]
        return opt


def read_scalars(opt):
    """(coef, step_size, bc2_sqrt, total_norm) of the last update and the (step_size, bc2_sqrt) of
    the current step, from the workspace"""
    w = opt._ws[SC_OFF:SC_OFF + 24].cpu().numpy().view(F32)
    return w[:4].copy(), w[4:6].copy()


def first_diff(got, want):
    bad = np.flatnonzero(A.bits(got) != A.bits(want))
    i = int(bad[0])
    return f"{len(bad)} of {len(want)} differ, first at {i}: got {got[i]!r} ({A.bits(got)[i]:#010x}) want " \
           f"{want[i]!r} ({A.bits(want)[i]:#010x})"


class Chain:
    """one ClipAdam on a Rig and the model's copy of its state (fp32, and fp64 with ref64)"""

    def __init__(self, dev, sizes, *, lr=1e-3, eps=1e-8, max_norm=None, seed=0, zero_state=False, zero_param=False,
                 offsets=None, fills=None, ref64=False):
        rng = np.random.default_rng(seed)
        self.sizes, self.lr, self.eps, self.max_norm = list(sizes), lr, eps, max_norm
        self.p = [(rng.standard_normal(n) * 0.05).astype(F32) for n in sizes]
        self.m = [(rng.standard_normal(n) * 0.01).astype(F32) for n in sizes]
        self.v = [(rng.random(n) * 1e-3).astype(F32) for n in sizes]  # v >= 0
        if zero_state:
            self.m, self.v = [np.zeros(n, F32) for n in sizes], [np.zeros(n, F32) for n in sizes]
        if zero_param:
            self.p = [np.zeros(n, F32) for n in sizes]
        self.rig = Rig(dev, sizes, offsets, fills)
        for k, a in (("param", self.p), ("exp_avg", self.m), ("exp_avg_sq", self.v)):
            self.rig.put(k, a)
        self.opt = self.rig.make_opt(lr=lr, betas=(B1, B2), eps=eps, max_norm=max_norm)
        self.hp = A.host_scalars(B1, B2, eps, max_norm)
        self.t = 0
        self.r64 = ([x.astype(F64) for x in self.p], [x.astype(F64) for x in self.m],
                    [x.astype(F64) for x in self.v]) if ref64 else None
        self.dev_state = None

    def set_step(self, t):
        self.opt._step.fill_(t)
        self.t = t

    def step(self, grads, *, want_total=None, ulps=0, prenormed=None, bc=None, bits=True):
        """one device step and the model's; asserts everything (a) lists.  want_total: the norm
        expected (default: the exact norm of `grads`), met within `ulps`.  prenormed: the partial
        count of an rth_adam_prenormed step, whose bias corrections `bc` the test wrote.
        bits=False: no equality asserted on p / m / v (run b)."""
        rig, opt = self.rig, self.opt
        rig.put("grad", grads)
        if prenormed is not None:
            opt.prenorm(prenormed)
        else:
            self.t += 1
        opt.step()
        total = F32(opt.total_norm.cpu().numpy()[0])
        sc, bcw = read_scalars(opt)
        assert int(opt._step.item()) == self.t
        want = A.exact_norm(grads) if want_total is None else F32(want_total)
        assert np.isfinite(total) and A.ulp_distance(total, want) <= ulps, (total, want)
        assert A.same_bits(sc[3], total) and A.same_bits(sc[1:3], bcw)
        if bc is None:
            ss, b2 = A.bias_corr(self.lr, B1, B2, self.t)  # the device's fp64 pow may differ in the last bit
            assert A.ulp_distance(bcw[0], ss) <= 1 and A.ulp_distance(bcw[1], b2) <= 1, (bcw, ss, b2)
        else:
            assert A.same_bits(bcw, np.array(bc, F32))
        out = [A.step32(p, g, m, v, total=total, step_size=bcw[0], bc2_sqrt=bcw[1], **self.hp)
               for p, g, m, v in zip(self.p, grads, self.m, self.v)]
        assert A.same_bits(sc[0], out[0][3]), (sc[0], out[0][3])
        self.coef = sc[0]
        self.p, self.m, self.v = ([o[k] for o in out] for k in range(3))
        self.total = total
        got = {}
        for k in KINDS:
            got[k], intact = rig.get(k)
            assert intact, f"the margins of {k} changed"
        for i, (x, y) in enumerate(zip(got["grad"], grads)):
            assert A.same_bits(x, y), f".grad of tensor {i} ({self.sizes[i]}) changed: " + first_diff(x, y)
        self.dev_state = (got["param"], got["exp_avg"], got["exp_avg_sq"])
        if bits:
            # m and v first: adds and multiplies only
            for name, dv, md in (("exp_avg", got["exp_avg"], self.m), ("exp_avg_sq", got["exp_avg_sq"], self.v),
                                 ("param", got["param"], self.p)):
                for i, (x, y) in enumerate(zip(dv, md)):
                    assert A.same_bits(x, y), f"step {self.t} {name} of tensor {i} ({self.sizes[i]}): " + first_diff(x, y)
        if self.r64 is not None:
            assert prenormed is None
            self.r64 = A.step64(*self.r64[:1], grads, *self.r64[1:], lr=self.lr, beta1=B1, beta2=B2, eps=self.eps,
                                max_norm=self.max_norm, t=self.t)[:3]

    def same_device_state(self, other):
        for name, xs, ys in zip(("param", "exp_avg", "exp_avg_sq"), self.dev_state, other.dev_state):
            for i, (x, y) in enumerate(zip(xs, ys)):
                assert A.same_bits(x, y), f"{name} of tensor {i} ({self.sizes[i]}): " + first_diff(x, y)
        assert A.same_bits(self.total, other.total) and A.same_bits(self.coef, other.coef)


# (lr, eps, max_norm): the conv learner's setting with every clip, and PPO's / DDPG's (the defaults)
SETTINGS = [(1e-4, 1.5e-4, None), (1e-4, 1.5e-4, 0.5), (1e-4, 1.5e-4, 40.0), (1e-4, 1.5e-4, 0.0), (1e-3, 1e-8, None)]
# the gradients' scale by step: norms of about 84, 1.3, 340, 84, 0.3, 170 -- max_norm = 40 and 0.5 clip some steps only
SCALE_EXPS = [0, -6, 2, 0, -8, 1]


def run_chain(dev, sizes, lr, eps, max_norm, *, bits, ref64=False, seed=7):
    ch = Chain(dev, sizes, lr=lr, eps=eps, max_norm=max_norm, seed=seed, ref64=ref64)
    rng = np.random.default_rng(seed + 100)
    coefs = []
    for e in SCALE_EXPS:
        ch.step(A.order_free_grads(rng, sizes, e), bits=bits)
        coefs.append(float(ch.coef))
    return ch, coefs


# ------------------------------------------------------------------ a. bit equality, vector path
@pytest.mark.parametrize("lr,eps,max_norm", SETTINGS)
def test_a_model_bits(dev, lr, eps, max_norm):
    ch, coefs = run_chain(dev, A.SIZES, lr, eps, max_norm, bits=True)
    if max_norm == 40.0:  # both sides of the clamp
        assert any(c == 1 for c in coefs) and any(c < 1 for c in coefs), coefs
    elif max_norm == 0.5:
        assert all(c > 0 for c in coefs) and sum(c < 1 for c in coefs) >= 4, coefs
    elif max_norm == 0.0:
        assert all(c == 0 for c in coefs), coefs
    else:
        assert all(c == 1 for c in coefs), coefs


def test_a_model_bits_32_tensors(dev):
    """RTH_MAX_PARAM_TENSORS segments"""
    run_chain(dev, A.SIZES + A.SIZES, 1e-4, 1.5e-4, 0.5, bits=True)


# ------------------------------------------------------------------ b. against fp64
@pytest.mark.parametrize("lr,eps,max_norm", SETTINGS)
def test_b_fp64_bound(dev, lr, eps, max_norm):
    ch, _ = run_chain(dev, A.SIZES, lr, eps, max_norm, bits=False, ref64=True)
    fails = []
    for name, ours, m32, r64 in zip(("param", "exp_avg", "exp_avg_sq"), ch.dev_state, (ch.p, ch.m, ch.v), ch.r64):
        for n, x, y, z in zip(A.SIZES, ours, m32, r64):
            scale = float(np.abs(z).max())
            e_ours = float(np.abs(x.astype(F64) - z).max())
            e_ref = float(np.abs(y.astype(F64) - z).max())
            bound = max(1.5 * e_ref, 1e-6 * scale)
            print(f"{name + ' [' + str(n) + '] max_norm ' + str(max_norm):44s} |ours - fp64| {e_ours:.3e}  "
                  f"|model - fp64| {e_ref:.3e}  bound {bound:.3e}  max|fp64| {scale:.3e}")
            if not e_ours <= bound:
                fails.append((name, n, e_ours, e_ref, bound))
    assert not fails, fails


# ------------------------------------------------------------------ c. general gradients
@pytest.mark.parametrize("max_norm", [0.5, 40.0])
def test_c_randn_gradients(dev, max_norm):
    ch = Chain(dev, A.SIZES, lr=1e-4, eps=1.5e-4, max_norm=max_norm, seed=11)
    rng = np.random.default_rng(12)
    for t in range(3):
        grads = [(rng.standard_normal(n) * (3.0 if t % 2 else 0.01)).astype(F32) for n in A.SIZES]
        ch.step(grads, ulps=1)


# ------------------------------------------------------------------ d. scalar paths and alignment
_aligned = {}


def aligned_step(dev):
    """one clipped step on aligned arrays with zeros for margins (the unguarded run): what (d) and
    (e) compare with"""
    if "ch" not in _aligned:
        _aligned["grads"] = A.order_free_grads(np.random.default_rng(21), A.SIZES, 0)
        ch = Chain(dev, A.SIZES, lr=1e-4, eps=1.5e-4, max_norm=0.5, seed=20, fills=ZEROS)
        ch.step(_aligned["grads"])
        _aligned["ch"] = ch
    return _aligned["ch"], _aligned["grads"]


@pytest.mark.parametrize("off", [4, 8, 12])
@pytest.mark.parametrize("kind", KINDS)
def test_d_one_array_misaligned(dev, kind, off):
    ref, grads = aligned_step(dev)
    ch = Chain(dev, A.SIZES, lr=1e-4, eps=1.5e-4, max_norm=0.5, seed=20, offsets={kind: off})
    for k in KINDS:
        for v in ch.rig.views(k):
            assert v.data_ptr() % 16 == (off if k == kind else 0)
    ch.step(grads)
    ch.same_device_state(ref)


# ------------------------------------------------------------------ e. guard bands
@pytest.mark.parametrize("fills", [GUARD, ALL_NAN], ids=["grad-nan", "all-nan"])
@pytest.mark.parametrize("offsets", [None, {"grad": 4}, {"param": 8}, {"exp_avg": 12, "exp_avg_sq": 4}],
                         ids=["vector", "grad+4", "param+8", "m+12,v+4"])
def test_e_guard_bands(dev, offsets, fills):
    ref, grads = aligned_step(dev)
    ch = Chain(dev, A.SIZES, lr=1e-4, eps=1.5e-4, max_norm=0.5, seed=20, offsets=offsets, fills=fills)
    ch.step(grads)  # the margins and .grad unchanged, the norm finite and exact
    assert 0 < ch.coef < 1  # the clip is active
    for xs in ch.dev_state:
        assert all(np.isfinite(x).all() for x in xs)
    ch.same_device_state(ref)


# ------------------------------------------------------------------ f. partial counts
@pytest.mark.parametrize("nparts", [1, 2, 255, 256, 257, 1279, 1280, 1281, 1536, MAX_PARTS])
def test_f_prenormed_partial_counts(dev, nparts):
    sizes = [5, 2049]
    rng = np.random.default_rng(nparts)
    bc = A.bias_corr(1e-3, B1, B2, 4)
    for pattern in "AB":
        ch = Chain(dev, sizes, lr=1e-3, eps=1e-8, max_norm=0.25, seed=30)
        ch.set_step(3)
        parts = np.full(MAX_PARTS, np.nan)
        if pattern == "A":  # integers: exact in any order, the sum below 2^22
            parts[:nparts] = 1 + np.arange(nparts) % 4
        else:  # only the last partial counts
            parts[:nparts] = 0.0
            parts[nparts - 1] = 7.0
        s = math.fsum(parts[:nparts].tolist())
        assert s == int(s) < 2 ** 22
        ws = ch.opt._ws
        ws[:SC_OFF].view(torch.float64).copy_(torch.from_numpy(parts))
        ws[SC_OFF:SC_OFF + 16].view(torch.float32).fill_(float("nan"))  # the update rewrites its scalars
        ws[SC_OFF + 16:SC_OFF + 24].view(torch.float32).copy_(torch.from_numpy(np.array(bc, F32)))
        grads = [rng.standard_normal(n).astype(F32) for n in sizes]
        ch.step(grads, want_total=F32(math.sqrt(s)), prenormed=nparts, bc=bc)
        assert 0 < ch.coef < 1
        assert int(ch.opt._step.item()) == 3  # prenormed does not advance the step count
        back = ws[:SC_OFF].view(torch.float64).cpu().numpy()
        assert np.array_equal(back.view(np.uint64), parts.view(np.uint64))  # the partials are read only


# ------------------------------------------------------------------ g. the clip boundary
def _sparse_grads(value):
    """four elements of `value` at the ends of different tensors, zero elsewhere: norm 2 |value|"""
    grads = [np.zeros(n, F32) for n in A.SIZES]
    for i, j in ((0, 0), (8, 1022), (13, 2048), (15, 6142)):
        assert j == A.SIZES[i] - 1
        grads[i][j] = value
    return grads


def test_g_clip_boundary_below_one(dev):
    """total = max_norm = 1: coef is the fp32 quotient 1 / (1 + 1e-6) < 1, the gradient is scaled"""
    ch = Chain(dev, A.SIZES, lr=1e-4, eps=1.5e-4, max_norm=1.0, seed=40)
    ch.step(_sparse_grads(0.5), want_total=1.0)
    assert ch.total == 1 and ch.coef == F32(1.0) / F32(1.0 + 2.0 ** -20) and ch.coef < 1
    ch.step(_sparse_grads(-0.5), want_total=1.0)


def test_g_clip_boundary_exactly_one(dev):
    """total = max_norm = 64: 64 + 1e-6 rounds to 64, coef is exactly 1: the unclipped step"""
    a = Chain(dev, A.SIZES, lr=1e-4, eps=1.5e-4, max_norm=64.0, seed=40)
    b = Chain(dev, A.SIZES, lr=1e-4, eps=1.5e-4, max_norm=None, seed=40)
    for value in (32.0, -32.0):
        a.step(_sparse_grads(value), want_total=64.0)
        b.step(_sparse_grads(value), want_total=64.0)
        assert a.total == 64 and A.same_bits(a.coef, F32(1.0))
        a.same_device_state(b)


@pytest.mark.parametrize("max_norm", [None, 40.0])
def test_g_zero_gradient(dev, max_norm):
    ch = Chain(dev, A.SIZES, lr=1e-4, eps=1.5e-4, max_norm=max_norm, seed=41, zero_state=True)
    p0 = [x.copy() for x in ch.p]
    ch.step([np.zeros(n, F32) for n in A.SIZES], want_total=0.0)
    assert A.same_bits(ch.total, F32(0.0)) and A.same_bits(ch.coef, F32(1.0))
    p, m, v = ch.dev_state
    for x, y, mm, vv in zip(p, p0, m, v):
        assert A.same_bits(x, y) and A.same_bits(mm, np.zeros_like(mm)) and A.same_bits(vv, np.zeros_like(vv))


# ------------------------------------------------------------------ h. edge values
@pytest.mark.parametrize("g", A.EDGE_VALUES, ids=lambda g: f"{g:g}")
def test_h_edge_values(dev, g):
    grads = [np.full(64, g, F32)]
    assert float(grads[0][0]) == g
    for zero_state in (True, False):
        for max_norm in (None, 40.0):
            # (with the zero state p starts at 0 as well: a move of 1e-19 shows there)
            ch = Chain(dev, [64], lr=1e-3, eps=1e-8, max_norm=max_norm, seed=50, zero_state=zero_state,
                       zero_param=zero_state)
            p0 = ch.p[0].copy()
            ch.step(grads)  # 64 equal squares: every partial sum is exact
            p, m, v = (x[0] for x in ch.dev_state)
            if max_norm is None:
                assert np.isfinite(p).all()
                if zero_state and abs(g) == 2.0 ** -80:  # v stays 0, the denominator is eps, p moves by m
                    assert (v == 0).all() and (m != 0).all() and (p != p0).all()
                if zero_state and abs(g) == 2.0 ** -70:
                    assert ((v > 0) & (v < np.finfo(F32).tiny)).all()
                if abs(g) == 2.0 ** 70:  # x / inf = 0: p stops moving
                    assert np.isposinf(v).all() and np.isfinite(m).all() and A.same_bits(p, p0)
            else:
                assert np.isfinite(p).all() and np.isfinite(v).all()  # 40 / 2^73 brings 2^70 back into range


# ------------------------------------------------------------------ i. the step count
@pytest.mark.parametrize("t0", [0, 9, 999, 10 ** 6 - 1])
def test_i_step_count(dev, t0):
    sizes = [5, 256, 2049]
    ch = Chain(dev, sizes, lr=1e-4, eps=1.5e-4, max_norm=0.5, seed=60)
    ch.set_step(t0)
    ch.step(A.order_free_grads(np.random.default_rng(61), sizes, 0))
    assert int(ch.opt._step.item()) == t0 + 1
    _, bcw = read_scalars(ch.opt)
    if t0 + 1 == 10 ** 6:
        assert A.same_bits(bcw[1], F32(1.0)) and A.ulp_distance(bcw[0], F32(1e-4)) <= 1


def test_i_repeatable(dev):
    """twenty steps from one restored state: the same bits every time"""
    sizes = A.SIZES
    ch = Chain(dev, sizes, lr=1e-4, eps=1.5e-4, max_norm=0.5, seed=62)
    grads = [(np.random.default_rng(63).standard_normal(n)).astype(F32) for n in sizes]
    ch.rig.put("grad", grads)
    saved = {k: ch.rig.buf[k].clone() for k in KINDS}
    first = None
    for _ in range(20):
        for k in KINDS:
            ch.rig.buf[k].copy_(saved[k])
        ch.opt._step.fill_(5)
        ch.opt.step()
        now = [ch.rig.buf[k].clone().view(torch.int32) for k in KINDS] + [ch.opt.total_norm.clone().view(torch.int32)]
        if first is None:
            first = now
            assert not torch.equal(now[0], saved["param"].view(torch.int32))
        assert all(torch.equal(x, y) for x, y in zip(now, first))
        assert int(ch.opt._step.item()) == 6
