"""The op-by-op Adam model of _adam_model.py, checked without a GPU (what test_exact_inputs_cpu.py
is to _exact_inputs.py): test_optim_edges_gpu.py holds the kernels to step32 bit for bit, so step32
itself is held here to an fp64 reference and to torch.

step32 against step64 with torch's fp32 CPU Adam (foreach=False, clip_grad_norm_(foreach=False))
as the fp32 yardstick, the project's bound per tensor:
    |model - fp64| <= max(1.5 |torch fp32 - fp64|, 1e-6 max|fp64|)
torch's CPU kernels are not bit-equal to the model (their vectorised lerp / addcmul fuse), so no
equality with torch is asserted.  step64 agrees with torch's fp64 CPU Adam to 1e-14 relative.
order_free_grads: the fp64 sum of squares is one double in three summation orders, and is not for
plain randn gradients.  bias_corr: bc2_sqrt is exactly 1 once beta2^t < 2^-25."""
import math

import numpy as np
import pytest
import torch

import _adam_model as A

F32, F64 = np.float32, np.float64
LR, EPS, B1, B2 = 1e-4, 1.5e-4, 0.9, 0.999


def _torch_chain(dtype, ps, max_norm):
    params = [torch.nn.Parameter(torch.tensor(p, dtype=dtype)) for p in ps]
    return params, torch.optim.Adam(params, lr=LR, betas=(B1, B2), eps=EPS, foreach=False)


def _torch_step(params, opt, grads, max_norm):
    for p, g in zip(params, grads):
        p.grad = torch.tensor(g, dtype=p.dtype)
    if max_norm is not None:
        torch.nn.utils.clip_grad_norm_(params, max_norm, foreach=False)
    opt.step()


def _torch_state(params, opt, key):
    return [opt.state[p][key].detach().numpy() for p in params]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("max_norm", [None, 40.0, 0.5])
def test_step32_within_bound_of_fp64(max_norm, seed):
    rng = np.random.default_rng(seed)
    p0 = [(rng.standard_normal(n) * 0.05).astype(F32) for n in A.SIZES]
    hp = A.host_scalars(B1, B2, EPS, max_norm)
    p32, m32, v32 = list(p0), [np.zeros(n, F32) for n in A.SIZES], [np.zeros(n, F32) for n in A.SIZES]
    p64, m64, v64 = [p.astype(F64) for p in p0], [np.zeros(n) for n in A.SIZES], [np.zeros(n) for n in A.SIZES]
    t32, o32 = _torch_chain(torch.float32, p0, max_norm)
    t64, o64 = _torch_chain(torch.float64, p0, max_norm)
    for t in range(1, 9):
        grads = [(rng.standard_normal(n) * (3.0 if t % 2 else 0.01)).astype(F32) for n in A.SIZES]
        total = A.exact_norm(grads)
        ss, b2 = A.bias_corr(LR, B1, B2, t)
        out = [A.step32(p, g, m, v, total=total, step_size=ss, bc2_sqrt=b2, **hp)
               for p, g, m, v in zip(p32, grads, m32, v32)]
        p32, m32, v32 = ([o[k] for o in out] for k in range(3))
        p64, m64, v64, _ = A.step64(p64, grads, m64, v64, lr=LR, beta1=B1, beta2=B2, eps=EPS, max_norm=max_norm, t=t)
        _torch_step(t32, o32, grads, max_norm)
        _torch_step(t64, o64, grads, max_norm)
    fails = []
    sets = (("p", p32, p64, [p.detach().numpy() for p in t32], [p.detach().numpy() for p in t64]),
            ("exp_avg", m32, m64, _torch_state(t32, o32, "exp_avg"), _torch_state(t64, o64, "exp_avg")),
            ("exp_avg_sq", v32, v64, _torch_state(t32, o32, "exp_avg_sq"), _torch_state(t64, o64, "exp_avg_sq")))
    for name, ours, ref64, th32, th64 in sets:
        for n, x, y, z, w in zip(A.SIZES, ours, ref64, th32, th64):
            scale = np.abs(y).max()
            e_model = np.abs(x.astype(F64) - y).max()
            e_torch = np.abs(z.astype(F64) - y).max()
            bound = max(1.5 * e_torch, 1e-6 * scale)
            if not e_model <= bound:
                fails.append((name, n, e_model, e_torch, bound))
            # step64 is torch's fp64 Adam
            assert np.abs(y - w).max() <= 1e-14 * scale, (name, n, np.abs(y - w).max(), scale)
    assert not fails, fails


def test_step32_scalars():
    """the clip coefficient: a quotient below 1 is kept, anything else is 1; no clipping: 1"""
    hp = A.host_scalars(max_norm=1.0)
    assert hp["clip"] and hp["w1"] == F32(1.0 - 0.9) and hp["w2"] == F32(1.0 - 0.999) and hp["eps"] == F32(1e-8)
    c = A.clip_coef(True, 1.0, F32(1.0))
    assert c == F32(1.0) / F32(1.0 + 2.0 ** -20) and c < 1  # 1 + 1e-6 rounds to 1 + 2^-20
    assert A.clip_coef(True, 64.0, F32(64.0)) == 1  # 64 + 1e-6 rounds to 64
    assert A.clip_coef(True, 40.0, F32(0.0)) == 1 and A.clip_coef(True, 0.0, F32(0.0)) == 0
    assert A.clip_coef(False, -1.0, F32(3.0)) == 1 and not A.host_scalars(max_norm=None)["clip"]
    # a zero gradient on zero state: p unchanged, m = v = +0
    p = np.array([1.5, -2.0], F32)
    z = np.zeros(2, F32)
    po, mo, vo, coef = A.step32(p, z, z, z, total=F32(0), step_size=F32(1e-3), bc2_sqrt=F32(0.03), **A.host_scalars(max_norm=40.0))
    assert coef == 1 and A.same_bits(po, p) and A.same_bits(mo, z) and A.same_bits(vo, z)


def test_step32_edge_values():
    """g g leaving fp32's range: v zero, subnormal, large and +inf, as the kernel's arithmetic"""
    hp = A.host_scalars(eps=1e-8, max_norm=None)
    ss, b2 = A.bias_corr(1e-3, 0.9, 0.999, 1)
    zero = np.zeros(1, F32)
    res = {g: A.step32(zero, np.array([g], F32), zero, zero, total=F32(abs(g)), step_size=ss, bc2_sqrt=b2, **hp)
           for g in A.EDGE_VALUES}
    tiny = np.finfo(F32).tiny
    for s in (1.0, -1.0):
        p, m, v, _ = res[s * 2.0 ** -80]
        assert v[0] == 0 and m[0] != 0 and p[0] != 0  # the denominator is eps: p still moves by m
        p, m, v, _ = res[s * 2.0 ** -70]
        assert 0 < v[0] < tiny
        p, m, v, _ = res[s * 2.0 ** 60]
        assert np.isfinite(v[0]) and np.isfinite(p[0]) and p[0] != 0
        p, m, v, _ = res[s * 2.0 ** 70]
        assert np.isposinf(v[0]) and np.isfinite(m[0]) and A.same_bits(p, zero)  # x / inf = 0: p stops moving
    p, m, v, _ = res[0.0]
    assert A.same_bits(p, zero) and A.same_bits(m, zero) and A.same_bits(v, zero)


def _sums(grads, rng):
    x = np.concatenate([g.astype(F64) for g in grads])
    sq = x * x

    def seq(a):
        s = 0.0
        for q in a.tolist():
            s += q
        return s

    fwd, rev = seq(sq), seq(sq[::-1])
    chunks = [sq[i:i + 2048] for i in range(0, len(sq), 2048)]
    parts = [seq(rng.permutation(c)) for c in chunks]
    perm = seq(np.array([parts[i] for i in rng.permutation(len(parts))]))
    return fwd, rev, perm


@pytest.mark.parametrize("scale_exp", [-6, 0, 2])
def test_order_free_grads_sum_in_any_order(scale_exp):
    rng = np.random.default_rng(5)
    grads = A.order_free_grads(rng, A.SIZES + A.SIZES, scale_exp)
    assert [len(g) for g in grads] == A.SIZES + A.SIZES and all(g.dtype == F32 for g in grads)
    k = np.concatenate(grads).astype(F64) * 2.0 ** (10 - scale_exp)
    assert np.array_equal(k, np.round(k)) and np.abs(k).max() <= 1024 and np.abs(k).max() > 512
    fwd, rev, perm = _sums(grads, rng)
    assert fwd == rev == perm == A.sum_squares(grads)
    assert A.exact_norm(grads) == F32(math.sqrt(fwd))


def test_plain_gradients_are_not_order_free():
    """the generator is what makes the norm order-free: randn gradients of the largest size
    sum to different doubles in different orders"""
    rng = np.random.default_rng(5)
    grads = [rng.standard_normal(max(A.SIZES)).astype(F32)]
    fwd, rev, perm = _sums(grads, rng)
    assert len({fwd, rev, perm}) > 1


def test_order_free_grads_refuses_an_inexact_sum():
    class Big:  # a generator whose draws would break the bound: 2^33 elements' worth of squares
        def integers(self, lo, hi, n):
            return np.full(n, 2 ** 27, dtype=np.int64)

    with pytest.raises(AssertionError, match="not exact"):
        A.order_free_grads(Big(), [4], 0)


@pytest.mark.parametrize("t", [1, 2, 10, 1000, 10 ** 6])
def test_bias_corr(t):
    ss, b2 = A.bias_corr(LR, B1, B2, t)
    assert ss.dtype == F32 and b2.dtype == F32
    assert ss == F32(LR / (1.0 - B1 ** t)) and b2 == F32(math.sqrt(1.0 - B2 ** t))
    if t == 1:
        assert ss == F32(LR / (1.0 - 0.9)) and b2 == F32(math.sqrt(1.0 - 0.999))
    assert (b2 == 1) == (B2 ** t < 2.0 ** -25)  # (none of these t lies between 2^-25 and the exact threshold 2^-24)
    if t == 10 ** 6:
        assert b2 == 1 and ss == F32(LR)


def test_bias_corr_reaches_one_at_the_threshold():
    """sqrt(1 - x) = 1 - x / 2 - ... rounds to 1.0 in fp32 exactly when it lies above 1 - 2^-25, the
    midpoint of 1 and the fp32 number below it: x < 2^-24, so certainly once x < 2^-25"""
    t0 = next(t for t in range(1, 10 ** 5) if B2 ** t < 2.0 ** -24)
    assert 16000 < t0 < 17000 and B2 ** (t0 + 1000) < 2.0 ** -25
    for t in (t0 - 100, t0 - 1):
        assert A.bias_corr(LR, B1, B2, t)[1] < 1
    for t in (t0 + 1, t0 + 100, t0 + 1000, 10 ** 5):
        assert A.bias_corr(LR, B1, B2, t)[1] == 1


def test_ulp_distance_and_bits():
    one = F32(1.0)
    assert A.ulp_distance(one, one) == 0 and A.ulp_distance(one, np.nextafter(one, F32(2))) == 1
    assert A.ulp_distance(np.nextafter(one, F32(0)), np.nextafter(one, F32(2))) == 2
    assert A.same_bits(np.array([0.0], F32), np.array([0.0], F32))
    assert not A.same_bits(np.array([0.0], F32), np.array([-0.0], F32))
    nan = np.array([np.nan], F32)
    assert A.same_bits(nan, nan.copy())
