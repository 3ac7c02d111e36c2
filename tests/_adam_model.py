"""clip_grad_norm_ + Adam as k_adam computes it, op by op (helper of test_adam_model_cpu.py,
test_optim_cpu.py and test_optim_edges_gpu.py; plain numpy, no import of the library).

The kernel's comments give its arithmetic exactly (reth_amd/csrc/optim.hip): every fp32 operation
is rounded on its own (radd / rsub / rmul under the no-contraction pragma), fp32 `/` and sqrtf are
the correctly rounded ones of the default build, the norm is an fp64 sum of exact squares rounded
to fp32 once after its square root, and the bias corrections are fp64 values rounded to fp32.
numpy's float32 arithmetic rounds every operation on its own and its divide and sqrt are the
correctly rounded IEEE ones, so step32 below is that specification: one numpy operation per
operation of adam1 / opt_scalars, in the kernel's order.  A correct kernel returns its bits.

The norm is the one order-dependent part.  order_free_grads makes it order-free: every gradient is
k 2^(scale_exp - 10) with an integer |k| <= 1024, so every square is an integer multiple of the
unit 2^(2 scale_exp - 20), at most 2^20 units, and the sum of all of them stays below 2^53 units --
every partial sum, in any order and any grouping, is an integer below 2^53 units and therefore
exact in fp64.  The only total_norm a correct kernel can return is exact_norm.
"""
import math

import numpy as np

F32, F64, U32, I32 = np.float32, np.float64, np.uint32, np.int32

# 16 tensors in one call: tails inside a float4 (1, 2, 3, 5, 1023, 1025, ...), PPO's and DDPG's
# real sizes (1, 2, 18, 64, 256), both sides of the boundary between a lane's two float4 groups
# (1,024) and of the workgroup boundary (2,048), and segments of two and three workgroups
SIZES = [1, 2, 3, 4, 5, 18, 64, 256, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 6143]

# gradients at which g * g leaves fp32's range: (w2 g) g is zero at 2^-80, subnormal at 2^-70,
# large at 2^60 and +inf at 2^70
EDGE_VALUES = [0.0, 2.0 ** -80, -2.0 ** -80, 2.0 ** -70, -2.0 ** -70, 2.0 ** 60, -2.0 ** 60, 2.0 ** 70, -2.0 ** 70]


def host_scalars(beta1=0.9, beta2=0.999, eps=1e-8, max_norm=None):
    """the scalars as adam_launch hands them to k_adam: python floats rounded to fp32 once
    (max_norm None or negative: no clipping)"""
    clip = max_norm is not None and max_norm >= 0
    return dict(w1=F32(1.0 - beta1), beta2=F32(beta2), w2=F32(1.0 - beta2), eps=F32(eps), clip=clip,
                max_norm=F32(max_norm if clip else -1.0))


def clip_coef(clip, max_norm, total):
    """opt_scalars: max_norm / (total + 1e-6) in fp32, clamped to 1 only if < 1"""
    if not clip:
        return F32(1.0)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        c = F32(max_norm) / (F32(total) + F32(1e-6))
    return c if c < F32(1.0) else F32(1.0)


def step32(p, g, m, v, *, w1, beta2, w2, eps, clip, max_norm, total, step_size, bc2_sqrt):
    """one tensor's update as k_adam's adam1 computes it; returns (p, m, v, coef), the inputs
    unchanged.  total: the fp32 norm of all gradients of the call before clipping."""
    p, g, m, v = (np.array(x, dtype=F32) for x in (p, g, m, v))
    w1, beta2, w2, eps, step_size, bc2_sqrt = (F32(x) for x in (w1, beta2, w2, eps, step_size, bc2_sqrt))
    assert all(x.dtype == F32 for x in (p, g, m, v))
    coef = clip_coef(clip, max_norm, total)
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        if clip:
            g = g * coef                    # rmul(g, coef)
        d = g - m                           # rsub(g, m)
        d = w1 * d                          # rmul(w1, .)
        m = m + d                           # radd(m, .)
        a = v * beta2                       # rmul(v, beta2)
        b = w2 * g                          # rmul(w2, g)
        b = b * g                           # rmul(., g)
        v = a + b                           # radd
        s = np.sqrt(v)                      # sqrtf(v)
        s = s / bc2_sqrt                    # / bc2_sqrt
        denom = s + eps                     # radd(., eps)
        u = (-step_size) * m                # rmul(-step_size, m)
        u = u / denom                       # / denom
        p = p + u                           # radd(p, .)
    assert p.dtype == F32 and m.dtype == F32 and v.dtype == F32
    return p, m, v, coef


def bias_corr(lr, beta1, beta2, t):
    """(step_size, bc2_sqrt) of step t: adam.py's python-float scalars rounded to fp32"""
    return F32(lr / (1.0 - beta1 ** t)), F32(math.sqrt(1.0 - beta2 ** t))


def sum_squares(grads):
    """the correctly rounded fp64 sum of the exact squares of every gradient element"""
    sq = []
    for g in grads:
        x = np.asarray(g, dtype=F64).ravel()
        sq.extend((x * x).tolist())  # an fp32 number's square is exact in fp64 (48 bits; the test's exponents fit)
    return math.fsum(sq)


def exact_norm(grads):
    """fp32(sqrt(sum of squares)): the kernel's (float) sqrt(double)"""
    return F32(math.sqrt(sum_squares(grads)))


def step64(ps, gs, ms, vs, *, lr, beta1, beta2, eps, max_norm, t):
    """the same step of all tensors in fp64 throughout (the high-precision reference): returns
    (ps, ms, vs, total), lists of fp64 arrays and the fp64 norm"""
    gs = [np.asarray(g, dtype=F64) for g in gs]
    total = math.sqrt(sum_squares(gs))
    coef = 1.0
    if max_norm is not None and max_norm >= 0:
        coef = min(max_norm / (total + 1e-6), 1.0)
    step_size, bc2_sqrt = lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t)
    po, mo, vo = [], [], []
    with np.errstate(over="ignore", under="ignore", invalid="ignore", divide="ignore"):
        for p, g, m, v in zip(ps, gs, ms, vs):
            p, m, v = (np.asarray(x, dtype=F64) for x in (p, m, v))
            g = g * coef
            m = m + (1.0 - beta1) * (g - m)
            v = v * beta2 + (1.0 - beta2) * g * g
            p = p - step_size * m / (np.sqrt(v) / bc2_sqrt + eps)
            po.append(p), mo.append(m), vo.append(v)
    return po, mo, vo, total


def order_free_grads(rng, sizes, scale_exp=0):
    """one fp32 gradient per size: k 2^(scale_exp - 10), k a random integer in [-1024, 1024].
    Every square is k^2 <= 2^20 units of 2^(2 scale_exp - 20) and the sum of all squares is below
    2^53 units (asserted), so the fp64 sum of squares is exact in every order: exact_norm is the
    only norm a correct kernel returns."""
    assert -100 <= scale_exp <= 100  # k 2^(scale_exp - 10) and its square are normal fp32 / fp64 numbers
    ks = [rng.integers(-1024, 1025, int(n)) for n in sizes]
    units = sum(int((k.astype(np.int64) ** 2).sum()) for k in ks)
    assert units < 2 ** 53, "the sum of squares is not exact in fp64"
    out = [(k * 2.0 ** (scale_exp - 10)).astype(F32) for k in ks]
    for k, g in zip(ks, out):
        assert np.array_equal(g.astype(F64), k * 2.0 ** (scale_exp - 10))
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(U32)


def same_bits(a, b):
    """bit equality of two fp32 arrays (the sign of zero and NaN payloads included)"""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    return a.shape == b.shape and bool(np.array_equal(a.view(U32), b.view(U32)))


def ulp_distance(a, b):
    """the number of fp32 numbers between two finite values of one sign (0: equal)"""
    a, b = F32(a), F32(b)
    assert np.isfinite(a) and np.isfinite(b) and (a >= 0) == (b >= 0)
    return abs(int(np.abs(a).view(I32)) - int(np.abs(b).view(I32)))
