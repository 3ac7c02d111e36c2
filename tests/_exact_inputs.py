"""Order-free inputs for the exact-split kernels (helper of test_exact_inputs_cpu.py and
test_exact_split_gpu.py; plain numpy / torch on the CPU, no import of the library).

Every generator returns a Case: the operands and the one fp32 result a correct kernel can return,
whatever its tile form, k split or reduce launch -- computed in fp64 and rounded once.  (The order
of the nine term pairs inside a chunk is free for class C only; a single product needs its three
terms added in a monotone order, as the kernels do: test_exact_inputs_cpu.py.)  The result does not depend on the summation order because either every output has ONE
nonzero product (classes A, B, D: "selection") or every product and every partial sum is an
integer multiple of one unit and stays below 2^22 units (class C: "dense").

A  one product per output: one operand holds arbitrary fp32 bit patterns (random, exponents in
   [-60, 60], plus the directed list DIRECTED), the other one +-2^j per row; with a bias chosen so
   that product + bias is exact in fp64 -- the kernel's single add is the reference's single
   rounding.  (For fp32 operands fp64-then-fp32 rounding of a sum is the correctly rounded fp32 sum
   anyway -- 53 >= 2 * 24 + 2, Figueroa 1995 -- the exponent placement only makes that plain.)
B  one product per output, the factors with p and q significant bits, p + q <= 24.
C  dense: small integers, and three-term integers a 2^18 + b 2^9 + c against a sparse 0 / +-1
   operand whose nonzeros straddle the 32-deep chunks and the k-split boundaries.
D  the uint8 forms of A, B and C (conv1 on bytes).
E  one +inf and one NaN in the pattern operand of A or C: the outputs whose dot product meets one
   are non-finite in the reference too (inf * 0 = NaN); all others keep their finite expectation.

Zeros: an accumulator starts at +0 and +0 + -0 = +0, so every zero sum is expected as +0.
"""
from dataclasses import dataclass, field

import numpy as np

F32, F64, U32 = np.float32, np.float64, np.uint32

# 23-bit mantissa fields (the significand is 1.m, 24 bits)
DIRECTED = np.array([
    0x7fffff,  # significand all ones: rounding to bf16 carries into the next binade, second term negative
    0x3fffff, 0x00ffff, 0x007fff,  # runs of ones below the bf16 cut (just below a tie / far above)
    0x028000, 0x548000,  # exact bf16 ties (low 16 bits == 0x8000) above an even bf16
    0x038000, 0x7f8000,  # ... above an odd bf16 (0x7f8000: the tie carries into the next binade)
    0x008001, 0x017fff,  # one ulp above / below a tie
    0x000000, 0x550000, 0x7f0000,  # already bf16
    0x2a8000,  # exactly 9 significant bits
    0x2a5b00,  # exactly 16
    0x2a5b80,  # exactly 17
    0x2a5b81,  # exactly 24
    0x00807f, 0x7f80ff,  # second term a tie as well
], dtype=U32)


def sig_bits(rng, n, p):
    """n mantissa fields of values with exactly p significant bits (leading and last bit set,
    the p - 2 between them random)"""
    if p == 1:
        return np.zeros(n, dtype=U32)
    m = rng.integers(0, 1 << 23, n, dtype=np.int64)
    low = 24 - p  # position of the last significant bit
    m = (m >> low << low) | (1 << low)
    return m.astype(U32)


def pattern_values(rng, shape, exp_axis, bits=24, directed=True, emin=-60, emax=60):
    """fp32 patterns of `shape`: the exponent depends on the index along exp_axis only (so that a
    bias per output column can sit near every product of that column), mantissas random with
    `bits` significant bits, a quarter of them from DIRECTED, a few +-0.  Returns (values, e)."""
    shape = tuple(int(s) for s in shape)
    n = int(np.prod(shape))
    mant = sig_bits(rng, n, bits) if bits < 24 else rng.integers(0, 1 << 23, n, dtype=np.int64).astype(U32)
    idx = rng.permutation(n)
    nd = n // 4 if directed and bits == 24 else 0
    mant[idx[:nd]] = DIRECTED[np.arange(nd) % len(DIRECTED)]
    sign = rng.integers(0, 2, n, dtype=np.int64).astype(U32)
    eshape = [1] * len(shape)
    eshape[exp_axis] = shape[exp_axis]
    e = rng.integers(emin, emax + 1, eshape)
    eb = np.broadcast_to(e + 127, shape).reshape(n).astype(U32)
    u = (sign << 31) | (eb << 23) | mant
    if directed:
        nz = max(n // 64, 2)
        u[idx[nd:nd + nz]] = sign[idx[nd:nd + nz]] << 31  # +-0
    return u.view(F32).reshape(shape).copy(), e.reshape(-1)


def pow2(rng, n, jmax=3, bits=1):
    """n values +-s 2^j, |j| <= jmax, s a significand of `bits` significant bits"""
    j = rng.integers(-jmax, jmax + 1, n)
    sign = rng.integers(0, 2, n, dtype=np.int64).astype(U32)
    u = (sign << 31) | ((j + 127).astype(U32) << 23) | sig_bits(rng, n, bits)
    return u.view(F32).copy(), j


def bias_near(rng, e):
    """an fp32 bias per entry of e (the exponents of the products it meets, known to +-4): any 24-bit
    significand, exponent within 20 of e, so product + bias spans at most 50 bits: exact in fp64"""
    n = len(e)
    d = rng.integers(-20, 21, n)
    u = (rng.integers(0, 2, n, dtype=np.int64).astype(U32) << 31) | ((e + d + 127).astype(U32) << 23) | \
        rng.integers(0, 1 << 23, n, dtype=np.int64).astype(U32)
    return u.view(F32).copy()


def assert_exact_f32(p):
    """the finite entries of the fp64 array p are fp32 numbers"""
    fin = np.isfinite(p)
    with np.errstate(over="ignore", invalid="ignore"):
        back = p.astype(F32).astype(F64)
    assert np.array_equal(back[fin], p[fin]), "a product or sum is not representable in fp32"


def assert_sum_exact_f64(p, b):
    """p + b (fp64, broadcast) is exact: the error term of Knuth's TwoSum is zero"""
    with np.errstate(invalid="ignore"):
        s = p + b
        bb = s - p
        err = (p - (s - bb)) + (b - bb)
    fin = np.isfinite(s)
    assert not np.any(err[fin] != 0), "product + bias is not exact in fp64"


def round_once(p, b=None, relu=False):
    """the expected fp32 result of the fp64 sums p: + 0 (a zero sum is +0), + bias, one rounding"""
    with np.errstate(invalid="ignore", over="ignore"):
        y = p + 0.0
        if b is not None:
            assert_sum_exact_f64(y, np.asarray(b, dtype=F64))
            y = y + np.asarray(b, dtype=F64)
        if relu:
            y = np.where(y < 0, 0.0, y)  # NaN passes, as in the kernels and in torch
        return y.astype(F32)


@dataclass
class Case:
    name: str
    ops: dict            # operand name -> array
    want: np.ndarray     # fp32 expectation (non-finite where the dot product meets an inf / NaN)
    pre: np.ndarray = None  # fp64 sums before bias / ReLU
    meta: dict = field(default_factory=dict)


def put_nonfinite(a):
    """class E: one +inf and one NaN at known places of the pattern operand"""
    flat = a.reshape(a.shape[0], -1)
    flat[1 % a.shape[0], (flat.shape[1] * 2) // 3] = np.inf
    flat[a.shape[0] - 1 - (2 % a.shape[0]) if a.shape[0] > 2 else 0, flat.shape[1] // 5] = np.nan


# ------------------------------------------------------------------------------------------ FC
# y [M, N] = x [M, K] w [N, K]^T (+ b [N]); the backward's two products are the same with the
# roles renamed (test_exact_split_gpu.py), so every class is written once for "a [R, K] b [C, K]^T".

def chunk_bounds(K):
    """the k positions where a 32-deep chunk or a k split (chunks * s // S for the split counts the
    kernels use) begins"""
    chunks = K // 32
    out = set(32 * c for c in range(1, chunks))
    for S in (2, 3, 4, 5, 8, 16, 32):
        out |= set(32 * (chunks * s // S) for s in range(1, S))
    out.discard(0)
    return sorted(b for b in out if 0 < b < K)


def select_positions(rng, rows, K):
    """one reduction index per row: every index when rows >= K, else both sides of chunk / split
    boundaries, the ends, and random ones"""
    if rows >= K:
        return np.concatenate([rng.permutation(K), rng.integers(0, K, rows - K)])
    cand = [0, K - 1, 31 % K]
    for b in chunk_bounds(K):
        cand += [b - 1, b]
    cand = np.unique(np.array(cand))
    rng.shuffle(cand)
    take = cand[:rows // 2]
    rest = rng.choice(K, rows - len(take), replace=rows - len(take) > K)
    return rng.permutation(np.concatenate([take, rest]))


def product_select(rng, R, C, K, dense, pbits=24, qbits=1, bias=False, relu=False, nonfinite=False, name="",
                   given=None):
    """classes A / B / E for out [R, C] = a [R, K] b [C, K]^T: the `dense` operand ("a" or "b")
    holds patterns (exponent fixed along the other operand's output index, see pattern_values),
    the other one nonzero per row.  a's values have pbits significant bits, b's qbits.  The bias
    is per column of out."""
    if dense == "a":
        if given is not None:  # a pattern operand made elsewhere (its exponents unknown: no bias)
            assert given.shape == (R, K) and not bias
            a, e = np.ascontiguousarray(given, dtype=F32), np.zeros(K, dtype=np.int64)
        else:
            a, e = pattern_values(rng, (R, K), 1, bits=pbits, directed=pbits == 24)
        sel = select_positions(rng, C, K)
        sv, j = pow2(rng, C, bits=qbits)
        b = np.zeros((C, K), dtype=F32)
        b[np.arange(C), sel] = sv
        ecol = e[sel] + j
        if nonfinite:
            put_nonfinite(a)
    else:
        b, e = pattern_values(rng, (C, K), 0, bits=qbits, directed=qbits == 24)
        sel = select_positions(rng, R, K)
        sv, j = pow2(rng, R, bits=pbits)
        a = np.zeros((R, K), dtype=F32)
        a[np.arange(R), sel] = sv
        ecol = e
        if nonfinite:
            put_nonfinite(b)
    with np.errstate(invalid="ignore"):
        pre = a.astype(F64) @ b.astype(F64).T
    assert_exact_f32(pre)
    bv = bias_near(rng, ecol) if bias else None
    return Case(name, {"a": a, "b": b, "bias": bv}, round_once(pre, bv, relu), pre,
                {"relu": relu, "dense": dense, "sel": sel})


def assert_dense_bound(a, b, unit):
    """class C: sum_k |a_k b_k| <= 2^22 units for every output (finite entries)"""
    with np.errstate(invalid="ignore"):
        s = np.abs(np.nan_to_num(a.astype(F64), nan=0.0, posinf=0.0)) @ np.abs(np.nan_to_num(b.astype(F64), nan=0.0, posinf=0.0)).T
    assert s.max() <= 2.0 ** 22 * unit, (s.max() / unit, "exceeds 2^22 units")


def product_small_ints(rng, R, C, K, ua=-7, ub=5, amax=15, bmax=15, bias=False, relu=False, nonfinite=False, name=""):
    """class C, fully dense: a = integers in [-amax, amax] times 2^ua, b likewise times 2^ub"""
    a = (rng.integers(-amax, amax + 1, (R, K)) * 2.0 ** ua).astype(F32)
    b = (rng.integers(-bmax, bmax + 1, (C, K)) * 2.0 ** ub).astype(F32)
    unit = 2.0 ** (ua + ub)
    assert_dense_bound(a, b, unit)
    if nonfinite:
        put_nonfinite(a)
    with np.errstate(invalid="ignore"):
        pre = a.astype(F64) @ b.astype(F64).T
    assert_exact_f32(pre)
    bv = (rng.integers(-1000, 1001, C) * unit).astype(F32) if bias else None
    return Case(name, {"a": a, "b": b, "bias": bv}, round_once(pre, bv, relu), pre, {"relu": relu, "unit": unit})


def three_term_ints(rng, shape):
    """integers a 2^18 + b 2^9 + c with a in [-1, 1], b, c in [-255, 255] of mixed signs: |x| < 2^19,
    up to 19 + 8 significant bits -- all three bf16 terms are nonzero for most of them"""
    a = rng.integers(-1, 2, shape)
    b = rng.integers(-255, 256, shape)
    c = rng.integers(-255, 256, shape)
    return a * (1 << 18) + b * (1 << 9) + c


def straddling_rows(rng, rows, K, per_row=8):
    """a [rows, K] operand of 0 / +-1 with per_row nonzeros per row: pairs (b - 1, b) on both sides
    of chunk and k-split boundaries"""
    bounds = np.array(chunk_bounds(K)) if K > 32 else np.array([K // 2])
    s = np.zeros((rows, K), dtype=F64)
    for r in range(rows):
        bs = rng.choice(bounds, min(per_row // 2, len(bounds)), replace=False)
        pos = np.concatenate([bs - 1, bs])
        s[r, pos] = rng.choice([-1.0, 1.0], len(pos))
    assert (np.count_nonzero(s, axis=1) <= per_row).all()
    return s


def product_three_term(rng, R, C, K, dense, ua=-9, ub=3, name=""):
    """class C, second member: three-term integers in the `dense` operand against 0 / +-1 with at
    most 8 nonzeros per row of the other, on the chunk and split boundaries"""
    if dense == "a":
        a = (three_term_ints(rng, (R, K)) * 2.0 ** ua).astype(F32)
        b = (straddling_rows(rng, C, K) * 2.0 ** ub).astype(F32)
    else:
        b = (three_term_ints(rng, (C, K)) * 2.0 ** ub).astype(F32)
        a = (straddling_rows(rng, R, K) * 2.0 ** ua).astype(F32)
    unit = 2.0 ** (ua + ub)
    assert_dense_bound(a, b, unit)
    pre = a.astype(F64) @ b.astype(F64).T
    assert_exact_f32(pre)
    return Case(name, {"a": a, "b": b, "bias": None}, round_once(pre), pre, {"relu": False, "unit": unit, "dense": dense})


PQ = [(24, 1), (16, 8), (12, 12), (8, 16), (1, 24)]


def product_cases(seed, R, C, K, bias=True, classes="ABCE"):
    """the named cases of one product shape out [R, C] = a [R, K] b [C, K]^T"""
    rng = np.random.default_rng(seed)
    out = []
    if "A" in classes:
        out.append(product_select(rng, R, C, K, "a", bias=bias, relu=False, name="A/patterns-in-a"))
        out.append(product_select(rng, R, C, K, "b", pbits=1, qbits=24, bias=bias, relu=bias, name="A/patterns-in-b"))
    if "B" in classes:
        for p, q in PQ:
            out.append(product_select(rng, R, C, K, "a" if p >= q else "b", pbits=p, qbits=q, name=f"B/{p}x{q}"))
    if "C" in classes:
        out.append(product_small_ints(rng, R, C, K, bias=bias, relu=bias, name="C/small-ints"))
        out.append(product_three_term(rng, R, C, K, "a", name="C/three-term-in-a"))
        out.append(product_three_term(rng, R, C, K, "b", name="C/three-term-in-b"))
    if "E" in classes:
        out.append(product_select(rng, R, C, K, "a", bias=bias, nonfinite=True, name="E/A-patterns-in-a"))
        out.append(product_select(rng, R, C, K, "b", pbits=1, qbits=24, bias=bias, nonfinite=True, name="E/A-patterns-in-b"))
        out.append(product_small_ints(rng, R, C, K, bias=bias, nonfinite=True, name="E/C-small-ints"))
    return out


def exponent_sweep(M=64, N=128, K=128):
    """class A on (64, 128, 128) over the whole exponent range: x[m][k] is a 24-bit pattern whose
    exponent walks E = -126 .. 127, then six fp32 subnormals (listed as -127), along the flattened
    index m K + k -- every exponent is met about 31 times -- and w selects column n with +1:
    y[m][n] = x[m][n].  Returns (x, w, want, exps), exps[m][n] the exponent behind output (m, n)."""
    rng = np.random.default_rng(4)
    E = np.concatenate([np.arange(-126, 128), np.full(6, -127)])
    idx = (np.arange(M)[:, None] * K + np.arange(K)[None, :]) % len(E)
    exps = E[idx]
    mant = rng.integers(0, 1 << 23, (M, K), dtype=np.int64)
    mant[:, ::3] = DIRECTED[(np.arange(M)[:, None] + np.arange(0, K, 3)[None, :]) % len(DIRECTED)]
    mant[exps == -127] |= 1  # subnormals: nonzero
    mant[exps == 127] &= 0x3fffff  # below (2 - 2^-8) 2^127, where the first bf16 term rounds to infinity
    sign = rng.integers(0, 2, (M, K), dtype=np.int64)
    u = (sign << 31) | ((exps + 127) << 23) | mant
    x = u.astype(U32).view(F32).copy()
    w = np.zeros((N, K), dtype=F32)
    w[np.arange(N), np.arange(N) % K] = 1.0
    want = x[:, np.arange(N) % K].copy()
    return x, w, want, exps[:, np.arange(N) % K]


# ---------------------------------------------------------------------------------------- conv
GEOMS = [(4, 84, 84, 32, 8, 4), (32, 20, 20, 64, 4, 2), (64, 9, 9, 64, 3, 1)]  # conv1, conv2, conv3


def _t(a, dtype=None):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype or torch.float64)


def _lattice_x(rng, geom, n, values):
    """x [n, cin, h, w] zero but for one channel of the pixels of a lattice of spacing k (offset
    and channel vary by sample and pixel): every k x k window holds exactly one nonzero.  values(m)
    -> m nonzero numbers."""
    cin, h, w, cout, k, s = geom
    x = np.zeros((n, cin, h, w), dtype=F64)
    for b in range(n):
        oy, ox = int(rng.integers(0, k)), int(rng.integers(0, k))
        ys, xs = np.arange(oy, h, k), np.arange(ox, w, k)
        yy, xx = np.meshgrid(ys, xs, indexing="ij")
        ci = rng.integers(0, cin, yy.shape)
        x[b, ci, yy, xx] = values(yy.size).reshape(yy.shape)
    return x


def conv_fwd(seed, geom, n, kind, negate=False, nonfinite=False):
    """forward cases, want = relu(conv2d(x, w) + b) [n, cout, ho, wo].  kind:
    "A/w"   lattice of +-2^j in x, patterns in w          "A/x"  patterns in x, one tap per co in w
    "B/pxq" lattice x with p bits against w with q bits   "C"    small integers, dense
    "C3"    three-term integers in x, w 0 / +-1 with 8 nonzeros per co around ci = 31 | 32, 63 | 0
    uint8 (geom conv1, x returned as uint8): "D/sel" lattice of bytes 2^j against 24-bit weights,
    "D/16"  lattice of any byte (255 included) against 16-bit weights, "D/C" dense bytes, small
    integer weights.  negate: w -> -w (the ReLU hides the negative half of one run)."""
    import torch.nn.functional as Fn

    rng = np.random.default_rng(seed)
    cin, h, wd, cout, k, s = geom
    u8 = kind.startswith("D")
    bias = None
    if kind in ("A/w", "D/sel", "D/16") or kind.startswith("B/"):
        p, q = (1, 24)
        if kind.startswith("B/"):
            p, q = (int(v) for v in kind[2:].split("x"))
        if kind == "D/sel":
            x = _lattice_x(rng, geom, n, lambda m: 2.0 ** rng.integers(0, 8, m))
        elif kind == "D/16":
            x = _lattice_x(rng, geom, n, lambda m: np.where(rng.random(m) < 0.2, 255, rng.integers(1, 256, m)).astype(F64))
            q = 16
        else:
            x = _lattice_x(rng, geom, n, lambda m: pow2(rng, m, bits=p)[0].astype(F64))
        w, e = pattern_values(rng, (cout, cin, k, k), 0, bits=q, directed=q == 24)
        if nonfinite:
            put_nonfinite(w)
        if not kind.startswith("B/"):
            bias = bias_near(rng, e + (4 if u8 else 0))
    elif kind == "A/x":
        x, e = pattern_values(rng, (n, cin, h, wd), 1)
        x = x.astype(F64)
        w = np.zeros((cout, cin, k, k), dtype=F32)
        ci, kh, kw = rng.integers(0, cin, cout), rng.integers(0, k, cout), rng.integers(0, k, cout)
        sv, j = pow2(rng, cout)
        w[np.arange(cout), ci, kh, kw] = sv
        bias = bias_near(rng, e[ci] + j)
        if nonfinite:
            put_nonfinite(x)
    elif kind in ("C", "D/C"):
        x = rng.integers(0, 256, (n, cin, h, wd)).astype(F64) if u8 else rng.integers(-15, 16, (n, cin, h, wd)) * 2.0 ** -6
        w = (rng.integers(-15, 16, (cout, cin, k, k)) * 2.0 ** 4).astype(F32)
        unit = 2.0 ** 4 if u8 else 2.0 ** -2
        assert cin * k * k * (255 if u8 else 15 * 2.0 ** -6) * 15 * 2.0 ** 4 <= 2.0 ** 22 * unit
        bias = (rng.integers(-1000, 1001, cout) * unit).astype(F32)
        if nonfinite:
            put_nonfinite(w if u8 else x)
    elif kind == "C3":
        x = three_term_ints(rng, (n, cin, h, wd)) * 2.0 ** -9
        w = np.zeros((cout, cin, k, k), dtype=F32)
        for co in range(cout):
            for t in rng.choice(k * k - 1, 2, replace=False):  # taps t and t + 1: ci 31 | 32 and 63 | 0 (cin = 64)
                for tap, c in ((t, cin // 2 - 1), (t, cin // 2), (t, cin - 1), (t + 1, 0)):
                    w[co, c, tap // k, tap % k] = rng.choice([-8.0, 8.0])
        assert 8 * 2.0 ** 19 <= 2.0 ** 22
    else:
        raise ValueError(kind)
    if negate:
        w = -w
    with np.errstate(invalid="ignore"):
        pre = Fn.conv2d(_t(x), _t(w), None, stride=s).numpy()
    assert_exact_f32(pre)
    b = None if bias is None else bias.astype(F64)[None, :, None, None]
    if b is None:
        bias = np.zeros(cout, dtype=F32)  # the forward entry point wants a bias
    want = round_once(pre, b, relu=True)
    xo = x.astype(np.uint8) if u8 else x.astype(F32)
    assert np.array_equal(np.nan_to_num(xo.astype(F64)), np.nan_to_num(x))
    return Case(kind, {"x": xo, "w": w, "bias": bias}, want, pre, {"relu": True})


def conv_dgrad(seed, geom, n, kind):
    """data-gradient cases, want = gx [n, cin, h, w] of gy [n, cout, ho, wo] and w.  kind:
    "A/w"  gy nonzero (one co each) on a lattice of spacing ceil(k / s): every input pixel lies in
           at most one nonzero window; patterns in w (uncovered pixels come back +0)
    "A/gy" patterns in gy; for every ci one nonzero (co, kh, kw) of w
    "B/pxq" as A/w with p bits in gy, q in w          "C" small integers, dense"""
    import torch

    rng = np.random.default_rng(seed)
    cin, h, wd, cout, k, s = geom
    ho, wo = (h - k) // s + 1, (wd - k) // s + 1
    if kind == "A/w" or kind.startswith("B/"):
        p, q = (1, 24) if kind == "A/w" else (int(v) for v in kind[2:].split("x"))
        d = -(-k // s)
        gy = np.zeros((n, cout, ho, wo), dtype=F64)
        for b in range(n):
            ys, xs = np.arange(int(rng.integers(0, d)), ho, d), np.arange(int(rng.integers(0, d)), wo, d)
            yy, xx = np.meshgrid(ys, xs, indexing="ij")
            gy[b, rng.integers(0, cout, yy.shape), yy, xx] = pow2(rng, yy.size, bits=p)[0].reshape(yy.shape)
        w, _ = pattern_values(rng, (cout, cin, k, k), 0, bits=q, directed=q == 24)
    elif kind == "A/gy":
        gy, _ = pattern_values(rng, (n, cout, ho, wo), 1)
        gy = gy.astype(F64)
        w = np.zeros((cout, cin, k, k), dtype=F32)
        w[rng.integers(0, cout, cin), np.arange(cin), rng.integers(0, k, cin), rng.integers(0, k, cin)] = pow2(rng, cin)[0]
    elif kind == "C":
        gy = rng.integers(-15, 16, (n, cout, ho, wo)) * 2.0 ** -6
        w = (rng.integers(-15, 16, (cout, cin, k, k)) * 2.0 ** 4).astype(F32)
        assert cout * k * k * 225 <= 2 ** 22
    else:
        raise ValueError(kind)
    pre = torch.nn.grad.conv2d_input((n, cin, h, wd), _t(w), _t(gy), stride=s).numpy()
    assert_exact_f32(pre)
    return Case(kind, {"gy": gy.astype(F32), "w": w}, round_once(pre), pre)


def conv_wgrad(seed, geom, n, kind, first=False, u8=False):
    """weight-gradient cases, want = gw [cout, cin, k, k] = sum over samples and output pixels of
    gy x.  Single-pixel kinds ("A", "B/pxq", and on bytes "D/sel", "D/16"): exactly one output
    pixel of one sample has a gradient -- every co, all different +-2^j (or q-bit values; on bytes
    24- / 16-bit values) -- while every other sample's x is random against a zero gradient.  The
    pixel: the last one of the last sample, or (first) pixel 0 of sample 0.  "C" / "D/C": small
    integers, dense, the gradient's range cut so that the bound holds."""
    import torch

    rng = np.random.default_rng(seed)
    cin, h, wd, cout, k, s = geom
    ho, wo = (h - k) // s + 1, (wd - k) // s + 1
    gy = np.zeros((n, cout, ho, wo), dtype=F64)
    b0, oy, ox = (0, 0, 0) if first else (n - 1, ho - 1, wo - 1)
    if kind in ("C", "D/C"):
        xmax = 255 if u8 else 15
        gmax = min(15, int(2 ** 22 // (n * ho * wo * xmax)))
        assert gmax >= 1 and n * ho * wo * xmax * gmax <= 2 ** 22
        x = rng.integers(0 if u8 else -15, xmax + 1, (n, cin, h, wd)).astype(F64)
        gy = rng.integers(-gmax, gmax + 1, (n, cout, ho, wo)) * 2.0 ** -5
        if u8:
            gy[rng.random(gy.shape) < 0.4] = 0  # the ReLU mask's zeros
    else:
        if u8:
            x = rng.integers(0, 256, (n, cin, h, wd)).astype(F64)
            win = (b0, slice(None), slice(oy * s, oy * s + k), slice(ox * s, ox * s + k))
            if kind == "D/sel":
                x[win] = 2.0 ** rng.integers(0, 8, (cin, k, k))
            else:
                x[win][rng.random((cin, k, k)) < 0.2] = 255
            g, _ = pattern_values(rng, (cout,), 0, bits=24 if kind == "D/sel" else 16, directed=False)
        else:
            p, q = (24, 1) if kind == "A" else (int(v) for v in kind[2:].split("x"))
            x, _ = pattern_values(rng, (n, cin, h, wd), 1, bits=p, directed=p == 24)
            x = x.astype(F64)
            if q == 1:  # all different: 32 exponents x 2 signs
                order = rng.permutation(64)[:cout]
                g = ((-1.0) ** (order & 1)) * 2.0 ** ((order >> 1) - 16)
            else:
                g = pow2(rng, cout, bits=q)[0]
        gy[b0, :, oy, ox] = g
    zw = torch.zeros((cout, cin, k, k), dtype=torch.float64)
    _, pre, _ = torch.ops.aten.convolution_backward(_t(gy), _t(x), zw, None, [s, s], [0, 0], [1, 1], False, [0, 0], 1,
                                                    [False, True, False])
    pre = pre.numpy()
    assert_exact_f32(pre)
    gb = gy.sum(axis=(0, 2, 3))
    assert_exact_f32(gb)
    return Case(kind, {"x": x.astype(np.uint8) if u8 else x.astype(F32), "gy": gy.astype(F32)}, round_once(pre), pre,
                {"gb": round_once(gb)})


# ------------------------------------------------------------------- the shapes the tests use
FC_X9_64 = [(64, 128, 32), (64, 128, 96), (192, 128, 3136)]     # k_fc_x9: M % 128 != 0
FC_X9_128 = [(128, 128, 32), (128, 256, 96), (512, 512, 3136)]  # k_fc_x9t
FC_F32 = [(1, 128, 32), (259, 128, 96), (512, 512, 3136)]       # k_fc_f32, the control
FC_ALL_PATTERNS = (1024, 128, 128)  # class A with every one of the 131,072 pattern values observed
FC_BWD = [(64, 128, 64), (128, 128, 64), (64, 512, 3136), (192, 256, 192)]  # (B, N, K)
CONV_FWD = {  # geometry index -> (sample counts, kinds, kinds with an inf and a NaN)
    2: ((1, 3, 5), ("A/w", "A/x", "B/12x12", "B/16x8", "B/8x16", "C", "C3"), ("A/w", "A/x", "C")),
    1: ((1, 3), ("A/w", "A/x", "B/12x12", "C", "C3"), ("A/w", "C")),
    0: ((1, 5), ("D/sel", "D/16", "D/C"), ("D/sel", "D/C")),
}
CONV_DGRAD_KINDS = ("A/w", "A/gy", "B/12x12", "B/16x8", "B/8x16", "C")
CONV_WGRAD_KINDS = ("A", "B/12x12", "B/16x8", "B/8x16", "B/1x24", "C")
