"""The order-free inputs of _exact_inputs.py, proven without a GPU.

Representability: for every class and shape test_exact_split_gpu.py uses, the sums before the bias
are fp32 numbers and the class C bound holds (the generators assert both), and torch's own fp32 CPU
product / convolution of the same operands returns the expectation bit for bit -- the inputs are
order-free for a reference that knows nothing of the split.

Discriminating power: a numpy model of the kernels' arithmetic -- the three-term round-to-nearest-
even split (common.hpp's bf16_rne_bits restated), nine partial products per k added in fp32, per
32-deep chunk, in the kernels' smallest-first pair order or in a shuffled one -- equals the
expectation bit for bit on every class, and stops doing so on the classes meant to cover it when
one term pair is removed, when two k positions of one term are swapped inside a chunk, or when the
truncation split of conv1's weight gradient loses its low term.

Known limit: the pairs (2,3), (3,2) and (3,3) cannot be reached.  An order-free input needs
p + q <= 24 significant bits per product (or one factor a power of two), so a second or third term
never meets a third one; the model without these pairs equals the full model on every class
(asserted below).  Their products lie below half an ulp of a single exact product: no exactness
test can see them, only the accuracy bounds of test_fc_gpu.py and test_conv_gpu.py do."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import _exact_inputs as X

F32, U32 = np.float32, np.uint32


def same_bits(got, want):
    """bit equality where want is finite (the sign of zero included), non-finite where it is not"""
    got, want = np.ascontiguousarray(got, dtype=F32), np.ascontiguousarray(want, dtype=F32)
    fin = np.isfinite(want)
    return bool(np.array_equal(got.view(U32)[fin], want.view(U32)[fin]) and not np.isfinite(got[~fin]).any())


# ---------------------------------------------------------------- representability, reference alone
ALL_FC = sorted(set(X.FC_X9_64 + X.FC_X9_128 + X.FC_F32 + [X.FC_ALL_PATTERNS]))


@pytest.mark.parametrize("shape", ALL_FC)
def test_fc_inputs_order_free_for_torch_fp32(shape):
    M, N, K = shape
    for c in X.product_cases(M + N + K, M, N, K, classes="A" if shape == X.FC_ALL_PATTERNS else "ABCE"):
        a, b, bias = (None if v is None else torch.from_numpy(v) for v in (c.ops["a"], c.ops["b"], c.ops["bias"]))
        y = a @ b.t()
        y = y + 0.0 if bias is None else y + bias
        y = torch.where(y < 0, torch.zeros(()), y) if c.meta["relu"] else y
        assert same_bits(y.numpy(), c.want), (shape, c.name)
        if c.name.startswith("E/"):
            bad = ~np.isfinite(c.want)
            assert 0 < bad.sum() <= 2 * max(M, N), (shape, c.name)  # contained: at most a row or column each


@pytest.mark.parametrize("B,N,K", X.FC_BWD)
def test_fc_bwd_inputs_order_free(B, N, K):
    """the backward's two products, gx = gy w (summed over n) and gw = gy^T x (over the batch row)"""
    for R, C, red in ((B, K, N), (N, K, B)):
        for c in X.product_cases(B + N + K, R, C, red, bias=False, classes="ABC"):
            y = torch.from_numpy(c.ops["a"]) @ torch.from_numpy(c.ops["b"]).t() + 0.0
            assert same_bits(y.numpy(), c.want), ((R, C, red), c.name)


@pytest.mark.parametrize("gi", [0, 1, 2])
def test_conv_fwd_inputs_order_free(gi):
    ns, kinds, ekinds = X.CONV_FWD[gi]
    geom = X.GEOMS[gi]
    for n in ns:
        for kind, nf in [(k, False) for k in kinds] + [(k, True) for k in ekinds]:
            for neg in (False, True):
                c = X.conv_fwd(100 * gi + n, geom, n, kind, negate=neg, nonfinite=nf)
                y = Fn.conv2d(torch.from_numpy(c.ops["x"]).float(), torch.from_numpy(c.ops["w"]), None, stride=geom[5])
                y = y + 0.0 + torch.from_numpy(c.ops["bias"])[None, :, None, None]
                y = torch.where(y < 0, torch.zeros(()), y)
                assert same_bits(y.numpy(), c.want), (gi, n, kind, nf, neg)


@pytest.mark.parametrize("gi", [1, 2])
def test_conv_grad_inputs_order_free(gi):
    geom = X.GEOMS[gi]
    cin, h, wd, cout, k, s = geom
    for n in (1, 3):
        for kind in X.CONV_DGRAD_KINDS:
            c = X.conv_dgrad(n, geom, n, kind)
            y = torch.nn.grad.conv2d_input((n, cin, h, wd), torch.from_numpy(c.ops["w"]), torch.from_numpy(c.ops["gy"]),
                                           stride=s) + 0.0
            assert same_bits(y.numpy(), c.want), (gi, n, kind)
            if kind == "A/w":
                assert (c.want == 0).any()  # uncovered pixels: expected +0
        for kind in X.CONV_WGRAD_KINDS:
            for first in (False, True):
                c = X.conv_wgrad(n, geom, n, kind, first=first)
                y = torch.nn.grad.conv2d_weight(torch.from_numpy(c.ops["x"]), (cout, cin, k, k),
                                                torch.from_numpy(c.ops["gy"]), stride=s) + 0.0
                assert same_bits(y.numpy(), c.want), (gi, n, kind, first)


def test_conv1_wgrad_u8_inputs_hold_their_bound():
    for n in (1, 7):
        for kind in ("D/sel", "D/16", "D/C"):
            c = X.conv_wgrad(n, X.GEOMS[0], n, kind, u8=True)  # the generator asserts exactness and the bound
            assert c.want.shape == (32, 4, 8, 8) and np.isfinite(c.want).all()


def test_exponent_sweep_covers_the_range():
    x, w, want, exps = X.exponent_sweep()
    assert set(range(-126, 128)) <= set(exps.reshape(-1).tolist()) and (exps == -127).any()
    assert same_bits(torch.from_numpy(x) @ torch.from_numpy(w).t(), want)


# ------------------------------------------------------------------------ the kernels' arithmetic
def rne_split(v):
    """v = t[0] + t[1] + t[2], each term the bf16 nearest (ties to even) to what is left"""
    out, r = [], np.ascontiguousarray(v, dtype=F32).copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for _ in range(3):
            u = r.view(U32).astype(np.uint64)
            u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16 << 16) & 0xffffffff
            h = u.astype(U32).view(F32)
            out.append(h)
            r = r - h  # exact: h is r's nearest bf16
    return out


def trunc_split(v):
    """conv.hip's split3_trunc: the high 16 bits, twice, then the rest"""
    v = np.ascontiguousarray(v, dtype=F32)
    t0 = (v.view(U32) & U32(0xffff0000)).view(F32)
    r1 = v - t0
    t1 = (r1.view(U32) & U32(0xffff0000)).view(F32)
    return [t0, t1, r1 - t1]


def one_term(v):
    z = np.zeros_like(v, dtype=F32)
    return [np.ascontiguousarray(v, dtype=F32), z, z]


SMALLEST_FIRST = [(2, 2), (2, 1), (1, 2), (2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)]  # fc_ta / fc_tb, 0-based


def model(a, b, pairs=SMALLEST_FIRST, shuffle=None, shuffle_pairs=False, split_a=rne_split, split_b=rne_split,
          mutate=None):
    """out [R, C] = a [R, K] b [C, K]^T as the kernels add it: per 32-deep chunk, per term pair, per
    k, one exact partial product added to an fp32 accumulator.  shuffle: a Generator that permutes
    the chunks and the k positions of every chunk (and, with shuffle_pairs, the pairs too)"""
    at, bt = split_a(a), split_b(b)
    if mutate:
        mutate(at, bt)
    K = a.shape[1]
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        starts = np.arange(0, K, 32)
        for c0 in (starts if shuffle is None else shuffle.permutation(starts)):
            ks, ps = np.arange(c0, min(c0 + 32, K)), list(pairs)
            if shuffle is not None:
                ks = shuffle.permutation(ks)
                if shuffle_pairs:
                    ps = [ps[i] for i in shuffle.permutation(len(ps))]
            for i, j in ps:
                for k in ks:
                    acc = acc + at[i][:, k, None] * bt[j][None, :, k]
    return acc


def finish(acc, c):
    y = acc if c.ops["bias"] is None else acc + c.ops["bias"][None, :]
    return np.where(y < 0, F32(0), y) if c.meta["relu"] else y


def test_split_is_exact_and_has_eight_bit_terms():
    v, _ = X.pattern_values(np.random.default_rng(0), (4096,), 0)
    for split in (rne_split, trunc_split):
        t = split(v)
        assert np.array_equal((t[0].astype(np.float64) + t[1] + t[2]).astype(F32).view(U32)[v != 0], v.view(U32)[v != 0])
        assert all(not (x.view(U32) & 0xffff).any() for x in t)  # every term is a bf16
    assert (rne_split(v)[1] * v < 0).any()  # a negative second term (the first rounded up)


MODEL_SHAPE = (64, 128, 96)  # three chunks; N >= K, so the selection reaches every k


@pytest.fixture(scope="module")
def cases():
    return X.product_cases(11, *MODEL_SHAPE)


def test_model_equals_expectation_in_both_orders(cases):
    """the kernels' order, and the chunks and the k positions of every chunk shuffled: bit-equal on
    every class.  The nine pairs shuffled as well: bit-equal on class C, whose every partial sum is
    an integer below 2^24 units"""
    for c in cases:
        assert same_bits(finish(model(c.ops["a"], c.ops["b"]), c), c.want), c.name
        assert same_bits(finish(model(c.ops["a"], c.ops["b"], shuffle=np.random.default_rng(5)), c), c.want), c.name
        if "C" in c.name:
            got = model(c.ops["a"], c.ops["b"], shuffle=np.random.default_rng(6), shuffle_pairs=True)
            assert same_bits(finish(got, c), c.want), c.name


def test_the_pair_order_is_part_of_the_claim(cases):
    """one product v 2^j is t3 + t2 + t1 in the accumulator.  Smallest first, every partial sum is a
    residual of the split (v - t1, then v): exact.  (Largest first, t1 + t2 = v - t3, is exact too.)
    An order that is not monotone is not: with the leading pair first and the rest ascending,
    t1 + t3 needs 25 bits whenever t1 was rounded up into the next binade.  So class A pins the
    order of the MFMA chain as well; class C, whose partial sums are all small integers, does not"""
    order = [SMALLEST_FIRST[-1]] + SMALLEST_FIRST[:-1]
    seen = [c.name for c in cases if not same_bits(finish(model(c.ops["a"], c.ops["b"], pairs=order), c), c.want)]
    assert {"A/patterns-in-a", "E/A-patterns-in-b"} <= set(seen), seen  # (E/A: class A with no ReLU over it)
    assert not [n for n in seen if "C" in n], seen
    for c in cases:
        assert same_bits(finish(model(c.ops["a"], c.ops["b"], pairs=SMALLEST_FIRST[::-1]), c), c.want), c.name


# a removed pair (A term, B term), 1-based as in the kernels' comments -> the classes meant to see it
COVER = {
    (1, 2): ["A/patterns-in-b", "B/12x12", "B/8x16"],
    (2, 1): ["A/patterns-in-a", "B/12x12", "B/16x8"],
    (1, 3): ["A/patterns-in-b", "B/1x24"],
    (3, 1): ["A/patterns-in-a", "B/24x1"],
    (2, 2): ["B/12x12"],
}


@pytest.mark.parametrize("pair", sorted(COVER))
def test_a_lost_term_pair_is_seen(cases, pair):
    left = [p for p in SMALLEST_FIRST if p != (pair[0] - 1, pair[1] - 1)]
    seen = [c.name for c in cases if not same_bits(finish(model(c.ops["a"], c.ops["b"], pairs=left), c), c.want)]
    assert set(COVER[pair]) <= set(seen), (pair, seen)


@pytest.mark.parametrize("pair", [(2, 3), (3, 2), (3, 3)])
def test_the_pairs_no_class_reaches(cases, pair):
    """the known limit of the docstring: without one of these pairs the model is unchanged"""
    left = [p for p in SMALLEST_FIRST if p != (pair[0] - 1, pair[1] - 1)]
    for c in cases:
        assert same_bits(finish(model(c.ops["a"], c.ops["b"], pairs=left), c), c.want), (pair, c.name)


def test_swapped_k_positions_of_one_term_are_seen(cases):
    """a's third terms at the first and the last k of every chunk change places -- wrong only where
    the third terms differ"""
    def swap(at, bt):
        t = at[2].copy()
        t[:, 0::32], t[:, 31::32] = at[2][:, 31::32], at[2][:, 0::32]
        at[2] = t

    seen = [c.name for c in cases if not same_bits(finish(model(c.ops["a"], c.ops["b"], mutate=swap), c), c.want)]
    assert "A/patterns-in-a" in seen and "C/three-term-in-a" in seen, seen


def _conv1_wgrad_as_product(c):
    """n = 1: gw [32, 256] = g [32, 400] cols [256, 400]^T (im2col, reduction over the 400 pixels)"""
    cols = Fn.unfold(torch.from_numpy(c.ops["x"]).float(), 8, stride=4)[0].numpy()  # [(ci, kh, kw), pixel]
    return c.ops["gy"][0].reshape(32, 400), cols, c.want.reshape(32, 256)


@pytest.mark.parametrize("kind", ["D/sel", "D/16", "D/C"])
def test_truncation_split_model_and_its_lost_low_term(kind):
    """conv1's weight gradient: the gradient split by truncation, the bytes exact in one bf16"""
    g, cols, want = _conv1_wgrad_as_product(X.conv_wgrad(1, X.GEOMS[0], 1, kind, u8=True))
    pairs = [(2, 0), (1, 0), (0, 0)]
    assert same_bits(model(g, cols, pairs=pairs, split_a=trunc_split, split_b=one_term), want)
    assert same_bits(model(g, cols, pairs=pairs, split_a=trunc_split, split_b=one_term, shuffle=np.random.default_rng(2)), want)
    lost = same_bits(model(g, cols, pairs=pairs[1:], split_a=trunc_split, split_b=one_term), want)
    assert lost == (kind != "D/sel")  # only the 24-bit gradient has a low term to lose
