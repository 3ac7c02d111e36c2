"""The exact area average behind the Atari preprocessing (helper of test_area_exact_cpu.py and
test_atari_edges_gpu.py; plain numpy in int64, no import of the library and none of the oracle's
area_tab / warp_frame / rgb2gray).

What is checked.  reth_amd/csrc/atari.hip and oracle.warp_frame both restate OpenCV's 8-bit
algorithms -- MaxAndSkip's max of two frames, the fixed-point RGB2GRAY and the general INTER_AREA
resize -- and both build their taps with the same few lines (computeResizeAreaTab), so comparing
one with the other cannot see a slip that is in both.  exact_warp says what the resize has to be
without any table: an output pixel is the area average of the gray source pixels its cell covers.
Input and output sizes are integers, so along one axis the overlap of source pixel s ([s, s + 1)
source pixels) and destination cell d ([d S / D, (d + 1) S / D)) is, in units of 1 / D source pixels,
the integer

    O[d, s] = max(0, min((d + 1) S, (s + 1) D) - max(d S, s D)),        sum_s O[d, s] = S,

and the area average of the gray image is num / den with num = Oy @ gray @ Ox^T and den = H W, an
exact integer quotient (num <= 255 H W, far inside int64).  Rounding half to even (OpenCV's
saturate_cast<uchar> is cvRound) is decided in integers too.

OpenCV itself is not installed where this suite runs, and no recorded OpenCV output is used: the
exact area average stands in for it.  What stays untested against real OpenCV is only which
neighbour it picks inside the band below.

BAND, derived and not measured.  An fp32 implementation with at most kMaxTaps = 8 taps per axis
computes sum_y beta_y (sum_x S alpha_x): per row 8 multiplies and 8 adds, then 8 multiplies and 8
adds over the rows, every one rounded once, every partial sum at most 255 (the weights are
positive and sum to 1); the fp32 weights themselves carry one rounding each (alpha, beta), which
adds two more relative roundings per product.  Along one path from a source pixel to the result
that is at most 8 + 8 additions, 2 multiplies and 2 weight roundings: 20 roundings of relative size
2^-24 on magnitudes <= 255, so |fp32 result - num / den| <= 20 * 255 * 2^-24 ~= 3.1e-4.  (The taps
OpenCV's table drops -- overlaps below 1e-3 source pixels -- do not occur: a nonzero overlap is at
least 1 / D >= 1 / 500 source pixels at every shape here.)  BAND = 1e-3 is about 3 x that bound.
A result further than BAND from a rounding tie must therefore round like the exact value; inside
the band either neighbour is accepted, and no pixel may ever be further than 0.5 + BAND from the
exact value.
"""
import numpy as np

BAND = 1e-3

# (in (H, W), out (oh, ow)): what the shape reaches in k_atari_step / area_tab
SHAPES = [
    ((210, 160), (84, 84)),    # the workload's own shape (used once, here)
    ((17, 13), (5, 4)),        # scales 3.4 / 3.25: 5 and 4 taps
    ((9, 130), (4, 65)),       # x scale exactly 2, y not an integer: the general path with an integer axis
    ((11, 70), (11, 65)),      # y scale exactly 1: one tap
    ((30, 300), (13, 129)),    # OW = 129: 192 threads, three waves, 63 idle lanes
    ((23, 19), (22, 3)),       # scale 1.045: nearly every cell straddles two rows
    ((40, 1030), (7, 500)),    # wide: 512 threads, 7 taps in y
    ((8, 8), (3, 5)),          # tiny
    ((5, 3), (1, 2)),          # one output row
    ((64, 100), (9, 15)),      # exactly 8 taps on both axes, the kMaxTaps limit
]
WORKLOAD = SHAPES[0]
SMALL = SHAPES[1]  # the shape of the ring / env-step tests

KINDS = ["random", "ramp", "flat255", "checker", "redgreen"]
SEED = 20240531


def shape_id(shape):
    (H, W), (oh, ow) = shape
    return f"{H}x{W}-{oh}x{ow}"


def make_pair(kind, H, W, j=0, seed=SEED):
    """frame pair j of an input kind: two uint8 [H, W, 3] frames
    random    uniform bytes, the two frames independent (seeded by the shape and j)
    ramp      a column ramp (x + 37 j) mod 256 in every channel of both frames
    flat255   255 everywhere: the result is 255 everywhere (weights sum to 1, the clamp holds)
    checker   a 0 / 255 checkerboard with cells of j + 1 pixels, both frames alike
    redgreen  one frame pure red, the other pure green (j odd: swapped): the max is per channel"""
    if kind == "random":
        rng = np.random.default_rng([seed, H, W, j])
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    f0 = np.zeros((H, W, 3), np.uint8)
    if kind == "ramp":
        f0[:] = ((np.arange(W) + 37 * j) % 256).astype(np.uint8)[None, :, None]
        return f0, f0.copy()
    if kind == "flat255":
        f0[:] = 255
        return f0, f0.copy()
    if kind == "checker":
        c = j + 1
        f0[:] = ((((np.arange(H)[:, None] // c) + (np.arange(W)[None, :] // c)) & 1) * 255).astype(np.uint8)[..., None]
        return f0, f0.copy()
    if kind == "redgreen":
        f1 = np.zeros((H, W, 3), np.uint8)
        f0[..., 0], f1[..., 1] = 255, 255
        return (f1, f0) if j & 1 else (f0, f1)
    raise ValueError(kind)


REDGREEN_GRAY = 226  # (255 * 4899 + 255 * 9617 + 8192) >> 14: red and green both present


def overlap(S, D):
    """int64 [D, S]: the overlap of destination cell d and source pixel s, in 1 / D source pixels"""
    d = np.arange(D, dtype=np.int64)[:, None]
    s = np.arange(S, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((d + 1) * S, (s + 1) * D) - np.maximum(d * S, s * D))


def gray_max(f0, f1):
    """int64 [H, W]: the per-channel max of the two frames, then (R 4899 + G 9617 + B 1868 + 8192) >> 14"""
    c = np.maximum(np.asarray(f0), np.asarray(f1)).astype(np.int64)
    return (c[..., 0] * 4899 + c[..., 1] * 9617 + c[..., 2] * 1868 + 8192) >> 14


def exact_from_gray(gray, oh, ow):
    gray = np.asarray(gray, dtype=np.int64)
    H, W = gray.shape
    num = overlap(H, oh) @ gray @ overlap(W, ow).T
    den = H * W
    q, r = np.divmod(num, den)
    up = (2 * r > den) | ((2 * r == den) & ((q & 1) == 1))  # half goes to the even neighbour
    rounded = q + up
    dist = np.abs(2 * r - den).astype(np.float64) / (2.0 * den)
    value = num.astype(np.float64) / den
    return rounded, dist, value


def exact_warp(f0, f1, oh, ow):
    """(rounded int64 [oh, ow], dist float64, value float64): the area average num / den of the
    gray image of max(f0, f1) rounded half to even, |frac(num / den) - 1/2|, and num / den in fp64"""
    return exact_from_gray(gray_max(f0, f1), oh, ow)


def check_warp(out, f0, f1):
    """a uint8 [oh, ow] result of either implementation against the exact area average:
    (a) |out - value| <= 0.5 + BAND at every pixel, none exempt
    (b) out == rounded wherever dist >= BAND
    returns (pixels that differ from rounded, the largest dist among them or 0.0)"""
    out = np.asarray(out)
    assert out.dtype == np.uint8 and out.ndim == 2, (out.dtype, out.shape)
    rounded, dist, value = exact_warp(f0, f1, *out.shape)
    err = np.abs(out.astype(np.float64) - value)
    assert np.all(err <= 0.5 + BAND), f"max |out - exact| = {err.max()} at {np.unravel_index(err.argmax(), err.shape)}"
    bad = out.astype(np.int64) != rounded
    off = bad & (dist >= BAND)
    assert not off.any(), (f"{int(off.sum())} pixels outside the band differ from the exactly rounded value, first at "
                           f"{tuple(np.argwhere(off)[0])}: got {out[off][0]}, exact {value[off][0]}")
    return int(bad.sum()), float(dist[bad].max()) if bad.any() else 0.0
