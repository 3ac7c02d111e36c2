"""oracle.warp_frame / oracle.area_tab against the exact area average of _area_exact.py, without a
GPU: the restatement the device kernel is compared with bit for bit (test_atari_gpu.py,
test_atari_edges_gpu.py) is itself an area average, at every shape and input kind of the helper.

The cap on the share of band pixels is a condition of the test, not a measurement: part (b) of
check_warp binds only outside the band, so a test whose random inputs sat mostly inside it would
check nothing.  The band pixels of random inputs are nearly all exact ties of small denominators.
"""
import numpy as np
import pytest

import _area_exact as X

SHAPE_IDS = [X.shape_id(s) for s in X.SHAPES]


@pytest.mark.parametrize("shape", X.SHAPES, ids=SHAPE_IDS)
def test_oracle_warp_is_the_area_average(orc, shape):
    (H, W), (oh, ow) = shape
    worst = 0.0
    for kind in X.KINDS:
        for j in range(3):
            f0, f1 = X.make_pair(kind, H, W, j)
            out = orc.warp_frame(f0, f1, oh, ow)
            nbad, d = X.check_warp(out, f0, f1)  # every mismatch with `rounded` has dist < BAND
            worst = max(worst, d)
            if kind == "flat255":
                assert np.all(out == 255)
            if kind == "redgreen":
                assert np.all(out == X.REDGREEN_GRAY)
    print(f"{X.shape_id(shape)}: largest dist at an oracle / rounded mismatch {worst:.3e}")
    assert worst < X.BAND


@pytest.mark.parametrize("shape", X.SHAPES, ids=SHAPE_IDS)
def test_random_inputs_sit_outside_the_band(shape):
    (H, W), (oh, ow) = shape
    cap = 0.01 if shape == X.WORKLOAD else 0.10
    inside = total = 0
    for j in range(3):
        f0, f1 = X.make_pair("random", H, W, j)
        _, dist, _ = X.exact_warp(f0, f1, oh, ow)
        inside += int((dist < X.BAND).sum())
        total += dist.size
        # a single pair of a small shape has too few pixels for a share: the cap is on the three
        # pairs the GPU test warps together; one pair alone must still leave pixels to check
        assert (dist >= X.BAND).any()
    print(f"{X.shape_id(shape)}: {inside} of {total} pixels within BAND of a tie ({inside / total:.2%})")
    assert inside <= cap * total


@pytest.mark.parametrize("S,D,count", [(64, 9, 8), (100, 15, 8), (65, 9, 9)] +
                         [(s, d, None) for (hw, o) in X.SHAPES for s, d in zip(hw, o)])
def test_oracle_area_tab(orc, S, D, count):
    tab = orc.area_tab(S, D, 1.0 / (D / S))
    assert len(tab) == D
    nxt = 0  # the first source pixel not yet covered
    for d, taps in enumerate(tab):
        assert taps, d
        src = [s for s, _ in taps]
        w = np.array([float(x) for _, x in taps], dtype=np.float64)
        assert all(isinstance(x, np.float32) for _, x in taps)
        assert np.all(w > 0) and abs(w.sum() - 1.0) <= 1e-6, (d, w.sum())
        assert src == list(range(src[0], src[0] + len(src))), (d, src)
        assert src[0] in (nxt - 1, nxt) and src[0] >= 0, (d, src, nxt)  # no gap between consecutive cells
        nxt = src[-1] + 1
        # against the integer overlaps: the same pixels, weights overlap / S
        ov = X.overlap(S, D)[d]
        assert src == list(np.nonzero(ov)[0]), (d, src)
        assert np.allclose(w, ov[src] / S, rtol=0, atol=1e-6), (d, w, ov[src] / S)
    assert tab[0][0][0] == 0 and nxt == S
    if count is not None:
        assert max(len(t) for t in tab) == count


def test_helper_integer_scale_box_by_hand():
    gray = np.array([[1, 3, 10, 20, 7, 9],
                     [5, 7, 30, 40, 8, 8],
                     [0, 0, 255, 255, 2, 3],
                     [0, 1, 255, 254, 4, 4],
                     ], dtype=np.int64)
    rounded, dist, value = X.exact_from_gray(gray, 2, 3)
    assert np.array_equal(value, [[4.0, 25.0, 8.0], [0.25, 254.75, 3.25]])
    assert np.array_equal(rounded, [[4, 25, 8], [0, 255, 3]])
    assert np.array_equal(dist, [[0.5, 0.5, 0.5], [0.25, 0.25, 0.25]])
    assert np.array_equal(X.overlap(6, 3), np.kron(np.eye(3, dtype=np.int64), [[3, 3]]))
    # gray of a frame pair: per-channel max, fixed point
    f0 = np.zeros((1, 2, 3), np.uint8)
    f1 = np.zeros((1, 2, 3), np.uint8)
    f0[0, 0], f1[0, 0] = (255, 0, 0), (0, 255, 0)
    f0[0, 1], f1[0, 1] = (10, 200, 30), (20, 100, 3)
    assert np.array_equal(X.gray_max(f0, f1), [[X.REDGREEN_GRAY, (20 * 4899 + 200 * 9617 + 30 * 1868 + 8192) >> 14]])


def test_helper_rounds_exact_ties_to_even():
    # 2 x 2 -> 1 x 1 is the mean of four: x.5 needs a sum of 4 q + 2
    for q in (0, 1, 2, 3, 126, 127, 253, 254):
        gray = np.array([[q, q], [q + 1, q + 1]], dtype=np.int64)
        rounded, dist, value = X.exact_from_gray(gray, 1, 1)
        assert value[0, 0] == q + 0.5 and dist[0, 0] == 0.0
        assert rounded[0, 0] == (q if q % 2 == 0 else q + 1)
    # a non-integer scale: 3 -> 2 columns, cells [0, 1.5) and [1.5, 3): (2 a + b) / 3 and (b + 2 c) / 3;
    # two rows -> one doubles the denominator: (2 a + b + 2 a' + b') / 6 = 2.5 at the sum 15
    gray = np.array([[3, 1, 0], [3, 2, 9]], dtype=np.int64)
    rounded, dist, value = X.exact_from_gray(gray, 1, 2)
    assert value[0, 0] == 2.5 and dist[0, 0] == 0.0 and rounded[0, 0] == 2
    assert rounded[0, 1] == 4 and abs(value[0, 1] - 21 / 6) < 1e-15 and abs(dist[0, 1] - 0.0) < 1e-15
    gray[1, 2] = 10  # (1 + 2 + 0 + 20) / 6 = 3.8333
    rounded, dist, value = X.exact_from_gray(gray, 1, 2)
    assert rounded[0, 1] == 4 and abs(dist[0, 1] - (0.5 - 1 / 6)) < 1e-15
