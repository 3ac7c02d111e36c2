"""reth_amd/csrc/atari.hip away from 210 x 160 -> 84 x 84, against references that do not share its code.

warp      k_atari_step's frames at every shape of _area_exact.SHAPES (5 and 4 taps, an integer axis,
          an axis of scale 1, OW = 129 / 500: three and eight waves with idle lanes, one output row,
          exactly kMaxTaps = 8 taps) x every input kind: (1) _area_exact.check_warp -- the exact
          integer area average, which shares no table code with the kernel; (2) bit-equal to
          oracle.warp_frame, the existing claim; (3) independent of the position in the batch.
          Each case prints the largest distance from a rounding tie at which the kernel differs
          from the exactly rounded value (always inside the band: on the MI355X 0.0, exact ties only).
create    rth_atari_create's rejections (too many taps, integer scales, upscaling, > 1024 columns).
step      rth_atari_step's ring semantics at stack 1 / 2 / 4 and ring 2 / 3 against a numpy model
          of the whole ring (FrameStack's deque per slot: drop the oldest, append; reset: k copies):
          reset None / mixed / all, out_frame together with frames, trailing sink stacks, guard
          bands around the ring and out_frame, every stack but the written one unchanged, n = 0,
          the argument errors.
env step  rth_atari_env_step (k_atari_env) called directly with the handles the actor tail assigns
          (actor.hip env_step_one: s0 = i ring + cur, s1 = i ring + (2 t) % ring, cur_slot =
          done ? (2 t + 1) % ring : s1's slot).  The tail never hands the sink stack N ring to
          s0_h / s1_h (it only pads forward batches), so the sink is here as a stack that must keep
          its bytes.
synth     rth_atari_synth_raw / rth_atari_synth_reset against numpy Philox (reth_amd.ppo.philox4x32,
          itself cross-checked with the oracle's C Philox): counter (index lo, index hi, t lo,
          stream | t hi << 8), key (seed lo, seed hi), little-endian words, at the sizes where the
          grid-stride loops (capped at 4096 and 64 workgroups) run a second time; rows with
          done == 0 untouched.
"""
import numpy as np
import pytest
import torch

import _area_exact as X

pytestmark = pytest.mark.gpu

FILL = 0xA5
BAND_BYTES = 64
SHAPE_IDS = [X.shape_id(s) for s in X.SHAPES]
_PRE = {}


def _pre(dev, shape, stack=4):
    from reth_amd.atari import AtariPreprocessor

    key = (shape, stack)
    if key not in _PRE:
        _PRE[key] = AtariPreprocessor(shape[0], shape[1], stack=stack, device=dev)
    return _PRE[key]


def _carve(dev, shape, dtype=torch.uint8):
    """a tensor of `shape` inside a larger uint8 buffer, BAND_BYTES of FILL on both sides, FILL inside"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    big = torch.full((BAND_BYTES + nbytes + BAND_BYTES,), FILL, dtype=torch.uint8, device=dev)
    view = big[BAND_BYTES:BAND_BYTES + nbytes].view(dtype).view(*shape)
    assert view.is_contiguous() and view.data_ptr() == big.data_ptr() + BAND_BYTES
    return big, view


def _bands_intact(big):
    b = big.cpu().numpy()
    return bool(np.all(b[:BAND_BYTES] == FILL) and np.all(b[-BAND_BYTES:] == FILL))


def _raw_batch(kind, shape, n=3):
    (H, W), _ = shape
    pairs = [X.make_pair(kind, H, W, j) for j in range(n)]
    return pairs, np.stack([np.stack(p) for p in pairs])  # [n, 2, H, W, 3]


# ------------------------------------------------------------------------------------------ warp
@pytest.mark.parametrize("kind", X.KINDS)
@pytest.mark.parametrize("shape", X.SHAPES, ids=SHAPE_IDS)
def test_warp_exact_area_oracle_and_position(dev, orc, shape, kind):
    _, (oh, ow) = shape
    pairs, raw = _raw_batch(kind, shape)
    pre = _pre(dev, shape)
    d_raw = torch.as_tensor(raw, device=dev)
    out = pre.warp(d_raw).cpu().numpy()
    assert out.shape == (3, oh, ow) and out.dtype == np.uint8
    worst = nbad = 0
    for j, (f0, f1) in enumerate(pairs):
        b, d = X.check_warp(out[j], f0, f1)
        nbad, worst = nbad + b, max(worst, d)
    print(f"{X.shape_id(shape)} {kind}: {nbad} pixels differ from the exactly rounded value, "
          f"largest dist at a mismatch {worst:.3e}")
    assert worst < X.BAND
    for j, (f0, f1) in enumerate(pairs):
        assert np.array_equal(out[j], orc.warp_frame(f0, f1, oh, ow)), j
    if kind == "flat255":
        assert np.all(out == 255)
    if kind == "redgreen":
        assert np.all(out == X.REDGREEN_GRAY)
    rev = pre.warp(torch.as_tensor(raw[::-1].copy(), device=dev)).cpu().numpy()
    assert np.array_equal(rev, out[::-1])
    for j in range(3):
        alone = pre.warp(d_raw[j:j + 1].clone()).cpu().numpy()
        assert np.array_equal(alone[0], out[j]), j


# ------------------------------------------------------------------------------------------ create
@pytest.mark.parametrize("in_hw,out_hw,msg", [
    ((65, 100), (9, 15), "too many taps"),
    ((8, 8), (4, 2), "integer scale"),
    ((8, 8), (8, 8), "integer scale"),
    ((8, 8), (9, 8), "only downscaling"),
    ((8, 1030), (3, 1025), "only downscaling"),
])
def test_create_rejects(dev, orc, in_hw, out_hw, msg):
    from reth_amd._lib import RethHipError
    from reth_amd.atari import AtariPreprocessor

    with pytest.raises(RethHipError, match=msg):
        AtariPreprocessor(in_hw, out_hw, device=dev)
    # a preprocessor made after the error warps correctly (the shape next to the taps limit)
    shape = ((64, 100), (9, 15))
    pre = AtariPreprocessor(*shape, device=dev)
    pairs, raw = _raw_batch("random", shape, n=1)
    out = pre.warp(torch.as_tensor(raw, device=dev)).cpu().numpy()
    X.check_warp(out[0], *pairs[0])
    assert np.array_equal(out[0], orc.warp_frame(*pairs[0], 9, 15))


# ------------------------------------------------------------------------------------------ step
def _oracle_frames(orc, raw, oh, ow):
    return np.stack([orc.warp_frame(r[0], r[1], oh, ow) for r in raw])


# (reset: None / "all" / "mixed" / "none" = an all-false mask, out_frame given)
STEP_PLAN = [("all", False), (None, False), ("mixed", True), (None, True), ("mixed", False), ("none", True),
             ("mixed", True)]


@pytest.mark.parametrize("ring", [2, 3])
@pytest.mark.parametrize("stack", [1, 2, 4])
def test_step_ring_model(dev, orc, stack, ring):
    shape = X.SMALL
    (H, W), (oh, ow) = shape
    n, sinks = 5, 2
    pre = _pre(dev, shape, stack)
    rng = np.random.default_rng([7, stack, ring])
    big, frames = _carve(dev, (n * ring + sinks, stack, oh, ow))
    model = rng.integers(0, 256, tuple(frames.shape), dtype=np.uint8)  # slots nobody wrote yet hold known bytes
    frames.copy_(torch.as_tensor(model, device=dev))
    obig, oframe = _carve(dev, (n, oh, ow))
    slot = rng.integers(0, ring, n).astype(np.int64)
    for t, (mode, with_out) in enumerate(STEP_PLAN):
        raw = rng.integers(0, 256, (n, 2, H, W, 3), dtype=np.uint8)
        new = (slot + 1) % ring
        mask = {None: np.zeros(n, bool), "none": np.zeros(n, bool), "all": np.ones(n, bool),
                "mixed": np.arange(n) % 2 == t % 2}[mode]
        oframe.fill_(FILL)
        d_raw, d_prev, d_new = (torch.as_tensor(a, device=dev) for a in (raw, slot, new))
        pre.step(d_raw, frames, ring, d_prev, d_new, reset=None if mode is None else torch.as_tensor(mask, device=dev),
                 out_frame=oframe if with_out else None)
        f = _oracle_frames(orc, raw, oh, ow)
        want = model.copy()
        for i in range(n):
            src, dst = model[i * ring + slot[i]], i * ring + new[i]
            want[dst] = np.stack([f[i]] * stack) if mask[i] else np.concatenate([src[1:], f[i][None]])
        got = frames.cpu().numpy()
        assert np.array_equal(got, want), (t, mode, np.argwhere((got != want).reshape(len(want), -1).any(1)).ravel())
        assert _bands_intact(big) and _bands_intact(obig), t
        o = oframe.cpu().numpy()
        assert np.array_equal(o, f) if with_out else np.all(o == FILL), t
        if with_out:
            assert np.array_equal(o, pre.warp(d_raw).cpu().numpy()), t
        assert np.array_equal(d_raw.cpu().numpy(), raw) and np.array_equal(d_prev.cpu().numpy(), slot) \
            and np.array_equal(d_new.cpu().numpy(), new), t
        model, slot = want, new
    assert np.array_equal(frames[n * ring:].cpu().numpy(), model[n * ring:])  # the sink stacks kept their bytes


def test_step_empty_batch_and_argument_errors(dev):
    from reth_amd._lib import RethHipError, call, ptr, stream_ptr

    shape = X.SMALL
    (H, W), (oh, ow) = shape
    n, ring, stack = 5, 2, 4
    pre = _pre(dev, shape, stack)
    big, frames = _carve(dev, (n * ring, stack, oh, ow))
    obig, oframe = _carve(dev, (n, oh, ow))
    raw = torch.zeros((n, 2, H, W, 3), dtype=torch.uint8, device=dev)
    slots = torch.zeros(n, dtype=torch.int64, device=dev)
    reset = torch.ones(n, dtype=torch.uint8, device=dev)
    s = stream_ptr()

    def untouched():
        torch.cuda.synchronize()
        return bool(torch.all(big == FILL)) and bool(torch.all(obig == FILL))

    # n = 0: OK, nothing launched, nothing written
    assert call("rth_atari_step", pre._h, ptr(raw), 0, ptr(frames), ring, stack, ptr(slots), ptr(slots), ptr(reset),
                ptr(oframe), s) == 0
    assert untouched()
    with pytest.raises(RethHipError, match="nothing to write"):
        call("rth_atari_step", pre._h, ptr(raw), n, None, ring, stack, ptr(slots), ptr(slots), ptr(reset), None, s)
    for bad in (dict(ring=1), dict(stack=0), dict(prev=None), dict(new=None)):
        a = dict(ring=ring, stack=stack, prev=ptr(slots), new=ptr(slots))
        a.update(bad)
        with pytest.raises(RethHipError, match="frame-ring arguments incomplete"):
            call("rth_atari_step", pre._h, ptr(raw), n, ptr(frames), a["ring"], a["stack"], a["prev"], a["new"],
                 ptr(reset), ptr(oframe), s)
    with pytest.raises(RethHipError, match="bad arguments"):
        call("rth_atari_step", pre._h, None, n, ptr(frames), ring, stack, ptr(slots), ptr(slots), ptr(reset), None, s)
    assert untouched()


# ------------------------------------------------------------------------------------------ env step
def test_env_step_direct_against_model(dev, orc):
    from reth_amd._lib import call, ptr, stream_ptr

    shape = X.SMALL
    (H, W), (oh, ow) = shape
    n, K, ring, T = 6, 4, 3, 5
    pre = _pre(dev, shape, K)
    rng = np.random.default_rng(11)
    big, frames = _carve(dev, (n * ring + 1, K, oh, ow))  # + the sink stack at n * ring
    model = rng.integers(0, 256, tuple(frames.shape), dtype=np.uint8)
    frames.copy_(torch.as_tensor(model, device=dev))
    cur = rng.integers(0, ring, n).astype(np.int64)
    base = np.arange(n, dtype=np.int64) * ring
    dones = [np.zeros(n), np.array([1, 0, 0, 1, 0, 1.0]), np.ones(n), np.array([0, 1, 1, 0, 0, 0.0]), np.zeros(n)]
    for t in range(1, T + 1):
        done = dones[t - 1].astype(np.float32)
        # the actor tail's assignment (actor.hip: env_step_one), before the frames are written
        nxt, rst = (2 * t) % ring, (2 * t + 1) % ring
        s0, s1 = base + cur, base + nxt
        cur = np.where(done != 0, rst, nxt).astype(np.int64)
        raw = rng.integers(0, 256, (n, 2, H, W, 3), dtype=np.uint8)
        reset_raw = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
        raw[0], raw[2], reset_raw[1], reset_raw[3] = 255, 0, 255, 0  # warp_pixel's clamp at both ends
        want = model.copy()
        for i in range(n):
            want[s1[i]] = np.concatenate([model[s0[i]][1:], orc.warp_frame(raw[i, 0], raw[i, 1], oh, ow)[None]])
        for i in np.nonzero(done)[0]:  # the reset screen alone: no pair max
            want[base[i] + cur[i]] = np.stack([orc.warp_frame(reset_raw[i], reset_raw[i], oh, ow)] * K)
            X.check_warp(want[base[i] + cur[i], 0], reset_raw[i], reset_raw[i])
        assert np.all(want[s1[0], K - 1] == 255) and np.all(want[s1[2], K - 1] == 0)
        if done[1] and done[3]:
            assert np.all(want[base[1] + cur[1]] == 255) and np.all(want[base[3] + cur[3]] == 0)
        before = torch.as_tensor(model, device=dev)
        results = []
        for variant in range(2):  # the reset rows of actors that are not done may hold anything
            rr = reset_raw.copy()
            rr[done == 0] = 255 if variant else rr[done == 0] // 2
            frames.copy_(before)
            ins = [torch.as_tensor(a, device=dev) for a in (raw, s0, s1, done, cur, rr)]
            d_raw, d_s0, d_s1, d_done, d_cur, d_rr = ins
            call("rth_atari_env_step", pre._h, ptr(d_raw), n, ptr(frames), ring, K, ptr(d_s0), ptr(d_s1), ptr(d_done),
                 ptr(d_cur), ptr(d_rr), stream_ptr())
            got = frames.cpu().numpy()
            results.append(got)
            # every stack the model does not write is in `want` as it was before the step
            assert np.array_equal(got, want), (t, variant, np.argwhere((got != want).reshape(len(want), -1).any(1)).ravel())
            assert _bands_intact(big), (t, variant)
            for d_x, x in zip(ins, (raw, s0, s1, done, cur, rr)):
                assert np.array_equal(d_x.cpu().numpy(), x), (t, variant)
        assert np.array_equal(results[0], results[1]), t
        model = want
    assert np.array_equal(model[n * ring], frames[n * ring].cpu().numpy())
    # n = 0 writes nothing
    frames.fill_(FILL)
    call("rth_atari_env_step", pre._h, ptr(d_raw), 0, ptr(frames), ring, K, ptr(d_s0), ptr(d_s1), ptr(d_done),
         ptr(d_cur), ptr(d_rr), stream_ptr())
    torch.cuda.synchronize()
    assert bool(torch.all(big == FILL))


# ------------------------------------------------------------------------------------------ synth
STREAM_ATARI, STREAM_ATARI_RESET = 5, 6  # csrc/common.hpp
SEED64 = 0x9E3779B97F4A7C15 ^ 0x0123456789ABCDEF
T_VALUES = [0, 7, 2 ** 32 + 7]


def _philox_bytes(index, t, stream, seed):
    """the generators' bytes for the counters `index` (uint64 array): 16 per counter, little-endian words"""
    from reth_amd.ppo import philox4x32

    index = np.asarray(index, dtype=np.uint64)
    c = philox4x32(index & np.uint64(0xFFFFFFFF), index >> np.uint64(32), t & 0xFFFFFFFF,
                   (stream | ((t >> 32) << 8)) & 0xFFFFFFFF, seed & 0xFFFFFFFF, seed >> 32)
    return np.ascontiguousarray(np.stack(c, axis=1).astype("<u4")).view(np.uint8).reshape(-1)


def test_numpy_philox_is_the_oracles(orc):
    from reth_amd.ppo import philox4x32

    ctrs = [(0, 0, 0, 0), (1, 0, 7, 5), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (1048578, 0, 7, 5 | (1 << 8)),
            (0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (81, 0, 7, 6 | (1 << 8))]
    keys = [(0, 0), (SEED64 & 0xFFFFFFFF, SEED64 >> 32), (0xFFFFFFFF, 0xFFFFFFFF), (0xA4093822, 0x299F31D0)]
    for c in ctrs:
        for k in keys:
            ours = np.array([int(w) for w in philox4x32(*c, *k)], dtype=np.uint32)
            assert np.array_equal(ours, orc.philox4x32(c, k)), (c, k)


@pytest.mark.parametrize("nvec", [1, 257, 4096 * 256 + 3], ids=lambda v: f"{16 * v}B")
def test_synth_raw_against_philox(dev, nvec):
    from reth_amd._lib import call, ptr, stream_ptr

    nbytes = 16 * nvec
    buf = torch.empty(nbytes + BAND_BYTES, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    index = np.arange(nvec, dtype=np.uint64)
    frames = []
    for t in T_VALUES:
        buf.fill_(FILL)
        t_dev = torch.tensor([t], dtype=torch.int64, device=dev)
        call("rth_atari_synth_raw", ptr(buf), nbytes, SEED64, ptr(t_dev), stream_ptr())
        got = buf.cpu().numpy()
        want = _philox_bytes(index, t, STREAM_ATARI, SEED64)
        bad = np.nonzero(got[:nbytes] != want)[0]
        assert bad.size == 0, (t, bad.size, "first wrong 16-byte vector", int(bad[0]) // 16)
        assert np.all(got[nbytes:] == FILL), t
        assert int(t_dev.item()) == t
        frames.append(got[:nbytes].copy())
    assert not any(np.array_equal(frames[a], frames[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


def test_synth_argument_errors(dev):
    from reth_amd._lib import RethHipError, call, ptr, stream_ptr

    buf = torch.full((256,), FILL, dtype=torch.uint8, device=dev)
    t_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    done = torch.ones(4, dtype=torch.float32, device=dev)
    s = stream_ptr()
    for p, nbytes in ((ptr(buf) + 4, 16), (ptr(buf) + 8, 32), (ptr(buf), 24), (ptr(buf), 8), (None, 16)):
        with pytest.raises(RethHipError, match="rth_atari_synth_raw: bad arguments"):
            call("rth_atari_synth_raw", p, nbytes, SEED64, ptr(t_dev), s)
    with pytest.raises(RethHipError, match="rth_atari_synth_raw: bad arguments"):
        call("rth_atari_synth_raw", ptr(buf), 16, SEED64, None, s)
    for p, n, fb in ((ptr(buf) + 4, 4, 16), (ptr(buf), 4, 24), (ptr(buf), 4, 0), (ptr(buf), 65536, 16)):
        with pytest.raises(RethHipError, match="rth_atari_synth_reset: bad arguments"):
            call("rth_atari_synth_reset", p, n, fb, SEED64, ptr(t_dev), ptr(done), s)
    assert call("rth_atari_synth_raw", ptr(buf), 0, SEED64, ptr(t_dev), s) == 0
    assert call("rth_atari_synth_reset", ptr(buf), 0, 16, SEED64, ptr(t_dev), ptr(done), s) == 0
    torch.cuda.synchronize()
    assert bool(torch.all(buf == FILL))


@pytest.mark.parametrize("vec", [5, 100800 // 16, 64 * 256 + 5], ids=lambda v: f"{16 * v}B")
def test_synth_reset_against_philox(dev, vec):
    from reth_amd._lib import call, ptr, stream_ptr

    n, fb = 4, 16 * vec
    buf = torch.empty(n * fb + BAND_BYTES, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    t = 2 ** 32 + 7
    t_dev = torch.tensor([t], dtype=torch.int64, device=dev)
    seed = SEED64 ^ 0xFFFF
    rows = _philox_bytes(np.arange(n * vec, dtype=np.uint64), t, STREAM_ATARI_RESET, seed).reshape(n, fb)
    for mask in ([1, 0, 1, 0], [0, 1, 0, 1], [0, 0, 0, 0]):
        done = np.array(mask, dtype=np.float32)
        d_done = torch.as_tensor(done, device=dev)
        runs = []
        for _ in range(2):  # a second call with the same inputs is bit-identical
            buf.fill_(FILL)
            call("rth_atari_synth_reset", ptr(buf), n, fb, seed, ptr(t_dev), ptr(d_done), stream_ptr())
            runs.append(buf.cpu().numpy())
        got = runs[0]
        assert np.array_equal(runs[0], runs[1])
        for i in range(n):
            row = got[i * fb:(i + 1) * fb]
            if done[i]:
                bad = np.nonzero(row != rows[i])[0]
                assert bad.size == 0, (mask, i, bad.size, "first wrong 16-byte vector", int(bad[0]) // 16)
            else:
                assert np.all(row == FILL), (mask, i)  # rows of running episodes keep their bytes
        assert np.all(got[n * fb:] == FILL), mask
        assert np.array_equal(d_done.cpu().numpy(), done) and int(t_dev.item()) == t
