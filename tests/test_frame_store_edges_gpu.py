"""The frame store's three device pieces against the host model of _frame_store_model.py:
k_frames_push (new frames and stack ids), the CONV_STACK branch of k_copy_rows (the gather that
assembles stacks) and the ids-out gather that feeds conv1 "frames in place"
(reth_amd/csrc/replay.hip).  HbmReplay(..., frame_store=F) is driven directly -- no actors, no
solver, no loop -- so the head can be put where a loop only gets by luck of its seed.

There are no tolerances: the model writes to id % F as the device does, so after every push
rep.frames, the stack table and the head equal the model's exactly, wrapped ring or not, and a
gathered stack equals model.gather of the row's stored ids.

The synthetic frame ring is random uint8 [n * ring_slots, K, H, W], redrawn in the written stacks
before each push (not real shifted stacks: a kernel that read another frame of the stack than
K-1 of s1 / 0 of the reset stack would show).  Per actor s0, s1 and the reset stack are three
different ring slots (current, +1, +2 mod ring_slots); the kernel's contract excludes aliasing.
F is a little more than one push's frames (max(2 n, K n) + 3), so every sequence wraps often.

Small stacks.  A stack row of at most 64 bytes -- (K, H, W) = (4, 4, 4), (2, 4, 8), (1, 8, 8) of
the geometries below -- used to be laid out by launch_copy as a one-lane-per-row column, where
k_copy_rows has no frame-stack arm: the ids were read as pixels and 4 x the row written as
floats, past the row and the buffer.  Such columns are chunked now; every gather here writes into
a buffer with sentinel guards (64 bytes before, 256 after) that must stay untouched.
"""
import ctypes

import numpy as np
import pytest
import torch

from _frame_store_model import FrameStoreModel

pytestmark = pytest.mark.gpu

# (K, H, W): 16-byte vectors per frame 1, 2, 4, 1, 256, 257, 513, 441 -- k_frames_push copies two
# vectors per lane per round of 256 lanes (second index clamped): fewer than 256, exactly 256,
# 257 (one lane has a second vector), 513 (a second round of one vector), the Atari size
GEOMS = [(4, 4, 4), (2, 4, 8), (1, 8, 8), (5, 4, 4), (4, 64, 64), (4, 257, 16), (3, 513, 16), (4, 84, 84)]
# large frames with few actors, many actors (the done count's strided loop past 256 lanes, the
# serial rank) with small frames
GEOM_ACTORS = [((4, 4, 4), 1), ((4, 4, 4), 3), ((4, 4, 4), 64), ((4, 4, 4), 257), ((4, 4, 4), 300),
               ((2, 4, 8), 3), ((2, 4, 8), 257), ((1, 8, 8), 1), ((1, 8, 8), 64), ((5, 4, 4), 3), ((5, 4, 4), 300),
               ((4, 64, 64), 1), ((4, 64, 64), 3), ((4, 257, 16), 3), ((3, 513, 16), 1), ((3, 513, 16), 3),
               ((4, 84, 84), 3)]
PATTERNS = ["none", "all", "first", "last", "random"]
SENTINEL = 0xA5
GUARD_LO, GUARD_HI = 64, 256


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


class Rig:
    """a frame-store replay [s0 stack, one float, s1 stack], a synthetic frame ring and the model"""

    def __init__(self, dev, geom, n, slots, seed, capacity=1, F=None):
        from reth_amd.replay import Column, FrameColumn, HbmReplay

        K, H, W = geom
        self.dev, self.geom, self.n, self.slots, self.K = dev, geom, n, slots, K
        self.F = F or max(2 * n, K * n) + 3
        self.rng = np.random.default_rng([seed, K, H, W, n, slots])
        self.rep = HbmReplay(capacity, [FrameColumn(geom), Column((), torch.float32), FrameColumn(geom)], device=dev,
                             frame_store=self.F)
        self.m = FrameStoreModel(self.F, K, H * W, n, slots)
        self.ring_h = self.rng.integers(0, 256, (n * slots, K, H, W), dtype=np.uint8)
        self.ring = torch.as_tensor(self.ring_h, device=dev)
        self.sid = torch.zeros((n * slots, K), dtype=torch.int32, device=dev)
        self.cur = self.rng.integers(0, slots, n)
        self.rows = [np.zeros((0, K), np.int32), np.zeros(0, np.float32), np.zeros((0, K), np.int32)]  # the replay's rows

    def _t(self, a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=self.dev)

    def _redraw(self, stacks):
        stacks = np.unique(stacks)
        self.ring_h[stacks] = self.rng.integers(0, 256, (len(stacks), *self.geom), dtype=np.uint8)
        self.ring[self._t(stacks, torch.int64)] = self._t(self.ring_h[stacks], torch.uint8)

    def place_head(self, v):
        self.rep.frame_head.fill_(v)
        self.m.head = int(v)

    def pattern(self, name):
        done = np.zeros(self.n, np.float32)
        if name == "all":
            done[:] = 1
        elif name == "first":
            done[0] = 1
        elif name == "last":
            done[-1] = 1
        elif name == "random":
            done[:] = self.rng.random(self.n) < 0.25
        return done

    def init(self):
        self.cur = self.rng.integers(0, self.slots, self.n)
        self._redraw(np.arange(self.n) * self.slots + self.cur)
        self.rep.push_frames(self.ring, self.n, self.slots, None, None, None, self._t(self.cur, torch.int64), self.sid,
                             init=True)
        self.m.push_init(self.ring_h, self.cur)

    def step(self, done):
        base = np.arange(self.n) * self.slots
        s0, s1 = base + self.cur, base + (self.cur + 1) % self.slots
        reset = (self.cur + 2) % self.slots
        self._redraw(np.concatenate([s1, (base + reset)[done != 0]]))
        self.cur = np.where(done != 0, reset, (self.cur + 1) % self.slots)
        self.s0_h, self.s1_h = s0, s1
        self.step_args = (self._t(s0, torch.int64), self._t(s1, torch.int64), self._t(done, torch.float32),
                          self._t(self.cur, torch.int64))
        self.rep.push_frames(self.ring, self.n, self.slots, *self.step_args, self.sid)
        self.m.push_step(self.ring_h, s0, s1, done, self.cur)

    def check(self, what=""):
        torch.cuda.synchronize()
        head = int(self.rep.frame_head)
        assert head == self.m.head, (what, head, self.m.head)
        sid = self.sid.cpu().numpy()
        bad = np.flatnonzero((sid != self.m.sid).any(1))
        assert bad.size == 0, (what, "stack table", bad[:4], sid[bad[:4]], self.m.sid[bad[:4]])
        store = self.rep.frames.view(self.F, -1).cpu().numpy()
        bad = np.flatnonzero((store != self.m.store).any(1))
        assert bad.size == 0, (what, "store frames", bad[:8])

    def append(self):
        """the step's rows, as DeviceActors.append hands them over: the s0 / s1 columns' source is
        the stack table, src_rows the stack handles"""
        s0, s1 = self._t(self.s0_h, torch.int64), self._t(self.s1_h, torch.int64)
        x = (len(self.rows[1]) + np.arange(self.n)).astype(np.float32)
        self.rep.append([self.sid, self._t(x, torch.float32), self.sid], torch.ones(self.n, device=self.dev),
                        src_rows=[s0, None, s1])
        for k, new in enumerate((self.m.sid[self.s0_h], x, self.m.sid[self.s1_h])):
            self.rows[k] = np.concatenate([self.rows[k], new])


def _head_positions(F, n, dones):
    return [0, F - 1, F - n, F - n - 1, F - n - (dones + 1) // 2, F - (n + 1) // 2, 2 ** 31 + 5, 2 ** 33 + F - 2]


@pytest.mark.parametrize("geom,n", GEOM_ACTORS, ids=_id)
def test_push_step_at_every_head_position(dev, geom, n):
    """one step from each head position with each done pattern: the step's frames ending exactly
    at the ring's end, the wrap inside the step frames, inside the reset frames, between the two,
    heads past 2^31 and 2^33 (int64 head -> % F -> int32 id)"""
    r = Rig(dev, geom, n, 3, seed=1)
    r.init()
    r.check("init")
    for name in PATTERNS:
        for j in range(8):
            done = r.pattern(name)
            head = _head_positions(r.F, n, int(done.sum()))[j]
            r.place_head(head)
            r.step(done)
            assert r.m.head == head + n + int(done.sum())
            r.check((name, head))


@pytest.mark.parametrize("geom,n", GEOM_ACTORS, ids=_id)
def test_push_init_at_every_head_position(dev, geom, n):
    """init mode (K frames per actor) from the same head positions scaled by K"""
    K = geom[0]
    r = Rig(dev, geom, n, 4, seed=2)
    kn = K * n
    for head in [0, r.F - 1, r.F - kn, r.F - kn - 1, r.F - (kn + 1) // 2, 2 ** 31 + 5, 2 ** 33 + r.F - 2]:
        r.place_head(head)
        r.init()
        assert r.m.head == head + kn
        r.check(("init", head))
    r.step(r.pattern("random"))  # the steps go on from the tuples of the last init
    r.check("step after init")


def _guarded(dev, nbytes):
    buf = torch.full((GUARD_LO + nbytes + GUARD_HI,), SENTINEL, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf, buf[GUARD_LO:GUARD_LO + nbytes]


def _guards_untouched(bufs):
    for k, (buf, body) in enumerate(bufs):
        lo, hi = buf[:GUARD_LO].cpu().numpy(), buf[GUARD_LO + body.numel():].cpu().numpy()
        assert (lo == SENTINEL).all(), (k, "bytes written before the output", np.flatnonzero(lo != SENTINEL)[:8])
        assert (hi == SENTINEL).all(), (k, "bytes written past the output", np.flatnonzero(hi != SENTINEL)[:8])


def _index_sets(rng, rows):
    """1, 5 and 257 rows, out of order, with repeats, first and last row included"""
    one = rng.integers(0, rows, 1)
    five = rng.integers(0, rows, 5)
    five[3] = five[0]
    many = rng.integers(0, rows, 257)
    many[[7, 100, 256]] = [rows - 1, 0, rows - 1]
    return [one, five, many]


def _gather_stacks(r, idx):
    """the gather that assembles stacks, every output column inside sentinel guards"""
    K, H, W = r.geom
    m = len(idx)
    bufs = [_guarded(r.dev, m * K * H * W), _guarded(r.dev, m * 4), _guarded(r.dev, m * K * H * W)]
    out = [bufs[0][1].view(m, K, H, W), bufs[1][1].view(torch.float32), bufs[2][1].view(m, K, H, W)]
    r.rep.gather(r._t(idx, torch.int64), out)
    torch.cuda.synchronize()
    _guards_untouched(bufs)
    for c in (0, 2):
        got = out[c].cpu().numpy().reshape(m, K, H * W)
        want = r.m.gather(r.rows[c][idx])
        bad = np.flatnonzero((got != want).reshape(m, -1).any(1))
        assert bad.size == 0, ("column", c, "gathered rows", bad[:8])
    assert np.array_equal(out[1].cpu().numpy(), r.rows[1][idx])


def _gather_ids(r, idx):
    """the ids-out gather: both stack columns' ids in one guarded allocation, as new_batch lays
    them out"""
    from reth_amd.replay import FrameStacks

    K, H, W = r.geom
    m = len(idx)
    bufs = [_guarded(r.dev, 2 * m * K * 4), _guarded(r.dev, m * 4)]
    ids = bufs[0][1].view(torch.int32).view(2 * m, K)
    out = [FrameStacks(ids[:m], r.rep.frames), bufs[1][1].view(torch.float32), FrameStacks(ids[m:], r.rep.frames)]
    r.rep.gather(r._t(idx, torch.int64), out)
    torch.cuda.synchronize()
    _guards_untouched(bufs)
    for c in (0, 2):
        assert np.array_equal(out[c].ids.cpu().numpy(), r.rows[c][idx])
        got = out[c].stacks().cpu().numpy().reshape(m, K, H * W)
        assert np.array_equal(got, r.m.gather(r.rows[c][idx]))
    assert np.array_equal(out[1].cpu().numpy(), r.rows[1][idx])
    return out


@pytest.mark.parametrize("slots", [3, 4])
@pytest.mark.parametrize("geom", GEOMS, ids=_id)
def test_sequence_and_gather(dev, geom, slots):
    """an init push and 3 ring_slots + 2 steps (every slot reused, tuples shifted through reset
    tuples, the store wrapped), compared after every push; the rows appended on the way gathered
    as stacks and, for 4-frame stacks, as ids"""
    from reth_amd._lib import RethHipError

    K = geom[0]
    n = 5 if geom[1] * geom[2] <= 64 else 3
    steps = 3 * slots + 2
    r = Rig(dev, geom, n, slots, seed=3, capacity=n * steps)
    r.init()
    r.check("init")
    names = ["random", "all", "random", "none", "first", "random", "last"]
    for t in range(steps):
        r.step(r.pattern(names[t % len(names)]))
        r.check(("step", t))
        r.append()
    assert r.m.head > 2 * r.F and r.rep.info()[0] == n * steps
    torch.cuda.synchronize()
    for c in (0, 2):  # the appended rows hold the tuples of their stacks at append time
        assert np.array_equal(r.rep.column_storage(c).cpu().numpy(), r.rows[c])
    sets = _index_sets(r.rng, n * steps)
    for idx in sets:
        _gather_stacks(r, idx)
    if K == 4:
        r.rep.set_frame_ids(True)
        for idx in sets:
            _gather_ids(r, idx)
        r.rep.set_frame_ids(False)
    else:
        with pytest.raises(RethHipError):  # id tuples are read as int4
            r.rep.set_frame_ids(True)
    _gather_stacks(r, sets[1])  # and the stacks again: ids-out is off / was never on
    r.check("after the gathers")


def test_conv1_in_place_across_a_wrap(dev):
    """rth_conv1_frames_bias_relu on gathered ids, after pushes that wrapped the store several
    times, is bit-equal to rth_conv_bias_relu on the model's stacks"""
    from reth_amd import _lib
    from test_conv_gpu import GEOMS as CONV_GEOMS
    from test_conv_gpu import _shape

    n, slots, steps = 7, 3, 10
    r = Rig(dev, (4, 84, 84), n, slots, seed=4, capacity=n * steps)
    r.place_head(r.F - 9)  # the init push itself straddles the ring's end
    r.init()
    for t in range(steps):
        r.step(r.pattern("random" if t != 4 else "all"))
        r.check(("step", t))
        r.append()
    assert r.m.head > 3 * r.F
    r.rep.set_frame_ids(True)
    idx = r.rng.permutation(n * steps)
    idx[5] = idx[0]
    ids = _gather_ids(r, idx)[2].ids  # s1: rows of the latest frames
    m = len(idx)
    stacks = torch.as_tensor(r.m.gather(r.rows[2][idx]).reshape(m, 4, 84, 84), device=dev).contiguous()
    g = torch.Generator().manual_seed(77)
    w = (torch.rand((32, 4, 8, 8), generator=g) * 2 - 1) / 16
    b = ((torch.rand(32, generator=g) * 2 - 1) * 0.1).to(dev)
    shape = _shape(_lib.CONV_U8_CHW, *CONV_GEOMS[0])
    pk = torch.empty(_lib.lib().rth_conv_packed_bytes(_lib.ctypes.byref(shape)) // 4, device=dev)
    _lib.call("rth_conv_pack", _lib.ctypes.byref(shape), w.to(dev).contiguous(memory_format=torch.channels_last)
              .data_ptr(), pk.data_ptr(), _lib.stream_ptr())
    y_st = torch.full((m, 20, 20, 32), float("nan"), device=dev)
    y_fr = torch.full((m, 20, 20, 32), float("nan"), device=dev)
    _lib.call("rth_conv_bias_relu", _lib.ctypes.byref(shape), stacks.data_ptr(), None, m, pk.data_ptr(), b.data_ptr(),
              y_st.data_ptr(), _lib.stream_ptr())
    _lib.call("rth_conv1_frames_bias_relu", _lib.ctypes.byref(shape), r.rep.frames.data_ptr(), ids.data_ptr(), m,
              pk.data_ptr(), b.data_ptr(), y_fr.data_ptr(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert not torch.isnan(y_fr).any() and (y_fr > 0).any()
    assert torch.equal(y_st, y_fr)


def test_refusals_launch_nothing(dev):
    """every refused call leaves the store, the stack table and the head as they were"""
    from reth_amd import _lib
    from reth_amd._lib import RethHipError
    from reth_amd.replay import Column, FrameColumn, HbmReplay

    r = Rig(dev, (4, 4, 4), 3, 3, seed=5)
    r.place_head(r.F - 2)
    r.init()
    r.step(r.pattern("all"))
    r.check("before")
    s0, s1, done, cur = r.step_args

    def push(n, stack):
        _lib.call("rth_replay_push_frames", r.rep._h, r.ring.data_ptr(), n, r.slots, stack, s0.data_ptr(), s1.data_ptr(),
                  done.data_ptr(), cur.data_ptr(), r.sid.data_ptr(), 0, _lib.stream_ptr())

    for n, stack in [(65536, 4), (3, 0), (3, 65)]:
        with pytest.raises(RethHipError):
            push(n, stack)
        r.check(("refused push", n, stack))
    with pytest.raises(RethHipError):  # attaching twice
        store, head = _lib.c_vp(), _lib.c_vp()
        _lib.call("rth_replay_frames_attach", r.rep._h, r.F, 16, ctypes.byref(store), ctypes.byref(head))
    r.check("refused attach")
    with pytest.raises(RethHipError):  # 9-byte frames
        HbmReplay(8, [FrameColumn((4, 3, 3))], device=dev, frame_store=8)
    plain = HbmReplay(8, [Column((), torch.float32)], device=dev)
    with pytest.raises(RethHipError):  # no store attached
        plain.push_frames(r.ring, r.n, r.slots, s0, s1, done, cur, r.sid)
    r.check("refused push without a store")
    push(3, 4)  # the same call with valid arguments is taken
    r.m.push_step(r.ring_h, r.s0_h, r.s1_h, done.cpu().numpy(), r.cur)
    r.check("accepted")
