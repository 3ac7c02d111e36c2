"""The frame-store model of _frame_store_model.py, checked without a GPU against a second,
independent bookkeeping: a dict from frame-ring stack to the full uint8 stack it holds, shifted
and reset the way the reference's FrameStack.step / FrameStack.reset do (append the new frame to a
deque of K; on reset, the first frame K times).  That bookkeeping knows no frame ids and no store:
it keeps the pixels.  The model keeps ids and one copy of every frame; while the store is large
enough, gathering a stack's ids must give back its pixels.

"Large enough" is decided per stack: frame number o (counting every frame pushed, in push order)
is overwritten by frame o + F, so a stack is intact while its oldest frame's number is at least
(frames pushed) - F.  The numbers are kept next to the pixels only to decide which stacks to
compare; with a store that holds the whole run every stack ever written must compare."""
import numpy as np
import pytest

from _frame_store_model import FrameStoreModel


class TrueStacks:
    """n actors over a frame ring of ring_slots stacks each, as the device actors use it: a step
    writes the shifted stack into the next slot, a done actor's reset stack goes one slot further
    and becomes its current one"""

    def __init__(self, n, slots, K, fshape, seed):
        self.n, self.slots, self.K, self.fshape = n, slots, K, fshape
        self.rng = np.random.default_rng(seed)
        self.ring = np.zeros((n * slots, K, *fshape), np.uint8)
        self.true = {}  # stack handle -> (uint8 [K, *fshape], the K frames' push numbers)
        self.cur = self.rng.integers(0, slots, n)
        self.pushed = 0  # frames drawn so far

    def _frame(self):
        self.pushed += 1
        return self.rng.integers(0, 256, self.fshape, dtype=np.uint8)

    def _put(self, st, stack, nums):
        self.true[st] = (stack, list(nums))
        self.ring[st] = stack

    def init(self):
        base = self.pushed
        for i in range(self.n):
            stack = np.stack([self._frame() for _ in range(self.K)])
            self._put(i * self.slots + self.cur[i], stack, [base + self.K * i + k for k in range(self.K)])
        return self.cur.copy()

    def step(self, p_done):
        base = self.pushed
        done = self.rng.random(self.n) < p_done
        s0 = np.arange(self.n) * self.slots + self.cur
        s1 = np.arange(self.n) * self.slots + (self.cur + 1) % self.slots
        for i in range(self.n):  # FrameStack.step: the deque drops its oldest frame
            stack, nums = self.true[s0[i]]
            self._put(s1[i], np.concatenate([stack[1:], self._frame()[None]]), nums[1:] + [base + i])
        self.cur = (self.cur + 1) % self.slots
        rank = 0
        for i in np.flatnonzero(done):  # FrameStack.reset: the first frame K times
            self.cur[i] = (self.cur[i] + 1) % self.slots
            f = self._frame()
            self._put(i * self.slots + self.cur[i], np.stack([f] * self.K), [base + self.n + rank] * self.K)
            rank += 1
        return s0, s1, done.astype(np.float32), self.cur.copy()


def _compare(m, t, head0):
    """every intact stack's gathered ids == its pixels; returns (compared, left out)"""
    same = out = 0
    for st, (stack, nums) in t.true.items():
        if min(nums) < t.pushed - m.F:
            out += 1
            continue
        got = m.gather(m.sid[st]).reshape(stack.shape)
        assert np.array_equal(got, stack), (st, nums, m.sid[st])
        assert [int(x) for x in m.sid[st]] == [(head0 + o) % m.F for o in nums]
        same += 1
    return same, out


@pytest.mark.parametrize("n,slots,K,fshape", [(1, 3, 4, (4, 4)), (3, 3, 1, (8, 8)), (5, 4, 5, (4, 4)), (7, 6, 2, (4, 8)),
                                              (33, 3, 4, (2, 8))])
@pytest.mark.parametrize("head0", [0, 2 ** 33 + 5])
def test_model_whole_run_in_store(n, slots, K, fshape, head0):
    """a store that holds every frame of the run: every stack ever written stays intact"""
    steps = 300
    F = K * n + 2 * n * steps
    t = TrueStacks(n, slots, K, fshape, seed=[n, slots, K])
    m = FrameStoreModel(F, K, int(np.prod(fshape)), n, slots, head=head0)
    m.push_init(t.ring, t.init())
    assert m.head == head0 + t.pushed == head0 + K * n
    dones = 0
    for _ in range(steps):
        s0, s1, done, cur = t.step(0.25)
        m.push_step(t.ring, s0, s1, done, cur)
        dones += int(done.sum())
        assert m.head == head0 + t.pushed
        same, out = _compare(m, t, head0)
        assert out == 0 and same == len(t.true)
    assert t.pushed == K * n + steps * n + dones and 0 < dones < steps * n
    assert len(t.true) == n * slots  # every ring slot was used


@pytest.mark.parametrize("n,slots,K,fshape", [(1, 8, 4, (4, 4)), (3, 3, 1, (8, 8)), (5, 4, 5, (4, 4)), (7, 6, 2, (4, 8))])
def test_model_wrapping_store(n, slots, K, fshape):
    """a store of a few steps' frames, wrapped many times: the stacks whose frames are all
    younger than F frames are intact (the current ones always are), the others are left out"""
    steps = 300
    F = 2 * n * K  # every current stack: its K frames came in K steps of at most 2 n frames each
    t = TrueStacks(n, slots, K, fshape, seed=[n, slots, K, 1])
    m = FrameStoreModel(F, K, int(np.prod(fshape)), n, slots)
    m.push_init(t.ring, t.init())
    left_out = 0
    for _ in range(steps):
        s0, s1, done, cur = t.step(0.25)
        m.push_step(t.ring, s0, s1, done, cur)
        assert m.head == t.pushed
        same, out = _compare(m, t, 0)
        assert same >= n  # each actor's current stack at least
        for i in range(n):
            nums = t.true[i * slots + cur[i]][1]
            assert min(nums) >= t.pushed - F
        left_out += out
    assert m.head > 20 * F
    assert left_out > 0


def test_model_all_done_and_none():
    n, slots, K = 4, 3, 3
    t = TrueStacks(n, slots, K, (4, 4), seed=9)
    m = FrameStoreModel(64, K, 16, n, slots)
    m.push_init(t.ring, t.init())
    for p in (1.0, 0.0, 1.0, 1.0, 0.0):
        s0, s1, done, cur = t.step(p)
        assert done.all() if p else not done.any()
        m.push_step(t.ring, s0, s1, done, cur)
        assert m.head == t.pushed
        _compare(m, t, 0)
    assert m.head == K * n + 5 * n + 3 * n


def test_model_refuses_a_push_larger_than_the_store():
    t = TrueStacks(4, 3, 4, (4, 4), seed=3)
    cur = t.init()
    with pytest.raises(ValueError):
        FrameStoreModel(15, 4, 16, 4, 3).push_init(t.ring, cur)
    FrameStoreModel(16, 4, 16, 4, 3).push_init(t.ring, cur)
    s0, s1, done = np.arange(4) * 3, np.arange(4) * 3 + 1, np.array([1, 1, 0, 0], np.float32)
    with pytest.raises(ValueError):  # 4 step frames + 2 reset frames
        FrameStoreModel(5, 4, 16, 4, 3).push_step(t.ring, s0, s1, done, cur)
    FrameStoreModel(6, 4, 16, 4, 3).push_step(t.ring, s0, s1, done, cur)
