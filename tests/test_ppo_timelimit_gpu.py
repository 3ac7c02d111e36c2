"""Bootstrapping device PPO's GAE through time-limit episode ends, on the GPU: rth_ppo_actor_step_tl
(csrc/ppo_actor.hpp) against the host envs and against rth_ppo_actor_step, rth_ppo_gae_finish_tl
against ppo_actors.gae on the kernel's own values and against rth_ppo_gae_finish, bounds / counters /
determinism / argument checks, PpoLoop with bootstrap_time_limit as the composition of its parts and
as a replayed graph, that it learns CartPole-v0 at 64 envs x 32 steps, and the example.

The step's tables are tests/_ppo_timelimit.py's (test_ppo_timelimit_cpu.py checks that they hold rows
of every kind); the finish's segments are test_ppo_gae_gpu.py's -- N = 37 envs at cap 12 with ragged
fills 0..12, one env at cap 300 and one at cap 4096 -- with truncation flags on top."""
import os
import runpy
import sys

import numpy as np
import pytest
import torch

from _ppo_edges import COLUMNS
from _ppo_timelimit import COLUMNS as STATE_COLUMNS
from _ppo_timelimit import LIMITS, SIZES, host_step, learn, step_table
from conftest import ROOT
from reth_amd import _lib
from reth_amd.ppo import PPOSolver, _params6
from reth_amd.ppo_actors import HostRollout, VecPpoActors
from reth_amd.solver import Box, Discrete
from test_ppo_actors_gpu import ENVS, NAMES, SEED, SHAPE, _solver
from test_ppo_gae_gpu import ENV, D, _bits, _dones, _load, _ragged_cases, _ulps, _value_net, _values

pytestmark = pytest.mark.gpu

NAN = float("nan")
G = 64  # guard elements around every buffer
TL = ("seg_trunc", "seg_term_s")


class Guarded(VecPpoActors):
    """every device buffer between two runs of NaN (integers: a canary)"""

    def _alloc(self, shape, dtype):
        n = int(np.prod(shape))
        canary = NAN if dtype.is_floating_point else 0x5A5A5A5A
        buf = torch.full((n + 2 * G,), canary, dtype=dtype, device=self.device)
        buf[G:G + n] = 0
        self.__dict__.setdefault("_guarded", []).append((buf, n))
        return buf[G:G + n].view(shape)

    def intact(self):
        torch.cuda.synchronize()
        for buf, n in self._guarded:
            for band in (buf[:G], buf[G + n:]):
                assert (torch.isnan(band) if buf.dtype.is_floating_point else band == 0x5A5A5A5A).all(), (buf.dtype, n)


@pytest.fixture(scope="module")
def solvers(dev):
    return {env: _solver(env) for env in ENVS}


@pytest.fixture(scope="module")
def value_nets(dev):
    return {1: _value_net(1.0), 256: _value_net(256.0)}


def _pair(env, n, limit, cap, cls=VecPpoActors):
    """two actor sets from the same start, the second without the option"""
    st, actions = step_table(env, n, limit)
    kw = dict(seed=SEED, max_episode_steps=limit, cap=cap, device="cuda")
    tl, base = cls(env, n, cap, time_limit_bootstrap=True, **kw), VecPpoActors(env, n, cap, **kw)
    for act in (tl, base):
        act.set_state(st)
    tl.seg_term_s.fill_(NAN)
    return tl, base, actions


def _drive(env, k, actions, rng, n):
    """the step's keywords: forced actions (CartPole, MountainCar) or uniforms (Acrobot)"""
    if env == "Acrobot-v1":
        return dict(uniforms=torch.as_tensor(rng.random(n), device="cuda"))
    return dict(action_in=torch.as_tensor(actions[k], dtype=torch.int64, device="cuda"))


# ---------------------------------------------------------------------------- the step
@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("env", ENVS)
def test_step_records_the_cause_and_the_final_observation(solvers, env, n, limit):
    """limit + 3 steps from the table's states.  Each step is replayed per env on the host env from
    the device's own fp64 state: seg_trunc equals the host's (time limit reached and not terminal)
    exactly -- so a both-causes row has trunc 0 -- and a truncated row's seg_term_s is within one f32
    spacing of float32(the host's observation after the step), test_classic_actors_gpu's bound for the
    step's observation; the other seg_term_s rows keep their NaN.  HostRollout, fed those host rows,
    ends with the device's flags.  Every buffer the step had before equals rth_ppo_actor_step's from
    the same start, bit for bit, after every step."""
    Dd = SHAPE[env][0]
    T = limit + 3
    tl, base, actions = _pair(env, n, limit, T)
    host = HostRollout(n, T, Dd)
    rng = np.random.default_rng(n + limit)
    kinds = np.zeros(4, np.int64)
    for k in range(T):
        before, steps = tl.state.cpu().numpy(), tl.ep_steps.cpu().numpy()
        obs0 = tl.current_obs().cpu().numpy()
        kw = _drive(env, k, actions, rng, n)
        tl.step(solvers[env], **kw)
        base.step(solvers[env], **kw)
        for name in NAMES:
            assert _bits(getattr(tl, name)) == _bits(getattr(base, name)), (k, name)
        a = tl.last_action.cpu().numpy()
        rows = [host_step(env, before[i][:STATE_COLUMNS[env]], steps[i], a[i], limit) for i in range(n)]
        done, terminal = np.array([r[2] for r in rows]), np.array([r[3] for r in rows])
        trunc = done & ~terminal
        limited = steps + 1 >= limit
        kinds += np.bincount(terminal + 2 * limited, minlength=4)
        host.store(obs0, a, [r[1] for r in rows], done, tl.last_logprob.cpu().numpy(), trunc=trunc,
                   term_s=np.stack([r[0] for r in rows]))
        got_trunc, got_term = tl.seg_trunc[:, k].cpu().numpy(), tl.seg_term_s[:, k].cpu().numpy()
        assert np.array_equal(tl.seg_done[:, k].cpu().numpy(), done.astype(np.float32)), k
        assert np.array_equal(got_trunc, trunc.astype(np.float32)), (k, got_trunc, trunc)
        assert (got_trunc[terminal & limited] == 0).all()  # both causes: terminal
        want = host.seg_term_s[:, k]
        assert np.isnan(got_term[~trunc]).all() and np.isnan(want[~trunc]).all(), k
        assert (np.abs(got_term[trunc] - want[trunc]) <= np.spacing(np.abs(want[trunc]))).all(), k
    assert _bits(tl.seg_trunc) == host.seg_trunc.tobytes() and _bits(tl.fill) == host.fill.tobytes()
    assert _bits(tl.seg_done) == host.seg_done.tobytes() and _bits(tl.seg_a) == host.seg_a.tobytes()
    assert int(tl.dropped.sum()) == 0 and (tl.fill == T).all() and base.seg_trunc is None
    # the table was not empty where it matters (CartPole: test_ppo_timelimit_cpu checks its first episodes)
    if env == "CartPole-v0":
        assert kinds[3] >= 1, kinds  # env 0 falls on the limit's step
    if n >= 9:
        assert kinds[2] >= n - 3 and (limit == 1 or (kinds[0] > 0 and kinds[1] >= 2)), kinds


@pytest.mark.parametrize("env", ENVS)
def test_a_dropped_row_writes_neither_column(solvers, env):
    """cap 3 under 8 steps at a limit of 2 (truncated rows at every second step): the rows of the
    first 3 steps are a cap-8 run's, the 5 dropped ones write nothing -- the NaN bands around both
    columns and the NaN rows of steps that were not truncated are intact"""
    n, limit = 9, 2
    small, base, actions = _pair(env, n, limit, 3, cls=Guarded)
    full, _, _ = _pair(env, n, limit, 8)
    rng_a, rng_b = np.random.default_rng(0), np.random.default_rng(0)
    actions = np.concatenate([actions, actions])[:8]
    for k in range(8):
        small.step(solvers[env], **_drive(env, k, actions, rng_a, n))
        full.step(solvers[env], **_drive(env, k, actions, rng_b, n))
    small.intact()
    assert (small.fill == 3).all() and (small.dropped == 5).all() and (full.fill == 8).all()
    assert _bits(small.seg_trunc) == _bits(full.seg_trunc[:, :3].contiguous())
    got, want = small.seg_term_s.cpu().numpy(), full.seg_term_s[:, :3].cpu().numpy()
    assert got.tobytes() == want.tobytes()  # NaN rows included
    trunc = small.seg_trunc.cpu().numpy() == 1
    assert trunc.sum() >= n - 2 and np.isnan(got[~trunc]).all() and np.isfinite(got[trunc]).all()
    for name in ("state", "t_dev", "stats", "cur_obs"):  # the env still steps
        assert _bits(getattr(small, name)) == _bits(getattr(full, name)), name


# ---------------------------------------------------------------------------- the finish
def _truncs(pattern, fills, cap, dones, seed=0):
    """float32 [N, cap] truncation flags and the done flags that go with them"""
    N = len(fills)
    tr, dn = np.zeros((N, cap), np.float32), dones.copy()
    rng = np.random.default_rng(seed + 17)
    if pattern == "every done":
        tr[:] = dn
    elif pattern == "random":  # some done rows, and a few rows that are not done (the selects take them too)
        tr[:] = ((dn == 1) & (rng.random((N, cap)) < 0.5)) | (rng.random((N, cap)) < 0.1)
    elif pattern == "last":
        for i, f in enumerate(fills):
            if f:
                tr[i, f - 1] = dn[i, f - 1] = 1.0
    elif pattern == "7 and 8":  # across the forward's tile edge
        tr[:, 7:9] = dn[:, 7:9] = 1.0
    elif pattern == "counts":  # 0, 1, 8 or 9 truncated rows per env: at and across one tile of the list
        for i, f in enumerate(fills):
            k = min((0, 1, 8, 9)[i % 4], f)
            rows = rng.choice(f, k, replace=False) if k else []
            tr[i, rows] = dn[i, rows] = 1.0
    elif pattern == "all":
        tr[:], dn[:] = 1.0, 1.0
    else:
        assert pattern == "none"
    return tr, dn


def _load_tl(act, cases, cap, dones, trunc, seed=0, poison=True):
    """test_ppo_gae_gpu._load plus the flags and random final observations -- NaN where trunc is 0"""
    seg = _load(act, cases, cap, dones, seed=seed)
    g = torch.Generator().manual_seed(200 + seed)
    term = torch.randn((act.N, cap, D), generator=g)
    seg["seg_trunc"], seg["term_clean"] = torch.as_tensor(trunc), term.clone()
    if poison:
        term[seg["seg_trunc"] == 0] = NAN
    seg["seg_term_s"] = term
    act.seg_trunc.copy_(seg["seg_trunc"])
    act.seg_term_s.copy_(term)
    return seg


def _finish_and_check(act, value, seg, gamma, lam, label):
    """one finish_gae with the flags; adv / ret against gae(trunc, v_term) on the kernel's own values:
    v from this call's batch_v, v_last and v_term from the same kernel's batch_v of further calls
    whose seg_s rows are cur_obs and the final observations.  Returns (the outputs, the ulps)."""
    fills = seg["fill"].numpy()
    n = int(fills.sum())
    v_last = _values(value, act.cur_obs[:, :D].contiguous()).cpu().numpy()
    v_term = _values(value, seg["term_clean"].reshape(-1, D).to("cuda")).cpu().numpy().reshape(act.N, act.cap)
    if act.batch_adv is None:
        act.finish_gae(value, 0.5, 0.5)
    for k in COLUMNS + ("fill",) + TL:
        getattr(act, k).copy_(seg[k])
    act._complete.fill_(3)
    gen0, dropped0 = act.gen.clone(), act.dropped.clone()
    for b in act.batch + [act.batch_adv, act.batch_v]:
        b.fill_(-77)
    act.n_dev.fill_(-5)
    (s, a, ret, lp, adv), n_dev = act.finish_gae(value, gamma, lam)
    assert int(n_dev) == n, label
    host = HostRollout(act.N, act.cap, D)
    for k in COLUMNS + ("fill", "seg_trunc"):
        getattr(host, k)[...] = seg[k].numpy()
    vseg, off = np.zeros((act.N, act.cap), np.float32), 0
    vn = act.batch_v[:n].cpu().numpy()
    for i, f in enumerate(fills):
        vseg[i, :f] = vn[off:off + f]
        off += f
    hs, ha, hret, hlp, hadv, hn = host.finish_gae(vseg, v_last, gamma, lam, v_term=v_term)
    assert hn == n
    assert _bits(s[:n]) == hs.tobytes() and _bits(a[:n]) == ha.tobytes() and _bits(lp[:n]) == hlp.tobytes(), label
    got_adv, got_ret = adv[:n].cpu().numpy(), ret[:n].cpu().numpy()
    assert np.isfinite(got_adv).all() and np.isfinite(got_ret).all() and np.isfinite(vn).all(), label
    ulps = max(_ulps(got_adv, hadv), _ulps(got_ret, hret))
    assert ulps <= 1.0, (label, ulps)
    for b in act.batch + [act.batch_adv, act.batch_v]:  # rows at n and beyond are left as they were
        assert (b[n:] == -77).all(), label
    assert (act.fill == 0).all() and (act._complete == 0).all() and _bits(act.gen) == _bits(gen0 + 1), label
    assert _bits(act.dropped) == _bits(dropped0), label
    for k in COLUMNS + TL:  # the segments' rows are read, not written
        assert _bits(getattr(act, k)) == _bits(seg[k].to(getattr(act, k).dtype)), (label, k)
    return [t[:n].clone() for t in (s, a, ret, lp, adv, act.batch_v)], ulps


def _tl_actors(n, cap, cls=Guarded):
    return cls(ENV, n, cap, max_episode_steps=8, cap=cap, device="cuda", time_limit_bootstrap=True)


@pytest.mark.parametrize("pattern", ["none", "every done", "random", "last", "7 and 8", "counts"])
def test_scan_on_ragged_segments(value_nets, pattern):
    """N = 37, cap 12, ragged fills, done rows at random: gamma x lambda in {0, 0.99, 1} x {0, 0.95, 1}
    on the plain value network, (0.99, 0.95) on the scaled one.  The same fp64 operations in the same
    order as gae(): 0 ulps are expected and 1 is allowed (test_ppo_gae_gpu's rule)."""
    cases, cap = _ragged_cases(), 12
    fills = [f for f, _ in cases]
    act = _tl_actors(len(cases), cap)
    trunc, dones = _truncs(pattern, fills, cap, _dones("random", fills, cap))
    counts = sorted({int(trunc[i, :f].sum()) for i, f in enumerate(fills)})
    if pattern == "counts":
        assert {0, 1, 8, 9} <= set(counts), counts
    if pattern == "7 and 8":
        assert 2 in counts and 1 in counts  # fills of 8 hold row 7 alone
    worst = 0.0
    seg = _load_tl(act, cases, cap, dones, trunc, seed=1)
    for gamma in (0.0, 0.99, 1.0):
        for lam in (0.0, 0.95, 1.0):
            worst = max(worst, _finish_and_check(act, value_nets[1], seg, gamma, lam, (pattern, gamma, lam))[1])
    seg = _load_tl(act, cases, cap, dones, trunc, seed=256)
    worst = max(worst, _finish_and_check(act, value_nets[256], seg, 0.99, 0.95, (pattern, "scaled"))[1])
    act.intact()
    print(f"gae finish tl, truncation pattern {pattern!r} (rows per env {counts}): max |adv, ret - gae| = {worst} fp32 ulps")


@pytest.mark.parametrize("cap", [300, 4096])
def test_scan_on_one_long_segment(value_nets, cap):
    """one env with a full segment, every pattern, and with every one of its rows truncated: the
    compacted list is the whole segment (512 tiles at cap 4096)"""
    act = _tl_actors(1, cap)
    cases, worst = [(cap, [])], 0.0
    for pattern in ("none", "every done", "random", "last", "7 and 8", "all"):
        trunc, dones = _truncs(pattern, [cap], cap, _dones("random", [cap], cap, seed=cap), seed=cap)
        seg = _load_tl(act, cases, cap, dones, trunc, seed=cap)
        worst = max(worst, _finish_and_check(act, value_nets[1], seg, 0.99, 0.95, (cap, pattern))[1])
    assert trunc.sum() == cap
    worst = max(worst, _finish_and_check(act, value_nets[256], seg, 1.0, 1.0, (cap, "all", "scaled"))[1])
    act.intact()
    print(f"gae finish tl, one env at cap {cap}: max |adv, ret - gae| = {worst} fp32 ulps")


def test_no_truncated_row_is_the_finish_without_the_option(value_nets):
    """trunc all zero and seg_term_s all NaN: every output of rth_ppo_gae_finish, bit for bit -- ragged
    at cap 12 and one env at cap 4096.  And with flags set, NaN in the seg_term_s rows whose trunc is 0
    changes no bit."""
    for cases, cap in ((_ragged_cases(), 12), ([(4096, [])], 4096)):
        fills = [f for f, _ in cases]
        dones = _dones("random", fills, cap, seed=cap)
        act, plain = _tl_actors(len(cases), cap), VecPpoActors(ENV, len(cases), cap, max_episode_steps=8, cap=cap, device="cuda")
        seg = _load_tl(act, cases, cap, dones, np.zeros_like(dones), seed=4)
        assert torch.isnan(act.seg_term_s).all()
        _load(plain, cases, cap, dones, seed=4)
        for gamma, lam in ((0.99, 0.95), (1.0, 1.0)):
            for x in (act, plain):
                for k in COLUMNS + ("fill",):
                    getattr(x, k).copy_(seg[k])
            got, want = act.finish_gae(value_nets[1], gamma, lam), plain.finish_gae(value_nets[1], gamma, lam)
            n = int(want[1])
            assert n == sum(fills) and int(got[1]) == n
            for x, y in zip(got[0] + [act.batch_v], want[0] + [plain.batch_v]):
                assert _bits(x[:n]) == _bits(y[:n]) and torch.isfinite(x[:n].float()).all()
            for k in ("fill", "gen", "_complete", "dropped"):
                assert _bits(getattr(act, k)) == _bits(getattr(plain, k)), k
        act.intact()
        # flags set: the rows that are not truncated hold NaN or numbers, the same bits
        trunc, dn = _truncs("random", fills, cap, dones)
        outs = []
        for poison in (True, False):
            seg = _load_tl(act, cases, cap, dn, trunc, seed=4, poison=poison)
            outs.append(_finish_and_check(act, value_nets[1], seg, 0.99, 0.95, (cap, "poison", poison))[0])
        assert trunc.sum() > 0 and (trunc == 0).sum() > 0
        for x, y in zip(*outs):
            assert _bits(x) == _bits(y)


def test_ten_repetitions_are_bit_identical_and_nothing_is_written_outside(value_nets):
    cases, cap = _ragged_cases(), 12
    fills = [f for f, _ in cases]
    act = _tl_actors(len(cases), cap)
    trunc, dones = _truncs("counts", fills, cap, _dones("random", fills, cap))
    first = None
    for rep in range(10):
        _load_tl(act, cases, cap, dones, trunc)
        act.n_dev.fill_(-5)
        (s, a, ret, lp, adv), n_dev = act.finish_gae(value_nets[1], 0.99, 0.95, normalize=True)
        out = [t.clone() for t in (s, a, ret, lp, adv, act.batch_v, n_dev)]
        first = out if first is None else first
        for x, y in zip(out, first):
            assert _bits(x) == _bits(y), rep
        assert (act.fill == 0).all() and (act._complete == 0).all() and (act.gen == rep + 1).all()
    assert act.finishes == 10 and act.normalizes == 10 and int(act.n_dev) == sum(fills)
    act.intact()
    # an empty rollout right behind it: n = 0, nothing written, the counters move as after the other finish
    for b in act.batch + [act.batch_adv, act.batch_v]:
        b.fill_(-77)
    act.finish_gae(value_nets[1], 0.99, 0.95)
    assert int(act.n_dev) == 0 and (act.gen == 11).all() and (act.fill == 0).all()
    for b in act.batch + [act.batch_adv, act.batch_v]:
        assert (b == -77).all()
    act.intact()


def test_steps_then_finish_agree_with_host_rollout(dev):
    """a real rollout: 7 steps of 9 CartPole envs under a time limit of 3 (truncated rows in every
    segment), the columns as the step leaves them, then the finish against HostRollout"""
    torch.manual_seed(2)
    solver = PPOSolver(Box(-1, 1, (4,)), Discrete(2), device=dev, impl="hip")
    act = VecPpoActors("CartPole-v0", 9, 7, seed=7, max_episode_steps=3, cap=7, device=dev, time_limit_bootstrap=True)
    for rollout in range(2):
        for _ in range(7):
            act.step(solver)
        host = HostRollout(9, 7, 4)
        for k in COLUMNS + ("fill",) + TL:
            getattr(host, k)[...] = getattr(act, k).cpu().numpy()
        assert host.seg_trunc.sum() >= 9 and (host.seg_trunc <= host.seg_done).all()
        cur = act.current_obs()
        term = torch.where(act.seg_trunc[..., None] == 1, act.seg_term_s, torch.zeros_like(act.seg_term_s))
        (s, a, ret, lp, adv), n_dev = act.finish_gae(solver, 0.99, 0.95)
        assert int(n_dev) == 63
        v_last = _values(solver, cur, "CartPole-v0").cpu().numpy()
        v_term = _values(solver, term.reshape(-1, 4).contiguous(), "CartPole-v0").cpu().numpy().reshape(9, 7)
        out = host.finish_gae(act.batch_v[:63].cpu().numpy().reshape(9, 7), v_last, 0.99, 0.95, v_term=v_term)
        assert max(_ulps(adv[:63].cpu().numpy(), out[4]), _ulps(ret[:63].cpu().numpy(), out[2])) <= 1.0
        assert (act.fill == 0).all() and (act.gen == rollout + 1).all()


def test_bad_arguments_are_refused_before_any_launch(value_nets):
    ERR_INVALID = -1
    cases, cap = _ragged_cases(), 12
    fills = [f for f, _ in cases]
    act = _tl_actors(len(cases), cap, cls=VecPpoActors)
    value = value_nets[1]
    act.finish_gae(value, 0.99, 0.95)  # the columns exist
    trunc, dones = _truncs("random", fills, cap, _dones("random", fills, cap))
    _load_tl(act, cases, cap, dones, trunc)
    bufs = act.batch + [act.batch_adv, act.batch_v]
    for b in bufs:
        b.fill_(-77)
    torch.cuda.synchronize()
    names = ("fill", "gen", "_complete", "n_dev", "dropped", "t_dev", "state") + COLUMNS + TL
    before = {k: getattr(act, k).clone() for k in names}
    lib, st = _lib.lib(), _lib.stream_ptr()
    vp = act._value_params(value)
    s, a, ret, lp = act.batch
    b = [s.data_ptr(), a.data_ptr(), ret.data_ptr(), act.batch_adv.data_ptr(), act.batch_v.data_ptr(), lp.data_ptr(),
         act.n_dev.data_ptr()]
    tl = [act.seg_trunc.data_ptr(), act.seg_term_s.data_ptr()]

    def args(**kw):
        x = act._args()
        for k, v in kw.items():
            setattr(x, k, v)
        return x

    def finish(x, gamma=0.99, lam=0.95, batch=b, cols=tl, value=vp):
        return lib.rth_ppo_gae_finish_tl(x if x is None else _lib.ctypes.byref(x), value, gamma, lam, *batch, *cols, st)

    for cols in ([None, tl[1]], [tl[0], None], [None, None]):  # NULL new pointers
        assert finish(args(), cols=cols) == ERR_INVALID and b"rth_ppo_gae_finish_tl" in lib.rth_last_error(), cols
    for gamma, lam in ((1.5, 0.95), (-0.1, 0.95), (0.99, 1.5), (0.99, -0.5), (NAN, 0.5), (0.5, NAN)):
        assert finish(args(), gamma, lam) == ERR_INVALID, (gamma, lam)
    for kw in (dict(cap=0), dict(cap=-1), dict(cap=4097), dict(env=7), dict(N=0), dict(seg_done=None), dict(cur_obs=None),
               dict(fill=None)):
        assert finish(args(**kw)) == ERR_INVALID and b"rth_ppo_gae_finish_tl" in lib.rth_last_error(), kw
    for j in range(7):
        assert finish(args(), batch=[None if k == j else p for k, p in enumerate(b)]) == ERR_INVALID, j
    assert finish(args(), value=None) == ERR_INVALID and finish(None) == ERR_INVALID
    # the step: NULL new pointers, a bad cap, the step's own checks
    solver = _solver(ENV)
    params = act._params(solver)

    def step(x, cols=tl):
        return lib.rth_ppo_actor_step_tl(x if x is None else _lib.ctypes.byref(x), *cols, st)

    good = act._args(params)
    for cols in ([None, tl[1]], [tl[0], None]):
        assert step(good, cols) == ERR_INVALID and b"rth_ppo_actor_step_tl" in lib.rth_last_error(), cols
    for kw in (dict(cap=0), dict(cap=4097), dict(actor=None), dict(max_episode_steps=0), dict(seg_s=None), dict(state=None)):
        x = act._args(params)
        for k, v in kw.items():
            setattr(x, k, v)
        assert step(x) == ERR_INVALID and b"rth_ppo_actor_step_tl" in lib.rth_last_error(), kw
    assert step(None) == ERR_INVALID
    torch.cuda.synchronize()
    for k, v in before.items():  # nothing ran
        assert _bits(getattr(act, k)) == _bits(v), k
    assert all(bool((t == -77).all()) for t in bufs)


# ---------------------------------------------------------------------------- the loop
def _loop(**kw):
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    kw = dict(dict(n_actors=9, horizon=5, max_episode_steps=3, seed=5, gae_lambda=0.95, bootstrap_time_limit=True), **kw)
    return PpoLoop(PpoLoopConfig(**kw), device="cuda", impl="hip")


def _same_params(a, b):
    for net in ("actor_network", "value_network"):
        for p, q in zip(_params6(getattr(a, net)), _params6(getattr(b, net))):
            assert _bits(p) == _bits(q), net


def _abi_calls(loop):
    act = loop.actors
    return act.launches + act.finishes + act.normalizes + loop.solver.hip_launches


ACTOR_BUFFERS = NAMES + ["batch_adv", "batch_v"] + list(TL)


@pytest.mark.parametrize("K", [1, 4])
@pytest.mark.parametrize("normalize", [False, True])
def test_the_loop_is_the_composition_of_its_parts(dev, normalize, K):
    """3 eager iterations at 9 envs x 5 steps under a time limit of 3 (truncated rows in every
    rollout): a second actor set stepped and finished by hand with the option and a second solver
    updated with update_device end with the loop's parameters and actor buffers, bit for bit; the
    ABI calls per iteration are the loop's as it was"""
    loop = _loop(normalize_adv=normalize, n_minibatches=K)
    cfg = loop.cfg
    assert loop.actors.cap == 5 and loop.actors.time_limit_bootstrap
    other = PPOSolver(Box(-1, 1, (4,)), Discrete(2), k_epochs=cfg.k_epochs, eps_clip=cfg.eps_clip,
                      learning_rate=cfg.learning_rate, device=dev, impl="hip", n_minibatches=K)
    other.sync_weights(loop.solver)
    other.seed = loop.solver.seed
    mine = VecPpoActors(cfg.env, 9, 5, seed=cfg.seed, max_episode_steps=3, cap=5, device=dev, time_limit_bootstrap=True)
    plain = VecPpoActors(cfg.env, 9, 5, seed=cfg.seed, max_episode_steps=3, cap=5, device=dev)
    differs = False
    for k in range(3):
        loop.iteration()
        for _ in range(5):
            mine.step(other)
            plain.step(other)
        assert int(mine.seg_trunc.sum()) >= 9
        batch, n_dev = mine.finish_gae(other, cfg.gamma, cfg.gae_lambda, normalize)
        old, _ = plain.finish_gae(other, cfg.gamma, cfg.gae_lambda, normalize)
        differs |= _bits(old[4]) != _bits(batch[4])
        n = int(n_dev)
        assert n == 45 and len(batch) == 5
        other.update_device([b[:n].clone() for b in batch])
        _same_params(loop.solver, other)
        for name in ACTOR_BUFFERS:
            assert _bits(getattr(loop.actors, name)) == _bits(getattr(mine, name)), (k, name)
        for x, y in zip(batch, loop.actors.batch + [loop.actors.batch_adv]):
            assert _bits(x) == _bits(y), k
    assert differs  # the option changed the advantages
    per_update = 3 * cfg.k_epochs if K == 1 else cfg.k_epochs * (1 + 3 * K)
    assert _abi_calls(loop) == 3 * (5 + 1 + int(normalize) + per_update)
    assert int(loop.actors.dropped.sum()) == 0 and (loop.actors.t_dev == 15).all()


@pytest.mark.parametrize("normalize", [False, True])
def test_captured_iterations_equal_eager_ones(dev, normalize):
    eager, graph = _loop(normalize_adv=normalize), _loop(normalize_adv=normalize)
    eager.run(4)
    graph.iteration()
    graph.capture()
    graph.run(3)
    torch.cuda.synchronize()
    _same_params(eager.solver, graph.solver)
    for k in ACTOR_BUFFERS:
        assert _bits(getattr(eager.actors, k)) == _bits(getattr(graph.actors, k)), k
    for x, y in zip(eager.actors.batch, graph.actors.batch):
        assert _bits(x) == _bits(y)
    for k in ("pushes", "launches", "finishes", "normalizes"):
        assert getattr(eager.actors, k) == getattr(graph.actors, k), k
    assert _abi_calls(eager) == _abi_calls(graph) == 4 * (5 + 1 + int(normalize) + 3 * eager.cfg.k_epochs)
    assert int(graph.actors.seg_trunc.sum()) >= 9 and int(graph.actors.n_dev) == 45


def test_refusals_and_the_default(dev):
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    with pytest.raises(ValueError, match="bootstrap_time_limit.*set gae_lambda"):
        _loop(gae_lambda=None, horizon=8)
    with pytest.raises(ValueError, match="the device envs are"):
        _loop(env="Pendulum-v0")
    with pytest.raises(RuntimeError, match="no torch fallback"):
        PpoLoop(PpoLoopConfig(gae_lambda=0.95, horizon=32, bootstrap_time_limit=True), device="cuda", impl="torch")
    for env in ("Acrobot-v1", "MountainCar-v0"):
        assert _loop(env=env).actors.seg_term_s.shape == (9, 5, SHAPE[env][0])
    # the default: neither buffer, the calls of before
    loop = _loop(bootstrap_time_limit=False)
    assert loop.actors.seg_trunc is None and loop.actors.seg_term_s is None and not loop.actors.time_limit_bootstrap
    loop.run(2)
    act = loop.actors
    assert (act.launches, act.finishes, act.normalizes, loop.solver.hip_launches) == (10, 2, 0, 2 * 3 * loop.cfg.k_epochs)


def test_it_learns_cartpole_with_the_bootstrap(dev):
    """CartPole-v0, 64 envs x 32 steps, lambda 0.95, normalised advantages, 50 iterations, seeds 0 / 1 /
    2, bootstrap_time_limit on, at the project's learning rate 0.01: the median of the envs' mean last
    finished episode length reaches the midpoint between the untrained actor's figure (measured here)
    and the limit of 200 -- test_ppo_gae_gpu.test_it_learns_cartpole_on_short_rollouts' criterion,
    unchanged.  Measured on an MI355X (profiles/r25/ppo_timelimit.txt): trained 194.8 / 155.8 / 195.8
    with the option beside 181.4 / 187.7 / 180.6 without it in the same session, untrained 22.0 / 26.3 /
    22.5: the median 194.8 against a midpoint of 111.2, so the other rates r24 measured were not needed.
    Reported, not asserted: the mean return target over the last rollout's truncated rows (5 / 2 / 14
    rows) is 88.7 / 51.4 / 90.7 with the bootstrap and 1.00 without -- the bias this removes."""
    trained, untrained, targets = learn(True)
    print(f"ppo_loop time-limit bootstrap CartPole-v0 64 x 32, 50 iterations, seeds 0/1/2: mean last finished length "
          f"{trained}, untrained {untrained}; mean ret on the last rollout's truncated rows (with the bootstrap, "
          f"without, rows) {targets}")
    mid = (float(np.median(untrained)) + 200.0) / 2
    assert max(untrained) < 60
    assert float(np.median(trained)) >= mid, (trained, untrained, mid)


# ---------------------------------------------------------------------------- the example
@pytest.mark.parametrize("graph", [False, True])
def test_example_runs_end_to_end(dev, graph, monkeypatch, capsys):
    path = os.path.join(ROOT, "examples", "cartpole_ppo_timelimit_hip.py")
    monkeypatch.setattr(sys, "argv", [path, "--updates", "3", "--seed", "1"] + (["--graph"] if graph else []))
    monkeypatch.setattr(sys, "path", list(sys.path))
    runpy.run_path(path, run_name="__main__")
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("cartpole_ppo_timelimit ")][-1]
    fields = dict(f.split("=") for f in line.split()[1:])
    assert fields["updates"] == "3" and fields["seed"] == "1" and fields["graph"] == str(int(graph))
    assert fields["env"] == "CartPole-v0" and fields["gae_lambda"] == "0.95" and fields["bootstrap_time_limit"] == "1"
    assert int(fields["env_steps"]) == 3 * 64 * 32 and int(fields["episodes"]) >= 64 and fields["dropped"] == "0"
    for k in ("mean_last_len", "untrained_mean_last_len"):
        assert 1 <= float(fields[k]) <= 200
    assert int(fields["hip_launches"]) == 3 * (32 + 1 + 1 + 3 * 4)
