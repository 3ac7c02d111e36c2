"""The device PPO actors (csrc/ppo_actor.hpp, reth_amd/ppo_actors.VecPpoActors) on the GPU: acting
against rth_ppo_act on the documented draws, the dynamics against the classic-control actors and
the host CartPole, the rollout's finish and carry against ppo_actors.HostRollout, determinism,
position independence / the grid-stride loop, buffer bounds and the argument checks.

N in {1, 9, 64}: 9 crosses a tile of 8 rows.  Segments here have cap <= 47 rows and the policies
spread their probabilities; segments past one pass of the finish's 256 lanes (cap 399 and 4096), ragged
counts over 600 envs and a saturated actor are in test_ppo_edges_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SEED = 0x1234ABCD5678
H = 64
ENVS = ["CartPole-v0", "Acrobot-v1", "MountainCar-v0"]
SHAPE = {"CartPole-v0": (4, 2, 4), "Acrobot-v1": (6, 3, 4), "MountainCar-v0": (2, 3, 2)}  # D, A, state columns
GAMMA = 0.99
# every device buffer of an actor set
NAMES = ["state", "ep_steps", "t_dev", "stats", "ret_stats", "cur_obs", "last_action", "last_logprob", "seg_s", "seg_a",
         "seg_r", "seg_done", "seg_logp", "fill", "gen", "dropped", "_complete", "n_dev"]


def _solver(env, seed=0):
    from reth_amd.ppo import PPOSolver
    from reth_amd.solver import Box, Discrete

    D, A, _ = SHAPE[env]
    torch.manual_seed(seed)
    s = PPOSolver(Box(-1, 1, (D,)), Discrete(A), device="cuda", impl="hip")
    with torch.no_grad():
        s.actor_network.action_layer[4].weight.mul_(4.0)  # the probabilities spread
    return s


@pytest.fixture(scope="module")
def solvers(dev):
    return {env: _solver(env) for env in ENVS}


def _actors(env, n, horizon=8, cls=None, **kw):
    from reth_amd.ppo_actors import VecPpoActors

    kw.setdefault("seed", SEED)
    kw.setdefault("max_episode_steps", 8)
    return (cls or VecPpoActors)(env, n, horizon, device="cuda", **kw)


def _states(env, n, rng):
    if env == "CartPole-v0":
        return rng.uniform(-0.15, 0.15, (n, 4))
    if env == "Acrobot-v1":
        return rng.uniform(-1.0, 1.0, (n, 4))
    return np.stack([rng.uniform(-1.0, 0.4, n), rng.uniform(-0.05, 0.05, n)], 1)


def _ppo_act(solver, obs, seed=0, counter=0, uniforms=None):
    """rth_ppo_act on dense rows -> (action, logprob)"""
    from reth_amd import _lib

    obs = obs.contiguous()
    n, D = obs.shape
    A = solver.dims[2]
    action = torch.full((n,), -7, dtype=torch.int64, device=obs.device)
    logprob = torch.full((n,), float("nan"), device=obs.device)
    _lib.call("rth_ppo_act", solver._arrays()["actor"], obs.data_ptr(), D, n, D, H, A,
              None if uniforms is None else uniforms.data_ptr(), seed, counter, action.data_ptr(), logprob.data_ptr(),
              None, _lib.stream_ptr())
    return action, logprob


def _bits(t):
    return t.cpu().numpy().tobytes()


def _snapshot(act):
    torch.cuda.synchronize()
    snap = {k: getattr(act, k).clone() for k in NAMES}
    snap.update({f"batch{j}": b.clone() for j, b in enumerate(act.batch)})
    return snap


def _same(a, b):
    for k in a:
        assert _bits(a[k]) == _bits(b[k]), k


# ---------------------------------------------------------------------------- acting
@pytest.mark.parametrize("t0", [0, 1_000_000])
@pytest.mark.parametrize("n", [1, 9, 64])
def test_acting_is_rth_ppo_act_on_the_documented_draw(solvers, n, t0):
    """last_action / last_logprob equal rth_ppo_act(current_obs, seed, counter = t) bit for bit"""
    for env in ("CartPole-v0", "Acrobot-v1"):
        solver = solvers[env]
        act = _actors(env, n)
        act.set_state(_states(env, n, np.random.default_rng(n)))
        act.t_dev.fill_(t0)
        for k in range(2):
            obs = act.current_obs()
            act.step(solver)
            a, lp = _ppo_act(solver, obs, SEED, t0 + 1 + k)
            assert _bits(act.last_action) == _bits(a) and _bits(act.last_logprob) == _bits(lp), (env, k)
            assert int(a.min()) >= 0 and torch.isfinite(lp).all()
        assert (act.t_dev == t0 + 2).all()


@pytest.mark.parametrize("n", [1, 9, 64])
def test_injected_uniforms_and_actions(solvers, n):
    env = "Acrobot-v1"
    solver, A = solvers[env], SHAPE[env][1]
    rng = np.random.default_rng(10 + n)
    st = _states(env, n, rng)
    act = _actors(env, n)
    act.set_state(st)
    obs = act.current_obs()
    u = torch.as_tensor(rng.random(n), device="cuda")
    act.step(solver, uniforms=u)
    a, lp, probs = solver.act_batch(obs, uniforms=u, return_probs=True)
    assert _bits(act.last_action) == _bits(a) and _bits(act.last_logprob) == _bits(lp)
    # a forced action: the stored log-probability is that action's (a uniform inside its CDF interval draws it)
    forced = torch.as_tensor(rng.integers(0, A, n), device="cuda")
    c = torch.cat([torch.zeros(n, 1, device="cuda", dtype=torch.float64), probs.double().cumsum(1)], 1)
    mid = ((c.gather(1, forced[:, None]) + c.gather(1, forced[:, None] + 1)) / 2)[:, 0].contiguous()
    a2, lp2 = solver.act_batch(obs, uniforms=mid)
    assert _bits(a2) == _bits(forced)
    act.set_state(st)
    act.step(solver, action_in=forced)
    assert _bits(act.last_action) == _bits(forced) and _bits(act.last_logprob) == _bits(lp2)
    assert _bits(act.seg_a[:, 1]) == _bits(forced) and _bits(act.seg_logp[:, 1]) == _bits(lp2)
    assert _bits(act.seg_s[:, 1]) == _bits(obs) and (act.fill == 2).all()


# ---------------------------------------------------------------------------- dynamics
@pytest.mark.parametrize("env", ENVS)
def test_dynamics_and_reset_equal_the_classic_control_actors(solvers, env):
    """the same seed and action_in sequence, 40 steps, a time limit of 8: state, ep_steps, stats and
    return statistics equal VecMlpActors' bit for bit (one env_dynamics / env_reset_draw)"""
    from reth_amd import model
    from reth_amd.mlp_actors import VecMlpActors

    D, A, _ = SHAPE[env]
    N = 9
    net = model.MLP_DQNNetwork((D,), A).to("cuda").requires_grad_(False)
    ref = VecMlpActors(env, N, seed=SEED, max_episode_steps=8, device="cuda")
    act = _actors(env, N, horizon=40)
    assert _bits(act.state) == _bits(ref.state)  # the reset is the documented draw
    assert _bits(act.current_obs()) == _bits(ref.current_obs())
    rng = np.random.default_rng(2)
    for t in range(40):
        a = torch.as_tensor(rng.integers(0, A, N), device="cuda")
        ref.step(net, a)
        act.step(solvers[env], action_in=a)
        for k in ("state", "ep_steps", "stats", "ret_stats", "t_dev"):
            assert _bits(getattr(act, k)) == _bits(getattr(ref, k)), (t, k)
        assert _bits(act.current_obs()) == _bits(ref.current_obs()), t
        assert _bits(act.seg_r[:, t]) == _bits(ref.reward) and _bits(act.seg_done[:, t]) == _bits(ref.done), t
    assert int(act.stats[:, 0].min()) >= 5 and (act.fill == 40).all() and int(act.dropped.sum()) == 0
    assert (act.cur_obs[:, D:] == 0).all()  # the pad floats


def test_cartpole_rows_match_the_host_env(solvers):
    """the rows (s0, r, done) against envs.make_host("CartPole-v0") stepped with the same actions from
    the device's states, by test_classic_actors_gpu.py's criterion: rewards and done flags exact,
    the observation within one f32 spacing of float32(host observation), a running episode's fp64
    state within 1e-12 max(1, |v|)"""
    from reth_amd import envs

    N, T = 9, 40
    act = _actors("CartPole-v0", N, horizon=T)
    rng = np.random.default_rng(4)
    st = _states("CartPole-v0", N, rng)
    st[:3, 2], st[:3, 3] = 0.2, 1.0  # about to fall
    act.set_state(st)
    worst = 0.0
    for t in range(T):
        before, steps = act.state.cpu().numpy(), act.ep_steps.cpu().numpy()
        a = rng.integers(0, 2, N)
        act.step(solvers["CartPole-v0"], action_in=torch.as_tensor(a, device="cuda"))
        after = act.state.cpu().numpy()
        s0, r, done = (getattr(act, k)[:, t].cpu().numpy() for k in ("seg_s", "seg_r", "seg_done"))
        for i in range(N):
            h = envs.make_host("CartPole-v0")
            h.max_episode_steps = 8
            h.state, h._t = tuple(before[i]), int(steps[i])
            o, hr, hd, _ = h.step(int(a[i]))
            want0 = before[i].astype(np.float32)
            assert (np.abs(s0[i] - want0) <= np.spacing(np.abs(want0))).all()
            assert r[i] == np.float32(hr) and bool(done[i]) == bool(hd), (t, i)
            if not hd:
                hs = np.asarray(h.state)
                worst = max(worst, float((np.abs(after[i] - hs) / np.maximum(1.0, np.abs(hs))).max()))
    print(f"CartPole env-step max |device - host| / max(1, |host|): {worst:.3e}")
    assert worst <= 1e-12
    assert int(act.stats[:, 0].sum()) >= N * 4


# ---------------------------------------------------------------------------- finish against HostRollout
def _load_host(act, host):
    """the device segments into a HostRollout"""
    for k in ("seg_s", "seg_a", "seg_r", "seg_done", "seg_logp", "fill", "dropped"):
        getattr(host, k)[...] = getattr(act, k).cpu().numpy().reshape(getattr(host, k).shape)
    host.complete[...] = act.complete.cpu().numpy()


def _check_finish(act, host, label, gamma=GAMMA):
    """one finish on both; returns the largest |ret| difference in fp32 ulps"""
    for b in act.batch:
        b.fill_(-77)
    (s, a, ret, lp), n_dev = act.finish(gamma)
    hs, ha, hret, hlp, n = host.finish(gamma)
    assert int(n_dev) == n, label
    assert _bits(s[:n]) == hs.tobytes() and _bits(a[:n]) == ha.tobytes() and _bits(lp[:n]) == hlp.tobytes(), label
    got = ret[:n].cpu().numpy()
    ulps = float((np.abs(got.astype(np.float64) - hret) / np.spacing(np.abs(hret)).astype(np.float64)).max()) if n else 0.0
    assert np.isfinite(got).all() and ulps <= 1.0, (label, ulps)
    for b in act.batch:  # rows at n and beyond are left as they were
        assert (b[n:] == -77).all(), label
    assert _bits(act.fill) == host.fill.tobytes() and _bits(act.complete) == host.complete.tobytes(), label
    for i in range(act.N):
        k = int(host.fill[i])
        for name in ("seg_s", "seg_a", "seg_r", "seg_done", "seg_logp"):
            assert _bits(getattr(act, name)[i, :k]) == getattr(host, name)[i, :k].tobytes(), (label, i, name)
    return ulps


def test_finish_on_handwritten_segments(solvers):
    """cap = 12; one env per case: (fill, done rows).  s, a, logp, n, the row order, the new fill /
    complete and the moved rows are exact; ret may differ by 1 fp32 ulp (the same fp64 operations in
    the same order, then one rounding) and is in fact 0 ulps off on an MI355X, here and across the
    carried rollouts below."""
    from reth_amd.ppo_actors import HostRollout

    cases = [(5, []),            # no done
             (4, [0]),           # a done at row 0
             (6, [5]),           # a done at the last stored row
             (9, [1, 4, 5]),     # three episodes (2, 3 and 1 rows) plus a tail of 3
             (12, [4, 11]),      # a full segment of whole episodes
             (10, [1]),          # m - e = 8 > e = 2: the move overlaps
             (0, []),            # nothing stored
             (12, [2])]          # a full segment, 9 rows carried over 3
    N = len(cases)
    act = _actors("Acrobot-v1", N, horizon=5)
    assert act.cap == 12
    g = torch.Generator().manual_seed(0)
    act.seg_s.copy_(torch.randn(act.seg_s.shape, generator=g))
    act.seg_a.copy_(torch.randint(0, 3, act.seg_a.shape, generator=g))
    act.seg_r.copy_(torch.randn(act.seg_r.shape, generator=g))
    act.seg_logp.copy_(-torch.rand(act.seg_logp.shape, generator=g))
    for i, (fill, dones) in enumerate(cases):
        act.fill[i] = fill
        for t in dones:
            act.seg_done[i, t] = 1.0
        act._complete[0, i] = dones[-1] + 1 if dones else 0
    host = HostRollout(N, 12, 6)
    _load_host(act, host)
    ulps = _check_finish(act, host, "first")
    print(f"finish: max |ret - HostRollout| = {ulps} fp32 ulps")
    assert host.fill.tolist() == [5, 3, 0, 3, 0, 8, 0, 9] and int(act.n_dev) == 1 + 6 + 6 + 12 + 2 + 3
    assert (act.gen == 1).all()
    # a second finish at once: nothing is complete, nothing moves
    before = _snapshot(act)
    assert _check_finish(act, host, "second") == 0.0 and int(act.n_dev) == 0
    for k in ("seg_s", "seg_a", "seg_r", "seg_done", "seg_logp", "fill"):
        assert _bits(getattr(act, k)) == _bits(before[k]), k
    # the carried episodes end: their rows come out with the new ones behind them
    for i in (0, 3, 5):
        f = int(act.fill[i])
        act.seg_done[i, f] = 1.0
        act.seg_done[i, :f] = 0.0
        act.fill[i] = f + 1
        act._complete[0, i] = f + 1  # gen = 2: slot 0 is live again
    _load_host(act, host)
    _check_finish(act, host, "third")
    assert int(act.n_dev) == 6 + 4 + 9


@pytest.mark.parametrize("n", [1, 9, 64])
def test_two_rollouts_agree_with_host_rollout_across_the_carry(solvers, n):
    """two rollouts of 8 steps with a time limit of 8; some envs start about to fall, so their next
    episode is still running at the boundary and is carried"""
    from reth_amd.ppo_actors import HostRollout

    env = "CartPole-v0"
    act = _actors(env, n, horizon=8)
    st = _states(env, n, np.random.default_rng(n))
    st[::2, 2], st[::2, 3] = 0.2, 1.5
    act.set_state(st)
    host = HostRollout(n, act.cap, 4)
    carried = 0
    for rollout in range(2):
        for _ in range(8):
            obs, run0 = act.current_obs().cpu().numpy(), act.ret_stats[:, 0].cpu().numpy()
            act.step(solvers[env])
            done = act.ep_steps.cpu().numpy() == 0
            run, _, last = (t.cpu().numpy() for t in act.return_stats())
            r = np.where(done, last, run) - run0
            host.store(obs, act.last_action.cpu().numpy(), r, done, act.last_logprob.cpu().numpy())
        assert _bits(act.fill) == host.fill.tobytes() and _bits(act.complete) == host.complete.tobytes()
        _check_finish(act, host, rollout)
        carried += int(host.fill.sum())
    assert carried > 0 and int(act.dropped.sum()) == 0


# ---------------------------------------------------------------------------- determinism
def _run(env, n, solver, steps=10, first=None):
    act = _actors(env, n, horizon=steps) if first is None else first
    act.reset()
    act.set_state(_states(env, n, np.random.default_rng(1)))
    for _ in range(steps):
        act.step(solver)
    act.finish(GAMMA)
    return act


def test_twenty_repetitions_are_bit_identical(solvers):
    env = "Acrobot-v1"
    act = _run(env, 9, solvers[env])
    first = _snapshot(act)
    assert int(first["n_dev"]) >= 9
    for _ in range(19):
        _same(first, _snapshot(_run(env, 9, solvers[env], first=act)))


def test_position_independence_grid_stride_and_single_env(solvers):
    """envs 0..8 of N = 8 * 1024 + 9 (1026 tiles > the 1024-workgroup grid: the grid-stride loop)
    equal an N = 9 run after 3 steps and a finish, with the same states injected by index (the draws
    are functions of the env index); N = 1 equals env 0 of N = 64"""
    env = "CartPole-v0"
    NB = 8 * 1024 + 9
    st = _states(env, NB, np.random.default_rng(9))
    sets = [_actors(env, n, horizon=3, max_episode_steps=2) for n in (NB, 64, 9, 1)]
    for act in sets:
        act.set_state(st[:act.N])
    per_env = ["state", "ep_steps", "t_dev", "stats", "cur_obs", "last_action", "last_logprob", "seg_s", "seg_a",
               "seg_r", "seg_done", "seg_logp", "fill"]
    for t in range(3):
        for act in sets:
            act.step(solvers[env])
        for k in per_env:
            big, mid, small, one = (getattr(act, k) for act in sets)
            assert _bits(big[:9]) == _bits(small) and _bits(mid[:9]) == _bits(small), (t, k)
            assert _bits(mid[:1]) == _bits(one), (t, k)
        assert _bits(sets[0].complete[:9]) == _bits(sets[2].complete)
    big = sets[0]
    assert (big.t_dev == 3).all() and (big.stats[:, 0] == 1).all() and (big.fill == 3).all()
    outs = [act.finish(GAMMA) for act in sets]
    n9 = int(outs[2][1])
    assert n9 == 18 and int(outs[0][1]) == 2 * NB and int(outs[3][1]) == 2
    for j in range(4):  # env-major: the first envs' rows come first
        assert _bits(outs[0][0][j][:n9]) == _bits(outs[2][0][j][:n9]), j
        assert _bits(outs[1][0][j][:2]) == _bits(outs[3][0][j][:2]), j
    assert (big.fill == 1).all() and (big.complete == 0).all()


# ---------------------------------------------------------------------------- bounds
def test_no_write_outside_any_buffer(solvers):
    from reth_amd.ppo_actors import VecPpoActors

    G = 64

    class Guarded(VecPpoActors):
        def _alloc(self, shape, dtype):
            n = int(np.prod(shape))
            canary = 12345.5 if dtype.is_floating_point else 0x5A5A5A5A
            buf = torch.full((n + 2 * G,), canary, dtype=dtype, device=self.device)
            buf[G:G + n] = 0
            self.__dict__.setdefault("_guarded", []).append((buf, n, canary))
            return buf[G:G + n].view(shape)

    def intact(act):
        torch.cuda.synchronize()
        for buf, n, canary in act._guarded:
            assert (buf[:G] == canary).all() and (buf[G + n:] == canary).all(), (buf.dtype, n)

    env = "Acrobot-v1"
    act = _actors(env, 9, horizon=8, cls=Guarded)
    assert len(act._guarded) == len(NAMES) + 4  # every device buffer of the set, and the batch's four
    for _ in range(2):
        for _ in range(8):
            act.step(solvers[env])
        act.finish(GAMMA)
    assert (act.t_dev == 16).all() and int(act.dropped.sum()) == 0 and int(act.n_dev) >= 9
    intact(act)
    # a segment that is too small: the same buffers seen as cap = 3 rows per env
    act.reset()
    act.cap = 3
    for _ in range(8):
        act.step(solvers[env])
    assert (act.fill == 3).all() and (act.dropped == 5).all() and (act.t_dev == 8).all()
    act.finish(GAMMA)
    assert int(act.n_dev) <= 9 * 3 and int(act.fill.max()) <= 3
    intact(act)


# ---------------------------------------------------------------------------- argument checks
def test_bad_arguments_are_refused_before_any_launch(solvers):
    from reth_amd import _lib

    ERR_INVALID = -1
    env = "CartPole-v0"
    solver = solvers[env]
    act = _actors(env, 9)
    act.step(solver)
    before = _snapshot(act)
    lib, s = _lib.lib(), _lib.stream_ptr()

    def args(**kw):
        a = act._args(act._params(solver))
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    null_params = (_lib.c_vp * 6)(*([act._params_key[0]] * 5 + [None]))
    common = [dict(env=7), dict(env=-1), dict(D=6), dict(A=3), dict(H=128), dict(N=0), dict(N=-3), dict(N=1 << 31),
              dict(cap=0), dict(cap=-1), dict(cap=4097), dict(max_episode_steps=0)]
    common += [{k: None} for k in ("fill", "complete", "gen", "dropped")]
    state = [dict(cur_obs=act.cur_obs.data_ptr() + 4)] + [{k: None} for k in ("state", "ep_steps", "t_dev", "stats",
                                                                                  "ret_stats", "cur_obs")]
    seg = [{k: None} for k in ("seg_s", "seg_a", "seg_r", "seg_done", "seg_logp")]
    step_only = [dict(actor=null_params), dict(actor=_lib.ctypes.POINTER(_lib.c_vp)()), dict(action=None),
                 dict(logprob=None)]
    for kw in common + state + seg + step_only:
        a = args(**kw)
        assert lib.rth_ppo_actor_step(_lib.ctypes.byref(a), s) == ERR_INVALID, kw
        assert b"rth_ppo_actor_step" in lib.rth_last_error(), kw
    for kw in common + state:
        a = args(**kw)
        assert lib.rth_ppo_env_reset(_lib.ctypes.byref(a), s) == ERR_INVALID, kw
        assert b"rth_ppo_env_reset" in lib.rth_last_error(), kw
    b = [t.data_ptr() for t in act.batch] + [act.n_dev.data_ptr()]
    for kw in common + seg:
        a = args(**kw)
        assert lib.rth_ppo_rollout_finish(_lib.ctypes.byref(a), GAMMA, *b, s) == ERR_INVALID, kw
        assert b"rth_ppo_rollout_finish" in lib.rth_last_error(), kw
    a = args()
    for j in range(5):
        assert lib.rth_ppo_rollout_finish(_lib.ctypes.byref(a), GAMMA, *[None if k == j else p for k, p in enumerate(b)],
                                          s) == ERR_INVALID, j
    assert lib.rth_ppo_rollout_finish(_lib.ctypes.byref(a), 1.5, *b, s) == ERR_INVALID
    assert lib.rth_ppo_actor_step(None, s) == ERR_INVALID and lib.rth_ppo_env_reset(None, s) == ERR_INVALID
    assert lib.rth_ppo_rollout_finish(None, GAMMA, *b, s) == ERR_INVALID
    with pytest.raises(ValueError, match="unknown env"):
        _actors("Pendulum-v0", 3)
    with pytest.raises(ValueError, match="actors run"):
        act._params_key = None
        act.step(solvers["Acrobot-v1"])
    with pytest.raises(ValueError, match="action_in"):
        act.step(solver, action_in=torch.zeros(9, device="cuda"))
    with pytest.raises(ValueError, match="uniforms"):
        act.step(solver, uniforms=torch.zeros(9, device="cuda"))
    _same(before, _snapshot(act))  # nothing ran
