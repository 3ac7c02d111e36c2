"""Vectorised PPO actors on one GPU, on the fused actor of csrc/ppo.hpp (csrc/ppo_actor.hpp).

Reference loop: reth/examples/ppo/run.py (examples/cartpole_ppo_hip.py here) with
algorithm/util.py:27-40: one host env; per env step one act with its copy back and an episode-buffer
append; on done the episode's discounted, normalised returns into the data buffer; every
UPDATE_INTERVAL steps one update on the data buffer -- complete episodes only -- while the rows of
the episode still running stay behind with their old log-probabilities.

Here N environments of one kind (CartPole-v0, Acrobot-v1 or MountainCar-v0: the dynamics, reset
draws and observation maps of csrc/env_actor.hpp) live in HBM.  step() is ONE launch for all of
them: the acting forward and log-softmax (rth_ppo_act's, bit for bit), one Categorical draw per env
from the Philox uniform of (seed, counter = the env's step count t, row = the env), the dynamics,
the time limit, the reset, and the row (s0, a, r, done, logp) appended to the env's rollout segment.
finish(gamma) is one launch too: per finished episode the reference's returns, the rows of all
finished episodes as one dense batch with a device row count, and the carry.  Nothing synchronises
with the host; every per-step scalar is device-resident, so a captured rollout replays.

Every env is its own worker: N envs each run their own copy of the reference's loop against the
one learner, which reads the learner's actor in place (the reference's sync_weights).  A batch holds
the envs' rows env-major, then in time order; the reference's single worker gives time order alone.

A segment holds cap = horizon + max_episode_steps - 1 rows: a rollout of `horizon` steps on top of a
carried episode, which has at most max_episode_steps - 1 rows.  So nothing is ever dropped
(`dropped` stays 0) as long as finish() follows every `horizon` steps.

finish_gae(value, gamma, lam) is the other estimator on the same segments: GAE(lambda) with the
value network's bootstrap at the rollout's edge (rth_ppo_gae_finish; gae() below is its scan).
Every stored row of every env enters the batch, with its advantage and its value as further
columns, and the segments are empty afterwards: there is no carry, so cap = horizon rows hold a
rollout (the keyword cap) and any horizon >= 1 runs.

time_limit_bootstrap=True keeps two more columns per segment -- seg_trunc (1 where the time limit
alone ended the row's episode) and seg_term_s (such a row's final observation, which the reset draw
has replaced in cur_obs by the time a finish runs) -- written by rth_ppo_actor_step_tl, and finish_gae
then bootstraps every truncated row from the value of the state it ended on
(rth_ppo_gae_finish_tl).  finish() does not read them.

HostRollout restates the store, the finishes and the carry in numpy with the kernel's arithmetic in
its order: the oracle of the GPU tests, testable without a GPU.
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .device_loop import VecEnvActors
from .ppo import _dims, _params6

H = 64  # the hidden width csrc/ppo.hpp builds
MAX_CAP = 4096  # rows per env (csrc/ppo_actor.hpp: kPpoMaxCap)

# env name -> (RTH_ENV_* id, obs_dim, num_actions, TimeLimit) (csrc/env_actor.hpp)
ENVS = {"CartPole-v0": (_lib.ENV_CARTPOLE, 4, 2, 200), "Acrobot-v1": (_lib.ENV_ACROBOT, 6, 3, 500),
        "MountainCar-v0": (_lib.ENV_MOUNTAINCAR, 2, 3, 200)}


class VecPpoActors(VecEnvActors):
    """N envs of `env` (a key of ENVS) stepped by one launch with the actor of a PPOSolver (or a
    ppo.ActorNetwork) at the env's (obs_dim, 64, num_actions).  horizon: the env steps between two
    finish() calls, which sizes the segments (module docstring).  cur_obs rows are obs_dim rounded
    up to 4 floats (the pad stays 0).  Episode statistics in int64 (episode_stats) and fp64 returns
    (return_stats).  max_episode_steps defaults to the env's TimeLimit.  cap: the rows per env's
    segment, 1..4096; None is finish()'s rule, horizon + max_episode_steps - 1.
    time_limit_bootstrap: step() records time-limit ends (seg_trunc, seg_term_s) and finish_gae()
    bootstraps through them (module docstring)."""
    _envs = ENVS

    def __init__(self, env, n_actors, horizon, seed=0, max_episode_steps=None, device=None, cap=None,
                 time_limit_bootstrap=False):
        self.horizon = int(horizon)
        self.time_limit_bootstrap = bool(time_limit_bootstrap)
        super().__init__(env, n_actors, seed, max_episode_steps, device, horizon=self.horizon)
        self.num_actions = ENVS[env][2]
        if cap is None:
            self.cap = self.horizon + self.max_episode_steps - 1
            if self.cap > MAX_CAP:
                raise ValueError(f"horizon + max_episode_steps - 1 = {self.cap} rows per env: at most {MAX_CAP}")
        else:  # finish_gae() has no carry: cap = horizon rows hold a rollout
            self.cap = int(cap)
            if not 1 <= self.cap <= MAX_CAP:
                raise ValueError(f"cap = {self.cap} rows per env: 1..{MAX_CAP}")
        N, D, cap, z = self.N, self.obs_dim, self.cap, self._alloc
        self.cur_obs = z((N, self.ld), torch.float32)
        self.last_action, self.last_logprob = z((N,), torch.int64), z((N,), torch.float32)
        # the rollout segments [N, cap, .]
        self.seg_s, self.seg_a = z((N, cap, D), torch.float32), z((N, cap), torch.int64)
        self.seg_r, self.seg_done, self.seg_logp = (z((N, cap), torch.float32) for _ in range(3))
        self.fill, self.gen, self.dropped = z((N,), torch.int32), z((N,), torch.int32), z((N,), torch.int64)
        self._complete = z((2, N), torch.int32)  # env i's live slot: gen[i] & 1
        self.seg_trunc = self.seg_term_s = None
        if self.time_limit_bootstrap:
            self.seg_trunc, self.seg_term_s = z((N, cap), torch.float32), z((N, cap, D), torch.float32)
        # the batch a finish() writes, persistent: N * cap rows hold any rollout
        self.batch = [z((N * cap, D), torch.float32), z((N * cap,), torch.int64), z((N * cap,), torch.float32),
                      z((N * cap,), torch.float32)]
        self.n_dev = z((1,), torch.int64)
        self.finishes = 0  # finish() / finish_gae() calls
        self.normalizes = 0  # rth_ppo_adv_normalize calls
        self.batch_adv = self.batch_v = None  # finish_gae()'s further columns, made by its first call
        self._value_key = self._value_arr = None
        self.reset()

    # ------------------------------------------------------------------ ABI arguments
    def _params(self, solver_or_actor):
        """the six parameter pointers of the actor as the ABI's array, rebuilt only when one moved"""
        actor = getattr(solver_or_actor, "actor_network", solver_or_actor)
        ps = _params6(actor)
        key = tuple(p.data_ptr() for p in ps)
        if key != self._params_key:
            dims = tuple(int(v) for v in _dims(actor))
            ok = all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in ps)
            if not ok or dims != (self.obs_dim, H, H, self.num_actions):
                raise ValueError(f"the {self.name} actors run ppo.ActorNetwork(({self.obs_dim},), {self.num_actions}, "
                                 f"{H}) in contiguous float32 on the GPU, got dims (D, H1, H2, A) = {dims}")
            self._params_arr = (_lib.c_vp * 6)(*key)
            self._params_key = key
        return self._params_arr

    def _args(self, params=None, action_in=None, uniforms=None):
        return _lib.PpoActorArgs(params, self.env_id, self.obs_dim, H, self.num_actions, ptr(self.state),
                                 ptr(self.ep_steps), ptr(self.t_dev), ptr(self.stats), ptr(self.ret_stats),
                                 ptr(self.cur_obs), ptr(action_in), ptr(uniforms), ptr(self.last_action),
                                 ptr(self.last_logprob), ptr(self.seg_s), ptr(self.seg_a), ptr(self.seg_r),
                                 ptr(self.seg_done), ptr(self.seg_logp), ptr(self.fill), ptr(self._complete),
                                 ptr(self.gen), ptr(self.dropped), self.seed, self.N, self.cap,
                                 self.max_episode_steps)

    # ------------------------------------------------------------------ env
    def reset(self):
        """env.reset() of every env (states from Philox(seed, env, t = 0)), empty segments, zeroed
        step counters and episode statistics"""
        args = self._args()
        call("rth_ppo_env_reset", _lib.ctypes.byref(args), stream_ptr())
        self.pushes = 0

    def observe(self, state):
        """the env's f32 observation [N, ld] (pad 0) of fp64 states [N, 4], computed by torch"""
        obs = torch.zeros((state.shape[0], self.ld), dtype=torch.float32, device=state.device)
        if self.env_id == _lib.ENV_ACROBOT:
            t = state[:, :2]
            obs[:, 0:4:2], obs[:, 1:4:2] = torch.cos(t).float(), torch.sin(t).float()
            obs[:, 4:6] = state[:, 2:4].float()
        else:
            obs[:, :self.obs_dim] = state[:, :self.obs_dim].float()
        return obs

    def _store_obs(self, obs):
        self.cur_obs.copy_(obs)

    def current_obs(self):
        """the observations [N, obs_dim] the envs act on next (a dense copy: the next step does not
        change it, also where obs_dim is the row stride)"""
        return self.cur_obs[:, :self.obs_dim].clone(memory_format=torch.contiguous_format)

    @property
    def complete(self):
        """int32 [N]: the stored rows that belong to finished episodes (a copy of the live slots)"""
        return torch.where((self.gen & 1) == 1, self._complete[1], self._complete[0])

    @torch.no_grad()
    def step(self, solver_or_actor, action_in=None, uniforms=None):
        """one env step for every actor, one launch, with the actor of a PPOSolver (or a
        ppo.ActorNetwork).  uniforms (float64 [N], device) replace the Philox draws; action_in
        (int64 [N], device) overrides the drawn action, and the stored log-probability is that
        action's."""
        if action_in is not None:
            self._check_action_in(action_in, torch.int64, self.N, "int64 device tensor [N]")
        if uniforms is not None and not (torch.is_tensor(uniforms) and uniforms.is_cuda and uniforms.is_contiguous()
                                         and uniforms.dtype == torch.float64 and uniforms.numel() == self.N):
            raise ValueError("uniforms: a contiguous float64 device tensor [N]")
        args = self._args(self._params(solver_or_actor), action_in, uniforms)
        if self.time_limit_bootstrap:
            call("rth_ppo_actor_step_tl", _lib.ctypes.byref(args), ptr(self.seg_trunc), ptr(self.seg_term_s), stream_ptr())
        else:
            call("rth_ppo_actor_step", _lib.ctypes.byref(args), stream_ptr())
        self.launches += 1
        self.pushes += 1

    # ------------------------------------------------------------------ rollout
    @torch.no_grad()
    def finish(self, gamma):
        """the end of a rollout, one launch: ([s, a, ret, logp] as [N * cap]-row device tensors of
        which the first n_dev[0] rows are the batch, n_dev int64 [1]).  The tensors are persistent
        (the next finish() overwrites them); rows at n and beyond are stale."""
        args = self._args()
        s, a, ret, logp = self.batch
        call("rth_ppo_rollout_finish", _lib.ctypes.byref(args), float(gamma), ptr(s), ptr(a), ptr(ret), ptr(logp),
             ptr(self.n_dev), stream_ptr())
        self.finishes += 1
        return self.batch, self.n_dev

    def _value_params(self, solver_or_value):
        """the six parameter pointers of the value network as the ABI's array (as _params)"""
        value = getattr(solver_or_value, "value_network", solver_or_value)
        ps = _params6(value)
        key = tuple(p.data_ptr() for p in ps)
        if key != self._value_key:
            dims = tuple(int(v) for v in _dims(value))
            ok = all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in ps)
            if not ok or dims != (self.obs_dim, H, H, 1):
                raise ValueError(f"the {self.name} GAE finish runs ppo.ValueNetwork(({self.obs_dim},), 1, {H}) in "
                                 f"contiguous float32 on the GPU, got dims (D, H1, H2, outputs) = {dims}")
            self._value_arr = (_lib.c_vp * 6)(*key)
            self._value_key = key
        return self._value_arr

    @torch.no_grad()
    def finish_gae(self, solver_or_value, gamma, lam, normalize=False):
        """the end of a rollout with GAE(lambda), one ABI call: ([s, a, ret, logp, adv], n_dev) with
        every stored row of every env (env-major, then time), the values of a PPOSolver's value
        network (or a ppo.ValueNetwork) and its value of cur_obs as the bootstrap (gae() below is
        the arithmetic).  The segments are empty afterwards: no carry.  batch_v holds the rows'
        values.  normalize: one more call, rth_ppo_adv_normalize over the n rows.  Persistent
        tensors, as finish()'s; rows at n and beyond are stale.  With time_limit_bootstrap a row
        whose seg_trunc is set bootstraps from the value of its seg_term_s row instead of nothing."""
        if self.batch_adv is None:
            self.batch_adv, self.batch_v = (self._alloc((self.N * self.cap,), torch.float32) for _ in range(2))
        args = self._args()
        s, a, ret, logp = self.batch
        tl = (ptr(self.seg_trunc), ptr(self.seg_term_s)) if self.time_limit_bootstrap else ()
        call("rth_ppo_gae_finish_tl" if tl else "rth_ppo_gae_finish", _lib.ctypes.byref(args),
             self._value_params(solver_or_value), float(gamma), float(lam), ptr(s), ptr(a), ptr(ret), ptr(self.batch_adv),
             ptr(self.batch_v), ptr(logp), ptr(self.n_dev), *tl, stream_ptr())
        self.finishes += 1
        if normalize:
            call("rth_ppo_adv_normalize", ptr(self.batch_adv), self.N * self.cap, ptr(self.n_dev), stream_ptr())
            self.normalizes += 1
        return [s, a, ret, logp, self.batch_adv], self.n_dev


def gae(r, done, v, v_last, gamma, lam, dtype=np.float32, trunc=None, v_term=None):
    """the kernel's GAE(lambda) of ONE env's rows (csrc/ppo_actor.hpp): (adv, ret) float32 [T] from
    float32 rewards, done flags and values and the value v_last of the state behind the last row;
    fp64, every operation rounded once, in the kernel's order (dtype=np.float64: before the final
    rounding).  trunc [T] (nonzero: the time limit alone ended the row's episode) with v_term [T]
    (the values of those rows' final observations; other entries are not read) is the scan of
    rth_ppo_gae_finish_tl: a truncated row bootstraps from v_term[t], and the lambda-chain is cut at
    every done row as before."""
    r, done, v = (np.asarray(x, np.float32).astype(np.float64) for x in (r, done, v))
    T = len(r)
    if trunc is not None:
        return _gae_tl(r, done, v, v_last, gamma, lam, dtype, np.asarray(trunc), np.asarray(v_term, np.float32))
    adv, ret = np.zeros(T, dtype), np.zeros(T, dtype)
    g = np.float64(gamma)
    gl = g * np.float64(lam)
    nv, run = np.float64(np.float32(v_last)), np.float64(0.0)
    for t in range(T - 1, -1, -1):
        nt = np.float64(1.0) - done[t]
        delta = (r[t] + (g * nv) * nt) - v[t]
        run = delta + (gl * nt) * run
        adv[t], ret[t] = run, run + v[t]  # rounded once by the store
        nv = v[t]
    return adv, ret


def _gae_tl(r, done, v, v_last, gamma, lam, dtype, trunc, v_term):
    """gae() with the truncation flags: the same operations on selected operands"""
    T = len(r)
    adv, ret = np.zeros(T, dtype), np.zeros(T, dtype)
    g = np.float64(gamma)
    gl = g * np.float64(lam)
    nxt, run = np.float64(np.float32(v_last)), np.float64(0.0)
    for t in range(T - 1, -1, -1):
        nt = np.float64(1.0) - done[t]
        nb = np.float64(1.0) if trunc[t] else nt
        nv = np.float64(v_term[t]) if trunc[t] else nxt
        delta = (r[t] + (g * nv) * nb) - v[t]
        run = delta + (gl * nt) * run
        adv[t], ret[t] = run, run + v[t]  # rounded once by the store
        nxt = v[t]
    return adv, ret


def episode_returns(r, done, gamma):
    """the kernel's returns of ONE episode (float32 [L] from float32 rewards and done flags):
    calculate_discount_rewards_with_dones with the sums in fp64, every operation rounded once, in
    the kernel's order"""
    r, done = np.asarray(r, np.float32), np.asarray(done)
    L = len(r)
    d = np.zeros(L, np.float32)
    run, g = np.float64(0.0), np.float64(gamma)
    for t in range(L - 1, -1, -1):
        if done[t]:
            d[t] = 0.0
        else:
            run = run * g + np.float64(r[t])
            d[t] = np.float32(run)
    d64 = d.astype(np.float64)
    mean = np.cumsum(d64)[-1] / np.float64(L)  # (cumsum: a sequential sum in increasing t)
    c = d64 - mean
    var = np.cumsum(c * c)[-1] / np.float64(L)
    return (c / (np.sqrt(var) + np.float64(1e-7))).astype(np.float32)


class HostRollout:
    """The rollout segments of N envs in numpy: store() is the step's append, finish() the kernel's
    finish and carry (csrc/ppo_actor.hpp), with its arithmetic in its order."""

    def __init__(self, n_envs, cap, obs_dim):
        self.N, self.cap, self.D = int(n_envs), int(cap), int(obs_dim)
        N, cap, D = self.N, self.cap, self.D
        self.seg_s, self.seg_a = np.zeros((N, cap, D), np.float32), np.zeros((N, cap), np.int64)
        self.seg_r, self.seg_done, self.seg_logp = (np.zeros((N, cap), np.float32) for _ in range(3))
        self.fill, self.complete = np.zeros(N, np.int32), np.zeros(N, np.int32)
        self.dropped = np.zeros(N, np.int64)
        # the time-limit columns (store(trunc=, term_s=)); term_s rows of other steps stay NaN
        self.seg_trunc, self.seg_term_s = np.zeros((N, cap), np.float32), np.full((N, cap, D), np.nan, np.float32)

    def store(self, s0, a, r, done, logp, trunc=None, term_s=None):
        """one step's rows, one per env: s0 [N, D], the others [N]; trunc [N] (the time limit alone
        ended the episode) with term_s [N, D] (the final observations, read where trunc is set)"""
        s0 = np.asarray(s0, np.float32).reshape(self.N, self.D)
        a, r, done, logp = (np.asarray(v).reshape(self.N) for v in (a, r, done, logp))
        if trunc is not None:
            trunc, term_s = np.asarray(trunc).reshape(self.N), np.asarray(term_s, np.float32).reshape(self.N, self.D)
        for i in range(self.N):
            f = int(self.fill[i])
            if f >= self.cap:
                self.dropped[i] += 1
                continue
            self.seg_s[i, f], self.seg_a[i, f], self.seg_r[i, f] = s0[i], a[i], r[i]
            self.seg_done[i, f], self.seg_logp[i, f] = (1.0 if done[i] else 0.0), logp[i]
            if trunc is not None:
                self.seg_trunc[i, f] = 1.0 if trunc[i] else 0.0
                if trunc[i]:
                    self.seg_term_s[i, f] = term_s[i]
            self.fill[i] = f + 1
            if done[i]:
                self.complete[i] = f + 1

    def finish(self, gamma):
        """(s [n, D], a [n], ret [n], logp [n], n): the rows of the finished episodes env-major,
        then in time order; the running episodes' rows move to the front of their segments"""
        out = [[], [], [], []]
        for i in range(self.N):
            m, e = int(self.fill[i]), int(self.complete[i])
            ret = np.zeros(e, np.float32)
            t0 = 0
            for t in range(e):
                if self.seg_done[i, t]:
                    ret[t0:t + 1] = episode_returns(self.seg_r[i, t0:t + 1], self.seg_done[i, t0:t + 1], gamma)
                    t0 = t + 1
            for o, col in zip(out, (self.seg_s[i, :e], self.seg_a[i, :e], ret, self.seg_logp[i, :e])):
                o.append(col.copy())
            if e:
                for col in (self.seg_s, self.seg_a, self.seg_r, self.seg_done, self.seg_logp):
                    col[i, :m - e] = col[i, e:m].copy()
            self.fill[i], self.complete[i] = m - e, 0
        s, a, ret, logp = (np.concatenate(o) for o in out)
        return s, a, ret, logp, len(a)

    def finish_gae(self, v, v_last, gamma, lam, v_term=None):
        """(s [n, D], a [n], ret [n], logp [n], adv [n], n): every stored row of every env,
        env-major, then in time order, with gae() on the rows' values v [N, cap] and the bootstrap
        values v_last [N]; the segments are empty afterwards.  v_term [N, cap]: the values of
        seg_term_s, read where seg_trunc is set -- gae() with the truncation flags."""
        v, v_last = np.asarray(v, np.float32).reshape(self.N, self.cap), np.asarray(v_last, np.float32).reshape(self.N)
        if v_term is not None:
            v_term = np.asarray(v_term, np.float32).reshape(self.N, self.cap)
        out = [[], [], [], [], []]
        for i in range(self.N):
            m = int(self.fill[i])
            tl = {} if v_term is None else dict(trunc=self.seg_trunc[i, :m], v_term=v_term[i, :m])
            adv, ret = gae(self.seg_r[i, :m], self.seg_done[i, :m], v[i, :m], v_last[i], gamma, lam, **tl)
            for o, col in zip(out, (self.seg_s[i, :m], self.seg_a[i, :m], ret, self.seg_logp[i, :m], adv)):
                o.append(col.copy())
        self.fill[:], self.complete[:] = 0, 0
        s, a, ret, logp, adv = (np.concatenate(o) for o in out)
        return s, a, ret, logp, adv, len(a)
