"""Vectorised classic-control actors on one GPU, on the fused MLP kernels (csrc/env_actor.hpp).

Reference actor loop: reth/reth/presets/worker.py:128-155 (Worker.step: exploration.act ->
solver.act, env.step, env.reset on done) and utils/nstep_adder.py:11-28, one host env and one
transition at a time.  Here N environments of one kind -- gym's CartPole-v0/v1, Acrobot-v1 or
MountainCar-v0, the dynamics of envs.py's host classes in fp64 -- live in HBM and step together in
ONE launch per env step: the acting forward of the MLP Q-network at the env's shape (bit-equal to
rth_mlp_q), ε-greedy with rth_eps_greedy's Philox draws, the dynamics, the reset of finished
episodes, the f32 observations into a per-env ring and the n-step push.  Emitted n-step rows come
out as ring handles and by value (row_obs0 / row_obs1 [N, obs_dim]), so
DQNSolver.calc_loss_device and HbmReplay.append consume them as dense tensors.  No host
synchronisation anywhere; every per-step scalar is device-resident, so a captured step replays.

The counterpart of actors.VecActors (conv observations) for 1-D observations; what it shares with
ddpg_actors.VecDdpgActors is device_loop.VecEnvActors.

VecMlpActors(env, n, ...) is the implementation, on rth_env_reset / rth_env_actor_step.
VecCartPoleActors(n, ...) is the same set fixed to CartPole-v0 through the CartPole entry points
(rth_cartpole_reset / rth_mlp_actor_step: adapters onto the same kernel, without return statistics).
"""
import numpy as np
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .actors import apex_epsilons
from .device_loop import VecEnvActors

OBS_DIM, NUM_ACTIONS = 4, 2  # CartPole's

# env name -> (RTH_ENV_* id, obs_dim, num_actions, TimeLimit) of the classic-control family (csrc/env_actor.hpp)
ENVS = {"CartPole-v0": (_lib.ENV_CARTPOLE, 4, 2, 200), "CartPole-v1": (_lib.ENV_CARTPOLE, 4, 2, 500),
        "Acrobot-v1": (_lib.ENV_ACROBOT, 6, 3, 500), "MountainCar-v0": (_lib.ENV_MOUNTAINCAR, 2, 3, 200)}


def row_columns(obs_dim):
    """replay columns of the rows [s0, a, r, s1, done], cast f4 / i8 / f4 / f4 / f4 as
    test/apex-dqn/worker.py:47-51 casts them"""
    from .replay import Column

    return [Column((obs_dim,), torch.float32), Column((), torch.int64), Column((), torch.float32),
            Column((obs_dim,), torch.float32), Column((), torch.float32)]


class VecMlpActors(VecEnvActors):
    """N envs of `env` (a key of ENVS) stepped by one launch at the env's network shape
    (obs_dim, 128, num_actions), with the env's reward, terminal rule and observation map.  The
    ring's rows are obs_dim rounded up to 4 floats (the pad stays 0); rows() are dense
    [N, obs_dim].  Episode statistics in int64 (episode_stats) and fp64 returns (return_stats).
    max_episode_steps defaults to the env's TimeLimit."""
    _envs = ENVS
    _reset_fn, _step_fn = "rth_env_reset", "rth_env_actor_step"

    def __init__(self, env, n_actors, n_step=1, gamma=0.99, eps=None, seed=0, max_episode_steps=None, nstep_mode=0,
                 device=None):
        self.n_step, self.gamma = int(n_step), float(gamma)
        self.gamma_n = float(np.float32(gamma ** n_step))
        super().__init__(env, n_actors, seed, max_episode_steps, device, n_step=self.n_step)
        self.num_actions = ENVS[env][2]
        ring = 4
        while ring < 2 * (self.n_step + 3):  # an emitted row's observations are at most n + 1 steps old, 2 slots a step
            ring *= 2
        self.ring = ring
        N, D, z = self.N, self.obs_dim, self._alloc
        self.obs_ring = z((N * ring + 1, self.ld), torch.float32)  # zero-filled once; last row: the sink
        self.cur_slot = z((N,), torch.int64)
        e = apex_epsilons(N) if eps is None else np.array(np.broadcast_to(np.asarray(eps, np.float64), (N,)))
        # float64, read by every step: overwrite in place (eps.copy_ / eps.fill_) to follow a schedule
        self.eps = z((N,), torch.float64)
        self.eps.copy_(torch.as_tensor(e, dtype=torch.float64))
        self.action, self.s0_h, self.s1_h = z((N,), torch.int64), z((N,), torch.int64), z((N,), torch.int64)
        self.reward, self.done = z((N,), torch.float32), z((N,), torch.float32)
        self.emit = z((N,), torch.int32)
        self.row_s0, self.row_a, self.row_s1 = z((N,), torch.int64), z((N,), torch.int64), z((N,), torch.int64)
        self.row_r, self.row_done = z((N,), torch.float32), z((N,), torch.float32)
        self.row_obs0, self.row_obs1 = z((N, D), torch.float32), z((N, D), torch.float32)
        self.q_out = None  # want_q(): the acting Q rows [N, A] (tests)
        self._base = torch.arange(N, device=self.device, dtype=torch.int64) * ring
        h = _lib.c_vp()
        with torch.cuda.device(self.device):
            call("rth_nstep_create", N, self.n_step, self.gamma, int(nstep_mode), torch.cuda.current_device(),
                 _lib.ctypes.byref(h))
        self._nstep = h.value
        self.reset()

    def __del__(self):
        if getattr(self, "_nstep", None):
            try:
                _lib.lib().rth_nstep_destroy(self._nstep)
            except Exception:
                pass
            self._nstep = None

    # ------------------------------------------------------------------ ABI arguments
    def _check_net(self, q_network, params):
        want = (self.obs_dim, 128, self.num_actions)
        if not q_network.hip_supported() or q_network.dims() != want:
            raise ValueError(f"the {self.name} actors run MLP_DQNNetwork(({want[0]},), {want[2]}) on the GPU, got "
                             f"dims {q_network.dims()}")

    def _args(self, params=None, action_in=None):
        return _lib.EnvActorArgs(params, self.env_id, self.obs_dim, 128, self.num_actions, ptr(self.state),
                                 ptr(self.ep_steps), ptr(self.t_dev), ptr(self.stats), ptr(self.ret_stats),
                                 ptr(self.obs_ring), ptr(self.cur_slot), ptr(self.eps), ptr(action_in),
                                 ptr(self.action), ptr(self.reward), ptr(self.done), ptr(self.s0_h), ptr(self.s1_h),
                                 ptr(self.emit), ptr(self.row_s0), ptr(self.row_a), ptr(self.row_s1), ptr(self.row_r),
                                 ptr(self.row_done), ptr(self.row_obs0), ptr(self.row_obs1), ptr(self.q_out),
                                 self.seed, self.N, self.ring, self.max_episode_steps)

    # ------------------------------------------------------------------ env
    def reset(self):
        """env.reset() of every env (states from Philox(seed, env, t = 0)), an empty adder, zeroed
        step counters and episode statistics"""
        s = stream_ptr()
        args = self._args()
        call(self._reset_fn, _lib.ctypes.byref(args), s)
        call("rth_nstep_reset", self._nstep, s)
        self.pushes = 0

    def want_q(self, on=True):
        """have every step also write its acting Q rows to q_out [N, A] (tests)"""
        self.q_out = self._alloc((self.N, self.num_actions), torch.float32) if on else None
        return self.q_out

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
        self.obs_ring[self._base + self.cur_slot] = obs

    def current_obs(self):
        """the observations [N, obs_dim] the envs act on next (a dense copy)"""
        return self.obs_ring[self._base + self.cur_slot][:, :self.obs_dim].contiguous()

    @property
    def warm(self):
        """every actor emits one n-step row per step once its deque is full"""
        return self.pushes > self.n_step

    @torch.no_grad()
    def step(self, q_network, action_in=None):
        """one env step for every actor, one launch; action_in (int64 [N], device) overrides the
        ε-greedy choice.  Returns True when rows were emitted (warm)."""
        if action_in is not None:
            self._check_action_in(action_in, torch.int64, self.N, "int64 device tensor [N]")
        args = self._args(self._params(q_network), action_in)
        call(self._step_fn, self._nstep, _lib.ctypes.byref(args), stream_ptr())
        self.launches += 1
        self.pushes += 1
        return self.warm

    # ------------------------------------------------------------------ rows
    def rows(self):
        """the emitted n-step rows [s0, a, r, s1, done] as the live dense device tensors the next
        step overwrites (valid once warm): what calc_loss_device / append consume"""
        return [self.row_obs0, self.row_a, self.row_r, self.row_obs1, self.row_done]

    def append(self, replay, td_abs):
        """Client.append of the emitted rows (every actor emits once warm)"""
        if not self.warm:
            raise RuntimeError("no rows yet: the adders fill during the first n_step steps")
        return replay.append(self.rows(), td_abs)

    def columns(self):
        """replay columns of the rows [s0, a, r, s1, done] at this env's obs_dim"""
        return row_columns(self.obs_dim)


class VecCartPoleActors(VecMlpActors):
    """VecMlpActors("CartPole-v0", ...) through rth_cartpole_reset / rth_mlp_actor_step: the same
    kernel, the same bits, no return statistics (a CartPole return is its length: episode_stats)."""
    obs_dim, num_actions = OBS_DIM, NUM_ACTIONS
    _reset_fn, _step_fn = "rth_cartpole_reset", "rth_mlp_actor_step"
    _keeps_returns = False

    def __init__(self, n_actors, n_step=1, gamma=0.99, eps=None, seed=0, max_episode_steps=200, nstep_mode=0,
                 device=None):
        super().__init__("CartPole-v0", n_actors, n_step, gamma, eps, seed, max_episode_steps, nstep_mode, device)

    def _args(self, params=None, action_in=None):  # rth_env_actor_args without env and ret_stats
        return _lib.MlpActorArgs(params, OBS_DIM, 128, NUM_ACTIONS, ptr(self.state), ptr(self.ep_steps),
                                 ptr(self.t_dev), ptr(self.stats), ptr(self.obs_ring), ptr(self.cur_slot),
                                 ptr(self.eps), ptr(action_in), ptr(self.action), ptr(self.reward), ptr(self.done),
                                 ptr(self.s0_h), ptr(self.s1_h), ptr(self.emit), ptr(self.row_s0), ptr(self.row_a),
                                 ptr(self.row_s1), ptr(self.row_r), ptr(self.row_done), ptr(self.row_obs0),
                                 ptr(self.row_obs1), ptr(self.q_out), self.seed, self.N, self.ring,
                                 self.max_episode_steps)

    @staticmethod
    def columns(obs_dim=OBS_DIM):
        return row_columns(obs_dim)
