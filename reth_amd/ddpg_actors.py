"""Vectorised continuous-control actors on one GPU, on DDPG's fused actor (csrc/ddpg_actor.hpp).

Reference actor loop: reth/reth/presets/worker.py:128-155 (Worker.step: exploration.act ->
solver.act, env.step, on done env.reset and exploration.reset) with utils/exploration.py:34-53
(OUNoiseExploration) and utils/noise.py (OUNoise), one host env and one transition at a time.
Here N Pendulum-v0 environments -- the dynamics of envs.Pendulum in fp64 -- live in HBM and step
together in ONE launch per env step: the acting forward of the 400-300 actor (bit-equal to
rth_ddpg_act), Ornstein-Uhlenbeck noise on counter-based normal draws scaled by a linear schedule,
the dynamics, the time limit and the reset of finished episodes.  DDPG has no n-step, so the
transition is the row: rows() are dense f32 tensors DDPGSolver.update_device and HbmReplay.append
consume.  No host synchronisation anywhere; every per-step scalar is device-resident, so a
captured step replays.

Every env is its own worker: its noise scale follows the schedule at the env's own act count, so
the schedule advances once per step() -- not once per transition of the set.

The counterpart of mlp_actors.VecMlpActors (discrete actions) for continuous ones; what the two
share is device_loop.VecEnvActors.
"""
import torch

from . import _lib
from ._lib import call, ptr, stream_ptr
from .ddpg import H1, H2
from .device_loop import VecEnvActors, as_tensor
from .schedule import Schedule

# env name -> (RTH_DDPG_ENV_* id, obs_dim, action_dim, TimeLimit) (csrc/ddpg_actor.hpp)
ENVS = {"Pendulum-v0": (_lib.DDPG_ENV_PENDULUM, 3, 1, 200)}


def _linear(epsilon):
    """a Schedule spec (a number, or "start,end,steps") as the kernel's (start, end, steps)"""
    s = Schedule.from_str(epsilon)
    if s.method == "const":
        return float(s.const), float(s.const), 1
    if s.method != "linear":
        raise ValueError(f"the device actors evaluate a linear noise schedule, got {epsilon!r}")
    return float(s.start), float(s.end), int(s.max_steps)


class VecDdpgActors(VecEnvActors):
    """N envs of `env` (a key of ENVS) stepped by one launch with the actor of a DDPGSolver (or a
    ddpg.Actor) at the env's (obs_dim, action_dim).  epsilon: the noise scale's schedule (a number
    or "start,end,steps"; 0 acts greedily); mu / theta / sigma: OUNoise's.  cur_obs rows are
    obs_dim rounded up to 4 floats (the pad stays 0); rows() are dense.  Episode statistics in
    int64 (episode_stats) and fp64 returns (return_stats).  max_episode_steps defaults to the
    env's TimeLimit."""
    _envs = ENVS

    def __init__(self, env, n_actors, epsilon="1,0.01,30000", mu=0.0, theta=0.15, sigma=0.2, seed=0,
                 max_episode_steps=None, device=None):
        self.mu, self.theta, self.sigma = float(mu), float(theta), float(sigma)
        self.eps_start, self.eps_end, self.eps_steps = _linear(epsilon)
        super().__init__(env, n_actors, seed, max_episode_steps, device)  # (t_dev: also the schedule's step)
        self.action_dim = ENVS[env][2]
        N, D, Ad, z = self.N, self.obs_dim, self.action_dim, self._alloc
        self.noise = z((N, Ad), torch.float64)     # the OU state
        self.cur_obs = z((N, self.ld), torch.float32)
        self.act_det = z((N, Ad), torch.float32)   # the noise-free action of the last step
        self.row_s0, self.row_s1 = z((N, D), torch.float32), z((N, D), torch.float32)
        self.row_a = z((N, Ad), torch.float32)
        self.row_r, self.row_done = z((N,), torch.float32), z((N,), torch.float32)
        self._dims = None  # the actor's (D, Ad, H1, H2), with the parameter cache
        self.reset()

    # ------------------------------------------------------------------ ABI arguments
    def _params(self, solver_or_actor):
        return super()._params(getattr(solver_or_actor, "actor", solver_or_actor))

    def _check_net(self, actor, params):
        dims = tuple(int(v) for v in actor.dims())
        ok = all(p.is_cuda and p.dtype == torch.float32 and p.is_contiguous() for p in params)
        if not ok or dims[:2] != (self.obs_dim, self.action_dim) or not _lib.lib().rth_ddpg_supported(*dims):
            raise ValueError(f"the {self.name} actors run ddpg.Actor(({self.obs_dim},), ({self.action_dim},)) in "
                             f"contiguous float32 on the GPU, got dims (D, Ad, H1, H2) = {dims}")
        self._dims = dims

    def _args(self, params=None, action_in=None, dims=None):
        # (the reset reads no network: it is given the reference's hidden widths to pass the shape check)
        D, Ad, h1, h2 = dims if dims is not None else (self.obs_dim, self.action_dim, H1, H2)
        return _lib.DdpgActorArgs(params, self.env_id, D, Ad, h1, h2, ptr(self.state), ptr(self.ep_steps),
                                  ptr(self.t_dev), ptr(self.stats), ptr(self.ret_stats), ptr(self.noise),
                                  ptr(self.cur_obs), ptr(action_in), ptr(self.act_det), ptr(self.row_s0),
                                  ptr(self.row_a), ptr(self.row_r), ptr(self.row_s1), ptr(self.row_done), self.seed,
                                  self.N, self.mu, self.theta, self.sigma, self.eps_start, self.eps_end,
                                  self.eps_steps, self.max_episode_steps, 0)

    # ------------------------------------------------------------------ env
    def reset(self):
        """env.reset() of every env (states from Philox(seed, env, t = 0)), the noise at mu, zeroed
        step counters and episode statistics"""
        args = self._args()
        call("rth_ddpg_env_reset", _lib.ctypes.byref(args), stream_ptr())
        self.pushes = 0

    def observe(self, state):
        """the env's f32 observation [N, ld] (pad 0) of fp64 states [N, 4], computed by torch"""
        obs = torch.zeros((state.shape[0], self.ld), dtype=torch.float32, device=state.device)
        obs[:, 0], obs[:, 1] = torch.cos(state[:, 0]).float(), torch.sin(state[:, 0]).float()
        obs[:, 2] = state[:, 1].float()
        return obs

    def _store_obs(self, obs):
        self.cur_obs.copy_(obs)

    @torch.no_grad()
    def set_state(self, states, steps=None, noise=None):
        """VecEnvActors.set_state and, optionally, the OU states [N, Ad] (tests)"""
        super().set_state(states, steps)
        if noise is not None:
            self.noise.copy_(as_tensor(noise).to(self.device, torch.float64).reshape(self.N, self.action_dim))

    def current_obs(self):
        """the observations [N, obs_dim] the envs act on next (a dense copy)"""
        return self.cur_obs[:, :self.obs_dim].contiguous()

    @torch.no_grad()
    def step(self, solver_or_actor, action_in=None):
        """one env step for every actor, one launch, with the actor of a DDPGSolver (or a
        ddpg.Actor); action_in (float32 [N, Ad], device) overrides the noisy action"""
        if action_in is not None:
            self._check_action_in(action_in, torch.float32, self.N * self.action_dim, "float32 device tensor [N, Ad]")
        params = self._params(solver_or_actor)
        args = self._args(params, action_in, self._dims)
        call("rth_ddpg_actor_step", _lib.ctypes.byref(args), stream_ptr())
        self.launches += 1
        self.pushes += 1

    # ------------------------------------------------------------------ rows
    def rows(self):
        """the step's transitions [s0, a, r, s1, done] as the live dense device tensors the next
        step overwrites: what update_device / append consume"""
        return [self.row_s0, self.row_a, self.row_r, self.row_s1, self.row_done]

    def columns(self):
        """replay columns of the rows [s0, a, r, s1, done]: the action stays a float vector"""
        from .replay import Column

        return [Column((self.obs_dim,), torch.float32), Column((self.action_dim,), torch.float32),
                Column((), torch.float32), Column((self.obs_dim,), torch.float32), Column((), torch.float32)]
