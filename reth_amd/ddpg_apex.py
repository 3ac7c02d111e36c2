"""DDPG with prioritized replay on one GPU and one stream: the device Pendulum loop.

The counterpart of mlp_apex.MlpApexDQN for DDPG's continuous actions.  Reference wiring:
reth/examples/ddpg/run.py (examples/pendulum_ddpg_hip.py here: worker.step_batch ->
buffer.append_batch -> buffer.sample -> trainer.step -> buffer.update_priorities) with the actor
side of presets/worker.py:128-155 and utils/exploration.py:34-53.  One iteration, entirely in HBM
and without host synchronisation:

    1. the actors' step                 one launch: act, OU noise, env, reset (N env steps)
    2. HbmReplay.append(rows, ones)     PrioritizedBuffer.append_batch: raw priority 1 per row
    3. once sample_start rows are stored:
       the schedules' step (PrioritizedBuffer.sample steps alpha and beta before it samples) ->
       sample_into (preallocated batch) -> DDPGSolver.update_device(batch, isw) ->
       update_priorities(idx, |td|)

Which of the steps run is decided on the host from counts it already knows (every actor emits one
row per step): nothing is read back.  capture() (device_loop.OneStreamLoop's, as iteration() and
the counters are) records the steady-state iteration as one HIP graph; every per-step scalar (env
step counters, FIFO tail, Philox counters, the schedules, Adam's step counts) is device-resident,
so the graph replays.

Every device env is its own worker, so the noise schedule advances once per iteration (per env
step of each env), where the reference's single worker advances it once per transition.

The loop needs DDPG's fused kernels (DDPGSolver.impl_active == "hip"): without them it refuses to
construct -- there is no torch fallback here.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from .ddpg import DDPGSolver
from .ddpg_actors import ENVS, VecDdpgActors
from .device_loop import OneStreamLoop
from .solver import Box


@dataclass
class DdpgApexConfig:
    env: str = "Pendulum-v0"           # a key of ddpg_actors.ENVS (examples/pendulum_ddpg.yaml: env.name)
    n_actors: int = 64                 # examples/ddpg/run.py: 64 env steps per training step
    batch_size: int = 64
    capacity: int = 100_000            # replay_buffer
    alpha: float = 0.6
    beta: str = "0.4,1,100000"
    gamma: float = 0.99                # solver
    tau: float = 0.001
    learning_rate_actor: float = 1e-4
    learning_rate_critic: float = 1e-3
    epsilon: str = "1,0.01,30000"      # worker.exploration
    ou_theta: float = 0.15             # utils/noise.py's defaults
    ou_sigma: float = 0.2
    ou_mu: float = 0.0
    sample_start: int = 1000           # rows stored before the first update (run.py's warm-up)
    cast_actions_to_long: bool = False  # examples/pendulum_ddpg_hip.py's docstring: the critic sees the actions taken
    max_episode_steps: Optional[int] = None  # None: the env's TimeLimit
    seed: int = 0


class DdpgApex(OneStreamLoop):
    _solver_counter, _solver_launches = "hip_launches", 3  # update_device's

    def __init__(self, cfg: DdpgApexConfig = None, device=None, impl=None):
        cfg = cfg if cfg is not None else DdpgApexConfig()
        super().__init__(cfg, device, ENVS)
        _, obs_dim, action_dim, _ = ENVS[cfg.env]
        self.solver = DDPGSolver(Box(-1.0, 1.0, (obs_dim,)), Box(-2.0, 2.0, (action_dim,)), gamma=cfg.gamma,
                                 tau=cfg.tau, learning_rate_actor=cfg.learning_rate_actor,
                                 learning_rate_critic=cfg.learning_rate_critic, device=self.device,
                                 cast_actions_to_long=cfg.cast_actions_to_long, impl=impl)
        if self.solver.impl_active != "hip":
            raise RuntimeError("DdpgApex runs on DDPG's fused kernels: the solver's active path is "
                               f"{self.solver.impl_active!r} (impl={impl!r}); there is no torch fallback")
        self.actors = self._make_actors(cfg.n_actors, epsilon=cfg.epsilon, seed=cfg.seed)
        self._make_replay()
        self._ones = torch.ones(cfg.n_actors, dtype=torch.float64, device=self.device)  # append_batch's priorities
        self._no_idx = torch.empty(0, dtype=torch.int64, device=self.device)
        self._no_w = torch.empty(0, dtype=torch.float32, device=self.device)

    def _make_actors(self, n, **kw):
        c = self.cfg
        return VecDdpgActors(c.env, n, mu=c.ou_mu, theta=c.ou_theta, sigma=c.ou_sigma,
                             max_episode_steps=self.max_episode_steps, device=self.device, **kw)

    # ------------------------------------------------------------------ one iteration
    def _body(self, learn):
        """the device work of one iteration; returns the update's |td| or None"""
        act, rep = self.actors, self.replay
        act.step(self.solver)
        rep.append(act.rows(), self._ones, raw=True)
        if not learn:
            return None
        rep.update_priorities(self._no_idx, self._no_w, step=True)  # alpha.step(), beta.step()
        rep.sample_into(self.cfg.batch_size, self.batch, self.idx, self.isw)
        td = self.solver.update_device(self.batch, self.isw)
        rep.update_priorities(self.idx, td)
        return td

    # ------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def greedy_eval(self, n_envs=256, seed=12345):
        """mean return of the first episode of each of n_envs envs of a separate actor set acting
        without noise (scale 0) under the current actor, from the fp64 return statistics.  Without
        a terminal state every env finishes its first episode at step max_episode_steps.  One host
        read, at the end."""
        ev = self._make_actors(n_envs, epsilon=0.0, seed=seed)
        for _ in range(self.max_episode_steps):
            ev.step(self.solver)
        return float(ev.return_stats()[2].mean().item())
