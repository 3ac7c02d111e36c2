"""Ape-X DQN for 1-D observations on one GPU and one stream: the device classic-control loop
(CartPole by default; MlpApexConfig.env names another env of mlp_actors.ENVS).

The counterpart of apex.ApexDQN (conv observations) on the fused MLP kernels.  Reference wiring:
reth/examples/dqn/run.py (worker.step_batch -> solver.calc_loss -> buffer.append_batch ->
buffer.sample -> trainer.step -> buffer.update_priorities) with the actor side of
presets/worker.py:128-155.  One iteration, entirely in HBM and without host synchronisation:

    1. the actors' step                 one launch: act, env, reset, n-step push (N env steps)
    2. solver.calc_loss_device(rows)    the emitted rows' |td|: their priorities
    3. HbmReplay.append                 PER insert of the N rows
    4. once sample_start rows are stored:
       sample_into (preallocated batch) -> solver.update_device(batch, isw) ->
       update_priorities(idx, |td|, step=True)

Which of the steps run is decided on the host from counts it already knows (every actor emits
one row per step once warm): nothing is read back.  The target sync runs on the host Interval
outside the iteration, as ApexDQN does it.  capture() (device_loop.OneStreamLoop's, as iteration()
and the counters are) records the steady-state iteration as one HIP graph; every per-step scalar
(env step counters, FIFO tail, Philox counters, the schedules, Adam's step count) is
device-resident, so the graph replays.

The loop needs the MLP's fused kernels (model.MLP_IMPL = "hip"): without them it refuses to
construct -- there is no torch fallback here.
"""
from dataclasses import dataclass
from typing import Optional

import torch

from . import model
from .device_loop import OneStreamLoop
from .mlp_actors import ENVS, VecMlpActors
from .schedule import Interval
from .solver import Box, DQNSolver, Discrete


@dataclass
class MlpApexConfig:
    n_actors: int = 64
    batch_size: int = 64
    capacity: int = 100_000
    n_step: int = 1
    gamma: float = 0.99
    alpha: float = 0.6                 # reth/examples/dqn/config.yaml
    beta: str = "0.4,1,100000"
    learning_rate: float = 1e-3
    adam_epsilon: float = 1e-8
    clip_value: float = 40.0
    double_q: bool = True
    update_target_interval: int = 200
    sample_start: int = 1000           # rows stored before the first update
    max_episode_steps: Optional[int] = None  # None: the env's TimeLimit (CartPole-v0 200, v1 500, ...)
    nstep_mode: int = 0
    eps: Optional[object] = None       # None: apex_epsilons(n_actors)
    seed: int = 0
    env: str = "CartPole-v0"           # a key of mlp_actors.ENVS: the reference's env.name (examples/dqn/config.yaml)


class MlpApexDQN(OneStreamLoop):
    _solver_counter, _solver_launches = "mlp_hip_launches", 2  # calc_loss_device + update_device

    def __init__(self, cfg: MlpApexConfig = None, device=None):
        cfg = cfg if cfg is not None else MlpApexConfig()
        if model.MLP_IMPL != "hip":
            raise RuntimeError('MlpApexDQN runs on the fused MLP kernels: set reth_amd.model.MLP_IMPL = "hip" before '
                               f"constructing it (MLP_IMPL is {model.MLP_IMPL!r}); there is no torch fallback")
        super().__init__(cfg, device, ENVS)
        _, obs_dim, num_actions, _ = ENVS[cfg.env]
        self.solver = DQNSolver(Box(-1, 1, (obs_dim,)), Discrete(num_actions), gamma=cfg.gamma,
                                clip_value=cfg.clip_value, double_q=cfg.double_q, dueling=True,
                                learning_rate=cfg.learning_rate, adam_epsilon=cfg.adam_epsilon,
                                update_target_interval=cfg.update_target_interval, device=self.device,
                                n_step=cfg.n_step)
        if self.solver.mlp_impl_active != "hip":
            raise RuntimeError("the MLP's HIP kernels are not active for this solver (rth_mlp_supported)")
        # the target sync: host Interval outside the (possibly captured) iteration, after every update
        self.solver.auto_target_update = False
        self._updated = Interval(self.solver.update_target, cfg.update_target_interval)
        self.actors = self._make_actors(cfg.n_actors, cfg.n_step, eps=cfg.eps, seed=cfg.seed,
                                        nstep_mode=cfg.nstep_mode)
        self._make_replay()

    def _make_actors(self, n, n_step, **kw):
        return VecMlpActors(self.cfg.env, n, n_step, self.cfg.gamma, max_episode_steps=self.max_episode_steps,
                            device=self.device, **kw)

    # ------------------------------------------------------------------ one iteration
    def _body(self, learn):
        """the device work of one iteration with warm actors; returns the update's |td| or None"""
        act = self.actors
        act.step(self.solver.q_network)
        td = self.solver.calc_loss_device(act.rows())
        act.append(self.replay, td)
        if not learn:
            return None
        self.replay.sample_into(self.cfg.batch_size, self.batch, self.idx, self.isw)
        td_b = self.solver.update_device(self.batch, self.isw)
        self.replay.update_priorities(self.idx, td_b, step=True)
        return td_b

    def _filling(self):
        """the adders fill: the next step emits no rows yet"""
        return self.actors.pushes < self.actors.n_step

    def _fill(self):
        self.actors.step(self.solver.q_network)

    @property
    def solver_calls(self):
        """calc_loss_device (one per iteration that emits rows) + update_device calls issued: what
        solver.mlp_hip_launches counts"""
        return self.rows_emitted // self.actors.N + self.updates
    # ------------------------------------------------------------------ evaluation
    @torch.no_grad()
    def greedy_eval(self, n_envs=256, seed=12345, max_steps=None, metric="length"):
        """mean length (metric="length") or mean return (metric="return", from the fp64 return
        statistics) of the first episode of each of n_envs greedy (ε = 0) envs of a separate
        actor set under the current online network, from the device statistics.  Every env finishes
        its first episode within max_episode_steps steps (TimeLimit); taking each env's first
        episode -- not every episode finished in the window -- keeps short episodes from counting
        more often than long ones.  One host read, at the end."""
        if metric not in ("length", "return"):
            raise ValueError('greedy_eval: metric is "length" or "return"')
        if metric == "return" and self.cfg.env.startswith("CartPole"):  # reward 1 a step: the return is the length
            metric = "length"
        ev = self._make_actors(n_envs, 1, eps=0.0, seed=seed)
        episodes, _, last = ev.episode_stats()
        if metric == "return":
            last = ev.return_stats()[2]
        first = torch.zeros(ev.N, dtype=last.dtype, device=self.device)
        seen = torch.zeros(ev.N, dtype=torch.bool, device=self.device)
        for _ in range(self.max_episode_steps if max_steps is None else int(max_steps)):
            ev.step(self.solver.q_network)
            fresh = ~seen & (episodes > 0)
            first = torch.where(fresh, last, first)
            seen |= fresh
        return float((first.sum() / seen.sum().clamp(min=1)).item())
