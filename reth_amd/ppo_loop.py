"""PPO on one GPU and one stream: the device on-policy loop.

The counterpart of ddpg_apex.DdpgApex for the on-policy learner.  Reference wiring:
reth/examples/ppo/run.py (examples/cartpole_ppo_hip.py here): UPDATE_INTERVAL env steps with the
acting solver's draws, complete episodes through calculate_discount_rewards_with_dones into the
data buffer, one trainer step of k_epochs full-batch epochs, the weights back to the acting solver.
One iteration here, entirely in HBM and without host synchronisation:

    1. `horizon` actor steps            one launch each: act, draw, env, reset, the rollout row
    2. the actors' finish               one launch: the finished episodes' returns, the dense
                                        batch and its device row count, the carry
    3. update_device(batch, n_rows)     k_epochs x (rth_ppo_grads_n, two Adam steps)

That is horizon + 1 + 3 k_epochs ABI calls.  The batch's row count never reaches the host: the
update takes it from the device.  capture() records an iteration as one HIP graph; every
per-step scalar (env step counters, segment fills, the row count, Adam's step counts) is
device-resident, so the graph replays.

Every device env is its own worker: N envs each run their own copy of the reference's loop
(ppo_actors' docstring), so an update sees N * horizon env steps where the reference's single worker
collects UPDATE_INTERVAL; the defaults, 10 x 200, are its 2,000.  The step reads the learner's actor
in place, which is what the reference's sync_weights achieves.  A batch holds the envs' rows
env-major, then in time order.

horizon >= max_episode_steps is required: then every env finishes at least one episode per
iteration and a batch has at least N rows (the reference's loop has no defined behaviour for an
empty batch either).

PpoLoopConfig.gae_lambda switches the estimator: GAE(lambda) with a value bootstrap at the rollout's
edge (ppo_actors.finish_gae, csrc/ppo_actor.hpp) instead of whole episodes' Monte-Carlo returns.
Then any horizon >= 1 runs, a segment is `horizon` rows without a carry, every stored row reaches
the learner at once (a batch is N * horizon rows), and step 2 / 3 become finish_gae and
update_device on the 5-column batch (rth_ppo_grads_adv): horizon + 1 (+ 1 with normalize_adv, the
advantages' normalisation) + 3 k_epochs ABI calls.  Many envs on short rollouts -- 64 x 32 -- is
what that is for.  None leaves everything above as it is.

PpoLoopConfig.n_minibatches = K > 1 makes each of the k_epochs a shuffled pass over the batch in K
minibatches with one optimiser step each (ppo.PPOSolver: rth_ppo_shuffle draws the order on the
device from its own device counter, so a replayed graph reshuffles): step 3 is then k_epochs x
(1 + 3 K) ABI calls.  K may not exceed the fewest rows a batch can hold (n_actors, or n_actors *
horizon with GAE), so no minibatch is ever empty.

PpoLoopConfig.bootstrap_time_limit (GAE only) removes the estimator's bias at time-limit ends: the
step records which done rows the limit alone ended and the observation they ended on, and the finish
bootstraps those rows from the value of that observation instead of treating them as terminal states
of value 0 (ppo_actors' time_limit_bootstrap; rth_ppo_actor_step_tl, rth_ppo_gae_finish_tl).  The
ABI calls per iteration are the same in number.

The loop needs PPO's fused kernels (PPOSolver.impl_active == "hip"): without them it refuses to
construct -- there is no torch fallback here.  It is not a device_loop.OneStreamLoop, which is
replay-shaped (rows flow into a replay, a batch is sampled out of it).
"""
from dataclasses import dataclass
from typing import Optional

import torch

from .ppo import MAX_MINIBATCHES, MAX_SHUFFLE_ROWS, PPOSolver
from .ppo_actors import ENVS, VecPpoActors
from .solver import Box, Discrete


@dataclass
class PpoLoopConfig:
    env: str = "CartPole-v0"           # a key of ppo_actors.ENVS (examples/cartpole_ppo.yaml: env.name)
    n_actors: int = 10
    horizon: int = 200                 # 10 x 200 = examples/ppo/run.py's UPDATE_INTERVAL of 2,000
    gamma: float = 0.99
    k_epochs: int = 4                  # solver
    eps_clip: float = 0.2
    learning_rate: float = 0.01
    max_episode_steps: Optional[int] = None  # None: the env's TimeLimit
    seed: int = 0
    gae_lambda: Optional[float] = None  # None: the reference's estimator; else GAE(lambda), any horizon >= 1
    normalize_adv: bool = False        # GAE only: the batch's advantages to mean 0, std 1
    n_minibatches: int = 1             # K > 1: every epoch is a shuffled pass of K optimiser steps (ppo.PPOSolver)
    bootstrap_time_limit: bool = False  # GAE only: bootstrap through episode ends that the time limit alone caused


class PpoLoop:
    def __init__(self, cfg: PpoLoopConfig = None, device=None, impl=None):
        cfg = cfg if cfg is not None else PpoLoopConfig()
        if cfg.env not in ENVS:
            raise ValueError(f"PpoLoopConfig.env {cfg.env!r}: the device envs are {', '.join(ENVS)}")
        self.cfg = cfg
        self.device = torch.device(device if device is not None else "cuda")
        _, obs_dim, num_actions, limit = ENVS[cfg.env]
        self.max_episode_steps = int(limit if cfg.max_episode_steps is None else cfg.max_episode_steps)
        self.gae = cfg.gae_lambda is not None
        if cfg.normalize_adv and not self.gae:
            raise ValueError("PpoLoopConfig.normalize_adv normalises GAE's advantages: set gae_lambda")
        if cfg.bootstrap_time_limit and not self.gae:
            raise ValueError("PpoLoopConfig.bootstrap_time_limit bootstraps GAE through time-limit ends: set gae_lambda")
        if self.gae and not 0.0 <= cfg.gae_lambda <= 1.0:
            raise ValueError(f"PpoLoopConfig.gae_lambda {cfg.gae_lambda}: None or 0..1")
        if self.gae and cfg.horizon < 1:
            raise ValueError(f"PpoLoopConfig.horizon {cfg.horizon}: at least 1")
        if not self.gae and cfg.horizon < self.max_episode_steps:
            raise ValueError(f"PpoLoopConfig.horizon {cfg.horizon} < max_episode_steps {self.max_episode_steps}: an "
                             "iteration must let every env finish an episode, or a batch could be empty")
        K = int(cfg.n_minibatches)
        if not 1 <= K <= MAX_MINIBATCHES:
            raise ValueError(f"PpoLoopConfig.n_minibatches {cfg.n_minibatches}: 1..{MAX_MINIBATCHES}")
        least = cfg.n_actors * cfg.horizon if self.gae else cfg.n_actors  # the fewest rows a batch can hold
        if K > least:
            raise ValueError(f"PpoLoopConfig.n_minibatches {K}: a batch can hold as few as {least} rows, and no "
                             "minibatch may be empty")
        torch.manual_seed(cfg.seed)
        self.solver = PPOSolver(Box(-1.0, 1.0, (obs_dim,)), Discrete(num_actions), k_epochs=cfg.k_epochs,
                                eps_clip=cfg.eps_clip, learning_rate=cfg.learning_rate, device=self.device, impl=impl,
                                n_minibatches=K)
        if self.solver.impl_active != "hip":
            raise RuntimeError("PpoLoop runs on PPO's fused kernels: the solver's active path is "
                               f"{self.solver.impl_active!r} (impl={impl!r}); there is no torch fallback")
        self.actors = VecPpoActors(cfg.env, cfg.n_actors, cfg.horizon, seed=cfg.seed,
                                   max_episode_steps=self.max_episode_steps, device=self.device,
                                   cap=cfg.horizon if self.gae else None,  # GAE: no carry
                                   time_limit_bootstrap=bool(cfg.bootstrap_time_limit))
        if K > 1 and self.actors.N * self.actors.cap > MAX_SHUFFLE_ROWS:
            raise ValueError(f"PpoLoopConfig.n_minibatches {K}: the batch capacity n_actors * cap = "
                             f"{self.actors.N * self.actors.cap} is above the shuffle's {MAX_SHUFFLE_ROWS} rows")
        self.iterations = self.env_steps = self.updates = 0
        # the last update's |loss| [N * cap]: rows beyond the batch are stale (K > 1: update_device's minibatch layout)
        self.last_loss_abs = None
        self._graph = None

    # ------------------------------------------------------------------ one iteration
    def _body(self):
        """the device work of one iteration; returns the update's |loss|"""
        act = self.actors
        for _ in range(self.cfg.horizon):
            act.step(self.solver)
        if self.gae:
            batch, n_dev = act.finish_gae(self.solver, self.cfg.gamma, self.cfg.gae_lambda, self.cfg.normalize_adv)
        else:
            batch, n_dev = act.finish(self.cfg.gamma)
        return self.solver.update_device(batch, n_rows=n_dev)

    def _mirrors(self):
        """the host mirrors, as (object, attribute, what one iteration adds), of what _body()
        advances on the device: recording it moves them, so capture() puts them back, and
        iteration() advances them after every replay"""
        act, T, K = self.actors, self.cfg.horizon, self.solver.n_minibatches
        return [(act, "pushes", T), (act, "launches", T), (act, "finishes", 1),
                (act, "normalizes", int(self.gae and self.cfg.normalize_adv)),
                (self.solver, "hip_launches", self.cfg.k_epochs * (3 * K + int(K > 1))),
                (self.solver, "shuffle_calls", self.cfg.k_epochs * int(K > 1))]

    def iteration(self):
        """one iteration on the current stream; never synchronises with the host"""
        if self._graph is not None:
            self._graph.replay()
            for o, name, add in self._mirrors():
                setattr(o, name, getattr(o, name) + add)
        else:
            self.last_loss_abs = self._body()
        self.iterations += 1
        self.env_steps += self.actors.N * self.cfg.horizon
        self.updates += 1

    def run(self, iterations):
        for _ in range(int(iterations)):
            self.iteration()

    # ------------------------------------------------------------------ graph
    def graph_ready(self):
        """an iteration has run: every persistent buffer of the update exists"""
        return self.updates >= 1

    def capture(self):
        """record one iteration, _body(), as one HIP graph on a side stream; iteration() replays it
        from then on.  Capturing records and does not run the iteration."""
        if self._graph is not None:
            return
        if not self.graph_ready():
            raise RuntimeError("capture() records the steady-state iteration: run iteration() once first "
                               "(graph_ready())")
        mirrors = self._mirrors()
        host = [getattr(o, name) for o, name, _ in mirrors]
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            keep = self._body()
        torch.cuda.current_stream(self.device).wait_stream(side)
        for (o, name, _), v in zip(mirrors, host):
            setattr(o, name, v)
        self._graph, self.last_loss_abs = g, keep

    # ------------------------------------------------------------------ evaluation
    def mean_last_length(self):
        """the envs' mean last finished episode length (0 for an env that has finished none).  One
        host read."""
        return float(self.actors.episode_stats()[2].double().mean().item())

    @torch.no_grad()
    def rollout_length(self, seed=12345):
        """the same measure for the current actor on a separate set of n_actors envs stepped
        max(horizon, max_episode_steps) times (every env finishes an episode; without GAE that is
        `horizon`), which leaves the loop's own envs and rollout as they are.  Before the first
        update: the untrained actor's figure.  One host read."""
        steps = max(self.cfg.horizon, self.max_episode_steps)
        # (its rows are never finished: with GAE a segment of one row, the rest counted in `dropped`)
        ev = VecPpoActors(self.cfg.env, self.cfg.n_actors, steps, seed=seed,
                          max_episode_steps=self.max_episode_steps, device=self.device, cap=1 if self.gae else None)
        for _ in range(steps):
            ev.step(self.solver)
        return float(ev.episode_stats()[2].double().mean().item())
