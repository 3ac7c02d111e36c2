"""What the 1-D device loops and their vectorised actor sets share.

OneStreamLoop: the base of mlp_apex.MlpApexDQN and ddpg_apex.DdpgApex -- the counters, the
iteration's skeleton and capture().  The host mirrors a capture puts back are the ones every
replay advances: _mirrors and iteration(), here once.  iteration(), run(), graph_ready() and the
counters never touch the device themselves; only capture() and the subclass's device work do.

VecEnvActors: the base of mlp_actors.VecMlpActors and ddpg_actors.VecDdpgActors -- the env lookup,
the per-env buffers every step kernel keeps (csrc/env_actor.hpp, csrc/ddpg_actor.hpp), the
parameter-pointer cache, set_state and the statistics.
"""
import numpy as np
import torch

from . import _lib
from .replay import HbmReplay


class OneStreamLoop:
    """A subclass makes self.solver and self.actors, then calls _make_replay().  It implements
    _body(learn), the device work of an iteration that emits rows (returns the update's |td| or
    None); a loop whose actors fill first overrides _filling and _fill (that iteration's device
    work: the actors' step alone)."""
    _solver_counter = _solver_launches = None  # the solver's host count of its launches: its name, and _body(True)'s

    def __init__(self, cfg, device, envs):
        if cfg.sample_start < 1 or cfg.batch_size < 1:
            raise ValueError("sample_start and batch_size must be >= 1")
        if cfg.env not in envs:
            raise ValueError(f"{type(cfg).__name__}.env {cfg.env!r}: the device envs are {', '.join(envs)}")
        self.cfg = cfg
        self.device = torch.device(device if device is not None else "cuda")
        self.max_episode_steps = int(envs[cfg.env][3] if cfg.max_episode_steps is None else cfg.max_episode_steps)
        torch.manual_seed(cfg.seed)
        self.iterations = self.env_steps = self.updates = 0
        self.rows_emitted = 0  # = rows appended: every emitted row is stored
        self.last_td = None  # the last iteration's update's |td| [B] or None; captured: the tensor a replay writes
        self._graph = self._graph_keep = None

    def _make_replay(self):
        cfg = self.cfg
        self.replay = HbmReplay(cfg.capacity, self.actors.columns(), cfg.alpha, cfg.beta, self.device,
                                seed=cfg.seed + 7919)
        self.batch, self.idx, self.isw = self.replay.new_batch(cfg.batch_size)

    # ------------------------------------------------------------------ the subclass's parts
    def _filling(self):
        """the next step emits no rows yet (n-step adders fill)"""
        return False

    def _mirrors(self):
        """the host mirrors, as (object, attribute), of what _body(True) advances on the device:
        recording it moves them, so capture() puts them back, and iteration() advances them after
        every replay"""
        act, rep = self.actors, self.replay
        return [(act, "pushes"), (act, "launches"), (self.solver, self._solver_counter),
                (rep.alpha, "cur_step"), (rep.beta, "cur_step")]

    def _updated(self):
        """after an iteration whose update ran, eager or replayed (MlpApexDQN: its target Interval)"""

    # ------------------------------------------------------------------ one iteration
    def _learning(self):
        """the update runs in this iteration: sample_start rows are stored (host counts only)"""
        return min(self.rows_emitted, self.cfg.capacity) >= self.cfg.sample_start

    def iteration(self):
        """one iteration on the current stream; never synchronises with the host"""
        N = self.actors.N
        if self._graph is not None:
            self._graph.replay()
            act, rep, solver = self.actors, self.replay, self.solver  # _mirrors, by one replayed iteration
            act.pushes += 1
            act.launches += 1
            setattr(solver, self._solver_counter, getattr(solver, self._solver_counter) + self._solver_launches)
            rep.alpha.step()
            rep.beta.step()
            self.rows_emitted += N
            learned = True
        elif self._filling():
            self._fill()
            learned = False
        else:
            self.rows_emitted += N  # this step emits N rows
            learned = self._learning()
            self.last_td = self._body(learned)
        self.iterations += 1
        self.env_steps += N
        if learned:
            self.updates += 1
            self._updated()

    def run(self, iterations):
        for _ in range(int(iterations)):
            self.iteration()

    # ------------------------------------------------------------------ graph
    def graph_ready(self):
        """the next iteration is the steady-state one: rows flow and the update runs, and has run
        once (its buffers exist)"""
        return not self._filling() and \
            min(self.rows_emitted + self.actors.N, self.cfg.capacity) >= self.cfg.sample_start and self.updates >= 1

    def capture(self):
        """record the steady-state iteration, _body(True), as one HIP graph on a side stream;
        iteration() replays it from then on.  Capturing records and does not run the iteration.
        After a capture the C library's host mirrors of the replay counters (HbmReplay.info) no
        longer advance -- the device state does; rows_emitted / updates here are the counts."""
        if self._graph is not None:
            return
        if not self.graph_ready():
            raise RuntimeError("capture() records the steady-state iteration: run iteration() until at least one "
                               "update has run (graph_ready())")
        mirrors = self._mirrors()
        host = [getattr(o, name) for o, name in mirrors]
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
            keep = self._body(True)
        torch.cuda.current_stream(self.device).wait_stream(side)
        for (o, name), v in zip(mirrors, host):
            setattr(o, name, v)
        self._graph, self._graph_keep, self.last_td = g, keep, keep


def as_tensor(v):
    return torch.as_tensor(np.asarray(v) if not torch.is_tensor(v) else v)


class VecEnvActors:
    """N envs of `env`, a key of the subclass's table _envs: name -> (env id, obs_dim, action
    size, TimeLimit).  `ge1`: further named integers of the subclass that must be >= 1.  A subclass
    implements _check_net(net, its six parameters), which raises ValueError unless the step kernel
    runs that network; observe(state), the f32 observations [N, ld] (pad 0) of fp64 states [N, 4];
    and _store_obs(obs), which makes them the observations the envs act on next."""
    _envs = None
    _keeps_returns = True

    def __init__(self, env, n_actors, seed, max_episode_steps, device, **ge1):
        if env not in self._envs:
            raise ValueError(f"{type(self).__name__}: unknown env {env!r} (device envs: {', '.join(self._envs)})")
        self.env = self.name = env
        self.env_id, self.obs_dim, _, limit = self._envs[env]
        self.ld = (self.obs_dim + 3) // 4 * 4  # the observation rows' stride in floats
        self.N, self.seed = int(n_actors), int(seed)
        self.max_episode_steps = int(limit if max_episode_steps is None else max_episode_steps)
        ge1 = {"n_actors": self.N, **ge1, "max_episode_steps": self.max_episode_steps}
        if min(ge1.values()) < 1:
            raise ValueError(f"{', '.join(list(ge1)[:-1])} and max_episode_steps must be >= 1")
        self.device = torch.device(device if device is not None else "cuda")
        N, z = self.N, self._alloc
        self.state = z((N, 4), torch.float64)
        self.ep_steps = z((N,), torch.int32)
        self.t_dev = z((N,), torch.int64)          # env steps taken by each env (the Philox counter)
        self.stats = z((N, 3), torch.int64)        # finished episodes, sum of their lengths, last length
        # running return, sum of the finished episodes' returns, last finished return
        self.ret_stats = z((N, 3), torch.float64) if self._keeps_returns else None
        self._params_key = self._params_arr = None
        self.pushes = 0    # env steps issued (host mirror of t_dev)
        self.launches = 0  # actor-step calls: one launch each

    def _alloc(self, shape, dtype):
        """a zero-filled device buffer (tests override it to surround every buffer with guards)"""
        return torch.zeros(shape, dtype=dtype, device=self.device)

    def _params(self, net):
        """the six parameter pointers of `net` as the ABI's array, rebuilt only when one moved"""
        ps = net._params6()
        key = tuple(p.data_ptr() for p in ps)
        if key != self._params_key:
            self._check_net(net, ps)
            self._params_arr = (_lib.c_vp * 6)(*key)
            self._params_key = key
        return self._params_arr

    def _check_action_in(self, action_in, dtype, numel, what):
        if not (torch.is_tensor(action_in) and action_in.is_cuda and action_in.dtype == dtype
                and action_in.numel() == numel and action_in.is_contiguous()):
            raise ValueError(f"action_in: a contiguous {what}")

    @torch.no_grad()
    def set_state(self, states, steps=None):
        """inject env states [N, 4] (float64; [N, k] fills the first k columns) and, optionally, the
        running episodes' step counts [N]; the observations the envs act on next become those of
        the states (tests)"""
        st = as_tensor(states).to(self.device, torch.float64).reshape(self.N, -1)
        self.state.zero_()
        self.state[:, :st.shape[1]] = st
        if steps is not None:
            self.ep_steps.copy_(as_tensor(steps).to(self.device, torch.int32).reshape(self.N))
        self._store_obs(self.observe(self.state))

    def episode_stats(self):
        """per-env device statistics (int64 [N] each): finished episodes, the sum of their lengths,
        the last finished length"""
        return self.stats[:, 0], self.stats[:, 1], self.stats[:, 2]

    def return_stats(self):
        """per-env device statistics (float64 [N] each): the running episode's return, the sum of
        the finished episodes' returns, the last finished return"""
        return self.ret_stats[:, 0], self.ret_stats[:, 1], self.ret_stats[:, 2]
