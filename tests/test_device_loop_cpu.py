"""device_loop.OneStreamLoop without a GPU: MlpApexDQN's and DdpgApex's host bookkeeping driven with
stub actors against the rule written out here -- which iterations fill, emit rows, learn, and when
the loop is graph-ready."""
from types import SimpleNamespace

import pytest

from reth_amd.ddpg_apex import DdpgApex
from reth_amd.device_loop import OneStreamLoop
from reth_amd.mlp_apex import MlpApexDQN

N, ITERS = 4, 12


class StubActors:
    def __init__(self, n_step):
        self.N, self.pushes, self.launches = N, 0, 0
        if n_step is not None:
            self.n_step = n_step

    def step(self, net):
        self.pushes += 1
        self.launches += 1


def _stub(base, n_step, sample_start, capacity):
    class Stub(base):
        def __init__(self):
            cfg = SimpleNamespace(env="stub", sample_start=sample_start, batch_size=2, capacity=capacity, seed=0,
                                  max_episode_steps=None)
            OneStreamLoop.__init__(self, cfg, "cpu", {"stub": (0, 1, 1, 5)})
            self.actors = StubActors(n_step)
            self.solver = SimpleNamespace(q_network=None)
            self.target_calls = 0
            self._updated = self._count_target
            self.learns = []

        def _count_target(self):
            self.target_calls += 1

        def _body(self, learn):
            self.actors.step(None)
            self.learns.append(learn)
            return "td" if learn else None

    return Stub()


@pytest.mark.parametrize("sample_start,capacity", [(10, 64), (10, 16), (20, 16)])
@pytest.mark.parametrize("n_step", [None, 1, 3])
def test_iteration_follows_the_rule(n_step, sample_start, capacity):
    loop = _stub(DdpgApex if n_step is None else MlpApexDQN, n_step, sample_start, capacity)
    n = n_step or 0
    assert loop.max_episode_steps == 5 and not loop.graph_ready()
    updates = solver_calls = 0
    for k in range(1, ITERS + 1):
        bodies = len(loop.learns)
        loop.iteration()
        filling = k <= n
        rows = N * max(0, k - n)
        learn = min(rows, capacity) >= sample_start
        updates += learn
        assert (len(loop.learns) == bodies) == filling, k
        if not filling:
            assert loop.learns[-1] is learn, k
            solver_calls += 2 if learn else 1
        assert (loop.iterations, loop.env_steps, loop.rows_emitted, loop.updates) == (k, N * k, rows, updates), k
        assert loop.actors.pushes == loop.actors.launches == k
        ready = k + 1 > n and min(rows + N, capacity) >= sample_start and updates >= 1
        assert loop.graph_ready() is ready, k
        if not filling:
            assert loop.last_td == ("td" if learn else None), k
        if n_step is not None:
            assert (loop.solver_calls, loop.target_calls) == (solver_calls, updates), k
    if capacity < sample_start:
        assert updates == 0 and not loop.graph_ready()
    else:
        assert updates >= 1 and loop.graph_ready()


@pytest.mark.parametrize("base,n_step", [(DdpgApex, None), (MlpApexDQN, 3)])
def test_capture_before_the_steady_state_is_refused(base, n_step, monkeypatch):
    import torch

    def touched(*a, **kw):
        raise AssertionError("capture() touched the device before its steady-state check")

    for name in ("CUDAGraph", "Stream", "current_stream", "graph"):
        monkeypatch.setattr(torch.cuda, name, touched)
    loop = _stub(base, n_step, 10, 64)
    loop.run(2)
    assert not loop.graph_ready()
    with pytest.raises(RuntimeError, match="steady-state"):
        loop.capture()
    assert loop._graph is None and loop.iterations == 2


@pytest.mark.parametrize("base,n_step,counter,launches", [(DdpgApex, None, "hip_launches", 3),
                                                         (MlpApexDQN, 3, "mlp_hip_launches", 2)])
def test_a_replay_advances_exactly_the_mirrors_a_capture_puts_back(base, n_step, counter, launches):
    from reth_amd.schedule import Schedule

    loop = _stub(base, n_step, 10, 64)
    loop.solver = SimpleNamespace(q_network=None, **{counter: 40})
    loop.replay = SimpleNamespace(alpha=Schedule.from_str("0.5,0.6,1000"), beta=Schedule.from_str("0.4,1,1000"))
    while not loop.graph_ready():
        loop.iteration()
    mirrors = loop._mirrors()
    assert [(o, a) for o, a in mirrors] == [(loop.actors, "pushes"), (loop.actors, "launches"), (loop.solver, counter),
                                           (loop.replay.alpha, "cur_step"), (loop.replay.beta, "cur_step")]
    before = [getattr(o, a) for o, a in mirrors]
    counts = (loop.iterations, loop.env_steps, loop.rows_emitted, loop.updates)
    bodies, replays, calls = len(loop.learns), [], getattr(loop, "solver_calls", None)
    loop._graph = SimpleNamespace(replay=lambda: replays.append(1))  # what capture() installs
    loop.run(3)
    assert len(replays) == 3 and len(loop.learns) == bodies
    assert [getattr(o, a) for o, a in mirrors] == [v + 3 * d for v, d in zip(before, (1, 1, launches, 1, 1))]
    assert (loop.iterations, loop.env_steps, loop.rows_emitted, loop.updates) == tuple(
        c + 3 * d for c, d in zip(counts, (1, N, N, 1)))
    if n_step is not None:
        assert loop.solver_calls == calls + 3 * 2 and loop.target_calls == loop.updates
