"""DdpgApex (reth_amd/ddpg_apex.py): the device Pendulum DDPG loop -- that it refuses to run
without the fused kernels, its bookkeeping, determinism, graph == eager, and the wiring between
the actors' rows, the replay and the update's priorities."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

CFG = dict(capacity=4096, n_actors=64, batch_size=64, sample_start=128)
K = 30


def _loop(impl=None, **kw):
    from reth_amd.ddpg_apex import DdpgApex, DdpgApexConfig

    return DdpgApex(DdpgApexConfig(**{**CFG, **kw}), device="cuda", impl=impl)


def _bytes(t):
    return t.detach().cpu().numpy().tobytes()


def _tensors(loop):
    """every parameter of the four nets, the Adam moments and step counts, the replay's priorities"""
    s = loop.solver
    out = {}
    for name, net in (("actor", s.actor), ("critic", s.critic), ("actor_target", s.actor_target),
                      ("critic_target", s.critic_target)):
        for k, p in net.named_parameters():
            out[f"{name}.{k}"] = p
    for name, net, opt in (("actor", s.actor, s.actor_optimizer), ("critic", s.critic, s.critic_optimizer)):
        for k, p in net.named_parameters():
            st = opt.state[p]
            out[f"{name}.{k}.exp_avg"], out[f"{name}.{k}.exp_avg_sq"] = st["exp_avg"], st["exp_avg_sq"]
            out[f"{name}.{k}.step"] = st["step"]
    for k, t in zip(("sum", "min", "value"), loop.replay.tree.export()):
        out[f"tree.{k}"] = t
    for k in ("state", "ep_steps", "t_dev", "stats", "ret_stats", "noise", "cur_obs"):
        out[f"actors.{k}"] = getattr(loop.actors, k)
    return out


def _host(loop):
    return dict(iterations=loop.iterations, env_steps=loop.env_steps, rows=loop.rows_emitted, updates=loop.updates,
                pushes=loop.actors.pushes, launches=loop.actors.launches, hip_launches=loop.solver.hip_launches,
                alpha=loop.replay.alpha.cur_step, beta=loop.replay.beta.cur_step)


def test_refuses_the_torch_path():
    with pytest.raises(RuntimeError, match="no torch fallback"):
        _loop(impl="torch")


def test_bookkeeping():
    loop = _loop(seed=3)
    N = CFG["n_actors"]
    assert loop.solver.impl_active == "hip" and loop.solver.cast_actions_to_long is False
    loop.iteration()
    assert loop.updates == 0 and loop.rows_emitted == N  # 64 rows stored: below sample_start
    assert not loop.graph_ready()
    loop.iteration()
    assert loop.updates == 1 and loop.rows_emitted == 2 * N  # the first iteration with >= 128 stored rows
    assert loop.graph_ready()
    loop.run(K - 2)
    torch.cuda.synchronize()
    assert loop.iterations == K and loop.env_steps == loop.rows_emitted == N * K and loop.updates == K - 1
    assert loop.replay.size == N * K
    assert loop.actors.launches == loop.actors.pushes == K and int(loop.actors.t_dev[0]) == K
    assert loop.solver.hip_launches == 3 * (K - 1)  # critic grads, actor grads, soft update per update
    # one schedule step per update (alpha is a constant: its one-step schedule stays at its end)
    assert loop.replay.beta.cur_step == K - 1 and loop.replay.info()[4] == K - 1 and loop.replay.alpha.cur_step == 1
    v = loop.replay.tree.export()[2]
    assert (v[:N * K] > 0).all() and (v[N * K:] == 0).all()
    assert int(loop.solver.actor_optimizer.state[loop.solver.actor.fc1.weight]["step"]) == K - 1


def test_two_loops_with_one_seed_agree():
    a, b = _loop(seed=5), _loop(seed=5)
    a.run(K)
    b.run(K)
    torch.cuda.synchronize()
    ta, tb = _tensors(a), _tensors(b)
    assert len(ta) == 24 + 36 + 3 + 7
    for k in ta:
        assert _bytes(ta[k]) == _bytes(tb[k]), k
    assert _host(a) == _host(b)
    assert float(ta["tree.value"].sum()) > 0 and int(ta["actor.fc1.weight.step"]) == K - 1


def test_graph_equals_eager():
    eager, graph = _loop(seed=7, max_episode_steps=9), _loop(seed=7, max_episode_steps=9)
    eager.run(K)
    with pytest.raises(RuntimeError, match="steady-state"):
        graph.capture()
    while not graph.graph_ready():
        graph.iteration()
    assert graph.iterations == 2
    graph.capture()
    assert graph._graph is not None and graph.iterations == 2 and graph.actors.launches == 2
    graph.run(K - graph.iterations)
    torch.cuda.synchronize()
    te, tg = _tensors(eager), _tensors(graph)
    for k in te:
        assert _bytes(te[k]) == _bytes(tg[k]), k
    assert _host(eager) == _host(graph)
    assert int(eager.actors.stats[:, 0].sum()) == 64 * (K // 9)  # episodes ended and reset under the graph too


def test_wiring_rows_priorities():
    from oracle import oracle as orc

    loop = _loop(seed=9)
    N, B = CFG["n_actors"], CFG["batch_size"]
    loop.iteration()  # no update yet: the stored rows carry the raw priority 1
    rows = [t.clone() for t in loop.actors.rows()]
    newest = torch.arange(0, N, device="cuda")
    for got, want in zip(loop.replay.gather(newest), rows):
        assert _bytes(got) == _bytes(want.reshape(got.shape))
    v = loop.replay.tree.export()[2]
    assert (v[:N] == 1.0).all() and (v[N:] == 0).all()
    for it in range(2, 6):
        loop.iteration()
        rows = [t.clone() for t in loop.actors.rows()]
        newest = torch.arange((it - 1) * N, it * N, device="cuda")
        for got, want in zip(loop.replay.gather(newest), rows):
            assert _bytes(got) == _bytes(want.reshape(got.shape))
        # the sampled rows' priorities are (|td| + 1e-6) ** alpha of this update's |td|; every other row keeps its own
        idx, td = loop.idx.cpu().numpy(), loop.last_td.cpu().numpy()
        assert idx.shape == (B,) and td.shape == (B,) and (idx >= 0).all() and (idx < it * N).all()
        want = orc.per_normalize(td.astype(np.float32), 0.6)
        v = loop.replay.tree.export()[2].cpu().numpy()
        uniq, counts = np.unique(idx, return_counts=True)
        once = np.isin(idx, uniq[counts == 1])
        assert once.sum() >= B // 2
        got = v[idx[once]].astype(np.float32)
        assert (np.abs(got - want[once]) <= np.spacing(np.abs(want[once]))).all()
        fresh = np.setdiff1d(np.arange((it - 1) * N, it * N), idx)
        assert (v[fresh] == 1.0).all() and (v[it * N:] == 0).all()
