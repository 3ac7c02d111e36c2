"""Microbench (development aid): the device Pendulum DDPG loop (reth_amd/ddpg_apex.py) at its
default configuration -- 64 device envs, B = 64, capacity 100,000 -- beside the host loop of
examples/pendulum_ddpg_hip.py --impl hip (one numpy Pendulum, 64 rth_ddpg_act launches with a
device-to-host read each, then one update), both in this process on one GPU.

Per iteration (64 env steps, one prioritized sample, one update), after a warm-up into the steady
state: DDPG_ACTORS_REPS (default 300) iterations, each between its own pair of HIP events (device
loop: eager, and replayed as one HIP graph) or host clock readings (host loop: it synchronises on
every act); median, 10th / 90th percentile, and the whole window's wall time per iteration.

The actor-step kernel's own time beside rth_ddpg_act at n = 64: each captured ten times into a HIP
graph, replayed between two events, three interleaved rounds.

With DDPG_ACTORS_TRACE=K the script only issues K eager steady-state iterations after the warm-up
(for a kernel trace: launches per iteration)."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from reth_amd.ddpg_apex import DdpgApex, DdpgApexConfig  # noqa: E402

REPS = int(os.environ.get("DDPG_ACTORS_REPS", "300"))
WARM = 100


def stats(v):
    v = np.asarray(v)
    return f"median {np.median(v):.1f} us  p10 {np.percentile(v, 10):.1f}  p90 {np.percentile(v, 90):.1f}"


def device_loop(graph):
    loop = DdpgApex(DdpgApexConfig(seed=0), impl="hip")
    while not loop.graph_ready():
        loop.iteration()
    if graph:
        loop.capture()
    loop.run(WARM)
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(REPS)]
    t0 = time.perf_counter()
    for e0, e1 in ev:
        e0.record()
        loop.iteration()
        e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e6 / REPS
    per = [e0.elapsed_time(e1) * 1e3 for e0, e1 in ev]
    return loop, per, wall


def host_loop():
    """examples/pendulum_ddpg_hip.py's loop, its iteration timed"""
    import pendulum_ddpg_hip as ex
    from reth_amd import envs
    from reth_amd.presets import get_replay_buffer, get_solver, get_trainer, get_worker

    torch.manual_seed(0)
    np.random.seed(0)
    env = envs.make_host("Pendulum-v0", seed=0)
    solver = get_solver(ex.CONFIG, env=env, impl="hip", cast_actions_to_long=False)
    worker = get_worker(ex.CONFIG, solver=solver, env=env, logger=False)
    trainer = get_trainer(ex.CONFIG, solver=solver, logger=False)
    buffer = get_replay_buffer(ex.CONFIG, device=solver.device)
    buffer.append_batch(worker.step_batch(1000))

    def iteration():
        buffer.append_batch(worker.step_batch(ex.BATCH_SIZE))
        data, indices, weights = buffer.sample(ex.BATCH_SIZE)
        loss = trainer.step(data, weights=weights)
        buffer.update_priorities(indices, loss)

    for _ in range(20):
        iteration()
    torch.cuda.synchronize()
    per = []
    t_all = time.perf_counter()
    for _ in range(REPS):
        t0 = time.perf_counter()
        iteration()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e6)
    wall = (time.perf_counter() - t_all) * 1e6 / REPS
    return per, wall


def kernel_times(loop):
    """the actor step (act + noise + env, N = 64) and rth_ddpg_act (n = 64) as graphs of ten launches"""
    act, solver = loop._make_actors(64, epsilon="1,0.01,30000", seed=1), loop.solver
    obs = act.current_obs()
    fns = {"rth_ddpg_actor_step N=64": lambda: act.step(solver), "rth_ddpg_act n=64": lambda: solver.act_batch(obs)}
    graphs = {}
    for name, fn in fns.items():
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(10):
                fn()
        graphs[name] = g
    res = {k: [] for k in graphs}
    for g in graphs.values():
        for _ in range(5):
            g.replay()
    torch.cuda.synchronize()
    for _ in range(3):
        for name, g in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(30):
                g.replay()
            e1.record()
            torch.cuda.synchronize()
            res[name].append(e0.elapsed_time(e1) * 1e3 / 300)
    for name, v in res.items():
        print(f"{name} (graph of 10, 30 replays): {' / '.join(f'{t:.1f}' for t in v)} us per launch", flush=True)


def main():
    if os.environ.get("DDPG_ACTORS_TRACE"):
        K = int(os.environ["DDPG_ACTORS_TRACE"])
        loop = DdpgApex(DdpgApexConfig(seed=0), impl="hip")
        while not loop.graph_ready():
            loop.iteration()
        warm = loop.iterations
        loop.run(K)
        torch.cuda.synchronize()
        print(f"{warm} warm-up iterations ({loop.updates - K} with an update), then {K} eager steady-state iterations",
              flush=True)
        return
    print(f"{torch.cuda.get_device_name(0)}; {REPS} timed iterations after {WARM} steady-state warm-up iterations",
          flush=True)
    res = {}
    for name, graph in (("device loop, eager", False), ("device loop, one replayed graph", True)):
        loop, per, wall = device_loop(graph)
        res[name] = (np.median(per), wall)
        print(f"{name}: per iteration (events) {stats(per)}; window wall {wall:.1f} us per iteration", flush=True)
    per, wall = host_loop()
    res["host"] = (np.median(per), wall)
    print(f"host loop (examples/pendulum_ddpg_hip.py --impl hip: 64 host env steps + one update): per iteration "
          f"(host clock) {stats(per)}; window wall {wall:.1f} us per iteration", flush=True)
    for name in ("device loop, eager", "device loop, one replayed graph"):
        print(f"host loop / {name}: {res['host'][1] / res[name][1]:.2f}x by window wall time, "
              f"{res['host'][0] / res[name][0]:.2f}x by medians", flush=True)
    kernel_times(loop)


if __name__ == "__main__":
    main()
