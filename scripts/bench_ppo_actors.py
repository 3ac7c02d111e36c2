"""Microbench (development aid): the device PPO rollout (csrc/ppo_actor.hpp, reth_amd/ppo_loop.py) at
the CartPole shape (D = 4, A = 2, H = 64), interleaved, three rounds of PPOA_REPS (default 100; 50
for a whole iteration) repetitions between two HIP events after a warm-up (host launch time
included: the events bracket the whole window):

  - the actor step at N = 10 / 64 / 256 beside rth_ppo_act (act_batch) at the same n;
  - finish() at N = 10, after a rollout of 200 steps each time (the rollout is outside the events);
  - rth_ppo_grads_n beside rth_ppo_grads at the same n = 2,000 rows (capacity 3,990), one epoch
    as update_device issues it (grads + two Adam steps) with k_epochs = 1;
  - one PpoLoop iteration (10 envs x 200 steps + finish + the update of 4 epochs) eager and as a
    replayed graph, beside the host loop of examples/cartpole_ppo_hip.py --impl hip for the same
    2,000 env steps + one update (wall clock, one update after one warm-up update);
  - examples/cartpole_ppo_loop_hip.py for 50 updates, eager and --graph (wall clock).

PPOA_SKIP_HOST=1 leaves the host loop out (it takes about a second per update)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from reth_amd.ppo import PPOSolver  # noqa: E402
from reth_amd.ppo_actors import VecPpoActors  # noqa: E402
from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig  # noqa: E402
from reth_amd.solver import Box, Discrete  # noqa: E402

dev = torch.device("cuda")
REPS = int(os.environ.get("PPOA_REPS", "100"))
OBS, ACT = Box(-1, 1, (4,)), Discrete(2)


def timed(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def rounds(name, fns, reps=REPS, unit="us", scale=1.0):
    """three interleaved rounds of every fn -> prints one line; returns the best of each"""
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(3):
        for k, fn in fns.items():
            res[k].append(timed(fn, reps) * scale)
    print(f"{name}: " + "  ".join(f"{k} {' / '.join(f'{t:.1f}' for t in v)} {unit}" for k, v in res.items()), flush=True)
    return {k: min(v) for k, v in res.items()}


def solver(k_epochs=4):
    torch.manual_seed(0)
    return PPOSolver(OBS, ACT, k_epochs=k_epochs, device=dev, impl="hip")


def main():
    s = solver()
    for n in (10, 64, 256):
        act = VecPpoActors("CartPole-v0", n, 200, device=dev)
        obs = torch.randn(n, 4, device=dev)

        def step(act=act):
            if act.pushes % 200 == 0:  # (keeps the segments from filling: the reset is one more launch in 200)
                act.reset()
            act.step(s)

        rounds(f"actor step N={n}", {"rth_ppo_actor_step": step, "rth_ppo_act (act_batch)": lambda: s.act_batch(obs)})
    # finish
    act = VecPpoActors("CartPole-v0", 10, 200, device=dev)
    res = []
    for _ in range(3 + 9):
        for _ in range(200):
            act.step(s)
        res.append(timed(lambda: act.finish(0.99), 1))
    print("finish N=10 after 200 steps (one launch between two events): " +
          " / ".join(f"{t:.1f}" for t in res[3:]) + " us", flush=True)
    # grads_n beside grads
    s1, s2 = solver(1), solver(1)
    cap, n = 3990, 2000
    g = torch.Generator().manual_seed(1)
    cols = [torch.randn(cap, 4, generator=g).to(dev), torch.randint(0, 2, (cap,), generator=g).to(dev),
            torch.randn(cap, generator=g).to(dev), (-0.69 + 0.1 * torch.randn(cap, generator=g)).float().to(dev)]
    head = [c[:n].contiguous() for c in cols]
    n_dev = torch.tensor([n], dtype=torch.int64, device=dev)
    best = rounds(f"one epoch at n={n} rows (grads + two Adam steps)",
                  {"rth_ppo_grads B=n": lambda: s1.update_device(head),
                   f"rth_ppo_grads_n capacity {cap}": lambda: s2.update_device(cols, n_rows=n_dev)})
    a, b = best["rth_ppo_grads B=n"], best[f"rth_ppo_grads_n capacity {cap}"]
    print(f"  rth_ppo_grads_n over rth_ppo_grads, best of 3: {b - a:+.1f} us ({b / a:.3f}x)", flush=True)
    # one iteration, eager and replayed
    eager, graph = PpoLoop(PpoLoopConfig(), device=dev), PpoLoop(PpoLoopConfig(), device=dev)
    graph.iteration()
    graph.capture()
    it = rounds("PpoLoop iteration (2,000 env steps + finish + update)", {"eager": eager.iteration, "graph": graph.iteration},
                reps=50, unit="ms", scale=1e-3)
    if not os.environ.get("PPOA_SKIP_HOST"):
        import cartpole_ppo_hip as host

        t = []
        for updates in (1, 2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            host.main(updates, "hip", 0, quiet=True)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        per = (t[1] - t[0]) * 1e3
        print(f"host loop (examples/cartpole_ppo_hip.py --impl hip), one update of 2,000 env steps: {per:.0f} ms wall "
              f"(2 updates {t[1]:.2f} s - 1 update {t[0]:.2f} s); over the device iteration: eager "
              f"{per / it['eager']:.1f}x, graph {per / it['graph']:.1f}x", flush=True)
    import cartpole_ppo_loop_hip as example

    for graph_on in (False, True):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        example.main(50, 0, graph_on)
        print(f"examples/cartpole_ppo_loop_hip.py --updates 50{' --graph' if graph_on else ''}: "
              f"{time.perf_counter() - t0:.2f} s wall (construction and the untrained rollout included)", flush=True)


if __name__ == "__main__":
    main()
