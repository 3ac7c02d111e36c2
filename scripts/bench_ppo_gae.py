"""Microbench (development aid): GAE(lambda) on the device PPO loop (csrc/ppo_actor.hpp
rth_ppo_gae_finish, csrc/ppo.hpp rth_ppo_grads_adv / rth_ppo_adv_normalize, reth_amd/ppo_loop.py) at
the CartPole shape (D = 4, A = 2, H = 64).  HIP events after a warm-up, three interleaved rounds
(host launch time included: the events bracket the whole window):

  - finish_gae() at 10 envs x 200 rows and 64 x 32 beside finish() at 10 x 200, each after a
    rollout that fills the segments (the rollout is outside the events), and finish_gae() of one
    env at cap 4096 (the serial fp64 scan's longest case);
  - one epoch at B = 2,000 rows as update_device issues it (grads + two Adam steps, k_epochs = 1)
    through rth_ppo_grads_adv beside rth_ppo_grads, PPOG_REPS (default 100) repetitions;
  - rth_ppo_adv_normalize at n = 2,048 and 65,536 rows;
  - one GAE iteration at 64 x 32 (32 steps + finish_gae + normalise + the update of 4 epochs), eager
    and as a replayed graph, beside the default iteration at 10 x 200;
  - examples/cartpole_ppo_gae_hip.py for 50 updates, seeds 0 / 1 / 2, eager, and seed 0 --graph
    (wall clock; the example prints the lengths)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from reth_amd._lib import call, ptr, stream_ptr  # noqa: E402
from reth_amd.ppo import PPOSolver  # noqa: E402
from reth_amd.ppo_actors import VecPpoActors  # noqa: E402
from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig  # noqa: E402
from reth_amd.solver import Box, Discrete  # noqa: E402

dev = torch.device("cuda")
REPS = int(os.environ.get("PPOG_REPS", "100"))
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
    # the finishes: each timed call ends one fresh rollout
    sets = {"finish 10 x 200": (VecPpoActors("CartPole-v0", 10, 200, device=dev), 200, False),
            "finish_gae 10 x 200": (VecPpoActors("CartPole-v0", 10, 200, device=dev, cap=200), 200, True),
            "finish_gae 64 x 32": (VecPpoActors("CartPole-v0", 64, 32, device=dev, cap=32), 32, True)}
    res = {k: [] for k in sets}
    for _ in range(3 + 9):
        for k, (act, steps, gae) in sets.items():
            for _ in range(steps):
                act.step(s)
            fn = (lambda act=act: act.finish_gae(s, 0.99, 0.95)) if gae else (lambda act=act: act.finish(0.99))
            res[k].append(timed(fn, 1))
    for k, v in res.items():
        print(f"{k} (one call between two events, after its rollout): " + " / ".join(f"{t:.1f}" for t in v[3:]) + " us",
              flush=True)
    long = VecPpoActors("CartPole-v0", 1, 4096, device=dev, cap=4096, max_episode_steps=200)
    t = []
    for _ in range(2 + 5):
        long.fill.fill_(4096)  # (rows of zeros: the scan's time does not depend on the values)
        t.append(timed(lambda: long.finish_gae(s, 0.99, 0.95), 1))
    print("finish_gae 1 x 4096 (the serial scan's longest case): " + " / ".join(f"{v:.1f}" for v in t[2:]) + " us",
          flush=True)
    # grads_adv beside grads
    s1, s2 = solver(1), solver(1)
    n = 2000
    g = torch.Generator().manual_seed(1)
    cols = [torch.randn(n, 4, generator=g).to(dev), torch.randint(0, 2, (n,), generator=g).to(dev),
            torch.randn(n, generator=g).to(dev), (-0.69 + 0.1 * torch.randn(n, generator=g)).float().to(dev)]
    adv = torch.randn(n, generator=g).to(dev)
    best = rounds(f"one epoch at B={n} rows (grads + two Adam steps)",
                  {"rth_ppo_grads": lambda: s1.update_device(cols),
                   "rth_ppo_grads_adv": lambda: s2.update_device(cols + [adv])})
    a, b = best["rth_ppo_grads"], best["rth_ppo_grads_adv"]
    print(f"  rth_ppo_grads_adv over rth_ppo_grads, best of 3: {b - a:+.1f} us ({b / a:.3f}x)", flush=True)
    # the normalisation
    big = torch.randn(65536, device=dev)
    counts = {n: torch.tensor([n], dtype=torch.int64, device=dev) for n in (2048, 65536)}
    rounds("rth_ppo_adv_normalize", {f"n={n}": (lambda c=c: call("rth_ppo_adv_normalize", ptr(big), 65536, ptr(c),
                                                                 stream_ptr())) for n, c in counts.items()})
    # one iteration, eager and replayed
    gae_cfg = dict(n_actors=64, horizon=32, gae_lambda=0.95, normalize_adv=True)
    loops = {"GAE 64 x 32 eager": PpoLoop(PpoLoopConfig(**gae_cfg), device=dev),
             "GAE 64 x 32 graph": PpoLoop(PpoLoopConfig(**gae_cfg), device=dev),
             "default 10 x 200 eager": PpoLoop(PpoLoopConfig(), device=dev),
             "default 10 x 200 graph": PpoLoop(PpoLoopConfig(), device=dev)}
    for k, loop in loops.items():
        loop.iteration()
        if k.endswith("graph"):
            loop.capture()
    rounds("PpoLoop iteration (2,048 / 2,000 env steps + finish + update)", {k: v.iteration for k, v in loops.items()},
           reps=50, unit="ms", scale=1e-3)
    import cartpole_ppo_gae_hip as example

    for seed, graph_on in ((0, False), (1, False), (2, False), (0, True)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        example.main(50, seed, graph_on)
        print(f"examples/cartpole_ppo_gae_hip.py --updates 50 --seed {seed}{' --graph' if graph_on else ''}: "
              f"{time.perf_counter() - t0:.2f} s wall (construction and the untrained rollout included)", flush=True)


if __name__ == "__main__":
    main()
