"""Microbench (development aid): the device classic-control loops (reth_amd/mlp_apex.py with
MlpApexConfig.env; csrc/env_actor.hpp) on one GPU, in this process, timed as
scripts/bench_mlp_actors.py times the CartPole loop -- three rounds over all cases in turn after a
warm-up, each figure a host clock around a window that ends in a device synchronise:

  actor step alone        one launch at N = 64: rth_mlp_actor_step (CartPole) and rth_env_actor_step
                          (CartPole, Acrobot, MountainCar)
  whole iteration         MlpApexDQN at N = 64, B = 64, eager and as a replayed HIP graph, for
                          CartPole-v0 (the loop as it was), Acrobot-v1 and MountainCar-v0

then the Acrobot learning curve of tests/test_mlp_apex_envs_gpu.py::test_learns_acrobot (seed 0,
greedy_eval(256) every 1,000 iterations up to CC_CURVE_ITERS, default 20,000; CC_CURVE_ITERS=0
skips it).

With CC_TRACE_ITERS=K and CC_TRACE_ENV=<env> the script only issues K eager steady-state
iterations of that env's loop (for a kernel trace: kernel calls / K = launches per iteration; run
it twice with different K to count the warm-up apart)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reth_amd import model  # noqa: E402
from reth_amd.mlp_actors import ENVS, VecCartPoleActors, VecMlpActors  # noqa: E402
from reth_amd.mlp_apex import MlpApexConfig, MlpApexDQN  # noqa: E402

REPS = int(os.environ.get("CC_REPS", "300"))
CURVE_ITERS = int(os.environ.get("CC_CURVE_ITERS", "20000"))
LOOP_ENVS = ["CartPole-v0", "Acrobot-v1", "MountainCar-v0"]


def window(fn, reps):
    """microseconds per call of fn over reps calls, host clock, synchronised at both ends"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def rounds(cases):
    """cases: name -> (fn, calls per window, warm-up calls); three rounds over all of them in turn"""
    res = {k: [] for k in cases}
    for fn, _, warm in cases.values():
        for _ in range(warm):
            fn()
    for _ in range(3):
        for k, (fn, reps, _) in cases.items():
            res[k].append(window(fn, reps))
    for k, v in res.items():
        print(f"{k}: {' / '.join(f'{t:.1f}' for t in v)} us  (median {sorted(v)[1]:.1f})", flush=True)


def make_loop(**cfg):
    model.MLP_IMPL = "hip"
    try:
        return MlpApexDQN(MlpApexConfig(**cfg))
    finally:
        model.MLP_IMPL = None


def device_loop(env, graph):
    loop = make_loop(env=env, n_actors=64, batch_size=64, seed=0)
    while not loop.graph_ready():
        loop.iteration()
    loop.run(5)
    if graph:
        loop.capture()
    return loop


def acrobot_curve(iterations, every=1000, **cfg):
    """the greedy mean first-episode length and return every `every` iterations (the graph is
    captured as soon as the loop is in its steady state)"""
    loop = make_loop(env="Acrobot-v1", n_actors=64, batch_size=64, learning_rate=1e-3, update_target_interval=200,
                     seed=0, **cfg)
    t0 = time.perf_counter()
    for k in range(iterations // every):
        for _ in range(every):
            if loop._graph is None and loop.graph_ready():
                loop.capture()
            loop.iteration()
        length, ret = loop.greedy_eval(256), loop.greedy_eval(256, metric="return")
        print(f"  {cfg} after {(k + 1) * every} iterations: greedy mean length {length:.1f}, return {ret:.1f} "
              f"({loop.updates} updates, {loop.env_steps} env steps, {time.perf_counter() - t0:.1f} s)", flush=True)


def main():
    dev = torch.device("cuda")
    print(f"device: {torch.cuda.get_device_name(0)}; windows of {REPS} calls", flush=True)
    if os.environ.get("CC_TRACE_ITERS"):
        K, env = int(os.environ["CC_TRACE_ITERS"]), os.environ.get("CC_TRACE_ENV", "Acrobot-v1")
        loop = device_loop(env, graph=False)
        before = loop.iterations
        loop.run(K)
        torch.cuda.synchronize()
        print(f"{env}: {K} eager steady-state iterations after {before} warm-up iterations ({loop.updates} updates in "
              f"all)", flush=True)
        return
    cases = {}
    torch.manual_seed(0)
    net = model.MLP_DQNNetwork((4,), 2).to(dev).requires_grad_(False)
    old = VecCartPoleActors(64, seed=1, device=dev)
    cases["actor step alone N=64, CartPole, rth_mlp_actor_step"] = ((lambda: old.step(net)), REPS, 50)
    for env in LOOP_ENVS:
        _, D, A, _ = ENVS[env]
        n = model.MLP_DQNNetwork((D,), A).to(dev).requires_grad_(False)
        a = VecMlpActors(env, 64, seed=1, device=dev)
        cases[f"actor step alone N=64, {env}, rth_env_actor_step"] = ((lambda a=a, n=n: a.step(n)), REPS, 50)
    loops = []
    for env in LOOP_ENVS:
        eager, graph = device_loop(env, False), device_loop(env, True)
        loops.append((env, eager))
        cases[f"{env} loop iteration, eager (64 env steps + one B=64 update)"] = (eager.iteration, REPS, 20)
        cases[f"{env} loop iteration, graph replay"] = (graph.iteration, REPS, 20)
    rounds(cases)
    for env, eager in loops:
        print(f"{env} host counters: {eager.actors.launches} actor launches in {eager.iterations} iterations; solver HIP "
              f"calls per steady-state iteration: 2", flush=True)
    if CURVE_ITERS:
        print("Acrobot-v1 learning curves (N = 64, B = 64, lr 1e-3, target interval 200, seed 0):", flush=True)
        acrobot_curve(CURVE_ITERS, n_step=1)
        acrobot_curve(CURVE_ITERS, n_step=3)


if __name__ == "__main__":
    main()
