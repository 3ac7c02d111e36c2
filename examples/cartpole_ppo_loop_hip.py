"""The reference's examples/ppo/run.py loop (CartPole-v0, PPO) with the rollout on the device:
reth_amd.ppo_loop.PpoLoop.  N envs step in one launch per env step, the finished episodes' returns
and the batch are built on the device, and the update takes its row count from the device: one
stream, no host synchronisation, optionally one HIP graph per update.

    python examples/cartpole_ppo_loop_hip.py [--updates 50] [--seed S] [--graph] [--n-actors N] [--horizon T]

The defaults, 10 envs x 200 steps, are the reference's 2,000 env steps per update
(examples/cartpole_ppo_hip.py is that loop on the host, one env step at a time).

Prints the envs' mean last finished episode length (CartPole-v0's return; at most 200) and the same
number for the untrained actor.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig  # noqa: E402

MAX_UPDATES = 50


def main(updates=MAX_UPDATES, seed=0, graph=False, n_actors=10, horizon=200):
    loop = PpoLoop(PpoLoopConfig(n_actors=n_actors, horizon=horizon, seed=seed), impl="hip")
    untrained = loop.rollout_length()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(updates):
        if graph and k == 1:
            loop.capture()
        loop.iteration()
    last = loop.mean_last_length()  # (the host read waits for the stream)
    seconds = time.perf_counter() - t0
    launches = loop.solver.hip_launches + loop.actors.launches + loop.actors.finishes
    print(f"cartpole_ppo_loop updates={loop.updates} seed={seed} graph={int(graph and updates > 1)} "
          f"n_actors={n_actors} horizon={horizon} env_steps={loop.env_steps} "
          f"episodes={int(loop.actors.episode_stats()[0].sum())} mean_last_len={last:.1f} "
          f"untrained_mean_last_len={untrained:.1f} dropped={int(loop.actors.dropped.sum())} "
          f"hip_launches={launches} seconds={seconds:.2f}")
    return loop, last, untrained


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=MAX_UPDATES)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--n-actors", type=int, default=10)
    ap.add_argument("--horizon", type=int, default=200)
    args = ap.parse_args()
    main(args.updates, args.seed, args.graph, args.n_actors, args.horizon)
