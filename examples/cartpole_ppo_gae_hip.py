"""PPO with GAE(lambda) on the device loop (reth_amd.ppo_loop.PpoLoop with gae_lambda): many envs
on short fixed rollouts.  64 envs x 32 steps per update, advantages from GAE(0.95) with the value
network's bootstrap at the rollout's edge, normalised over the batch; every stored row reaches the
learner at once, and nothing waits for an episode to end.  One stream, no host synchronisation,
optionally one HIP graph per update.

    python examples/cartpole_ppo_gae_hip.py [--updates 50] [--seed S] [--graph] [--env CartPole-v0]
                                            [--n-actors 64] [--horizon 32] [--gae-lambda 0.95]

(examples/cartpole_ppo_loop_hip.py is the reference's estimator, whole episodes' returns, on the
same loop; examples/cartpole_ppo_gae.yaml holds these values.)

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


def main(updates=MAX_UPDATES, seed=0, graph=False, env="CartPole-v0", n_actors=64, horizon=32, gae_lambda=0.95):
    cfg = PpoLoopConfig(env=env, n_actors=n_actors, horizon=horizon, seed=seed, gae_lambda=gae_lambda,
                        normalize_adv=True)
    loop = PpoLoop(cfg, impl="hip")
    untrained = loop.rollout_length()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(updates):
        if graph and k == 1:
            loop.capture()
        loop.iteration()
    last = loop.mean_last_length()  # (the host read waits for the stream)
    seconds = time.perf_counter() - t0
    act = loop.actors
    launches = loop.solver.hip_launches + act.launches + act.finishes + act.normalizes
    print(f"cartpole_ppo_gae updates={loop.updates} seed={seed} graph={int(graph and updates > 1)} env={env} "
          f"n_actors={n_actors} horizon={horizon} gae_lambda={gae_lambda} env_steps={loop.env_steps} "
          f"episodes={int(act.episode_stats()[0].sum())} mean_last_len={last:.1f} "
          f"untrained_mean_last_len={untrained:.1f} dropped={int(act.dropped.sum())} "
          f"hip_launches={launches} seconds={seconds:.2f}")
    return loop, last, untrained


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--updates", type=int, default=MAX_UPDATES)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--env", default="CartPole-v0")
    ap.add_argument("--n-actors", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=32)
    ap.add_argument("--gae-lambda", type=float, default=0.95)
    args = ap.parse_args()
    main(args.updates, args.seed, args.graph, args.env, args.n_actors, args.horizon, args.gae_lambda)
