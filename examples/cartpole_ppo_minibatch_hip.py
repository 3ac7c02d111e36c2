"""PPO with shuffled minibatch epochs on the device loop (reth_amd.ppo_loop.PpoLoop with
n_minibatches): 64 envs x 32 steps per update, GAE(0.95) advantages normalised over the batch, and
each of the k_epochs passes over the 2,048 rows in a new random order, cut into 4 minibatches with
one optimiser step each -- 16 steps per update where the full-batch loop takes 4.  The order is drawn
on the device (rth_ppo_shuffle), so there is still one stream, no host synchronisation and,
optionally, one HIP graph per update, whose replays reshuffle.

    python examples/cartpole_ppo_minibatch_hip.py [--updates 50] [--seed S] [--graph] [--env CartPole-v0]
                                                  [--n-actors 64] [--horizon 32] [--gae-lambda 0.95]
                                                  [--n-minibatches 4] [--learning-rate 0.01]

(examples/cartpole_ppo_gae_hip.py is the same loop on full-batch epochs;
examples/cartpole_ppo_minibatch.yaml holds these values.)

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
LEARNING_RATE = 0.01


def main(updates=MAX_UPDATES, seed=0, graph=False, env="CartPole-v0", n_actors=64, horizon=32, gae_lambda=0.95,
         n_minibatches=4, learning_rate=LEARNING_RATE):
    cfg = PpoLoopConfig(env=env, n_actors=n_actors, horizon=horizon, seed=seed, gae_lambda=gae_lambda,
                        normalize_adv=True, n_minibatches=n_minibatches, learning_rate=learning_rate)
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
    print(f"cartpole_ppo_minibatch updates={loop.updates} seed={seed} graph={int(graph and updates > 1)} env={env} "
          f"n_actors={n_actors} horizon={horizon} gae_lambda={gae_lambda} n_minibatches={n_minibatches} "
          f"learning_rate={learning_rate} env_steps={loop.env_steps} shuffles={loop.solver.shuffle_calls} "
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
    ap.add_argument("--n-minibatches", type=int, default=4)
    ap.add_argument("--learning-rate", type=float, default=LEARNING_RATE)
    args = ap.parse_args()
    main(args.updates, args.seed, args.graph, args.env, args.n_actors, args.horizon, args.gae_lambda,
         args.n_minibatches, args.learning_rate)
