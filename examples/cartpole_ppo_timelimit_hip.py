"""PPO with GAE(lambda) that bootstraps through time-limit episode ends (reth_amd.ppo_loop.PpoLoop
with gae_lambda and bootstrap_time_limit).  CartPole-v0 ends an episode that survives 200 steps --
the success case -- and GAE as it stood scored that last state as if the pole had fallen.  Here the
step records which done rows the limit alone ended and the observation they ended on, and the finish
bootstraps those rows from the value of that observation.  64 envs x 32 steps per update, as
examples/cartpole_ppo_gae_hip.py; one stream, no host synchronisation, optionally one HIP graph per
update.

    python examples/cartpole_ppo_timelimit_hip.py [--updates 50] [--seed S] [--graph] [--env CartPole-v0]
                                                  [--n-actors 64] [--horizon 32] [--gae-lambda 0.95]
                                                  [--no-bootstrap]

(examples/cartpole_ppo_timelimit.yaml holds these values; --no-bootstrap is cartpole_ppo_gae_hip.py's
estimator, for comparison.)

Prints the envs' mean last finished episode length (CartPole-v0's return; at most 200), the same
number for the untrained actor, and the rows of the last rollout that the time limit truncated.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig  # noqa: E402

MAX_UPDATES = 50


def main(updates=MAX_UPDATES, seed=0, graph=False, env="CartPole-v0", n_actors=64, horizon=32, gae_lambda=0.95,
         bootstrap=True):
    cfg = PpoLoopConfig(env=env, n_actors=n_actors, horizon=horizon, seed=seed, gae_lambda=gae_lambda,
                        normalize_adv=True, bootstrap_time_limit=bootstrap)
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
    truncated = int(act.seg_trunc.sum()) if bootstrap else 0  # (the last rollout's rows stay in the segments)
    print(f"cartpole_ppo_timelimit updates={loop.updates} seed={seed} graph={int(graph and updates > 1)} env={env} "
          f"n_actors={n_actors} horizon={horizon} gae_lambda={gae_lambda} bootstrap_time_limit={int(bootstrap)} "
          f"env_steps={loop.env_steps} episodes={int(act.episode_stats()[0].sum())} mean_last_len={last:.1f} "
          f"untrained_mean_last_len={untrained:.1f} truncated_rows={truncated} dropped={int(act.dropped.sum())} "
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
    ap.add_argument("--no-bootstrap", action="store_true")
    args = ap.parse_args()
    main(args.updates, args.seed, args.graph, args.env, args.n_actors, args.horizon, args.gae_lambda,
         not args.no_bootstrap)
