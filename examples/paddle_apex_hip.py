"""Ape-X DQN on the conv path, learning the device-resident Paddle game (csrc/game.hpp,
VecActors(env="paddle")): the captured two-stream loop of reth_amd/apex.py -- 84x84x4 uint8 frame
stacks, frame-store replay, conv torso, dueling heads, TD / Huber, Adam, weights slot -- with a
real control problem in place of the synthetic frames.

    python examples/paddle_apex_hip.py [iterations]

Prints, at a few checkpoints, the greedy (ε = 0) policy's mean return over 256 separate eval envs
(each env's first episode) next to the random policy's over the same envs.  Returns lie in
[-balls, +balls]; a paddle that tracks the ball gets +balls.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

ITERATIONS = 60000
CHECKPOINTS = (0, 2500, 5000, 10000, 20000, 40000, 60000)


def main(iterations=ITERATIONS, checkpoints=CHECKPOINTS, eval_envs=256, **cfg):
    from reth_amd.apex import ApexConfig, ApexDQN

    base = dict(env="paddle", balls_per_episode=5, n_actors=256, num_actions=6, capacity=1 << 17, batch_size=512,
                sample_start=20000, update_target_interval=500, hip_graph=True, frame_store=True, seed=0)
    base.update(cfg)
    config = ApexConfig(**base)
    ax = ApexDQN(config, device=torch.device("cuda:0"))
    print(f"config: {config}")
    random = ax.greedy_eval(eval_envs, eps=1.0)
    print(f"random policy: mean return {random:+.2f} over {eval_envs} eval envs")
    marks = sorted({min(c, iterations) for c in checkpoints} | {iterations})
    done, busy, curve = 0, 0.0, []
    for mark in marks:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(mark - done):
            ax.iteration()
        torch.cuda.synchronize()
        busy += time.perf_counter() - t0
        done = mark
        ret = ax.greedy_eval(eval_envs)
        curve.append((done, ret))
        print(f"iteration {done}: greedy mean return {ret:+.2f} (random {random:+.2f}); {ax.updates} updates, "
              f"{ax.env_steps:,} env steps, {busy:.1f} s in the loop"
              f"{' (graph)' if ax._graphs is not None else ''}", flush=True)
    ax.close()
    return curve, random


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else ITERATIONS)
