"""Acrobot DQN entirely on the device: vectorised Acrobot-v1 actors (the generic classic-control
step, csrc/env_actor.hpp), the PER replay and the MLP learner on the fused HIP kernels, one
stream, no host synchronisation in the loop (reth_amd/mlp_apex.py with env="Acrobot-v1").  The
iterations run eagerly until the loop is in its steady state, then as one replayed HIP graph.

    python examples/acrobot_apex_hip.py [iterations]

Prints env-steps/s, updates/s and the greedy policy's mean return (ε = 0, a separate set of envs;
-1 a step until the tip swings above the bar, -500 at the time limit) every `eval_every` iterations.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from reth_amd import model  # noqa: E402

ITERATIONS = 12000


def main(iterations=ITERATIONS, eval_every=1000, eval_envs=256, graph=True, **cfg):
    from reth_amd.mlp_apex import MlpApexConfig, MlpApexDQN

    cfg.setdefault("env", "Acrobot-v1")
    cfg.setdefault("n_step", 3)  # the configuration of profiles/r11/classic_control.txt's curve
    prev, model.MLP_IMPL = model.MLP_IMPL, "hip"  # read by DQNSolver at construction
    try:
        loop = MlpApexDQN(MlpApexConfig(**cfg))
    finally:
        model.MLP_IMPL = prev
    done = 0
    while done < iterations:
        k = min(eval_every, iterations - done)
        torch.cuda.synchronize()
        steps0, upd0, t0 = loop.env_steps, loop.updates, time.perf_counter()
        for _ in range(k):
            if graph and loop._graph is None and loop.graph_ready():
                loop.capture()
            loop.iteration()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        done += k
        print(f"iteration {done}: {(loop.env_steps - steps0) / dt:,.0f} env-steps/s, {(loop.updates - upd0) / dt:,.0f} "
              f"updates/s, greedy mean return {loop.greedy_eval(eval_envs, metric='return'):.1f}"
              f"{' (graph)' if loop._graph is not None else ''}")
    return loop


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else ITERATIONS)
