"""Pendulum DDPG entirely on the device: vectorised Pendulum-v0 actors with Ornstein-Uhlenbeck
exploration (csrc/ddpg_actor.hpp), the PER replay and DDPG's update on the fused HIP kernels, one
stream, no host synchronisation in the loop (reth_amd/ddpg_apex.py).  The wiring is
examples/pendulum_ddpg_hip.py's -- the reference's examples/ddpg/run.py -- with 64 device envs in
place of the one host env: per iteration 64 env steps, one prioritized sample of 64, one update.

    python examples/pendulum_ddpg_apex_hip.py [--iterations N] [--seed S] [--graph] [--eval-every E]

--graph replays the steady-state iteration as one HIP graph once it is reached; without it every
iteration is issued eagerly.  Prints the greedy policy's mean return (no noise, a separate set of
256 envs, first episodes) every E iterations and at the end, beside a random policy's (uniform
torques in [-2, 2] on the same device envs).
"""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

ITERATIONS = 100000  # the reference's MAX_TS


@torch.no_grad()
def random_policy_return(loop, n_envs=256, seed=12345):
    """mean first-episode return of uniform random torques in [-2, 2] on a separate actor set"""
    ev = loop._make_actors(n_envs, epsilon=0.0, seed=seed)
    g = torch.Generator(device=ev.device)
    g.manual_seed(seed)
    for _ in range(ev.max_episode_steps):
        a = torch.rand((ev.N, ev.action_dim), generator=g, device=ev.device, dtype=torch.float32) * 4.0 - 2.0
        ev.step(loop.solver, a)
    return float(ev.return_stats()[2].mean().item())


def main(iterations=ITERATIONS, seed=0, graph=False, eval_every=10000, eval_envs=256, **cfg):
    from reth_amd.ddpg_apex import DdpgApex, DdpgApexConfig

    loop = DdpgApex(DdpgApexConfig(seed=seed, **cfg), impl="hip")
    rand = random_policy_return(loop, eval_envs)
    done, wall = 0, 0.0
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
        wall += dt
        done += k
        print(f"iteration {done}: {(loop.env_steps - steps0) / dt:,.0f} env-steps/s, {(loop.updates - upd0) / dt:,.0f} "
              f"updates/s, greedy mean return {loop.greedy_eval(eval_envs):.1f}"
              f"{' (graph)' if loop._graph is not None else ''}", flush=True)
    final = loop.greedy_eval(eval_envs)
    print(f"pendulum_ddpg_apex seed={seed} iterations={iterations} env_steps={loop.env_steps} updates={loop.updates} "
          f"greedy_mean_return={final:.1f} random_policy={rand:.1f} loop_wall_s={wall:.1f} "
          f"graph={loop._graph is not None}", flush=True)
    return loop, final, rand


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=ITERATIONS)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--graph", action="store_true")
    ap.add_argument("--eval-every", type=int, default=10000)
    args = ap.parse_args()
    main(args.iterations, args.seed, args.graph, args.eval_every)
