"""The reference's examples/ddpg/run.py loop (Pendulum-v0, DDPG, prioritized replay, OU noise) on
this package: one solver shared by the worker and the trainer, 1000 warm-up transitions, then per
training step 64 environment steps, one prioritized sample of 64 and one update.

    python examples/pendulum_ddpg_hip.py [--impl hip|torch] [--steps N] [--seed S]

--impl hip runs the update and the acting forward on the fused kernels of csrc/ddpg.hpp, --impl
torch on the reference's formulation (nn.Linear, autograd, torch.optim.Adam); the default takes
the kernels where they apply.

cast_actions_to_long=False: the reference casts the replayed actions to torch.long before the
critic sees them (ddpg_solver.py:72), so its critic only ever learns Q(s, trunc(a)) -- for an
actor whose output lies in (-1, 1) that is Q(s, 0), and the actor's gradient carries no signal.
The solver keeps that behaviour as its default for parity; an example that is meant to learn feeds
the critic the actions that were taken.

Prints the mean return of the last 10 finished episodes beside a random policy's.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reth_amd import envs  # noqa: E402
from reth_amd.buffer import PrioritizedBuffer  # noqa: E402
from reth_amd.presets import get_replay_buffer, get_solver, get_trainer, get_worker  # noqa: E402

BATCH_SIZE = 64
MAX_TS = 100000
CONFIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pendulum_ddpg.yaml")


def random_policy_return(seed, episodes=10):
    """mean return of uniform random torques in [-2, 2] over `episodes` episodes"""
    env = envs.make_host("Pendulum-v0", seed=seed)
    rng = np.random.RandomState(seed)
    returns = []
    for _ in range(episodes):
        env.reset()
        total, done = 0.0, False
        while not done:
            _, r, done, _ = env.step(rng.uniform(-2.0, 2.0, size=1))
            total += r
        returns.append(total)
    return float(np.mean(returns))


def main(steps=MAX_TS, impl=None, seed=0, quiet=False):
    torch.manual_seed(seed)
    np.random.seed(seed)
    env = envs.make_host("Pendulum-v0", seed=seed)
    solver = get_solver(CONFIG, env=env, impl=impl, cast_actions_to_long=False)
    kw = {"logger": False} if quiet else {}
    worker = get_worker(CONFIG, solver=solver, env=env, **kw)  # shared solver
    trainer = get_trainer(CONFIG, solver=solver, **kw)
    buffer = get_replay_buffer(CONFIG, device=solver.device)
    assert isinstance(buffer, PrioritizedBuffer)
    returns = []
    worker.on_episode_end.append(lambda: returns.append(worker.recent_rewards[-1]) if worker.recent_rewards else None)

    buffer.append_batch(worker.step_batch(1000))
    for _ in range(steps):
        buffer.append_batch(worker.step_batch(BATCH_SIZE))
        data, indices, weights = buffer.sample(BATCH_SIZE)
        loss = trainer.step(data, weights=weights)
        buffer.update_priorities(indices, loss)
    last = float(np.mean(returns[-10:])) if returns else float("nan")
    rand = random_policy_return(seed)
    print(f"pendulum_ddpg impl={solver.impl_active} seed={seed} steps={steps} episodes={len(returns)} "
          f"mean_return_last10={last:.1f} random_policy={rand:.1f} hip_launches={solver.hip_launches}")
    return solver, last, rand


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["hip", "torch"], default=None)
    ap.add_argument("--steps", type=int, default=MAX_TS)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    main(args.steps, args.impl, args.seed)
