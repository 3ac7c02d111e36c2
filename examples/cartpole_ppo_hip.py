"""The reference's examples/ppo/run.py loop (CartPole-v0, PPO) on this package: a learner solver and
an acting solver; per update 2,000 environment steps with the acting solver's own draws, complete
episodes through calculate_discount_rewards_with_dones (gamma = 0.99) into the data buffer, then
one trainer step (k_epochs full-batch epochs), the weights back to the acting solver and a clear.

    python examples/cartpole_ppo_hip.py [--impl hip|torch] [--updates N] [--seed S]

--impl hip runs the update and the acting forward on the fused kernels of csrc/ppo.hpp, --impl
torch on the reference's formulation (nn.Sequential, Categorical, autograd, torch.optim.Adam); the
default takes the kernels where they apply.

Prints the mean length of the last 10 finished episodes (CartPole-v0's return; at most 200).
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reth_amd import envs  # noqa: E402
from reth_amd.buffer import DynamicSizeBuffer  # noqa: E402
from reth_amd.ppo import calculate_discount_rewards_with_dones  # noqa: E402
from reth_amd.presets import get_solver, get_trainer, get_worker  # noqa: E402

MAX_UPDATES = 50
GAMMA = 0.99
UPDATE_INTERVAL = 2000
CONFIG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cartpole_ppo.yaml")


def main(updates=MAX_UPDATES, impl=None, seed=0, quiet=False):
    torch.manual_seed(seed)
    np.random.seed(seed)
    env = envs.make_host("CartPole-v0", seed=seed)
    solver = get_solver(CONFIG, env=env, impl=impl)
    act_solver = get_solver(CONFIG, env=env, impl=impl)
    kw = {"logger": False} if quiet else {}
    worker = get_worker(CONFIG, solver=act_solver, env=env, **kw)
    trainer = get_trainer(CONFIG, solver=solver, **kw)
    episode_buffer = DynamicSizeBuffer(64, device=solver.device)
    data_buffer = DynamicSizeBuffer(64, device=solver.device)
    act_solver.sync_weights(solver)
    lengths, steps = [], 0
    for _ in range(updates):
        for _ in range(UPDATE_INTERVAL):
            a, logprob = act_solver.act(worker.s0)
            s0, a, r, s1, done = worker.step(a)
            steps += 1
            episode_buffer.append((s0, a, r, logprob, done))
            if done:
                s0, a, r, logprob, done = episode_buffer.data
                lengths.append(len(r))
                r = calculate_discount_rewards_with_dones(r, done, GAMMA)
                data_buffer.append_batch((s0, a, r, logprob))
                episode_buffer.clear()
        trainer.step(data_buffer.data)
        act_solver.sync_weights(solver)
        data_buffer.clear()
    last = float(np.mean(lengths[-10:])) if lengths else float("nan")
    launches = solver.hip_launches + act_solver.hip_launches
    print(f"cartpole_ppo impl={solver.impl_active} updates={updates} seed={seed} env_steps={steps} "
          f"episodes={len(lengths)} mean_len_last10={last:.1f} hip_launches={launches}")
    return solver, last


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--impl", choices=["hip", "torch"], default=None)
    ap.add_argument("--updates", type=int, default=MAX_UPDATES)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    main(args.updates, args.impl, args.seed)
