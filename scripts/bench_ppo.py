"""Microbench (development aid): PPOSolver's calls at the CartPole shape (D = 4, A = 2, H = 64) on
the reference's formulation (impl="torch": nn.Sequential, Categorical, autograd, two
torch.optim.Adam) vs the fused kernels (impl="hip": csrc/ppo.hpp, rth_clip_adam), both in this
process, interleaved, three rounds of PPO_REPS (default 100) repetitions between two HIP events
after a warm-up: update_device (k_epochs = 4 epochs) at B = 2,048 and B = 64 eager (host launch
time included: the events bracket the whole window), one act (with its copy to the host) and
act_batch(256).  PPO_ONLY=hip|torch runs one path alone; with PPO_TRACE_UPDATES=K the script only
issues K eager updates at B = PPO_B (for a kernel trace: launches per update)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reth_amd.ppo import PPOSolver  # noqa: E402
from reth_amd.solver import Box, Discrete  # noqa: E402

dev = torch.device("cuda")
REPS = int(os.environ.get("PPO_REPS", "100"))
ONLY = os.environ.get("PPO_ONLY")
PATHS = [p for p in ("torch", "hip") if ONLY in (None, p)]
OBS, ACT = Box(-1, 1, (4,)), Discrete(2)


def solver(path):
    torch.manual_seed(0)
    s = PPOSolver(OBS, ACT, device=dev, impl=path)
    assert s.impl_active == path
    return s


def batch(B):
    """states, actions, returns and old log-probabilities near the fresh policy's (ratios near 1)"""
    g = torch.Generator().manual_seed(B)
    return [torch.randn(B, 4, generator=g).to(dev), torch.randint(0, 2, (B,), generator=g).to(dev),
            torch.randn(B, generator=g).to(dev), (np.log(0.5) + 0.1 * torch.randn(B, generator=g)).float().to(dev)]


def timed(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    solvers = {p: solver(p) for p in PATHS}
    if os.environ.get("PPO_TRACE_UPDATES"):
        K, B = int(os.environ["PPO_TRACE_UPDATES"]), int(os.environ.get("PPO_B", "2048"))
        data = batch(B)
        for s in solvers.values():
            for _ in range(K):
                s.update_device(data)
        torch.cuda.synchronize()
        print(f"{PATHS}: {K} update_device calls at B={B}, k_epochs={solvers[PATHS[0]].k_epochs}", flush=True)
        return
    cases = {}
    for B in (2048, 64):
        data = batch(B)
        for p, s in solvers.items():
            cases.setdefault(f"update_device B={B} eager", {})[p] = lambda s=s, data=data: s.update_device(data)
    state = np.array([0.01, -0.02, 0.03, 0.04], np.float32)
    states = torch.randn(256, 4, device=dev)
    for p, s in solvers.items():
        cases.setdefault("act (one state, to the host)", {})[p] = lambda s=s: s.act(state)
        cases.setdefault("act_batch(256)", {})[p] = lambda s=s: s.act_batch(states)
    for name, fns in cases.items():
        res = {p: [] for p in fns}
        for fn in fns.values():
            for _ in range(10):
                fn()
        torch.cuda.synchronize()
        for _ in range(3):
            for p, fn in fns.items():
                res[p].append(timed(fn))
        line = "  ".join(f"{p} {' / '.join(f'{t:.1f}' for t in v)} us" for p, v in res.items())
        if len(res) == 2:
            line += f"  (torch / hip, best of 3: {min(res['torch']) / min(res['hip']):.2f}x)"
        print(f"{name}: {line}", flush=True)
    for p, s in solvers.items():
        print(f"{p}: hip_launches {s.hip_launches}", flush=True)


if __name__ == "__main__":
    main()
