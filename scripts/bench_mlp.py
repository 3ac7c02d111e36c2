"""Microbench (development aid): the MLP Q-network's solver calls (CartPole: D = 4, A = 2) on the
default torch path (MLP_IMPL = None: nn.Linear forwards, rth_td_huber, autograd, rth_clip_adam) vs
the fused kernels (MLP_IMPL = "hip": rth_mlp_q / rth_mlp_dqn_grads, rth_clip_adam), both in this
process, interleaved, three rounds of MLP_REPS (default 300) repetitions between two HIP events
after a warm-up: update_device at B = 64 and 512 eager (host launch time included: the events
bracket the whole window) and as a replayed single-stream HIP graph, one act (with its .item()
sync) and act_batch(256).  MLP_ONLY=hip|torch runs one path alone; with MLP_TRACE_UPDATES=K the
script only issues K eager updates at B = MLP_TRACE_B (for a kernel trace: launches per update)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reth_amd import model  # noqa: E402
from reth_amd.solver import Box, DQNSolver, Discrete  # noqa: E402

dev = torch.device("cuda")
REPS = int(os.environ.get("MLP_REPS", "300"))
ONLY = os.environ.get("MLP_ONLY")
PATHS = [p for p in ("torch", "hip") if ONLY in (None, p)]


def solver(path):
    model.MLP_IMPL = "hip" if path == "hip" else None
    try:
        torch.manual_seed(0)
        s = DQNSolver(Box(-1, 1, (4,)), Discrete(2), learning_rate=1e-4, update_target_interval=None, device=dev)
    finally:
        model.MLP_IMPL = None
    assert s.mlp_impl_active == (path if path == "hip" else None)
    return s


def batch(B):
    g = torch.Generator().manual_seed(B)
    return [torch.randn(B, 4, generator=g).to(dev), torch.randint(0, 2, (B,), generator=g).to(dev),
            torch.randn(B, generator=g).to(dev), torch.randn(B, 4, generator=g).to(dev),
            (torch.rand(B, generator=g) < 0.1).float().to(dev)]


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
    if os.environ.get("MLP_TRACE_UPDATES"):  # K eager updates at B = MLP_TRACE_B (64) and nothing else: under
        # `rocprofv3 --kernel-trace --stats` (with MLP_ONLY) the per-kernel call counts / K are the
        # launches per update (the solver's construction adds a few fills and copies)
        B, K = int(os.environ.get("MLP_TRACE_B", "64")), int(os.environ["MLP_TRACE_UPDATES"])
        data, isw = batch(B), torch.rand(B, dtype=torch.float64, device=dev) * 0.9 + 0.1
        for s in solvers.values():
            for _ in range(K):
                s.update_device(data, isw)
        torch.cuda.synchronize()
        print(f"{PATHS}: {K} update_device calls at B={B}", flush=True)
        return
    cases = {}  # name -> {path: callable}
    keep = []
    for B in (64, 512):
        data = batch(B)
        isw = torch.rand(B, dtype=torch.float64, device=dev) * 0.9 + 0.1
        for p, s in solvers.items():
            cases.setdefault(f"update_device B={B} eager", {})[p] = lambda s=s, d=data, w=isw: s.update_device(d, w)
            side = torch.cuda.Stream(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                for _ in range(3):
                    s.update_device(data, isw)
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                keep.append(s.update_device(data, isw))
            cases.setdefault(f"update_device B={B} graph replay", {})[p] = graph.replay
    state = np.array([0.01, -0.02, 0.03, 0.04], np.float32)
    states = torch.randn(256, 4, device=dev)
    for p, s in solvers.items():
        cases.setdefault("act (one state, with .item())", {})[p] = lambda s=s: s.act(state)
        cases.setdefault("act_batch(256)", {})[p] = lambda s=s: s.act_batch(states)
    for name, fns in cases.items():
        res = {p: [] for p in fns}
        for fn in fns.values():
            for _ in range(20):
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
        print(f"{p}: mlp_hip_launches {s.mlp_hip_launches}", flush=True)


if __name__ == "__main__":
    main()
