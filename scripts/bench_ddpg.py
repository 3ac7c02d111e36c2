"""Microbench (development aid): DDPGSolver's calls at the Pendulum shape (D = 3, Ad = 1, 400-300
hidden units) on the reference's formulation (impl="torch": nn.Linear, autograd, two
torch.optim.Adam, twelve soft-update expressions) vs the fused kernels (impl="hip": csrc/ddpg.hpp,
rth_clip_adam), both in this process, interleaved, three rounds of DDPG_REPS (default 300)
repetitions between two HIP events after a warm-up: update_device at B = 64 eager (host launch
time included: the events bracket the whole window) and as a replayed single-stream HIP graph, one
act (with its device-to-host copy) and act_batch(256).  DDPG_ONLY=hip|torch runs one path alone;
with DDPG_TRACE_UPDATES=K the script only issues K eager updates (for a kernel trace: launches per
update).  The torch path's optimizers are capturable Adam under the graph (a device step count);
eager it is the reference's plain torch.optim.Adam."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from reth_amd.ddpg import DDPGSolver, generate_ddpg_model  # noqa: E402
from reth_amd.solver import Box  # noqa: E402

dev = torch.device("cuda")
REPS = int(os.environ.get("DDPG_REPS", "300"))
ONLY = os.environ.get("DDPG_ONLY")
PATHS = [p for p in ("torch", "hip") if ONLY in (None, p)]
OBS, ACT = Box(-1, 1, (3,)), Box(-2, 2, (1,))


def solver(path, capturable=False):
    torch.manual_seed(0)
    models = generate_ddpg_model(OBS, ACT, 1e-4, 1e-3)
    s = DDPGSolver(OBS, ACT, models=models, device=dev, impl=path, cast_actions_to_long=False)
    if capturable:  # torch's Adam with its step count on the device, so that the update captures
        s.actor_optimizer = torch.optim.Adam(s.actor.parameters(), 1e-4, capturable=True)
        s.critic_optimizer = torch.optim.Adam(s.critic.parameters(), 1e-3, capturable=True)
    assert s.impl_active == path
    return s


def batch(B):
    g = torch.Generator().manual_seed(B)
    return [torch.randn(B, 3, generator=g).to(dev), (torch.rand(B, 1, generator=g) * 4 - 2).to(dev),
            torch.randn(B, generator=g).to(dev), torch.randn(B, 3, generator=g).to(dev),
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
    B = int(os.environ.get("DDPG_B", "64"))
    data, isw = batch(B), torch.rand(B, device=dev) * 0.9 + 0.1
    solvers = {p: solver(p) for p in PATHS}
    if os.environ.get("DDPG_TRACE_UPDATES"):
        K = int(os.environ["DDPG_TRACE_UPDATES"])
        for s in solvers.values():
            for _ in range(K):
                s.update_device(data, isw)
        torch.cuda.synchronize()
        print(f"{PATHS}: {K} update_device calls at B={B}", flush=True)
        return
    cases, keep = {}, []
    for p, s in solvers.items():
        cases.setdefault(f"update_device B={B} eager", {})[p] = lambda s=s: s.update_device(data, isw)
        gs = solver(p, capturable=(p == "torch"))
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            for _ in range(3):
                gs.update_device(data, isw)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        try:
            with torch.cuda.graph(graph, stream=side):
                keep.append((gs, gs.update_device(data, isw)))
        except RuntimeError as e:  # reported, not hidden: the comparison then lacks this path
            print(f"update_device B={B} graph replay: {p} did not capture: {e}", flush=True)
            continue
        cases.setdefault(f"update_device B={B} graph replay", {})[p] = graph.replay
    state = np.array([0.6, -0.8, 0.3], np.float32)
    states = torch.randn(256, 3, device=dev)
    for p, s in solvers.items():
        cases.setdefault("act (one state, to numpy)", {})[p] = lambda s=s: s.act(state)
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
        print(f"{p}: hip_launches {s.hip_launches}", flush=True)


if __name__ == "__main__":
    main()
