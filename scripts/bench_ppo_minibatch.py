"""Microbench (development aid): shuffled minibatch epochs on the device PPO loop
(csrc/ppo_shuffle.hpp rth_ppo_shuffle, reth_amd/ppo.py PPOSolver(n_minibatches), reth_amd/ppo_loop.py)
at the CartPole shape (D = 4, A = 2, H = 64).  HIP events after a warm-up, three interleaved rounds
(host launch time included: the events bracket the whole window):

  - rth_ppo_shuffle at n = 2,048 / 8,192 / 65,536 rows, K = 4, D = 4 (the 5-column batch);
  - one 64 x 32 GAE iteration (32 steps + finish_gae + normalise + the update of 4 epochs) at K = 1 and
    K = 4, eager and as a replayed graph;
  - with --parent TREE (a checkout of the parent commit whose library is built): the K = 1 iteration of
    that tree and of this one, each in a process of its own, three alternating rounds;
  - with --learn: the learning test's figures (CartPole-v0, 64 x 32, K = 4, 50 iterations, seeds
    0 / 1 / 2) at learning rates 0.01 and 0.003, and K = 1 at 0.01 beside them.

PPOMB_ROOT selects the tree whose reth_amd is imported (default: this one); --k1-only measures the
K = 1 iteration alone, with nothing the parent commit lacks."""
import argparse
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("PPOMB_ROOT") or HERE
sys.path.insert(0, ROOT)
from reth_amd import _lib  # noqa: E402
from reth_amd._lib import call, ptr, stream_ptr  # noqa: E402
from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig  # noqa: E402

dev = torch.device("cuda")
REPS = int(os.environ.get("PPOMB_REPS", "100"))
GAE = dict(n_actors=64, horizon=32, gae_lambda=0.95, normalize_adv=True)


def timed(fn, reps=REPS):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def rounds(name, fns, reps=REPS, unit="us", scale=1.0):
    """three interleaved rounds of every fn -> prints one line; returns the best of each"""
    res = {k: [] for k in fns}
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(3):
        for k, fn in fns.items():
            res[k].append(timed(fn, reps) * scale)
    print(f"{name}: " + "  ".join(f"{k} {' / '.join(f'{t:.1f}' for t in v)} {unit}" for k, v in res.items()), flush=True)
    return {k: min(v) for k, v in res.items()}


def iteration_rounds(name, configs):
    loops = {}
    for k, cfg in configs.items():
        for mode in ("eager", "graph"):
            loops[f"{k} {mode}"] = PpoLoop(PpoLoopConfig(**cfg), device=dev)
    for k, loop in loops.items():
        loop.iteration()
        if k.endswith("graph"):
            loop.capture()
    return rounds(name, {k: v.iteration for k, v in loops.items()}, reps=50, unit="ms", scale=1e-3)


def shuffle_rounds():
    B, K, D = 65536, 4, 4
    g = torch.Generator().manual_seed(1)
    s, a = torch.randn(B, D, generator=g).to(dev), torch.randint(0, 2, (B,), generator=g).to(dev)
    ret, adv, old = (torch.randn(B, generator=g).to(dev) for _ in range(3))
    fns = {}
    keep = []
    for n in (2048, 8192, 65536):
        Mcap = -(-n // K)
        z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)
        mb = [z((K * Mcap, D)), z(K * Mcap, torch.int64), z(K * Mcap), z(K * Mcap), z(K * Mcap), z(K, torch.int64),
              z(n, torch.int32), z(_lib.lib().rth_ppo_shuffle_workspace(n) // 8, torch.int64)]
        counter = z(1, torch.int64)
        keep.append((mb, counter))
        fns[f"n={n}"] = (lambda n=n, mb=mb, counter=counter: call(
            "rth_ppo_shuffle", ptr(s), D, ptr(a), ptr(ret), ptr(adv), ptr(old), n, None, D, K, 12345, ptr(counter), None,
            *[ptr(t) for t in mb], stream_ptr()))
    rounds("rth_ppo_shuffle K=4 D=4 (keys, ranks by counting, gather: two launches)", fns)


def learn():
    for K, lr in ((4, 0.01), (4, 0.003), (1, 0.01)):
        trained, untrained = [], []
        for seed in (0, 1, 2):
            loop = PpoLoop(PpoLoopConfig(seed=seed, n_minibatches=K, learning_rate=lr, **GAE), device=dev)
            untrained.append(round(loop.rollout_length(), 1))
            loop.run(50)
            trained.append(round(loop.mean_last_length(), 1))
        print(f"CartPole-v0 64 x 32, K = {K}, learning rate {lr}, 50 iterations, seeds 0/1/2: mean last finished "
              f"length {trained}, untrained {untrained}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k1-only", action="store_true")
    ap.add_argument("--parent", default=None)
    ap.add_argument("--learn", action="store_true")
    args = ap.parse_args()
    if args.k1_only:
        tree = "this tree" if os.path.samefile(ROOT, HERE) else "the parent's tree"
        iteration_rounds(f"PpoLoop 64 x 32 GAE iteration, {tree}", {"K=1": GAE})
        return
    shuffle_rounds()
    iteration_rounds("PpoLoop 64 x 32 GAE iteration (2,048 env steps + finish + normalise + update)",
                     {"K=1": dict(GAE, n_minibatches=1), "K=4": dict(GAE, n_minibatches=4)})
    if args.parent:
        for rnd in range(3):
            for tree in (args.parent, HERE):
                subprocess.run([sys.executable, os.path.abspath(__file__), "--k1-only"], check=True,
                               env=dict(os.environ, PPOMB_ROOT=os.path.abspath(tree)))
    if args.learn:
        learn()


if __name__ == "__main__":
    main()
