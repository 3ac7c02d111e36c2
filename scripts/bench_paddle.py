"""Microbench (development aid): what the Paddle game (VecActors(env="paddle"), csrc/game.hpp)
costs against the synthetic env, on one GPU, in this process.

  loop    ms/step of the captured two-stream Ape-X loop (256 actors, B = 512, frame store) with
          env="paddle" and env="synthetic": three rounds over both in turn after a warm-up, each
          figure a host clock around PADDLE_ITERS iterations that ends in a device synchronise
  tail    the actor tail launch alone, rth_game_actor_tail against rth_actor_tail (N = 256, A = 6,
          with the rth_actor_prologue launch that advances the step counter, and that launch
          alone): PADDLE_TAIL_REPS launches captured in one HIP graph, replayed, three rounds
"""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from reth_amd import _lib  # noqa: E402
from reth_amd._lib import call, ptr, stream_ptr  # noqa: E402
from reth_amd.actors import VecActors  # noqa: E402
from reth_amd.apex import ApexConfig, ApexDQN  # noqa: E402

ITERS = int(os.environ.get("PADDLE_ITERS", "1000"))
TAIL_REPS = int(os.environ.get("PADDLE_TAIL_REPS", "200"))


def window(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def rounds(cases, unit, scale):
    res = {k: [] for k in cases}
    for _ in range(3):
        for k, (fn, reps) in cases.items():
            res[k].append(window(fn, reps) * scale)
    for k, v in res.items():
        print(f"{k}: {' / '.join(f'{t:.4f}' for t in v)} {unit}  (median {sorted(v)[1]:.4f})", flush=True)
    return {k: sorted(v)[1] for k, v in res.items()}


def loop(env):
    ax = ApexDQN(ApexConfig(env=env, n_actors=256, capacity=1 << 17, batch_size=512, hip_graph=True, frame_store=True,
                            seed=0), device=torch.device("cuda:0"))
    while ax._graphs is None:
        ax.iteration()
    for _ in range(300):
        ax.iteration()
    torch.cuda.synchronize()
    return ax


def tail_graph(env, reps, with_tail=True):
    """a HIP graph of `reps` x (rth_actor_prologue [+ the env's tail launch]) on N = 256 actors"""
    N, A = 256, 6
    dev = torch.device("cuda:0")
    act = VecActors(N, A, device=dev, seed=1, channels_last=True, env=env)
    g = torch.Generator(device=dev).manual_seed(0)
    q = torch.randn((N, A + 1), device=dev, generator=g)
    qcache = torch.randn((N * act.ring + 1, A + 1), device=dev, generator=g)
    prev, cur = act._sets
    td = torch.empty(N, dtype=torch.float32, device=dev)
    args = _lib.ActorTailArgs(ptr(q), ptr(act.eps), ptr(act.t_dev), ptr(act.action), ptr(qcache), ptr(prev.s0),
                              ptr(prev.a), ptr(prev.s1), ptr(prev.r), ptr(prev.done), ptr(td), ptr(act.frames),
                              ptr(act.cur_slot), ptr(act.reward), ptr(act.done), ptr(act.s0_h), ptr(act.s1_h), act.seed,
                              N, act.gamma_n, act.p_reward, act.p_done, act.ring, A, 0)
    game = act._game_args() if env == "paddle" else None
    keep = (act, q, qcache, td, args, game)

    def one():
        s = stream_ptr()
        call("rth_actor_prologue", ptr(act.t_dev), ptr(act.cur_slot), N, act.ring, ptr(act.hx), s)
        if not with_tail:
            return
        out = (ptr(act.emit), ptr(cur.s0), ptr(cur.a), ptr(cur.r), ptr(cur.s1), ptr(cur.done), s)
        if game is not None:
            call("rth_game_actor_tail", act._nstep, _lib.ctypes.byref(args), _lib.ctypes.byref(game), *out)
        else:
            call("rth_actor_tail", act._nstep, _lib.ctypes.byref(args), *out)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(8):
            one()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        for _ in range(reps):
            one()
    graph.keep = keep
    return graph


def main():
    print(f"device: {torch.cuda.get_device_name(0)}; loop windows of {ITERS} iterations, tail graphs of {TAIL_REPS} "
          f"launches", flush=True)
    graphs = {"prologue + game tail (paddle)": tail_graph("paddle", TAIL_REPS),
              "prologue + tail (synthetic)": tail_graph("synthetic", TAIL_REPS),
              "prologue alone": tail_graph("synthetic", TAIL_REPS, with_tail=False)}
    for gr in graphs.values():
        gr.replay()
    med = rounds({k: (gr.replay, 20) for k, gr in graphs.items()}, "us / launch pair", 1e6 / TAIL_REPS)
    p, s, pro = (med[k] for k in graphs)
    print(f"tail alone: paddle {p - pro:.2f} us, synthetic {s - pro:.2f} us, ratio {(p - pro) / (s - pro):.3f}", flush=True)
    loops = {"paddle": loop("paddle"), "synthetic": loop("synthetic")}
    med = rounds({f"loop env={k}": (ax.iteration, ITERS) for k, ax in loops.items()}, "ms / step", 1e3)
    print(f"loop: paddle / synthetic = {med['loop env=paddle'] / med['loop env=synthetic']:.4f} (medians)", flush=True)
    for ax in loops.values():
        ax.close()


if __name__ == "__main__":
    main()
