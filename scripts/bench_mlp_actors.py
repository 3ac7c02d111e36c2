"""Microbench (development aid): the device CartPole loop (reth_amd/mlp_apex.py, mlp_actors.py)
against the host loop of examples/cartpole_dqn_hip.py, on one GPU, in this process, three
rounds over all cases in turn after a warm-up, each figure a host clock around a window that ends
in a device synchronise (the baseline is host-bound: its .item() syncs are part of what it costs):

  actor step alone        rth_mlp_actor_step at N = 64 / 256 / 2048 (MLPA_REPS steps per window)
  whole iteration         MlpApexDQN at N = 64, B = 64: eager and as a replayed HIP graph
  baseline                the example's loop body -- worker.step_batch(64), solver.calc_loss,
                          buffer.append_batch, buffer.sample(64), trainer.step, update_priorities --
                          with MLP_IMPL = "hip", and its two dominant parts alone

With MLPA_TRACE_ITERS=K the script only issues K eager steady-state iterations (for a kernel
trace: kernel calls / K = launches per iteration; the warm-up before them is counted apart by
running the trace twice with different K)."""
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
from reth_amd import model  # noqa: E402
from reth_amd.mlp_actors import VecCartPoleActors  # noqa: E402
from reth_amd.mlp_apex import MlpApexConfig, MlpApexDQN  # noqa: E402

REPS = int(os.environ.get("MLPA_REPS", "300"))
BASE_REPS = int(os.environ.get("MLPA_BASE_REPS", "10"))


def window(fn, reps):
    """microseconds per call of fn over reps calls, host clock, synchronised at both ends"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / reps


def rounds(cases):
    """cases: name -> (fn, calls per window, warm-up calls); three rounds over all of them in turn"""
    res = {k: [] for k in cases}
    for fn, _, warm in cases.values():
        for _ in range(warm):
            fn()
    for _ in range(3):
        for k, (fn, reps, _) in cases.items():
            res[k].append(window(fn, reps))
    for k, v in res.items():
        print(f"{k}: {' / '.join(f'{t:.1f}' for t in v)} us  (median {sorted(v)[1]:.1f})", flush=True)
    return {k: sorted(v)[1] for k, v in res.items()}


def device_loop(graph):
    model.MLP_IMPL = "hip"
    try:
        loop = MlpApexDQN(MlpApexConfig(n_actors=64, batch_size=64, seed=0))
    finally:
        model.MLP_IMPL = None
    while not loop.graph_ready():
        loop.iteration()
    loop.run(5)
    if graph:
        loop.capture()
    return loop


def host_loop():
    import cartpole_dqn
    from reth_amd.presets import get_replay_buffer, get_solver, get_trainer, get_worker

    cfg = os.path.join(ROOT, "examples", "cartpole_dqn.yaml")
    model.MLP_IMPL = "hip"
    try:
        solver = get_solver(cfg)
    finally:
        model.MLP_IMPL = None
    assert solver.mlp_impl_active == "hip"
    worker, trainer, buffer = get_worker(cfg, solver=solver), get_trainer(cfg, solver=solver), get_replay_buffer(cfg)
    buffer.append_batch(worker.step_batch(1000))
    B = cartpole_dqn.BATCH_SIZE
    state = {}

    def body():
        data = worker.step_batch(B)
        solver.calc_loss(data)
        buffer.append_batch(data)
        data, indices, weights = buffer.sample(B)
        state["batch"] = data
        loss = trainer.step(data)
        buffer.update_priorities(indices, loss)

    body()
    return body, (lambda: worker.step_batch(B)), (lambda: trainer.step(state["batch"]))


def main():
    dev = torch.device("cuda")
    print(f"device: {torch.cuda.get_device_name(0)}; windows of {REPS} device steps / {BASE_REPS} host-loop iterations",
          flush=True)
    if os.environ.get("MLPA_TRACE_ITERS"):
        K = int(os.environ["MLPA_TRACE_ITERS"])
        loop = device_loop(graph=False)
        before = loop.iterations
        loop.run(K)
        torch.cuda.synchronize()
        print(f"{K} eager steady-state iterations after {before} warm-up iterations "
              f"({loop.updates} updates in all)", flush=True)
        return
    torch.manual_seed(0)
    net = model.MLP_DQNNetwork((4,), 2).to(dev)
    net.requires_grad_(False)
    actors = {n: VecCartPoleActors(n, seed=1, device=dev) for n in (64, 256, 2048)}
    eager, graph = device_loop(False), device_loop(True)
    body, step_batch, train = host_loop()
    cases = {f"actor step alone N={n} (one launch, N env steps)": ((lambda a=a: a.step(net)), REPS, 50)
             for n, a in actors.items()}
    cases["device loop iteration, eager (64 env steps + one B=64 update)"] = (eager.iteration, REPS, 20)
    cases["device loop iteration, graph replay"] = (graph.iteration, REPS, 20)
    cases["host loop iteration of examples/cartpole_dqn_hip.py (64 env steps + one B=64 update)"] = (body, BASE_REPS, 2)
    cases["  its worker.step_batch(64) alone"] = (step_batch, BASE_REPS, 2)
    cases["  its trainer.step alone"] = (train, BASE_REPS, 2)
    med = rounds(cases)
    names = list(cases)
    for n, k in zip(actors, names):
        print(f"N={n}: {n / med[k]:.2f} M env-steps/s in the actor step alone", flush=True)
    host = med[names[5]]
    for k in names[3:5]:
        print(f"host loop / {k.split(' (')[0]}: {host / med[k]:.1f}x (medians)", flush=True)
    print(f"device loop host counters: {eager.actors.launches} actor launches in {eager.iterations} iterations; "
          f"solver HIP calls per steady-state iteration: 2", flush=True)


if __name__ == "__main__":
    main()
