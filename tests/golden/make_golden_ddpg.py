"""Regenerates tests/golden/ddpg_pendulum_b64.npz from the reference's DDPG.

Loads reth/reth/algorithm/ddpg/ddpg_model.py and ddpg_solver.py at run time with make_golden.py's
loader and shims (gym is a stub, the package __init__ files are skipped) and records DATA only:

    seed                      torch.manual_seed before the four networks are built
    init/<net>/<param>        SHA-1 (hex, as bytes) of each freshly initialised fp32 tensor of the four
                              networks (actor, actor_target, critic, critic_target)
    s0, a, r, s1, done, w     a B = 64 batch: D = 3, Ad = 1, a uniform in (-2, 2), ~10 % done,
                              IS weights in [0.1, 1]
    upd<k>_abs_td             the fp32 |td| of update k = 0, 1, 2 on that batch (weights = w)
    act_states, act           four fixed states and act() on them after the updates
    final/<net>/<param>       the online actor's and critic's parameters after the updates (fp32)
    tsum/<net>/<param>        fp64 sums of the two target networks' tensors after the updates

    python tests/golden/make_golden_ddpg.py        (RETH_REFERENCE names the reference checkout)
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

SEED, B, D, AD = 7, 64, 3, 1
NETS = ("actor", "actor_target", "critic", "critic_target")


def sha1(t):
    return hashlib.sha1(np.ascontiguousarray(t.detach().numpy()).tobytes()).hexdigest()


def main():
    import torch

    mg.load_reference()
    mg._pkg("reth.algorithm.ddpg")
    model_mod = mg._load("reth.algorithm.ddpg.ddpg_model", "reth/reth/algorithm/ddpg/ddpg_model.py")
    solver_mod = mg._load("reth.algorithm.ddpg.ddpg_solver", "reth/reth/algorithm/ddpg/ddpg_solver.py")
    Box = sys.modules["gym"].spaces.Box

    torch.manual_seed(SEED)
    obs, act = Box(-1, 1, (D,)), Box(-2, 2, (AD,))
    # the solver's own construction (ddpg_solver.py:30-37), hashed before its update_target
    # overwrites the two freshly drawn targets
    models = model_mod.generate_ddpg_model(obs, act, 0.0001, 0.001, None)
    out = {"seed": np.int64(SEED)}
    for name in NETS:
        for k, v in models[name].state_dict().items():
            out[f"init/{name}/{k}"] = np.bytes_(sha1(v))
    solver = solver_mod.DDPGSolver(obs, act, models=models, device="cpu")

    rng = np.random.default_rng(SEED)
    th0, th1 = rng.uniform(-np.pi, np.pi, B), rng.uniform(-np.pi, np.pi, B)
    s0 = np.stack([np.cos(th0), np.sin(th0), rng.uniform(-8, 8, B)], 1).astype(np.float32)
    s1 = np.stack([np.cos(th1), np.sin(th1), rng.uniform(-8, 8, B)], 1).astype(np.float32)
    a = rng.uniform(-2, 2, (B, AD)).astype(np.float32)
    r = (-rng.uniform(0, 16, B)).astype(np.float32)
    done = (rng.random(B) < 0.1).astype(np.float32)
    done[1] = 1.0
    w = rng.uniform(0.1, 1.0, B).astype(np.float32)
    out.update(s0=s0, a=a, r=r, s1=s1, done=done, w=w)
    for k in range(3):
        out[f"upd{k}_abs_td"] = solver.update([s0, a, r, s1, done], weights=w).numpy().astype(np.float32)
    states = np.array([[1, 0, 0], [0, 1, 2.5], [-1, 0, -8], [0.6, -0.8, 0.3]], dtype=np.float32)
    out["act_states"] = states
    out["act"] = np.stack([solver.act(s) for s in states]).astype(np.float32)
    for name in ("actor", "critic"):
        for k, v in getattr(solver, name).state_dict().items():
            out[f"final/{name}/{k}"] = v.numpy().astype(np.float32)
    for name in ("actor_target", "critic_target"):
        for k, v in getattr(solver, name).state_dict().items():
            out[f"tsum/{name}/{k}"] = np.float64(v.double().sum().item())
    path = os.path.join(HERE, "ddpg_pendulum_b64.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
