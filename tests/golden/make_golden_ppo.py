"""Regenerates tests/golden/ppo_cartpole_b64.npz from the reference's PPO.

Loads reth/reth/algorithm/ppo/ppo_model.py, ppo_solver.py and algorithm/util.py at run time with
make_golden.py's loader and shims (gym is a stub, the package __init__ files are skipped) and
records DATA only:

    seed                      torch.manual_seed before the two networks are built
    init/<net>/<param>        SHA-1 (hex, as bytes) of each freshly initialised fp32 tensor (actor, value)
    keys/<net>                the state_dict keys, newline-joined
    states, actions, old_logprobs, returns
                              a B = 64 batch: D = 4, A = 2; CartPole-like states, the actions and
                              log-probabilities of the reference's own act() on them (the torch
                              generator as the seed and the construction left it), returns from
                              the reference's calculate_discount_rewards_with_dones
    upd<k>_abs_loss           the fp32 |loss| of update k = 0, 1, 2 on that batch (4 epochs each)
    final/<net>/<param>       both networks' parameters after the updates (fp32)
    act_seed, act_states, act_actions, act_logprobs
                              torch.manual_seed(act_seed), then act() on four fixed states
    ret/<i>/r, done, with_dones, plain
                              (r, done) sequences and both return functions' outputs
    drift_param, drift_loss, ratio_margin
                              see below

The seed is chosen.  Adam's g / (sqrt(v) + 1e-8) amplifies rounding where a gradient element is
~1e-9, and a ratio within rounding of 1 +- eps_clip flips the clip decision, so the reference's own
fp32 run can differ from the same formulation in fp64 by 1e-4 in a parameter.  Seeds 0..63 are
run in fp32 (the reference) and in fp64 (the restatement below); only seeds whose every ratio of
every epoch stays more than 1e-4 from 1 +- eps_clip (in fp64) qualify, and of those the one with
the smallest parameter drift max |fp32 - fp64| is kept.  drift_param and drift_loss record that
seed's drifts (parameters; |loss| over the three updates), ratio_margin its smallest distance.

    python tests/golden/make_golden_ppo.py        (RETH_REFERENCE names the reference checkout)
"""
import copy
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402

B, D, A, UPDATES, SEEDS, MARGIN = 64, 4, 2, 3, 64, 1e-4
NETS = (("actor", "actor_network"), ("value", "value_network"))


def sha1(t):
    return hashlib.sha1(np.ascontiguousarray(t.detach().numpy()).tobytes()).hexdigest()


def batch_inputs(util):
    """the states and the returns: the same for every seed"""
    rng = np.random.default_rng(19)
    states = np.stack([rng.uniform(-2.4, 2.4, B), rng.uniform(-3, 3, B), rng.uniform(-0.21, 0.21, B),
                       rng.uniform(-3, 3, B)], 1).astype(np.float32)
    done = np.zeros(B, bool)
    done[[9, 30, 31, 63]] = True
    returns = util.calculate_discount_rewards_with_dones(np.ones(B), done, 0.99)
    return states, returns.astype(np.float32)


def fp64_run(actor, value, batch, k_epochs, eps_clip, lr):
    """ppo_solver.py:72-98 in fp64 on copies of the two networks: (|loss| per update, the smallest
    distance of a ratio from a clip bound)"""
    import torch
    import torch.nn.functional as F
    from torch.distributions import Categorical

    actor, value = copy.deepcopy(actor).double(), copy.deepcopy(value).double()
    opt_a, opt_v = torch.optim.Adam(actor.parameters(), lr=lr), torch.optim.Adam(value.parameters(), lr=lr)
    states, actions, returns, old = (torch.as_tensor(x) for x in batch)
    states, returns, old = states.double(), returns.double(), old.double()
    losses, margin = [], float("inf")
    for _ in range(UPDATES):
        for _ in range(k_epochs):
            dist = Categorical(actor(states))
            v = torch.squeeze(value(states))
            ratios = torch.exp(dist.log_prob(actions) - old)
            adv = returns - v.detach()
            loss = (-torch.min(ratios * adv, torch.clamp(ratios, 1 - eps_clip, 1 + eps_clip) * adv)
                    + 0.5 * F.mse_loss(v, returns) - 0.01 * dist.entropy())
            rho = ratios.detach()
            margin = min(margin, float(torch.minimum((rho - (1 - eps_clip)).abs(), (rho - (1 + eps_clip)).abs()).min()))
            opt_a.zero_grad()
            opt_v.zero_grad()
            loss.mean().backward()
            opt_a.step()
            opt_v.step()
        losses.append(loss.detach().abs().numpy())
    return actor, value, losses, margin


def run_seed(seed, model_mod, solver_mod, gym, states, returns):
    import torch

    torch.manual_seed(seed)
    obs, act = gym.spaces.Box(-1, 1, (D,)), gym.spaces.Discrete(A)
    models = model_mod.generate_discrite_ppo_model(obs, act, hidden_size=64, learning_rate=0.01)
    out = {"seed": np.int64(seed)}
    for name, key in NETS:
        sd = models[key].state_dict()
        out[f"keys/{name}"] = np.bytes_("\n".join(sd))
        for k, v in sd.items():
            out[f"init/{name}/{k}"] = np.bytes_(sha1(v))
    solver = solver_mod.PPOSolver(obs, act, models=models, device=torch.device("cpu"))
    acts = [solver.act(s) for s in states]
    actions = np.array([a for a, _ in acts], np.int64)
    old = np.array([lp for _, lp in acts], np.float32)
    batch = (states, actions, returns, old)
    a64, v64, loss64, margin = fp64_run(solver.actor_network, solver.value_network, batch, solver.k_epochs,
                                        solver.eps_clip, 0.01)
    out.update(states=states, actions=actions, old_logprobs=old, returns=returns)
    drift_loss = 0.0
    for k in range(UPDATES):
        out[f"upd{k}_abs_loss"] = solver.update(batch).numpy().astype(np.float32)
        drift_loss = max(drift_loss, float(np.abs(out[f"upd{k}_abs_loss"] - loss64[k]).max()))
    drift_param = 0.0
    for (name, key), n64 in zip(NETS, (a64, v64)):
        for (k, v), w in zip(getattr(solver, key).state_dict().items(), n64.state_dict().values()):
            out[f"final/{name}/{k}"] = v.numpy().astype(np.float32)
            drift_param = max(drift_param, float((v.double() - w).abs().max()))
    out.update(drift_param=np.float64(drift_param), drift_loss=np.float64(drift_loss), ratio_margin=np.float64(margin))
    out["act_seed"] = np.int64(seed + 1000)
    out["act_states"] = np.array([[0, 0, 0, 0], [1.2, -0.5, 0.1, 0.8], [-2.0, 1.5, -0.15, -2.0],
                                  [0.3, 0.2, 0.05, -0.4]], dtype=np.float32)
    torch.manual_seed(int(out["act_seed"]))
    res = [solver.act(s) for s in out["act_states"]]
    out["act_actions"] = np.array([a for a, _ in res], np.int64)
    out["act_logprobs"] = np.array([lp for _, lp in res], np.float32)
    return out


def main():
    mg.load_reference()
    mg._pkg("reth.algorithm.ppo")
    model_mod = mg._load("reth.algorithm.ppo.ppo_model", "reth/reth/algorithm/ppo/ppo_model.py")
    solver_mod = mg._load("reth.algorithm.ppo.ppo_solver", "reth/reth/algorithm/ppo/ppo_solver.py")
    util = sys.modules["reth.algorithm.util"]
    gym = sys.modules["gym"]
    states, returns = batch_inputs(util)
    best = None
    qualified = 0
    for seed in range(SEEDS):
        out = run_seed(seed, model_mod, solver_mod, gym, states, returns)
        ok = float(out["ratio_margin"]) > MARGIN
        qualified += ok
        print(f"seed {seed:2d}: ratio margin {float(out['ratio_margin']):.2e} drift param "
              f"{float(out['drift_param']):.2e} loss {float(out['drift_loss']):.2e}{'' if ok else '  (out)'}")
        if ok and (best is None or float(out["drift_param"]) < float(best["drift_param"])):
            best = out
    if best is None:
        raise SystemExit(f"no seed in 0..{SEEDS - 1} keeps every ratio {MARGIN} from the clip bounds")
    print(f"{qualified} of {SEEDS} seeds qualify; kept seed {int(best['seed'])}")
    # the return functions: a done in mid-sequence, a done at the end, none, constant rewards
    rng = np.random.default_rng(5)
    seqs = [(np.ones(12), np.array([0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 1], bool)),
            (rng.uniform(-1, 2, 9), np.array([0, 0, 1, 0, 0, 0, 1, 0, 0], bool)),
            (rng.uniform(0, 1, 5).astype(np.float32), np.zeros(5, bool)),
            (np.ones(200), np.arange(200) == 199)]
    best["ret/n"] = np.int64(len(seqs))
    for i, (r, done) in enumerate(seqs):
        best[f"ret/{i}/r"], best[f"ret/{i}/done"] = r, done
        best[f"ret/{i}/with_dones"] = util.calculate_discount_rewards_with_dones(r, done, 0.99)
        best[f"ret/{i}/plain"] = util.calculate_discount_rewards(r, 0.99)
    path = os.path.join(HERE, "ppo_cartpole_b64.npz")
    np.savez_compressed(path, **best)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
