"""Microbench (development aid): bootstrapping device PPO's GAE through time-limit ends
(csrc/ppo_actor.hpp rth_ppo_actor_step_tl / rth_ppo_gae_finish_tl, reth_amd/ppo_loop.py
bootstrap_time_limit) at the CartPole shape (D = 4, A = 2, H = 64).  HIP events after a warm-up, three
interleaved rounds (host launch time included: the events bracket the whole window):

  - rth_ppo_actor_step_tl beside rth_ppo_actor_step at N = 64;
  - the _tl finish with no truncated row and with every row truncated beside rth_ppo_gae_finish, at
    64 x 32 and 10 x 200 (full segments written directly; the fills are restored outside the events);
  - one iteration at 64 x 32 with the option on and off, eager and as a replayed graph;
  - the default (option off) iteration of this tree beside the one of another checkout (--parent-tree,
    a built tree of the parent commit), each in a process of its own, alternating, PPOT_PROCS (default
    3) processes per tree: 64 x 32 with GAE, and PpoLoopConfig()'s 10 x 200;
  - 50 iterations at 64 x 32, seeds 0 / 1 / 2, with the option on and off: the envs' mean last finished
    episode length, and with the option on the mean return target of the last rollout's truncated
    rows through both finishes (--learning-rates, default 0.01).

Every line goes to stdout and to --out (default profiles/r25/ppo_timelimit.txt)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPS = int(os.environ.get("PPOT_REPS", "100"))
PROCS = int(os.environ.get("PPOT_PROCS", "3"))
GAE_CFG = dict(n_actors=64, horizon=32, gae_lambda=0.95, normalize_adv=True)


def timed(torch, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def child(tree):
    """the default iterations of the tree at `tree`, three rounds of 50 each after a warm-up -> one JSON line"""
    sys.path.insert(0, tree)
    import torch

    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    loops = {"GAE 64 x 32": PpoLoop(PpoLoopConfig(**GAE_CFG), device="cuda"), "default 10 x 200": PpoLoop(PpoLoopConfig(), device="cuda")}
    res = {k: [] for k in loops}
    for loop in loops.values():
        for _ in range(5):
            loop.iteration()
    torch.cuda.synchronize()
    for _ in range(3):
        for k, loop in loops.items():
            res[k].append(timed(torch, loop.iteration, 50) * 1e-3)
    print(json.dumps(res))


def main(out, parent_tree, learning_rates):
    sys.path.insert(0, ROOT)
    import torch

    from reth_amd.ppo import PPOSolver
    from reth_amd.ppo_actors import VecPpoActors
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig
    from reth_amd.solver import Box, Discrete

    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    log = open(out, "w")

    def say(line):
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    def rounds(name, fns, reps=REPS, unit="us", scale=1.0, before=None):
        res = {k: [] for k in fns}
        for k, fn in fns.items():
            for _ in range(3):
                if before:
                    before(k)
                fn()
        torch.cuda.synchronize()
        for _ in range(3):
            for k, fn in fns.items():
                if before:  # one call between two events, its input restored outside them
                    t = []
                    for _ in range(reps):
                        before(k)
                        t.append(timed(torch, fn, 1))
                    res[k].append(sorted(t)[len(t) // 2] * scale)
                else:
                    res[k].append(timed(torch, fn, reps) * scale)
        say(f"{name}: " + "  ".join(f"{k} {' / '.join(f'{t:.1f}' for t in v)} {unit}" for k, v in res.items()))
        return res

    dev = torch.device("cuda")
    say(f"bootstrapping GAE through time-limit ends on {torch.cuda.get_device_name(0)}; HIP events, three interleaved "
        f"rounds, {REPS} repetitions a round unless noted")
    torch.manual_seed(0)
    s = PPOSolver(Box(-1, 1, (4,)), Discrete(2), device=dev, impl="hip")
    # the step
    assert 6 * REPS + 6 <= 4096, "PPOT_REPS: every timed step stores its row"
    steps = {"rth_ppo_actor_step": VecPpoActors("CartPole-v0", 64, 32, device=dev, cap=4096),
             "rth_ppo_actor_step_tl": VecPpoActors("CartPole-v0", 64, 32, device=dev, cap=4096, time_limit_bootstrap=True)}
    rounds("actor step N=64 (segments of 4096 rows: every step stores its row)",
           {k: (lambda a=a: a.step(s)) for k, a in steps.items()})
    assert all(int(a.dropped.sum()) == 0 for a in steps.values())
    # the finishes on full segments
    for n, cap in ((64, 32), (10, 200)):
        sets = {"rth_ppo_gae_finish": (VecPpoActors("CartPole-v0", n, cap, device=dev, cap=cap), None),
                "_tl, no row truncated": (VecPpoActors("CartPole-v0", n, cap, device=dev, cap=cap, time_limit_bootstrap=True), 0.0),
                "_tl, every row truncated": (VecPpoActors("CartPole-v0", n, cap, device=dev, cap=cap, time_limit_bootstrap=True), 1.0)}
        g = torch.Generator().manual_seed(n)
        seg_s, seg_r = torch.randn((n, cap, 4), generator=g).to(dev), torch.randn((n, cap), generator=g).to(dev)
        for act, flag in sets.values():
            act.seg_s.copy_(seg_s), act.seg_r.copy_(seg_r)
            if flag is not None:
                act.seg_trunc.fill_(flag), act.seg_done.fill_(flag), act.seg_term_s.copy_(seg_s.flip(1))
        rounds(f"finish_gae {n} x {cap} (the median of one call between two events)",
               {k: (lambda a=a: a.finish_gae(s, 0.99, 0.95)) for k, (a, _) in sets.items()}, reps=max(REPS // 4, 5),
               before=lambda k: sets[k][0].fill.fill_(cap))
    # one iteration
    loops = {}
    for option in (False, True):
        for graph in (False, True):
            loop = PpoLoop(PpoLoopConfig(bootstrap_time_limit=option, **GAE_CFG), device=dev)
            loop.iteration()
            if graph:
                loop.capture()
            loops[f"option {'on' if option else 'off'} {'graph' if graph else 'eager'}"] = loop
    rounds("PpoLoop iteration 64 x 32 (2,048 env steps + finish + normalise + update)",
           {k: v.iteration for k, v in loops.items()}, reps=50, unit="ms", scale=1e-3)
    del loops
    # the default path beside the parent commit's, a process each
    if parent_tree:
        res = {"this tree": [], "parent": []}
        for _ in range(PROCS):
            for k, tree in (("this tree", ROOT), ("parent", os.path.abspath(parent_tree))):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tree], capture_output=True, text=True,
                                   check=True)
                res[k].append(json.loads(p.stdout.strip().splitlines()[-1]))
        for shape in res["this tree"][0]:
            for k, runs in res.items():
                best = [min(r[shape]) for r in runs]
                say(f"default iteration {shape}, option off, {k}: best of 3 rounds x 50 in each of {PROCS} alternating "
                    f"processes " + " / ".join(f"{t:.2f}" for t in best) + f" ms (spread {max(best) - min(best):.2f} ms; all rounds "
                    + "; ".join(" / ".join(f"{t:.2f}" for t in r[shape]) for r in runs) + ")")
    else:
        say("default iteration beside the parent commit's: not measured (no --parent-tree)")
    # learning
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from _ppo_timelimit import learn

    for lr in learning_rates:
        for option in (True, False):
            trained, untrained, targets = learn(option, learning_rate=lr)
            mid = (sorted(untrained)[1] + 200.0) / 2
            say(f"CartPole-v0 64 x 32, lambda 0.95, normalised, 50 iterations, learning rate {lr}, seeds 0/1/2, option "
                f"{'on' if option else 'off'}: mean last finished length " + " / ".join(f"{t:.1f}" for t in trained)
                + " (median " + f"{sorted(trained)[1]:.1f}), untrained " + " / ".join(f"{t:.1f}" for t in untrained)
                + f", midpoint {mid:.1f}")
            for seed, (on, off, rows) in enumerate(targets):
                say(f"  seed {seed}: mean ret over the last rollout's {rows} truncated rows, the trained value network: "
                    f"{on:.2f} with the bootstrap, {off:.2f} without")
    log.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25", "ppo_timelimit.txt"))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--learning-rates", type=float, nargs="*", default=[0.01])
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        child(args.child)
    else:
        main(args.out, args.parent_tree, args.learning_rates)
