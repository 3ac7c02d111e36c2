"""Inputs for the PPO kernels where training takes them and the comfortable tests do not (helper of
test_ppo_edges_cpu.py and test_ppo_edges_gpu.py; torch / numpy on the CPU, nothing runs on a GPU).

A. Rollout segments longer than one pass of the finish's workgroup (256 lanes, csrc/ppo_actor.hpp):
   tables of (fill, done rows), one env per entry, at cap = 399 (the CartPole loop's segment) and
   cap = 4096 (kPpoMaxCap), random columns for them, a ragged random table for N = 600 envs, and
   the rows that end every carried episode before the third finish.

B. Saturated policies: test_ppo_gpu.case with the actor's last weight scaled by 256 or 1024
   instead of 4, so that logits are in the hundreds, exp(z - max) underflows and probabilities round
   to 0.0f and 1.0f.  The reference is the reference's update (ppo_solver.py:72-96) on
   F.log_softmax of the logits: the kernels' function, which has no clamp.  Categorical(probs)
   clamps the probabilities to [1.19e-7, 1 - 1.19e-7] and is another function here.
"""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from reth_amd.ppo import ENT_COEF, VF_COEF, _params6
from test_ppo_gpu import EPS, RHO, _nets

# ---------------------------------------------------------------------------- A. the finish
# (fill, done rows), one env each
FINISH_399 = [(399, [198]),
              (399, [0]),               # e = 1, keep = 398: a shift by one row across two chunks
              (399, [398]),             # one episode of 399 rows, nothing kept
              (257, [255, 256]),        # an episode of one row at row 256
              (399, []),                # nothing complete
              (300, [256]),             # the owner lane is lane 0 on its second trip
              (399, [100, 199, 398]),
              (258, [0, 257])]
FINISH_4096 = [(4096, [0]),             # keep = 4095: 16 overlapping chunks, 24,570 floats shifted by 6
               (4096, [4095]),          # one episode of 4096 rows
               (4096, [2047]),
               (4096, [255, 256, 257, 511, 512, 4000]),
               (513, [256])]
# what the first finish gives
FINISH_399_N, FINISH_399_LEFT = 1770, [200, 398, 0, 0, 399, 43, 0, 0]
FINISH_4096_N, FINISH_4096_LEFT = 10403, [4095, 0, 2048, 95, 256]

COLUMNS = ("seg_s", "seg_a", "seg_r", "seg_done", "seg_logp")


def random_finish_cases(n_envs=600, cap=12, seed=0):
    """per env a fill in 0..cap and 0..3 done rows among the stored ones: ragged `complete`"""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n_envs):
        fill = int(rng.integers(0, cap + 1))
        k = min(int(rng.integers(0, 4)), fill)
        cases.append((fill, sorted(int(t) for t in rng.choice(fill, k, replace=False)) if k else []))
    return cases


def finish_segments(cases, cap, D=6, A=3, seed=0, zero_rewards=False):
    """random columns [N, cap, .] (CPU tensors) with the table's done rows, fill and complete"""
    N = len(cases)
    g = torch.Generator().manual_seed(seed)
    seg = dict(seg_s=torch.randn((N, cap, D), generator=g), seg_a=torch.randint(0, A, (N, cap), generator=g),
               seg_r=torch.randn((N, cap), generator=g), seg_done=torch.zeros((N, cap)),
               seg_logp=-torch.rand((N, cap), generator=g))
    if zero_rewards:
        seg["seg_r"].zero_()
    seg["fill"] = torch.tensor([f for f, _ in cases], dtype=torch.int32)
    seg["complete"] = torch.tensor([d[-1] + 1 if d else 0 for _, d in cases], dtype=torch.int32)
    for i, (fill, dones) in enumerate(cases):
        assert 0 <= fill <= cap and all(0 <= t < fill for t in dones) and dones == sorted(dones)
        seg["seg_done"][i, dones] = 1.0
    return seg


def load_segments(host, seg):
    """finish_segments' columns into a HostRollout"""
    for k in COLUMNS + ("fill", "complete"):
        getattr(host, k)[...] = seg[k].numpy()


def carried_endings(fills, cap):
    """(env, done row, new fill) that ends every carried episode: one more row, a done row, behind the
    carried ones; a segment that is full (no episode is that long in a loop, the table has one) ends at
    its last row instead"""
    return [(i, min(f, cap - 1), min(f + 1, cap)) for i, f in enumerate(int(v) for v in fills) if f > 0]


# ---------------------------------------------------------------------------- B. saturated policies
# (B, D, A), the factor on the actor's last weight
SATURATED = [((67, 7, 3), 256), ((130, 17, 6), 256), ((257, 64, 18), 256), ((130, 17, 6), 1024),
             ((257, 64, 18), 1024), ((64, 4, 2), 1024)]
DEEP_LOGP = -104.0  # exp(-104) < 2^-150: the probability is 0.0f
VARIANTS = ("as is", "hidden units reversed", "batch reversed")


def _forward(ps, x):
    h = torch.tanh(F.linear(x, ps[0], ps[1]))
    h = torch.tanh(F.linear(h, ps[2], ps[3]))
    return F.linear(h, ps[4], ps[5])


def clip_class(rho, adv):
    """(below / inside / above the clip range) x (sign of the advantage) as 0..5"""
    return torch.where(rho < 1 - EPS, 0, torch.where(rho > 1 + EPS, 2, 1)) * 2 + (adv > 0).long()


@functools.lru_cache(maxsize=None)
def saturated_case(B, D, A, scale):
    """test_ppo_gpu.case with the last weight scaled by `scale`: the first seed's networks and batch
    (CPU tensors; shared, never modified) at which, in fp64, all six classes are present, all six
    also among the deep rows (forced least probable action with logp < -104), one row's largest
    probability rounds to 1.0f and another's is below 0.9"""
    for seed in range(40):
        torch.manual_seed(seed)
        nets = _nets(D, A)
        with torch.no_grad():
            nets[0].action_layer[4].weight.mul_(float(scale))
        s, ret = torch.randn(B, D), torch.randn(B)
        a64, v64 = _nets(D, A, torch.float64, nets)
        with torch.no_grad():
            z64 = _forward(_params6(a64), s.double())
            logp64 = F.log_softmax(z64, 1)
            adv = ret.double() - v64(s.double()).squeeze(-1)
        g = torch.Generator().manual_seed(1000 + seed)
        a = torch.multinomial(logp64.exp(), 1, generator=g)[:, 0]
        forced = torch.arange(B) % 3 == 0
        a = torch.where(forced, logp64.argmin(1), a)
        rho = torch.tensor(RHO, dtype=torch.float64)[torch.arange(B) % len(RHO)]
        picked = logp64.gather(1, a[:, None])[:, 0]
        old = (picked - rho.log()).float()
        where = clip_class(rho, adv)
        deep = forced & (picked < DEEP_LOGP)
        pmax = logp64.max(1).values.exp()
        if (len(set(where.tolist())) != 6 or len(set(where[deep].tolist())) != 6
                or not float(pmax.max()) > 1 - 2.0 ** -25 or not float(pmax.min()) < 0.9):
            continue
        return dict(seed=seed, shape=(B, D, A), scale=scale, nets=nets, s=s, a=a, ret=ret, old=old, deep=deep,
                    min_logp=float(logp64.min()), max_z=float(z64.abs().max()),
                    exp_underflows_in_fp64=bool(((z64 - z64.max(1, keepdim=True).values).exp() == 0).any()))
    raise AssertionError(f"no qualifying seed in 0..39 for {(B, D, A)} x {scale}")


@functools.lru_cache(maxsize=None)
def saturated_ref(shape, scale, dtype, variant="as is"):
    """ppo_solver.py:72-96 on log_softmax of the logits, torch ops on the CPU in `dtype`: probs, the
    log-probabilities, |loss|, the loss mean and the twelve gradients (actor, then value), computed
    once per case.  The variants evaluate the same function in another summation order -- the hidden
    units of both hidden layers reversed, or the batch reversed -- and return it in the case's."""
    c = saturated_case(*shape, scale)
    assert variant in VARIANTS
    hidden, batch = variant == VARIANTS[1], variant == VARIANTS[2]

    def params(net):
        w1, b1, w2, b2, w3, b3 = (p.detach().to(dtype) for p in _params6(net))
        if hidden:
            w1, b1, w2, b2, w3 = w1.flip(0), b1.flip(0), w2.flip(0).flip(1), b2.flip(0), w3.flip(1)
        return [p.clone().contiguous().requires_grad_() for p in (w1, b1, w2, b2, w3, b3)]

    def grads(ps):
        g1, c1, g2, c2, g3, c3 = (p.grad for p in ps)
        if hidden:
            g1, c1, g2, c2, g3 = g1.flip(0), c1.flip(0), g2.flip(0).flip(1), c2.flip(0), g3.flip(1)
        return [g1, c1, g2, c2, g3, c3]

    order = (lambda t: t.flip(0).contiguous()) if batch else (lambda t: t)
    actor, value = params(c["nets"][0]), params(c["nets"][1])
    s, ret, old, a = order(c["s"].to(dtype)), order(c["ret"].to(dtype)), order(c["old"].to(dtype)), order(c["a"])
    logp_all = F.log_softmax(_forward(actor, s), 1)
    probs = logp_all.exp()
    entropy = -(probs * logp_all).sum(1)
    logp = logp_all.gather(1, a[:, None])[:, 0]
    v = torch.squeeze(_forward(value, s), -1)
    ratios = torch.exp(logp - old)
    adv = ret - v.detach()
    rho = ratios.detach()
    ratio_ok = float(torch.minimum((rho - (1 - EPS)).abs(), (rho - (1 + EPS)).abs()).min()) > 0.04
    loss = (-torch.min(ratios * adv, torch.clamp(ratios, 1 - EPS, 1 + EPS) * adv) + VF_COEF * F.mse_loss(v, ret)
            - ENT_COEF * entropy)
    loss.mean().backward()
    return dict(probs=order(probs.detach()), logp_all=order(logp_all.detach()), logp=order(logp.detach()),
                loss_abs=order(loss.detach().abs()), loss_mean=loss.detach().mean(), grads=grads(actor) + grads(value),
                ratio_ok=ratio_ok, classes=order(clip_class(rho, adv)))


def worst_fp32(shape, scale, pick):
    """pick(ref) of the three fp32 evaluations -> (the elementwise farthest from fp64, fp64, each
    evaluation's max |fp32 - fp64|): one torch evaluation is one draw of the summation order's error,
    so the reference's own error is the largest of the three"""
    r64 = pick(saturated_ref(shape, scale, torch.float64))
    r32 = torch.stack([pick(saturated_ref(shape, scale, torch.float32, v)).double() for v in VARIANTS])
    err = (r32 - r64).abs()
    worst = r32.gather(0, err.argmax(0, keepdim=True))[0]
    return worst, r64, [float(e.max()) for e in err]
