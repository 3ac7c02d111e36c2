"""The PPO kernels where training takes them (inputs: _ppo_edges.py, premises: test_ppo_edges_cpu.py).

A. rth_ppo_rollout_finish (csrc/ppo_actor.hpp) on segments longer than one pass of its 256 lanes,
   against ppo_actors.HostRollout by test_ppo_actors_gpu._check_finish's criteria: s, a, logp, n, the
   row order, the new fill / complete and the moved rows exact, ret within 1 fp32 ulp.  Three
   finishes each (the table; at once again; after every carried episode has ended), in buffers with
   64 canary elements on either side.

B. rth_ppo_act / rth_ppo_grads / rth_ppo_actor_step (csrc/ppo.hpp) on saturated policies -- logits
   in the hundreds, probabilities of exactly 0.0f and 1.0f -- against fp64 on log_softmax of the
   logits.  The bound is the project's, |ours - fp64| <= max(1.5 e_ref, 1e-6 max|fp64|) per tensor,
   with e_ref the largest |fp32 - fp64| of three torch fp32 evaluations of the reference (as is,
   hidden units reversed, batch reversed): at these logits an fp32 evaluation's error is that of
   the last layer's summation order, of which one evaluation is one draw."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from _ppo_edges import (COLUMNS, FINISH_399, FINISH_399_LEFT, FINISH_399_N, FINISH_4096, FINISH_4096_LEFT,
                        FINISH_4096_N, SATURATED, VARIANTS, carried_endings, finish_segments, random_finish_cases,
                        saturated_case, saturated_ref, worst_fp32)
from reth_amd.ppo import _params6
from reth_amd.ppo_actors import HostRollout, VecPpoActors
from test_ppo_actors_gpu import (NAMES, SEED, _actors, _bits, _check_finish, _load_host, _ppo_act, _snapshot, _solver,
                                 _states)
from test_ppo_gpu import GRAD_NAMES, _check, _params, inverse_cdf, ppo_act, ppo_grads, uniforms_for
from test_ppo_loop_gpu import _grads

pytestmark = pytest.mark.gpu

G = 64  # canary elements on either side of every buffer


class Guarded(VecPpoActors):
    """test_no_write_outside_any_buffer's allocation: every device buffer between two canary runs"""

    def _alloc(self, shape, dtype):
        n = int(np.prod(shape))
        canary = 12345.5 if dtype.is_floating_point else 0x5A5A5A5A
        buf = torch.full((n + 2 * G,), canary, dtype=dtype, device=self.device)
        buf[G:G + n] = 0
        self.__dict__.setdefault("_guarded", []).append((buf, n, canary))
        return buf[G:G + n].view(shape)


def _intact(act):
    torch.cuda.synchronize()
    assert len(act._guarded) == len(NAMES) + 4  # every device buffer of the set, and the batch's four
    for buf, n, canary in act._guarded:
        assert (buf[:G] == canary).all() and (buf[G + n:] == canary).all(), (buf.dtype, n)


# ---------------------------------------------------------------------------- A. the finish
def _three_finishes(cases, cap, horizon, max_episode_steps, gamma, n_want=None, left_want=None, **kw):
    """the table through three finishes on the device and on the oracle -> the largest |ret| difference
    in fp32 ulps"""
    N = len(cases)
    zero = kw.get("zero_rewards", False)
    act = _actors("Acrobot-v1", N, horizon=horizon, cls=Guarded, max_episode_steps=max_episode_steps)
    assert act.cap == cap and act.obs_dim == 6
    seg = finish_segments(cases, cap, **kw)
    for k in COLUMNS + ("fill",):
        getattr(act, k).copy_(seg[k])
    act._complete[0].copy_(seg["complete"])  # gen = 0: slot 0 is live
    host = HostRollout(N, cap, 6)
    _load_host(act, host)
    assert host.complete.tolist() == seg["complete"].tolist()
    ulps = _check_finish(act, host, "first", gamma)
    n = int(act.n_dev)
    assert n == int(seg["complete"].sum()) and (n_want is None or n == n_want)
    assert not zero or not act.batch[2][:n].any()  # zero variance: every return is 0
    assert left_want is None or host.fill.tolist() == left_want
    assert (act.gen == 1).all()
    # a second finish at once: nothing is complete, nothing moves
    before = _snapshot(act)
    assert _check_finish(act, host, "second", gamma) == 0.0 and int(act.n_dev) == 0
    for k in COLUMNS + ("fill",):
        assert _bits(getattr(act, k)) == _bits(before[k]), k
    # every carried episode ends: its rows come out first, with their old log-probabilities
    ends = carried_endings(host.fill, cap)
    for i, row, fill in ends:
        act.seg_done[i, row] = 1.0
        act.fill[i] = fill
        act._complete[0, i] = fill  # gen = 2: slot 0 is live again
    _load_host(act, host)
    ulps = max(ulps, _check_finish(act, host, "third", gamma))
    assert int(act.n_dev) == sum(fill for _, _, fill in ends) and not act.fill.any()
    assert not zero or not act.batch[2][:int(act.n_dev)].any()
    lp, off = act.batch[3], 0
    for i, row, fill in ends:
        m, e = cases[i][0], int(seg["complete"][i])
        assert _bits(lp[off:off + m - e]) == seg["seg_logp"][i, e:m].numpy().tobytes(), i
        off += fill
    _intact(act)
    return ulps


@pytest.mark.parametrize("gamma,zero_rewards", [(0.99, False), (0.0, False), (1.0, False), (0.99, True)])
def test_finish_past_one_pass_at_cap_399(dev, gamma, zero_rewards):
    """cap = 399, the CartPole loop's segment: two trips of every 256-lane loop, a carry of two chunks
    (a shift by one row among them), episodes across and at row 256; also at gamma 0 and 1 and with
    all rewards 0 (zero variance: every return is 0).  ret is 0 fp32 ulps from HostRollout on an MI355X
    in all four runs."""
    ulps = _three_finishes(FINISH_399, 399, 200, 200, gamma, FINISH_399_N, FINISH_399_LEFT, zero_rewards=zero_rewards)
    print(f"finish, cap 399, gamma {gamma}, zero rewards {zero_rewards}: max |ret - HostRollout| = {ulps} fp32 ulps")


def test_finish_at_the_largest_cap(dev):
    """cap = 4096 (kPpoMaxCap, 32 KB of dynamic LDS): a carry of 4095 rows over one (16 overlapping
    chunks, the observations 24,570 floats shifted by 6), one episode of 4096 rows on one lane, episodes
    at and around rows 256 and 512.  ret is 0 fp32 ulps from HostRollout on an MI355X."""
    ulps = _three_finishes(FINISH_4096, 4096, 3597, 500, 0.99, FINISH_4096_N, FINISH_4096_LEFT)
    print(f"finish, cap 4096: max |ret - HostRollout| = {ulps} fp32 ulps")


def test_finish_with_ragged_counts_over_600_envs(dev):
    """N = 600, cap = 12, per env a random fill and 0..3 random done rows: the batch offset of env i sums
    i ragged counts in up to three trips.  n and every batch row against the oracle; ret is 0 fp32 ulps
    from it on an MI355X."""
    ulps = _three_finishes(random_finish_cases(), 12, 5, 8, 0.99, seed=1)
    print(f"finish, N = 600: max |ret - HostRollout| = {ulps} fp32 ulps")


def _scripted_action(act, t):
    """CartPole: push towards the pole's lean (which balances up to the time limit), except in two
    windows per env in which the cart is pushed left until the pole falls"""
    obs = act.cur_obs[:, :4]
    i = torch.arange(act.N, device=obs.device)
    fall = ((t >= 60 + 7 * i) & (t < 85 + 7 * i)) | ((t >= 370 + 7 * i) & (t < 395 + 7 * i))
    return torch.where(fall, 0, (obs[:, 2] + 0.5 * obs[:, 3] > 0).long())


def test_stepped_rollouts_at_the_workloads_cap(dev):
    """CartPole-v0, N = 3, horizon 200, the default time limit (cap = 399), three rollouts: the step's
    store and the finish meet at the workload's size.  An untrained policy ends episodes after 20 to 30
    steps, so `complete` stays below 200 + 30; the actions are scripted instead (_scripted_action), the
    log-probabilities are the actor's for them.  Seed SEED: the counts at the three finishes are
    complete = [88, 96, 93], [311, 300, 301] and [200, 12, 11]; ret is 0 fp32 ulps from HostRollout."""
    env, N = "CartPole-v0", 3
    solver = _solver(env)
    act = _actors(env, N, horizon=200, cls=Guarded, max_episode_steps=None)
    assert act.cap == 399
    host = HostRollout(N, act.cap, 4)
    counts, worst, carried = [], 0.0, np.zeros(N, np.int32)
    for rollout in range(3):
        for k in range(200):
            act.step(solver, action_in=_scripted_action(act, rollout * 200 + k))
        _load_host(act, host)
        counts.append(host.complete.tolist())
        assert (host.fill == carried + 200).all()
        worst = max(worst, _check_finish(act, host, rollout))
        carried = host.fill.copy()
    print(f"stepped CartPole, cap 399: complete at the three finishes {counts}, max |ret - HostRollout| = {worst} ulps")
    assert int(act.dropped.sum()) == 0 and (act.t_dev == 600).all()
    assert max(max(c) for c in counts) > 256
    _intact(act)


# ---------------------------------------------------------------------------- B. saturated policies
def _check3(label, ours, shape, scale, pick, fails):
    """the module docstring's bound on one tensor, each evaluation's error printed"""
    worst, r64, errs = worst_fp32(shape, scale, pick)
    print(f"{label:44s} e_ref " + "  ".join(f"{v} {e:.3e}" for v, e in zip(VARIANTS, errs)))
    assert torch.isfinite(ours).all(), label
    _check(label, ours, worst, r64, fails)


def _uniforms(B, dev, seed):
    u = torch.rand(B, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(dev)
    u[0], u[1] = 0.0, 1.0 - 2.0 ** -53
    return u


@pytest.mark.parametrize("shape,scale", SATURATED, ids=str)
def test_act_on_a_saturated_policy(dev, shape, scale):
    B, D, A = shape
    c = saturated_case(*shape, scale)
    assert saturated_ref(shape, scale, torch.float64)["ratio_ok"]
    u = _uniforms(B, dev, 5)
    action, logprob, probs = ppo_act(_params(c, dev)[0], c["s"].to(dev), D, A, uniforms=u)
    assert int(action.min()) >= 0 and int(action.max()) < A
    fails = []
    tag = f"{shape} x {scale} seed {c['seed']} "
    _check3(tag + "probs", probs, shape, scale, lambda r: r["probs"], fails)
    pick = lambda t: t.gather(1, action.cpu()[:, None])[:, 0]
    _check3(tag + "logprob", logprob, shape, scale, lambda r: pick(r["logp_all"]), fails)
    assert not fails, fails
    assert bool((probs == 0.0).any()) and bool((probs == 1.0).any())
    assert np.array_equal(action.cpu().numpy(), inverse_cdf(probs, u))
    assert int(action[0]) == int((probs[0] > 0).nonzero()[0])  # u = 0: the first action with a probability
    # p_j = exp(logp_j): exp in fp64 on the host, rounded once (a probability may be subnormal)
    assert torch.allclose(logprob.cpu().double().exp().float(), pick(probs.cpu()), rtol=1e-6, atol=0)
    assert torch.allclose(logprob.exp(), pick(probs.cpu()).to(dev), rtol=1e-6, atol=0)


@pytest.mark.parametrize("shape,scale", SATURATED, ids=str)
def test_grads_on_a_saturated_policy(dev, shape, scale):
    """|loss|, the loss mean, the new log-probabilities and the twelve gradients within the module
    docstring's bound, then the bit-for-bit relations, which are checked before the bound is asserted.

    This test found the one change to the kernel.  With the last layer summed in fp32 (dense.hpp's
    order, as the hidden layers are) |loss| of (257, 64, 18) x 256 was 5.429e-05 against a bound of
    5.407e-05: row 3, a deep row inside the clip range whose |advantage| 3.01 is the batch's largest, had
    its logit difference z_a - max z (-84.5 and 55.0) 1.4e-05 off, 1.9 fp32 spacings of a logit, and
    rho |adv| carried that into the loss.  ppo_forward_rows now sums the last layer's 64 products in fp64
    and rounds the logit once: that tensor is 2.02e-05 off, and on an MI355X all 102 tensors (act and
    grads, six cases) are inside the bound -- the worst of each kind at 0.31 (probs), 0.58 (the drawn
    action's log-probability), 0.45 (|loss|), 0.42 (loss mean), 0.14 (new log-probabilities), 0.74 (actor
    gradients) and 0.67 (value gradients) of it."""
    B, D, A = shape
    c = saturated_case(*shape, scale)
    P = _params(c, dev)
    assert saturated_ref(shape, scale, torch.float64)["ratio_ok"]
    loss_abs, loss_mean, grads, ws = ppo_grads(P, c, dev)
    fails = []
    tag = f"{shape} x {scale} seed {c['seed']} "
    _check3(tag + "|loss|", loss_abs, shape, scale, lambda r: r["loss_abs"], fails)
    _check3(tag + "loss mean", loss_mean.view(()), shape, scale, lambda r: r["loss_mean"], fails)
    _check3(tag + "new logp", ws[:B], shape, scale, lambda r: r["logp"], fails)
    for k, (name, g) in enumerate(zip(GRAD_NAMES, grads)):
        assert g.shape == saturated_ref(shape, scale, torch.float64)["grads"][k].shape
        _check3(tag + name, g, shape, scale, lambda r, k=k: r["grads"][k], fails)
    # evaluate only: the same loss bit for bit, the gradient buffers left alone
    keep = [torch.full_like(g, float("nan")) for g in grads]
    la2, lm2, _, ws2 = ppo_grads(P, c, dev, backward=False, grads=keep)
    assert torch.equal(la2, loss_abs) and torch.equal(lm2, loss_mean) and torch.equal(ws2[:B], ws[:B])
    assert all(bool(torch.isnan(k).all()) for k in keep)
    # the new log-probabilities are rth_ppo_act's for those actions, bit for bit -- on the rows whose
    # action a uniform can draw: a deep row's CDF interval is empty in fp32 (those go through
    # action_in: test_actor_step_on_a_saturated_policy)
    x, a = c["s"].to(dev), c["a"].to(dev)
    _, _, probs = ppo_act(P[0], x, D, A, uniforms=torch.zeros(B, dtype=torch.float64, device=dev))
    cdf = torch.cat([torch.zeros(B, 1), torch.as_tensor(np.cumsum(probs.cpu().numpy(), axis=1, dtype=np.float32))], 1)
    can = (cdf.gather(1, c["a"][:, None] + 1) > cdf.gather(1, c["a"][:, None]))[:, 0]
    assert not can[c["deep"]].any() and can[torch.arange(B) % 3 != 0].all()
    action, logprob, _ = ppo_act(P[0], x, D, A, uniforms=uniforms_for(probs, c["a"]))
    assert torch.equal(action.cpu()[can], c["a"][can]) and torch.equal(logprob.cpu()[can], ws[:B].cpu()[can])
    if (shape, scale) == ((130, 17, 6), 1024):
        # rth_ppo_grads_n at capacity B + 63, NaN rows and actions out of range behind the count
        full = [x, a, c["ret"].to(dev), c["old"].to(dev)]
        want = _grads(P, full, B, D, A)
        pad = lambda t: torch.full((63, *t.shape[1:]), 99 if t.dtype == torch.int64 else float("nan"), dtype=t.dtype,
                                   device=dev)
        cols = [torch.cat([t, pad(t)]) for t in full]
        got = _grads(P, cols, B + 63, D, A, torch.tensor([B], dtype=torch.int64, device=dev))
        for k, (g, w, mine) in enumerate(zip(got[0], want[0], grads)):
            assert _bits(g) == _bits(w) == _bits(mine), k
        assert _bits(got[1][:B]) == _bits(want[1]) == _bits(loss_abs) and torch.isnan(got[1][B:]).all()
        assert _bits(got[2]) == _bits(want[2]) == _bits(loss_mean)
        assert _bits(got[3][:B]) == _bits(want[3][:B]) == _bits(ws[:B])
    assert not fails, fails


def test_actor_step_on_a_saturated_policy(dev):
    """Acrobot-v1 (D 6, A 3), the actor's last weight scaled by 1024, N = 9"""
    env, N, D, A = "Acrobot-v1", 9, 6, 3
    solver = _solver(env)
    with torch.no_grad():
        solver.actor_network.action_layer[4].weight.mul_(256.0)  # 4 x 256, both powers of two
    st = _states(env, N, np.random.default_rng(3))
    act = _actors(env, N)
    act.set_state(st)
    obs = act.current_obs()
    act.step(solver)
    a, lp = _ppo_act(solver, obs, SEED, 1)
    assert _bits(act.last_action) == _bits(a) and _bits(act.last_logprob) == _bits(lp) and torch.isfinite(lp).all()
    assert _bits(act.seg_a[:, 0]) == _bits(a) and _bits(act.seg_logp[:, 0]) == _bits(lp)
    # each row's least probable action (by fp64 on the host), forced
    ps = [p.detach() for p in _params6(solver.actor_network)]
    h = obs.cpu().double()
    for w, b, f in zip(ps[0::2], ps[1::2], (torch.tanh, torch.tanh, lambda t: t)):
        h = f(F.linear(h, w.cpu().double(), b.cpu().double()))
    logp64 = F.log_softmax(h, 1)
    least = logp64.argmin(1).to(dev)
    want64 = logp64.min(1).values
    print("saturated Acrobot actor: fp64 logp of the least probable action", [round(float(v)) for v in want64])
    assert int((want64 < -104).sum()) >= 3 and float(h.abs().max()) > 100
    act.set_state(st)
    act.step(solver, action_in=least)
    got = act.seg_logp[:, 1]
    assert _bits(act.seg_a[:, 1]) == _bits(least) and _bits(act.last_logprob) == _bits(got)
    assert torch.isfinite(got).all()
    assert _bits(act.seg_s[:, 1]) == _bits(obs)
    # rth_ppo_act's log-softmax for those actions: rth_ppo_grads' new log-probabilities are its rows
    # (test_grads_on_a_saturated_policy), also where the probability is 0 and no uniform draws the action
    ps = [p.contiguous() for p in ps]
    c = dict(shape=(N, D, A), s=obs.cpu(), a=least.cpu(), ret=torch.zeros(N), old=torch.zeros(N))
    value = [p.detach().contiguous() for p in _params6(solver.value_network)]
    _, _, _, ws = ppo_grads([ps, value], c, dev, backward=False)
    assert _bits(got) == _bits(ws[:N])
    _, _, probs = ppo_act(ps, obs, D, A, uniforms=torch.zeros(N, dtype=torch.float64, device=dev))
    p_least = probs.gather(1, least[:, None])[:, 0]
    zero = (p_least == 0).cpu()
    assert int(zero.sum()) >= 3 and bool(zero[want64 < -104.5].all()) and not bool(zero[want64 > -103].any())
    draw = p_least > 1e-6  # a uniform inside the action's CDF interval draws it
    if bool(draw.any()):
        a2, lp2, _ = ppo_act(ps, obs, D, A, uniforms=uniforms_for(probs, least))
        assert torch.equal(a2[draw], least[draw]) and torch.equal(lp2[draw], got[draw])


def test_each_saturated_row_alone_equals_the_batch(dev):
    shape, scale = (130, 17, 6), 1024
    B, D, A = shape
    c = saturated_case(*shape, scale)
    ps, x = _params(c, dev)[0], c["s"].to(dev)
    u = _uniforms(B, dev, 6)
    out = ppo_act(ps, x, D, A, uniforms=u)
    assert bool((out[2] == 0).any()) and bool((out[2] == 1).any())
    one = [ppo_act(ps, x[i:i + 1], D, A, uniforms=u[i:i + 1]) for i in range(B)]
    flip = ppo_act(ps, x.flip(0).contiguous(), D, A, uniforms=u.flip(0).contiguous())
    for k in range(3):
        assert torch.equal(torch.cat([o[k] for o in one]), out[k]) and torch.equal(flip[k].flip(0), out[k])
