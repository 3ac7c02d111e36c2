"""PPO on MI355X: reth.algorithm.PPOSolver's interface on fused HIP actor-value kernels.

Reference: reth/reth/algorithm/ppo/ppo_solver.py:15-125, ppo_model.py:6-68 and
algorithm/util.py:27-53 (the discounted returns).  The actor (Linear D->64, tanh, Linear 64->64,
tanh, Linear 64->A, softmax) and the value network (the same torso, Linear 64->1) keep the
reference's module structure, parameter names, construction order and RNG draws, so under one
torch.manual_seed both networks are the reference's element for element and the weights stream
(the actor's state_dict) loads on either side.

impl="torch" is the reference's formulation (nn.Sequential, Categorical, autograd, two
torch.optim.Adam) on the solver's device: the yardstick.  impl="hip" runs csrc/ppo.hpp: per epoch
one rth_ppo_grads call (both forwards, ratio, clipped surrogate, entropy, value error, twelve
gradients) and the two Adam steps (ClipAdam without a clip); act / act_batch are one rth_ppo_act
launch, which draws the action by inverse CDF from a counter-based Philox uniform of (the
solver's seed, its call counter, the row).  impl=None takes "hip" where it applies (a GPU, fp32,
a shape rth_ppo_supported builds) and "torch" elsewhere; asked for explicitly, "hip" raises
instead.  solver.impl_active names the path that runs and solver.hip_launches counts its ABI calls.
n_minibatches = K > 1 turns every epoch into a shuffled pass of K optimiser steps: rth_ppo_shuffle
(csrc/ppo_shuffle.hpp) draws the order on the device and the same gradient kernels take each slice;
shuffle_keys / minibatch_perm restate the order in numpy.

The kernels take the log-softmax of the logits; the reference's Categorical(probs=softmax(z))
clamps the probabilities to [1.19e-7, 1 - 1.19e-7] first.  The two agree wherever no probability
leaves that range.
"""
import io

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Categorical

from . import _lib
from ._lib import call, ptr, stream_ptr
from .optim import ClipAdam
from .solver import Algorithm

VF_COEF, ENT_COEF = 0.5, 0.01  # ppo_solver.py:89-90
PARAM_KEYS = ["0.weight", "0.bias", "2.weight", "2.bias", "4.weight", "4.bias"]


class ActorNetwork(nn.Module):
    """ppo_model.py:6-22"""

    def __init__(self, input_shape, output_shape, n_latent_var):
        super().__init__()
        self.action_layer = nn.Sequential(
            nn.Linear(input_shape[0], n_latent_var), nn.Tanh(), nn.Linear(n_latent_var, n_latent_var), nn.Tanh(),
            nn.Linear(n_latent_var, output_shape), nn.Softmax(dim=-1))

    def forward(self, x):
        return self.action_layer(x)

    def _seq(self):
        return self.action_layer


class ValueNetwork(nn.Module):
    """ppo_model.py:25-40"""

    def __init__(self, input_shape, output_shape, n_latent_var):
        super().__init__()
        self.value_layer = nn.Sequential(
            nn.Linear(input_shape[0], n_latent_var), nn.Tanh(), nn.Linear(n_latent_var, n_latent_var), nn.Tanh(),
            nn.Linear(n_latent_var, output_shape))

    def forward(self, x):
        return self.value_layer(x)

    def _seq(self):
        return self.value_layer


def _params6(net):
    seq = net._seq()
    return [seq[0].weight, seq[0].bias, seq[2].weight, seq[2].bias, seq[4].weight, seq[4].bias]


def _dims(net):
    """(D, H1, H2, outputs)"""
    seq = net._seq()
    return seq[0].in_features, seq[0].out_features, seq[2].out_features, seq[4].out_features


def generate_discrite_ppo_model(observation_space, action_space, hidden_size=64, learning_rate=0.01):
    """ppo_model.py:43-68: the value network, its Adam, the actor, its Adam -- in that order"""
    assert hasattr(action_space, "n"), "PPO is built for Discrete action spaces"
    obs_shape = tuple(observation_space.shape)
    value_network = ValueNetwork(obs_shape, 1, hidden_size)
    value_optimizer = torch.optim.Adam(value_network.parameters(), lr=learning_rate)
    actor_network = ActorNetwork(obs_shape, int(action_space.n), hidden_size)
    actor_optimizer = torch.optim.Adam(actor_network.parameters(), lr=learning_rate)
    return {"value_network": value_network, "value_optimizer": value_optimizer, "actor_network": actor_network,
            "actor_optimizer": actor_optimizer}


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _normalise(discounted_r):
    discounted_r -= discounted_r.mean()
    discounted_r /= discounted_r.std() + 1e-7  # the population std
    return discounted_r


def calculate_discount_rewards_with_dones(r, done, gamma=0.99):
    """util.py:27-40: a row with `done` gets 0 and leaves the running sum as it is (it is not
    reset); the result is normalised by its mean and its population std + 1e-7"""
    r, done = _np(r), _np(done)
    discounted_r = np.zeros_like(r, dtype=np.float32)
    running_add = 0
    for t in reversed(range(len(r))):
        if done[t]:
            discounted_r[t] = 0
        else:
            running_add = running_add * gamma + r[t]
            discounted_r[t] = running_add
    return _normalise(discounted_r)


def calculate_discount_rewards(r, gamma=0.99):
    """util.py:43-53"""
    r = _np(r)
    discounted_r = np.zeros_like(r, dtype=np.float32)
    running_add = 0
    for t in reversed(range(len(r))):
        running_add = running_add * gamma + r[t]
        discounted_r[t] = running_add
    return _normalise(discounted_r)


# ---------------------------------------------------------------------- shuffled minibatches
# The host restatement of rth_ppo_shuffle's permutation (csrc/ppo_shuffle.hpp), in numpy alone.
STREAM_PPO_SHUFFLE = 14  # the shuffle keys' Philox stream word
MAX_MINIBATCHES, MAX_SHUFFLE_ROWS = 64, 65536  # rth_ppo_shuffle's limits on K and B
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (csrc/common.hpp) on arrays of counter words, broadcast against each other;
    the four output words as uint32 arrays.  The 32-bit words live in uint64 lanes, where a
    32 x 32 product is exact."""
    u = lambda v: np.asarray(v, dtype=np.uint64) & _U32
    c0, c1, c2, c3 = np.broadcast_arrays(u(c0), u(c1), u(c2), u(c3))
    k0, k1 = u(k0), u(k1)
    for rnd in range(10):
        if rnd:
            k0, k1 = (k0 + np.uint64(0x9E3779B9)) & _U32, (k1 + np.uint64(0xBB67AE85)) & _U32
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def shuffle_keys(seed, counter, n):
    """the n sort keys of shuffle number `counter` under `seed`: uint64 [n], all 64 bits of
    c[0] | c[1] << 32 of the block {lane i, counter lo, counter hi, 14} under the key (seed lo, seed hi)"""
    seed, counter = int(seed) & (2 ** 64 - 1), int(counter) & (2 ** 64 - 1)
    lanes = np.arange(int(n), dtype=np.uint64)
    c = philox4x32(lanes, counter & 0xFFFFFFFF, counter >> 32, STREAM_PPO_SHUFFLE, seed & 0xFFFFFFFF, seed >> 32)
    return c[0].astype(np.uint64) | (c[1].astype(np.uint64) << np.uint64(32))


def minibatch_perm(seed, counter, n, K, keys=None):
    """(perm int64 [n], sizes int64 [K]) of one shuffled pass over n rows in K minibatches: perm is
    the stable argsort of the keys (shuffle_keys, or `keys`' first n), minibatch m is the rows
    perm[m * M : m * M + sizes[m]] with M = ceil(n / K) and sizes[m] = clamp(n - m * M, 0, M)"""
    n, K = int(n), int(K)
    keys = shuffle_keys(seed, counter, n) if keys is None else np.asarray(keys, dtype=np.uint64)[:n]
    perm = np.argsort(keys, kind="stable").astype(np.int64)
    M = -(-n // K)
    sizes = np.clip(n - np.arange(K, dtype=np.int64) * M, 0, M)
    return perm, sizes


class PPOSolver(Algorithm):
    """ppo_solver.py:15-125 with its constructor arguments, plus impl (module docstring) and
    n_minibatches.  update_device's |loss| on the HIP path is a persistent buffer per batch size,
    overwritten by the next call of that size (a captured update replays into it).

    n_minibatches = K > 1: each of the k_epochs passes draws a new random order of the batch's rows
    (minibatch_perm of the solver's seed and shuffle_calls, which counts the passes) and takes one
    optimiser step on each of K minibatches of M = ceil(n / K) rows, in increasing order; the last may
    be shorter.  On the HIP path a pass is one rth_ppo_shuffle, which draws the order on the device and
    lays the batch out as K slices of pitch Mcap = ceil(B / K), then per slice the gradient call
    (rth_ppo_grads_adv / rth_ppo_grads_n with the slice's device row count) and the two Adam steps:
    k_epochs (1 + 3 K) ABI calls.  A slice without rows (n < K (K - 1) + 1 can leave some) is an Adam
    step on zero gradients there; the torch path refuses it.  K = 1 is the full-batch epoch, without
    a shuffle."""

    def __init__(self, observation_space, action_space, models=None, k_epochs=4, eps_clip=0.2, learning_rate=0.01,
                 hidden_size=64, device=None, impl=None, n_minibatches=1):
        if impl not in (None, "hip", "torch"):
            raise ValueError(f"PPOSolver: impl={impl!r} (None, 'hip' or 'torch')")
        if not 1 <= int(n_minibatches) <= MAX_MINIBATCHES:
            raise ValueError(f"PPOSolver: n_minibatches={n_minibatches} (1..{MAX_MINIBATCHES})")
        self.n_minibatches = int(n_minibatches)
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        dev = torch.device(device)
        if dev.type == "cuda":
            if not torch.cuda.is_available():
                raise RuntimeError("no HIP device visible")
            dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.device = dev
        if models is None:
            models = generate_discrite_ppo_model(observation_space, action_space, hidden_size=hidden_size,
                                                 learning_rate=learning_rate)
        for k in ("actor_network", "value_network", "actor_optimizer", "value_optimizer"):
            assert models[k] is not None, k
        self.actor_network, self.value_network = models["actor_network"].to(dev), models["value_network"].to(dev)
        self.actor_optimizer, self.value_optimizer = models["actor_optimizer"], models["value_optimizer"]
        assert hasattr(action_space, "n"), "PPO is built for Discrete action spaces"
        self.k_epochs, self.eps_clip = int(k_epochs), eps_clip
        self.impl = impl
        self.hip_launches = 0  # ABI calls of the HIP path (tests: no silent fallback)
        why = self._hip_unsupported()
        if impl == "hip" and why:
            raise ValueError(f"PPOSolver(impl='hip'): {why}")
        self.impl_active = "torch" if impl == "torch" or why else "hip"
        self.shuffle_calls = 0  # shuffled passes so far: the shuffle's Philox counter (the HIP path's device copy: _shuffle_counter)
        self.last_perm = None   # the last pass's order (HIP: device int32 [B], the first n entries; torch: int64 [n])
        if self.impl_active == "torch" and self.n_minibatches > 1:
            self.seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if self.impl_active == "hip":
            D, H, _, A = _dims(self.actor_network)
            self.dims = (D, H, A)
            lr = lambda opt: opt.param_groups[0]["lr"]
            self.actor_optimizer = ClipAdam(self.actor_network.parameters(), lr=lr(self.actor_optimizer),
                                            max_norm=None)
            self.value_optimizer = ClipAdam(self.value_network.parameters(), lr=lr(self.value_optimizer),
                                            max_norm=None)
            # persistent gradient buffers (fixed addresses: a captured update replays)
            self._grads = {}
            for net in (self.actor_network, self.value_network):
                self._grads[net] = [torch.zeros_like(p) for p in _params6(net)]
                for p, g in zip(_params6(net), self._grads[net]):
                    p.grad = g
            self._per_batch = {}
            self._per_shuffle = {}
            self._shuffle_counter = torch.zeros(1, dtype=torch.int64, device=dev)  # shuffle_calls, on the device
            self._arrays()
            # the Categorical draws: Philox of (seed, calls so far, row)
            self.seed = int(torch.randint(0, 2 ** 62, (1,)).item())
            self.act_calls = 0

    # ------------------------------------------------------------------ HIP plumbing
    def _hip_unsupported(self):
        """why the HIP kernels do not apply to this solver (None: they do)"""
        if self.device.type != "cuda":
            return f"device {self.device} is not a GPU"
        a, v = self.actor_network, self.value_network
        if not (type(a) is ActorNetwork and type(v) is ValueNetwork):
            return "the models are not reth_amd.ppo.ActorNetwork / ValueNetwork"
        for n in (a, v):
            for p in _params6(n):
                if p.dtype != torch.float32 or not p.is_contiguous():
                    return "parameters must be contiguous float32"
        (D, H1, H2, A), dv = _dims(a), _dims(v)
        if not (H1 == H2 and dv == (D, H1, H1, 1) and _lib.lib().rth_ppo_supported(D, H1, A)):
            return (f"shapes (D, H, H, outputs) = {_dims(a)} / {dv} are not built (one hidden width H = 64, D in "
                    "1..64, A in 2..18)")
        return None

    def _arrays(self):
        """the ABI's host pointer arrays, rebuilt when a parameter's storage moved"""
        a, v = self.actor_network, self.value_network
        key = tuple(p.data_ptr() for n in (a, v) for p in _params6(n))
        if getattr(self, "_key", None) != key:
            mk = lambda ts: (_lib.c_vp * len(ts))(*[t.data_ptr() for t in ts])
            self._ptrs = dict(actor=mk(_params6(a)), value=mk(_params6(v)), actor_grads=mk(self._grads[a]),
                              value_grads=mk(self._grads[v]))
            self._key = key
        return self._ptrs

    def _buffers(self, B):
        """(workspace, |loss| [B], loss mean [1]) of a batch size, persistent"""
        if B not in self._per_batch:
            size = _lib.lib().rth_ppo_workspace(B, *self.dims)
            if size <= 0:
                _lib.check(-1, "rth_ppo_workspace")
            f = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)
            self._per_batch[B] = (f(size // 4), f(B), f(1))
        return self._per_batch[B]

    def _tensor(self, x, dtype):
        return (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(self.device, dtype)

    def _matrix(self, x, cols):
        """a float32 device matrix [n, cols] with unit column stride"""
        x = self._tensor(x, torch.float32).reshape(-1, cols)
        return x if x.stride(1) == 1 and x.stride(0) >= cols else x.contiguous()

    def _hip_update(self, batch, n_rows=None):
        states, actions, returns, logprobs = batch[:4]
        D, H, A = self.dims
        s = self._matrix(states, D)
        a = self._tensor(actions, torch.long).reshape(-1).contiguous()
        ret = self._tensor(returns, torch.float32).reshape(-1).contiguous()
        old = self._tensor(logprobs, torch.float32).reshape(-1).contiguous()
        B = s.shape[0]
        adv = self._tensor(batch[4], torch.float32).reshape(-1).contiguous() if len(batch) == 5 else None
        if a.numel() != B or ret.numel() != B or old.numel() != B or (adv is not None and adv.numel() != B):
            raise ValueError("batch columns disagree in length")
        if n_rows is not None and not (torch.is_tensor(n_rows) and n_rows.device == self.device
                                       and n_rows.dtype == torch.int64 and n_rows.numel() == 1):
            raise ValueError("n_rows: an int64 tensor [1] on the solver's device")
        if self.n_minibatches > 1:
            return self._hip_update_minibatches(s, a, ret, adv, old, B, n_rows)
        ws, loss_abs, loss_mean = self._buffers(B)
        fn, count = ("rth_ppo_grads", ()) if n_rows is None else ("rth_ppo_grads_n", (ptr(n_rows),))
        given = ()
        if adv is not None:  # the advantage as given, with or without a device row count
            fn, given, count = "rth_ppo_grads_adv", (ptr(adv),), (ptr(n_rows),)
        for _ in range(self.k_epochs):
            p = self._arrays()
            call(fn, p["actor"], p["value"], ptr(s), s.stride(0), ptr(a), ptr(ret), *given, ptr(old), B, D, H, A,
                 float(self.eps_clip), VF_COEF, ENT_COEF, p["actor_grads"], p["value_grads"], ptr(loss_abs),
                 ptr(loss_mean), ptr(ws), *count, stream_ptr())
            self.actor_optimizer.step()
            self.value_optimizer.step()
            self.hip_launches += 3
        self.last_loss = loss_mean.view(())
        return loss_abs

    def _shuffle_buffers(self, B):
        """the minibatch copy of a batch of capacity B (K slices of pitch Mcap), its row counts, the
        permutation, |loss| in that layout and the shuffle's workspace: persistent, so a captured
        update replays"""
        if B not in self._per_shuffle:
            K, D = self.n_minibatches, self.dims[0]
            if K > B or B > MAX_SHUFFLE_ROWS:
                raise ValueError(f"PPOSolver: n_minibatches={K} needs a batch capacity in {K}..{MAX_SHUFFLE_ROWS}, "
                                 f"got {B}")
            size = _lib.lib().rth_ppo_shuffle_workspace(B)
            if size <= 0:
                _lib.check(-1, "rth_ppo_shuffle_workspace")
            Mcap = -(-B // K)
            z = lambda shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=self.device)
            m = dict(Mcap=Mcap, s=z((K * Mcap, D)), a=z(K * Mcap, torch.int64), ret=z(K * Mcap), adv=z(K * Mcap),
                     logp=z(K * Mcap), n=z(K, torch.int64), perm=z(B, torch.int32), loss_abs=z(K * Mcap),
                     ws=z(size // 8, torch.int64))
            self._per_shuffle[B] = m
        return self._per_shuffle[B]

    def _hip_update_minibatches(self, s, a, ret, adv, old, B, n_rows):
        D, H, A = self.dims
        K = self.n_minibatches
        mb = self._shuffle_buffers(B)
        Mcap = mb["Mcap"]
        ws, _, loss_mean = self._buffers(Mcap)
        fn = "rth_ppo_grads_n" if adv is None else "rth_ppo_grads_adv"
        for _ in range(self.k_epochs):
            call("rth_ppo_shuffle", ptr(s), s.stride(0), ptr(a), ptr(ret), ptr(adv), ptr(old), B, ptr(n_rows), D, K,
                 self.seed, ptr(self._shuffle_counter), None, ptr(mb["s"]), ptr(mb["a"]), ptr(mb["ret"]),
                 None if adv is None else ptr(mb["adv"]), ptr(mb["logp"]), ptr(mb["n"]), ptr(mb["perm"]), ptr(mb["ws"]),
                 stream_ptr())
            self.shuffle_calls += 1
            for m in range(K):
                r = slice(m * Mcap, (m + 1) * Mcap)
                given = () if adv is None else (ptr(mb["adv"][r]),)
                p = self._arrays()
                call(fn, p["actor"], p["value"], ptr(mb["s"][r]), D, ptr(mb["a"][r]), ptr(mb["ret"][r]), *given,
                     ptr(mb["logp"][r]), Mcap, D, H, A, float(self.eps_clip), VF_COEF, ENT_COEF, p["actor_grads"],
                     p["value_grads"], ptr(mb["loss_abs"][r]), ptr(loss_mean), ptr(ws), ptr(mb["n"][m:]), stream_ptr())
                self.actor_optimizer.step()
                self.value_optimizer.step()
            self.hip_launches += 1 + 3 * K
        self.last_perm = mb["perm"]
        self.last_loss = loss_mean.view(())
        return mb["loss_abs"]

    def _hip_act(self, states, uniforms, return_probs):
        D, H, A = self.dims
        x = self._matrix(states, D)
        n = x.shape[0]
        u = None if uniforms is None else self._tensor(uniforms, torch.float64).reshape(-1).contiguous()
        if u is not None and u.numel() != n:
            raise ValueError("one uniform per state")
        action = torch.empty(n, dtype=torch.int64, device=self.device)
        logprob = torch.empty(n, dtype=torch.float32, device=self.device)
        probs = torch.empty((n, A), dtype=torch.float32, device=self.device) if return_probs else None
        call("rth_ppo_act", self._arrays()["actor"], ptr(x), x.stride(0), n, D, H, A, ptr(u), self.seed,
             self.act_calls, ptr(action), ptr(logprob), ptr(probs), stream_ptr())
        self.act_calls += 1
        self.hip_launches += 1
        return (action, logprob, probs) if return_probs else (action, logprob)

    # ------------------------------------------------------------------ the reference's formulation
    def _evaluate_policy(self, state, action):
        dist = Categorical(self.actor_network(state))
        return dist.log_prob(action), torch.squeeze(self.value_network(state)), dist.entropy()

    def _torch_update(self, batch):
        states, actions, rewards, logprobs = batch[:4]
        given = self._tensor(batch[4], torch.float32) if len(batch) == 5 else None
        actions = self._tensor(actions, torch.long)
        states = self._tensor(states, torch.float32)
        rewards = self._tensor(rewards, torch.float32)
        logprobs = self._tensor(logprobs, torch.float32)
        if self.n_minibatches > 1:
            return self._torch_update_minibatches(states, actions, rewards, logprobs, given)
        for _ in range(self.k_epochs):
            loss = self._torch_step(states, actions, rewards, logprobs, given)
        self.last_loss = loss.detach().mean()
        return loss.detach().abs()

    def _torch_step(self, states, actions, rewards, logprobs, given):
        """one optimiser step on these rows; their loss"""
        new_logprobs, state_values, dist_entropy = self._evaluate_policy(states, actions)
        ratios = torch.exp(new_logprobs - logprobs.detach())
        advantages = rewards - state_values.detach() if given is None else given
        surr1 = ratios * advantages
        surr2 = torch.clamp(ratios, 1 - self.eps_clip, 1 + self.eps_clip) * advantages
        loss = -torch.min(surr1, surr2) + VF_COEF * F.mse_loss(state_values, rewards) - ENT_COEF * dist_entropy
        self.actor_optimizer.zero_grad()
        self.value_network.zero_grad()
        loss.mean().backward()
        self.actor_optimizer.step()
        self.value_optimizer.step()
        return loss

    def _torch_update_minibatches(self, states, actions, rewards, logprobs, given):
        """the HIP path's schedule on the reference's formulation: per pass minibatch_perm's order
        and one step per minibatch; |loss| in the HIP path's layout [K * Mcap] (Mcap = M here: the
        rows are the capacity), NaN where a slice has no row"""
        K, n = self.n_minibatches, states.shape[0]
        M = -(-n // K)
        for _ in range(self.k_epochs):
            perm, sizes = minibatch_perm(self.seed, self.shuffle_calls, n, K)
            self.shuffle_calls += 1
            if int(sizes.min()) == 0:
                raise ValueError(f"PPOSolver(impl='torch'): {n} rows in {K} minibatches of {M} leave a minibatch empty")
            out = torch.full((K * M,), float("nan"), device=self.device)
            for m in range(K):
                rows = torch.as_tensor(perm[m * M:m * M + int(sizes[m])], device=self.device)
                loss = self._torch_step(states[rows], actions[rows], rewards[rows], logprobs[rows],
                                        None if given is None else given[rows])
                out[m * M:m * M + len(rows)] = loss.detach().abs()
        self.last_perm = torch.as_tensor(perm, device=self.device)
        self.last_loss = loss.detach().mean()
        return out

    # ------------------------------------------------------------------ public
    def update_device(self, batch, weights=None, n_rows=None):
        """ppo_solver.py:63-100 on batch = (states, actions, returns, old log-probabilities): k_epochs
        full-batch epochs; the last epoch's |loss| [B] on the device, no host synchronisation
        (weights is accepted and ignored, as in the reference).  n_rows (a device int64 [1]): the
        batch is the first min(n_rows, B) rows of the columns, counted on the device
        (rth_ppo_grads_n; buffers are kept per capacity B, and |loss| beyond the count is stale).
        The torch path reads n_rows on the host and slices: the yardstick only.  A fifth column,
        the advantages, is taken as given where the reference forms returns - values (GAE:
        ppo_actors.finish_gae); the value loss still uses the returns (rth_ppo_grads_adv).

        n_minibatches = K > 1 (the class docstring): the result is the last pass's |loss| in minibatch
        layout [K * Mcap], Mcap = ceil(B / K): row m * Mcap + j is batch row last_perm[m * M + j] with
        M = ceil(n / K), and rows beyond a minibatch's count are stale.  solver.last_perm is that
        pass's permutation (on the device, its first n entries), last_loss the last minibatch's mean,
        and shuffle_calls has advanced by k_epochs."""
        if len(batch) not in (4, 5):
            raise ValueError("batch: (states, actions, returns, old log-probabilities[, advantages])")
        if self.impl_active == "hip":
            return self._hip_update(batch, n_rows)
        if n_rows is not None:
            n = int(n_rows)
            batch = [b[:n] for b in batch]
        return self._torch_update(batch)

    def update(self, batch, weights=None):
        return self.update_device(batch, weights).cpu()

    @torch.no_grad()
    def act_batch(self, states, uniforms=None, return_probs=False):
        """one Categorical draw per state: (actions int64 [n], log-probabilities float32 [n]) on the
        device, no host synchronisation; return_probs adds the probabilities [n, A].  uniforms
        (float64 in [0, 1), one per state) replace the generator's draws: inverse CDF over the
        running fp32 sum of the probabilities."""
        if self.impl_active == "hip":
            return self._hip_act(states, uniforms, return_probs)
        D = _dims(self.actor_network)[0]
        probs = self.actor_network(self._tensor(states, torch.float32).reshape(-1, D))
        if uniforms is None:
            action = Categorical(probs).sample()
        else:
            u = self._tensor(uniforms, torch.float64).reshape(-1, 1)
            action = (probs.cumsum(1).double() <= u).sum(1).clamp(max=probs.shape[1] - 1)
        logprob = Categorical(probs).log_prob(action)
        return (action, logprob, probs) if return_probs else (action, logprob)

    def act(self, state):
        """ppo_solver.py:102-109: (action, its log-probability) of one state as python numbers"""
        if self.impl_active == "hip":
            action, logprob = self.act_batch(state)
            return int(action[0]), float(logprob[0])
        state = self._tensor(state, torch.float32).unsqueeze(0)
        dist = Categorical(self.actor_network(state))
        action = dist.sample()
        return action.item(), dist.log_prob(action).item()

    @torch.no_grad()
    def sync_weights(self, src_ppo):
        """ppo_solver.py:111-114: both networks from another PPOSolver, in place"""
        assert isinstance(src_ppo, PPOSolver)
        for dst, src in ((self.actor_network, src_ppo.actor_network), (self.value_network, src_ppo.value_network)):
            dst.load_state_dict(src.state_dict())

    def load_weights(self, stream):
        states = torch.load(stream, map_location=self.device, weights_only=True)
        self.actor_network.load_state_dict(states)

    def save_weights(self, stream=None):
        if stream is None:
            stream = io.BytesIO()
        torch.save(self.actor_network.state_dict(), stream)
        return stream
