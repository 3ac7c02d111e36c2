"""DDPG on MI355X: reth.algorithm.DDPGSolver's interface on fused HIP actor-critic kernels.

Reference: reth/reth/algorithm/ddpg/ddpg_solver.py:11-130, ddpg_model.py:64-162 and
algorithm/util.py:15-24 (soft_update).  The actor (fc1 D->400, fc2 400->300, fc3 300->Ad; ReLU,
ReLU, tanh) and the critic (fc1 D->400, fc2 400+Ad->300 on cat(relu(fc1(s)), a), fc3 300->1) keep
the reference's parameter names, construction order and RNG draws, so under one torch.manual_seed
the four networks are the reference's element for element.

impl="torch" is the reference's formulation (nn.Linear, autograd, two torch.optim.Adam) on the
solver's device: the yardstick.  impl="hip" runs the update on csrc/ddpg.hpp: one
rth_ddpg_critic_grads call (both target forwards, the critic forward, td, the loss, the critic's
six gradients), Adam (ClipAdam without a clip), one rth_ddpg_actor_grads call on the updated
critic, Adam, and one rth_soft_update launch over the twelve target tensors; act / act_batch are
one rth_ddpg_act launch.  impl=None takes "hip" where it applies (a GPU, fp32, a shape
rth_ddpg_supported builds) and "torch" elsewhere; asked for explicitly, "hip" raises instead.
solver.impl_active names the path that runs and solver.hip_launches counts its ABI calls.

The reference casts the batch's actions to torch.long before the critic sees them
(ddpg_solver.py:72), which truncates continuous actions toward zero.  That is the default here
too (cast_actions_to_long=True); False feeds the critic the actions as stored.
"""
import io

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from ._lib import call, ptr, stream_ptr
from .optim import ClipAdam
from .solver import Algorithm, Box

H1, H2 = 400, 300
PARAM_NAMES = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias"]


def fanin_init(size, fanin=None):
    """ddpg_model.py:64-73: uniform in +-1/sqrt(size[0]) -- the OUTPUT width of a Linear weight;
    the quirk is part of the definition"""
    v = 1.0 / np.sqrt(fanin or size[0])
    return torch.empty(size).uniform_(-v, v)


class _Net(nn.Module):
    def _build(self, d_in, d_mid, d_out, h1, h2, eps):
        # the reference's order of construction and of RNG draws: each Linear's default init,
        # then its weight redrawn
        self.fc1 = nn.Linear(d_in, h1)
        self.fc1.weight.data = fanin_init(self.fc1.weight.data.size())
        self.fc2 = nn.Linear(d_mid, h2)
        self.fc2.weight.data = fanin_init(self.fc2.weight.data.size())
        self.fc3 = nn.Linear(h2, d_out)
        self.fc3.weight.data.uniform_(-eps, eps)

    def _params6(self):
        return [self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias, self.fc3.weight, self.fc3.bias]

    def dims(self):
        """(D, Ad, H1, H2)"""
        return self.fc1.in_features, self.action_dim, self.fc1.out_features, self.fc2.out_features


class Actor(_Net):
    """ddpg_model.py:76-97"""

    def __init__(self, obs_shape, action_shape, eps=0.03, h1=H1, h2=H2):
        super().__init__()
        self.action_dim = int(action_shape[0])
        self._build(obs_shape[0], h1, self.action_dim, h1, h2, eps)

    def forward(self, state):
        x = torch.relu(self.fc1(state))
        x = torch.relu(self.fc2(x))
        return torch.tanh(self.fc3(x))


class Critic(_Net):
    """ddpg_model.py:100-122"""

    def __init__(self, obs_shape, action_shape, eps=0.03, h1=H1, h2=H2):
        super().__init__()
        self.action_dim = int(action_shape[0])
        self._build(obs_shape[0], h1 + self.action_dim, 1, h1, h2, eps)

    def forward(self, state, action):
        x = torch.cat((torch.relu(self.fc1(state)), action), dim=1)
        x = torch.relu(self.fc2(x))
        return self.fc3(x)


def generate_ddpg_model(observation_space, action_space, learning_rate_actor, learning_rate_critic, is_image=None,
                        h1=H1, h2=H2):
    """ddpg_model.py:125-162: actor, actor_target, critic, critic_target in that order, then the
    two Adam optimizers"""
    action_shape, obs_shape = tuple(action_space.shape), tuple(observation_space.shape)
    if is_image is None:
        is_image = len(obs_shape) == 3
    if is_image:
        raise NotImplementedError("DDPG on image observations (ConvActor / ConvCritic) is not rebuilt")
    actor, actor_target = Actor(obs_shape, action_shape, h1=h1, h2=h2), Actor(obs_shape, action_shape, h1=h1, h2=h2)
    critic, critic_target = (Critic(obs_shape, action_shape, h1=h1, h2=h2),
                             Critic(obs_shape, action_shape, h1=h1, h2=h2))
    return {"actor": actor, "actor_target": actor_target,
            "actor_optimizer": torch.optim.Adam(actor.parameters(), learning_rate_actor),
            "critic": critic, "critic_target": critic_target,
            "critic_optimizer": torch.optim.Adam(critic.parameters(), learning_rate_critic)}


def soft_update(target, source, tau=0.001):
    """util.py:15-24"""
    for tp, p in zip(target.parameters(), source.parameters()):
        tp.data.copy_(tp.data * (1.0 - tau) + p.data * tau)


class DDPGSolver(Algorithm):
    """ddpg_solver.py:11-130 with its constructor arguments, plus cast_actions_to_long and impl
    (module docstring).  update_device's |td| on the HIP path is a persistent buffer per batch
    size, overwritten by the next call of that size (a captured update replays into it)."""

    def __init__(self, observation_space, action_space, models=None, gamma=0.99, tau=0.001, learning_rate=None,
                 learning_rate_actor=0.0001, learning_rate_critic=0.001, is_image=None, device=None,
                 cast_actions_to_long=True, impl=None):
        if impl not in (None, "hip", "torch"):
            raise ValueError(f"DDPGSolver: impl={impl!r} (None, 'hip' or 'torch')")
        if device is None:
            device = "cuda" if torch.cuda.is_available() else "cpu"
        dev = torch.device(device)
        if dev.type == "cuda":
            if not torch.cuda.is_available():
                raise RuntimeError("no HIP device visible")
            dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
        self.device = dev
        if is_image or (is_image is None and len(tuple(observation_space.shape)) == 3):
            raise NotImplementedError("DDPG on image observations (ConvActor / ConvCritic) is not rebuilt")
        if learning_rate_actor is None:
            learning_rate_actor = learning_rate
        if learning_rate_critic is None:
            learning_rate_critic = learning_rate
        if models is None:
            models = generate_ddpg_model(observation_space, action_space, learning_rate_actor, learning_rate_critic,
                                         is_image)
        for k in ("actor", "actor_target", "actor_optimizer", "critic", "critic_target", "critic_optimizer"):
            assert models[k] is not None, k
        self.actor, self.actor_target = models["actor"].to(dev), models["actor_target"].to(dev)
        self.critic, self.critic_target = models["critic"].to(dev), models["critic_target"].to(dev)
        self.actor_optimizer, self.critic_optimizer = models["actor_optimizer"], models["critic_optimizer"]
        self.actor_target.requires_grad_(False)
        self.critic_target.requires_grad_(False)
        assert isinstance(action_space, Box) or hasattr(action_space, "shape")
        self.action_space = action_space
        self.action_dim = int(tuple(action_space.shape)[0])
        self.gamma, self.tau = gamma, tau
        self.cast_actions_to_long = bool(cast_actions_to_long)
        self.impl = impl
        self.hip_launches = 0  # ABI calls of the HIP path (tests: no silent fallback)
        why = self._hip_unsupported()
        if impl == "hip" and why:
            raise ValueError(f"DDPGSolver(impl='hip'): {why}")
        self.impl_active = "torch" if impl == "torch" or why else "hip"
        if self.impl_active == "hip":
            self.dims = self.actor.dims()
            lr = lambda opt: opt.param_groups[0]["lr"]
            self.actor_optimizer = ClipAdam(self.actor.parameters(), lr=lr(self.actor_optimizer), max_norm=None)
            self.critic_optimizer = ClipAdam(self.critic.parameters(), lr=lr(self.critic_optimizer), max_norm=None)
            # persistent gradient buffers (fixed addresses: a captured update replays)
            self._grads = {}
            for net in (self.actor, self.critic):
                self._grads[net] = [torch.zeros_like(p) for p in net._params6()]
                for p, g in zip(net._params6(), self._grads[net]):
                    p.grad = g
            self._per_batch = {}
            self._arrays()
        self.update_target()

    # ------------------------------------------------------------------ HIP plumbing
    def _nets(self):
        return self.actor, self.critic, self.actor_target, self.critic_target

    def _hip_unsupported(self):
        """why the HIP kernels do not apply to this solver (None: they do)"""
        if self.device.type != "cuda":
            return f"device {self.device} is not a GPU"
        a, c, at, ct = self._nets()
        if not (type(a) is Actor and type(at) is Actor and type(c) is Critic and type(ct) is Critic):
            return "the models are not reth_amd.ddpg.Actor / Critic"
        if not (a.dims() == c.dims() == at.dims() == ct.dims()):
            return f"the four networks disagree in shape: {[n.dims() for n in self._nets()]}"
        for n in self._nets():
            for p in n._params6():
                if p.dtype != torch.float32 or not p.is_contiguous():
                    return "parameters must be contiguous float32"
        if not _lib.lib().rth_ddpg_supported(*a.dims()):
            return (f"shape (D, Ad, H1, H2) = {a.dims()} is not built (D in 1..64, Ad in 1..8, H1 and H2 multiples "
                    "of 4 in 4..512)")
        return None

    def _arrays(self):
        """the ABI's host pointer arrays, rebuilt when a parameter's storage moved"""
        key = tuple(p.data_ptr() for n in self._nets() for p in n._params6())
        if getattr(self, "_key", None) != key:
            mk = lambda ts: (_lib.c_vp * len(ts))(*[t.data_ptr() for t in ts])
            a, c, at, ct = self._nets()
            tgt, src = at._params6() + ct._params6(), a._params6() + c._params6()
            self._ptrs = dict(actor=mk(a._params6()), critic=mk(c._params6()), actor_target=mk(at._params6()),
                              critic_target=mk(ct._params6()), actor_grads=mk(self._grads[a]),
                              critic_grads=mk(self._grads[c]), soft_target=mk(tgt), soft_source=mk(src),
                              soft_numel=(_lib.c_i64 * len(tgt))(*[t.numel() for t in tgt]), soft_n=len(tgt))
            self._key = key
        return self._ptrs

    def _buffers(self, B):
        """(workspace, |td| [B], critic loss [1], actor loss [1]) of a batch size, persistent"""
        if B not in self._per_batch:
            size = _lib.lib().rth_ddpg_workspace(B, *self.dims)
            if size <= 0:
                _lib.check(-1, "rth_ddpg_workspace")
            f = lambda n: torch.zeros(n, dtype=torch.float32, device=self.device)
            self._per_batch[B] = (f(size // 4), f(B), f(1), f(1))
        return self._per_batch[B]

    def _matrix(self, x, cols):
        """a float32 device matrix [n, cols] with unit column stride"""
        x = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(self.device, torch.float32)
        x = x.reshape(-1, cols)
        return x if x.stride(1) == 1 and x.stride(0) >= cols else x.contiguous()

    def _column(self, x):
        x = (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(self.device, torch.float32)
        return x.reshape(-1).contiguous()

    def _actions(self, a):
        a = a if torch.is_tensor(a) else torch.as_tensor(np.asarray(a))
        if self.cast_actions_to_long:  # ddpg_solver.py:72: truncation toward zero
            a = a.to(torch.long)
        return a.to(self.device)

    def _hip_critic(self, batch, weights, backward):
        s0, a, r, s1, done = batch
        D, Ad, h1, h2 = self.dims
        s0, s1, a = self._matrix(s0, D), self._matrix(s1, D), self._matrix(self._actions(a), Ad)
        r, done = self._column(r), self._column(done)
        isw = None if weights is None else self._column(weights)
        B = s0.shape[0]
        if s1.shape[0] != B or a.shape[0] != B or r.numel() != B or done.numel() != B or (
                isw is not None and isw.numel() != B):
            raise ValueError("batch columns disagree in length")
        ws, td_abs, loss_c, _ = self._buffers(B)
        p = self._arrays()
        call("rth_ddpg_critic_grads", p["critic"], p["actor_target"], p["critic_target"], ptr(s0), s0.stride(0),
             ptr(a), a.stride(0), ptr(r), ptr(done), ptr(s1), s1.stride(0), ptr(isw), B, D, Ad, h1, h2,
             float(self.gamma), p["critic_grads"] if backward else None, ptr(td_abs), ptr(loss_c), ptr(ws),
             stream_ptr())
        self.hip_launches += 1
        return s0, td_abs, loss_c

    def _hip_update(self, batch, weights):
        s0, td_abs, loss_c = self._hip_critic(batch, weights, backward=True)
        self.critic_optimizer.step()
        D, Ad, h1, h2 = self.dims
        B = s0.shape[0]
        ws, _, _, loss_a = self._buffers(B)
        p = self._arrays()
        call("rth_ddpg_actor_grads", p["actor"], p["critic"], ptr(s0), s0.stride(0), B, D, Ad, h1, h2,
             p["actor_grads"], ptr(loss_a), ptr(ws), stream_ptr())
        self.actor_optimizer.step()
        call("rth_soft_update", p["soft_target"], p["soft_source"], p["soft_numel"], p["soft_n"], float(self.tau),
             stream_ptr())
        self.hip_launches += 2
        self.last_critic_loss, self.last_actor_loss = loss_c.view(()), loss_a.view(())
        return td_abs

    def _hip_act(self, states):
        D, Ad, h1, h2 = self.dims
        x = self._matrix(states, D)
        out = torch.empty((x.shape[0], Ad), dtype=torch.float32, device=self.device)
        call("rth_ddpg_act", self._arrays()["actor"], ptr(x), x.stride(0), x.shape[0], D, Ad, h1, h2, ptr(out),
             stream_ptr())
        self.hip_launches += 1
        return out

    # ------------------------------------------------------------------ the reference's formulation
    def _torch_tensors(self, batch, weights):
        s0, a, r, s1, done = batch
        f = lambda x, dt: (x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).to(self.device, dt)
        a = self._actions(a).reshape(-1, self.action_dim)
        w = None if weights is None else f(weights, torch.float32).reshape(-1)
        return f(s0, torch.float32), a, f(r, torch.float32), f(s1, torch.float32), f(done, torch.float32), w

    def _torch_td(self, s0, a, r, s1, done):
        with torch.no_grad():
            a1 = self.actor_target(s1)
            target_q = self.critic_target(s1, a1)
            y = r[:, None] + (1 - done[:, None]) * self.gamma * target_q
        return (self.critic(s0, a) - y).squeeze(1)

    def _torch_update(self, batch, weights):
        s0, a, r, s1, done, w = self._torch_tensors(batch, weights)
        td = self._torch_td(s0, a, r, s1, done)
        td_abs = td.detach().abs()
        critic_loss = td.pow(2)
        if w is not None:
            critic_loss = critic_loss * w
        critic_loss = critic_loss.mean()
        self.critic_optimizer.zero_grad()
        critic_loss.backward()
        self.critic_optimizer.step()
        actor_loss = (-self.critic(s0, self.actor(s0))).mean()  # with the critic just updated
        self.actor_optimizer.zero_grad()
        actor_loss.backward()
        self.actor_optimizer.step()
        soft_update(self.actor_target, self.actor, self.tau)
        soft_update(self.critic_target, self.critic, self.tau)
        self.last_critic_loss, self.last_actor_loss = critic_loss.detach(), actor_loss.detach()
        return td_abs

    # ------------------------------------------------------------------ public
    @torch.no_grad()
    def update_target(self):
        """target <- online for both pairs (ddpg_solver.py:64-66), in place"""
        for t, s in ((self.actor_target, self.actor), (self.critic_target, self.critic)):
            torch._foreach_copy_(list(t.parameters()), [p.detach() for p in s.parameters()])

    def update_device(self, batch, weights=None):
        """ddpg_solver.py:68-110 returning |td| [B] on the device, no host synchronisation"""
        if self.impl_active == "hip":
            return self._hip_update(batch, weights)
        return self._torch_update(batch, weights)

    def update(self, batch, weights=None):
        return self.update_device(batch, weights).cpu()

    def calc_loss_device(self, batch):
        """|td| [B] without an update"""
        if self.impl_active == "hip":
            return self._hip_critic(batch, None, backward=False)[1]
        s0, a, r, s1, done, _ = self._torch_tensors(batch, None)
        with torch.no_grad():
            return self._torch_td(s0, a, r, s1, done).abs()

    def calc_loss(self, batch):
        return self.calc_loss_device(batch).cpu()

    @torch.no_grad()
    def act_batch(self, states):
        """the actor's actions of n states as a float32 device tensor [n, Ad], no host synchronisation"""
        if self.impl_active == "hip":
            return self._hip_act(states)
        x = (states if torch.is_tensor(states) else torch.as_tensor(np.asarray(states))).to(self.device, torch.float32)
        return self.actor(x.reshape(-1, self.actor.fc1.in_features))

    @torch.no_grad()
    def act(self, state):
        """ddpg_solver.py:112-118: the action of one state as a numpy array [Ad] (not clipped)"""
        return self.act_batch(state)[0].cpu().numpy()

    def load_weights(self, stream):
        states = torch.load(stream, map_location=self.device, weights_only=True)
        self.actor.load_state_dict(states)
        self.update_target()

    def save_weights(self, stream=None):
        if stream is None:
            stream = io.BytesIO()
        torch.save(self.actor.state_dict(), stream)
        return stream
