"""The device CartPole actors (csrc/mlp_actor.hpp), the parts that need no GPU: both entry points
check their arguments before any HIP call (so the checks run on a host without a device, as
test_mlp_cpu relies on for rth_mlp_workspace), and the Python modules import."""
import ctypes

import pytest

from reth_amd import _lib

FAKE = 0x1000  # a non-NULL "device pointer": no check dereferences it, and nothing is launched


def _args(**over):
    params = (_lib.c_vp * 6)(*[FAKE] * 6)
    kw = dict(params=params, D=4, H=128, A=2, seed=1, N=8, ring=8, max_episode_steps=200)
    for name, typ in _lib.MlpActorArgs._fields_:
        if typ is _lib.c_vp:
            kw[name] = FAKE
    kw["action_in"] = kw["q_out"] = None  # the nullable ones
    kw.update(over)
    a = _lib.MlpActorArgs(**kw)
    a._keep = params
    return a


class _FakeNStep(ctypes.Structure):
    """the leading fields of the library's rth_nstep (N, n): only read by the checks"""
    _fields_ = [("N", ctypes.c_int64), ("n", ctypes.c_int32), ("gamma", ctypes.c_double), ("mode", ctypes.c_int32),
                ("device", ctypes.c_int), ("mem", ctypes.c_void_p), ("st", ctypes.c_void_p * 6)]


def _step(args, N=8, n=1, handle=True):
    h = _FakeNStep(N, n, 0.99, 0, 0, None)
    lib = _lib.lib()
    rc = lib.rth_mlp_actor_step(ctypes.addressof(h) if handle else None, ctypes.byref(args), None)
    return rc, lib.rth_last_error()


def _reset(args):
    lib = _lib.lib()
    return lib.rth_cartpole_reset(ctypes.byref(args), None), lib.rth_last_error()


BAD_SHAPES = [dict(D=5), dict(D=3), dict(A=3), dict(A=1), dict(H=64), dict(D=0), dict(A=19)]
BAD_COMMON = [dict(N=0), dict(N=-1), dict(N=1 << 31), dict(ring=3), dict(ring=0), dict(max_episode_steps=0),
              dict(max_episode_steps=-5)]
STATE_PTRS = ["state", "ep_steps", "t_dev", "stats", "obs_ring", "cur_slot"]
STEP_PTRS = ["eps", "action", "reward", "done", "s0_h", "s1_h", "emit", "row_s0", "row_a", "row_s1", "row_r",
             "row_done", "row_obs0", "row_obs1"]


@pytest.mark.parametrize("over", BAD_SHAPES + BAD_COMMON + [{p: None} for p in STATE_PTRS])
def test_reset_rejects(over):
    rc, msg = _reset(_args(**over))
    assert rc != 0 and b"rth_cartpole_reset" in msg, (over, msg)


@pytest.mark.parametrize("over", BAD_SHAPES + BAD_COMMON + [{p: None} for p in STATE_PTRS + STEP_PTRS + ["params"]])
def test_step_rejects(over):
    rc, msg = _step(_args(**over))
    assert rc != 0 and b"rth_mlp_actor_step" in msg, (over, msg)


def test_step_rejects_adder_mismatch_and_null():
    rc, msg = _step(_args(N=8), N=9)
    assert rc != 0 and b"rth_mlp_actor_step" in msg and b"adder" in msg
    rc, msg = _step(_args(), handle=False)
    assert rc != 0 and b"rth_mlp_actor_step" in msg
    rc, msg = _step(_args(ring=8), n=3)  # an emitted row's observations would be overwritten: ring < 2 (n + 2)
    assert rc != 0 and b"rth_mlp_actor_step" in msg and b"ring" in msg
    lib = _lib.lib()
    assert lib.rth_mlp_actor_step(None, None, None) != 0 and b"rth_mlp_actor_step" in lib.rth_last_error()
    assert lib.rth_cartpole_reset(None, None) != 0 and b"rth_cartpole_reset" in lib.rth_last_error()


def test_step_rejects_null_parameter():
    params = (_lib.c_vp * 6)(*([FAKE] * 5 + [None]))
    rc, msg = _step(_args(params=params))
    assert rc != 0 and b"rth_mlp_actor_step" in msg


def test_struct_layout_matches_header():
    """26 pointers / int64 fields of 8 bytes, the seed, N and two int32: no padding surprises"""
    assert ctypes.sizeof(_lib.MlpActorArgs) == 8 * 26 + 8 + 8 + 4 + 4


def test_modules_import_without_gpu():
    from reth_amd import mlp_actors, mlp_apex

    assert mlp_actors.VecCartPoleActors and mlp_apex.MlpApexDQN
    cols = mlp_actors.VecCartPoleActors.columns()
    assert [c.shape for c in cols] == [(4,), (), (), (4,), ()]
