"""Bootstrapping GAE through time-limit ends, the parts that need no GPU: ppo_actors.gae with
truncation flags (the numpy restatement of rth_ppo_gae_finish_tl's scan, csrc/ppo_actor.hpp) against
gae without them -- the splitting identity, exact bits -- and at its edges, HostRollout's two further
columns and its row order, PpoLoopConfig's default and refusal, and the input check of the GPU step
test: its CartPole tables hold rows of every kind."""
import numpy as np
import pytest

from _ppo_timelimit import KINDS, LIMITS, SIZES, first_episode_kinds, step_table
from reth_amd.ppo_actors import HostRollout, gae


def _rows(T, seed, p_done=0.15):
    rng = np.random.default_rng(seed)
    r, v, v_term = (rng.standard_normal(T).astype(np.float32) for _ in range(3))
    done = (rng.random(T) < p_done).astype(np.float32)
    return r, done, v, np.float32(rng.standard_normal()), v_term


def _same(a, b):
    return all(x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------- the scan
@pytest.mark.parametrize("gamma", [0.0, 0.99, 1.0])
@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("T", [1, 2, 33, 200])
def test_a_truncated_row_splits_the_scan(T, gamma, lam):
    """one truncated row at t (every position for small T, a spread for T = 200): rows [0..t] equal
    gae without flags on those rows with done[t] = 0 and v_last = v_term[t]; the rows behind t equal
    gae on them alone.  Bit for bit, in fp32 and before the final rounding."""
    r, done, v, v_last, v_term = _rows(T, 10 * T)
    for t in (range(T) if T <= 33 else (0, 1, 57, 198, 199)):
        trunc = np.zeros(T, np.float32)
        trunc[t], dn = 1.0, done.copy()
        dn[t] = 1.0  # the step stores done = 1 on a truncated row
        for dtype in (np.float32, np.float64):
            adv, ret = gae(r, dn, v, v_last, gamma, lam, dtype, trunc=trunc, v_term=v_term)
            cut = dn[:t + 1].copy()
            cut[t] = 0.0
            head = gae(r[:t + 1], cut, v[:t + 1], v_term[t], gamma, lam, dtype)
            tail = gae(r[t + 1:], dn[t + 1:], v[t + 1:], v_last, gamma, lam, dtype)
            assert adv.dtype == ret.dtype == dtype and adv.shape == (T,)
            assert _same((adv[:t + 1], ret[:t + 1]), head), (t, dtype)
            assert _same((adv[t + 1:], ret[t + 1:]), tail), (t, dtype)


@pytest.mark.parametrize("T", [1, 2, 33, 200])
def test_no_truncated_row_is_the_scan_without_flags(T):
    """trunc all zero: gae without the argument, bit for bit, whatever v_term holds (NaN here)"""
    r, done, v, v_last, _ = _rows(T, T)
    for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.0, 0.0)):
        for dtype in (np.float32, np.float64):
            want = gae(r, done, v, v_last, gamma, lam, dtype)
            got = gae(r, done, v, v_last, gamma, lam, dtype, trunc=np.zeros(T), v_term=np.full(T, np.nan))
            assert _same(got, want) and np.isfinite(got[0]).all()
    # and the positional signature of before
    assert _same(gae(r, done, v, v_last, 0.99, 0.95, np.float64), gae(r, done, v, v_last, 0.99, 0.95, dtype=np.float64))


def test_edges_of_the_selects():
    r, _, v, v_last, v_term = _rows(12, 3, p_done=0.0)
    done, trunc = np.zeros(12, np.float32), np.zeros(12, np.float32)
    done[[4, 11]], trunc[11] = 1.0, 1.0
    # a truncated last row ignores v_last ...
    a = gae(r, done, v, v_last, 0.99, 0.95, trunc=trunc, v_term=v_term)
    b = gae(r, done, v, np.float32(1e6), 0.99, 0.95, trunc=trunc, v_term=v_term)
    assert _same(a, b)
    # ... and bootstraps from v_term: delta = r + gamma v_term - v, in fp64, rounded once
    want = (np.float64(r[11]) + np.float64(0.99) * np.float64(v_term[11])) - np.float64(v[11])
    assert a[0][11] == np.float32(want) and a[1][11] == np.float32(want + np.float64(v[11]))
    # a terminal done row (trunc 0) still bootstraps nothing, whatever v_term and the next value are
    assert a[0][4] == np.float32(np.float64(r[4]) - np.float64(v[4]))
    v2, vt2 = v.copy(), v_term.copy()
    v2[5], vt2[4] = 1e6, 1e6
    c = gae(r, done, v2, v_last, 0.99, 0.95, trunc=trunc, v_term=vt2)
    assert _same((a[0][:5], a[1][:5]), (c[0][:5], c[1][:5]))
    # v_term of rows that are not truncated is not read
    vt3 = np.full(12, np.nan, np.float32)
    vt3[11] = v_term[11]
    assert _same(a, gae(r, done, v, v_last, 0.99, 0.95, trunc=trunc, v_term=vt3))
    # the lambda-chain is cut at a truncated row: rows behind it do not reach across
    trunc[4] = 1.0
    d = gae(r, done, v, v_last, 0.99, 0.95, trunc=trunc, v_term=v_term)
    r2 = r.copy()
    r2[5:] += 100.0
    e = gae(r2, done, v, v_last, 0.99, 0.95, trunc=trunc, v_term=v_term)
    assert _same((d[0][:5], d[1][:5]), (e[0][:5], e[1][:5])) and not np.array_equal(d[0][5:], e[0][5:])
    assert d[0][4] != a[0][4]  # the bootstrap moved the truncated row


# ---------------------------------------------------------------------------- HostRollout
def test_host_rollout_keeps_the_two_columns_and_the_row_order():
    """ragged fills (env 1 skips a step by being full), a truncated row per env at its own place:
    finish_gae(v_term=) is gae(trunc=, v_term=) per env, env-major then time; without v_term the
    flags are ignored; term_s rows of steps that were not truncated stay NaN"""
    N, cap, D, T = 3, 4, 2, 5
    rng = np.random.default_rng(0)
    host = HostRollout(N, cap, D)
    plain = HostRollout(N, cap, D)
    host.fill[1] = plain.fill[1] = 2  # env 1: two rows already there, so its last step is dropped
    trunc_at = {0: 1, 1: 0, 2: 3}
    for t in range(T):
        s0, term = rng.standard_normal((N, D)).astype(np.float32), rng.standard_normal((N, D)).astype(np.float32)
        a, r, lp = rng.integers(0, 2, N), rng.standard_normal(N).astype(np.float32), -rng.random(N).astype(np.float32)
        trunc = np.array([trunc_at[i] == t for i in range(N)])
        if t == 2:
            host.store(s0, a, r, trunc, lp)  # without the keywords: as before
            plain.store(s0, a, r, trunc, lp)
            continue
        host.store(s0, a, r, trunc, lp, trunc=trunc, term_s=term)
        plain.store(s0, a, r, trunc, lp)
        for i in range(N):
            f = int(host.fill[i]) - 1
            if trunc[i] and host.dropped[i] == 0:
                assert host.seg_trunc[i, f] == 1.0 and np.array_equal(host.seg_term_s[i, f], term[i])
    assert host.fill.tolist() == [4, 4, 4] and host.dropped.tolist() == [1, 3, 1]
    assert host.seg_trunc.tolist() == [[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]
    assert np.isnan(host.seg_term_s[host.seg_trunc == 0]).all() and np.isfinite(host.seg_term_s[host.seg_trunc == 1]).all()
    for k in ("seg_s", "seg_a", "seg_r", "seg_done", "seg_logp", "fill", "complete", "dropped"):
        assert np.array_equal(getattr(host, k), getattr(plain, k)), k
    v, v_term = (rng.standard_normal((N, cap)).astype(np.float32) for _ in range(2))
    v_last = rng.standard_normal(N).astype(np.float32)
    seg = {k: getattr(host, k).copy() for k in ("seg_r", "seg_done", "seg_trunc", "seg_a")}
    s, a, ret, lp, adv, n = host.finish_gae(v, v_last, 0.99, 0.95, v_term=v_term)
    assert n == 12 and (host.fill == 0).all()
    for i in range(N):
        want = gae(seg["seg_r"][i], seg["seg_done"][i], v[i], v_last[i], 0.99, 0.95, trunc=seg["seg_trunc"][i],
                   v_term=v_term[i])
        assert _same((adv[4 * i:4 * i + 4], ret[4 * i:4 * i + 4]), want), i
        assert np.array_equal(a[4 * i:4 * i + 4], seg["seg_a"][i])
    ps, pa, pret, plp, padv, pn = plain.finish_gae(v, v_last, 0.99, 0.95)
    assert pn == 12 and np.array_equal(ps, s) and np.array_equal(pa, a) and np.array_equal(plp, lp)
    assert not np.array_equal(padv, adv)
    for i in range(N):
        assert _same((padv[4 * i:4 * i + 4], pret[4 * i:4 * i + 4]), gae(seg["seg_r"][i], seg["seg_done"][i], v[i], v_last[i],
                                                                       0.99, 0.95))


# ---------------------------------------------------------------------------- the config
def test_config_default_and_refusal():
    from reth_amd.ppo_loop import PpoLoop, PpoLoopConfig

    assert PpoLoopConfig().bootstrap_time_limit is False
    assert PpoLoopConfig(gae_lambda=0.95, bootstrap_time_limit=True).bootstrap_time_limit is True
    # refused before anything touches a device
    with pytest.raises(ValueError, match="bootstrap_time_limit.*set gae_lambda"):
        PpoLoop(PpoLoopConfig(bootstrap_time_limit=True), device="cpu")
    with pytest.raises(ValueError, match="the device envs are"):
        PpoLoop(PpoLoopConfig(env="Pendulum-v0", gae_lambda=0.95, bootstrap_time_limit=True), device="cpu")


# ---------------------------------------------------------------------------- the GPU step test's inputs
def test_the_step_tables_hold_rows_of_every_kind():
    """the CartPole tables of test_ppo_timelimit_gpu's step test, stepped on the host: every table has
    a both-causes row (env 0 falls on exactly the limit's step) and, from N = 9 on, time-limit-only
    rows; every table with a limit above 1 has rows that are not done and, from N = 9 on,
    terminal-only rows.  So no kind is compared on an empty set."""
    total = dict.fromkeys(KINDS, 0)
    for limit in LIMITS:
        for n in SIZES:
            st, actions = step_table("CartPole-v0", n, limit)
            assert st.shape == (n, 4) and actions.shape == (limit + 3, n) and (actions[:, 0] == 1).all()
            kinds = first_episode_kinds("CartPole-v0", st, actions, limit)
            assert kinds["both"] >= 1, (limit, n, kinds)
            assert kinds["time limit only"] >= (n - 3 if n >= 9 else 0), (limit, n, kinds)
            if limit > 1:
                assert kinds["not done"] >= limit - 1 and kinds["terminal only"] >= (2 if n >= 9 else 0), (limit, n, kinds)
            for k in KINDS:
                total[k] += kinds[k]
    assert all(total[k] >= 6 for k in KINDS), total
    for env in ("Acrobot-v1", "MountainCar-v0"):  # the other envs: terminal-only and time-limit-only rows
        st, actions = step_table(env, 9, 5)
        kinds = first_episode_kinds(env, st, actions, 5)
        assert kinds["terminal only"] >= 2 and kinds["time limit only"] >= 6 and kinds["not done"] >= 20, (env, kinds)
