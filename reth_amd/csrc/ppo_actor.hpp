// Device-resident PPO actors on the fused actor of ppo.hpp: the rollout of the reference's on-policy
// loop (reth/examples/ppo/run.py with algorithm/util.py:27-40) kept in HBM.  Three entry points on
// one argument block: rth_ppo_env_reset, rth_ppo_actor_step (one launch per env step of N envs) and
// rth_ppo_rollout_finish (one launch per update: the returns of the finished episodes, the dense
// batch, its device row count and the carry of the episodes still running); rth_ppo_gae_finish is
// the finish of the other estimator, GAE(lambda), on the same segments.  The counterpart of
// env_actor.hpp for an on-policy learner; the environments, their reset draws and observation
// maps are env_actor.hpp's (env_dynamics / env_reset_draw / env_store_obs, templated on the env):
//   RTH_ENV_CARTPOLE D 4, A 2;  RTH_ENV_ACROBOT D 6, A 3;  RTH_ENV_MOUNTAINCAR D 2, A 3;  H = 64.
// No host synchronisation, no atomics, no grid-wide agreement: everything an env touches is private
// to its lane (step) or its workgroup (finish).
//
// The step.  Per tile of kPpoRows rows the acting forward and the log-softmax of ppo.hpp
// (ppo_stage_net, ppo_forward_rows, ppo_log_softmax: a row's probabilities and log-probabilities
// equal rth_ppo_act's bit for bit), then one lane per env i:
//   t    = t_dev[i] + 1                     every env carries its own copy of the step count
//   u    = uniforms_in[i] where given, else philox_uniform(seed, counter = t, lane = i, STREAM_PPO):
//          the uniform rth_ppo_act draws for (seed, counter = t, row = i)
//   a    = ppo_inverse_cdf(p_i, u), or action_in[i] where given (clamped into [0, A));
//   logp = logp_i[a], the log-probability of the action taken
//   env_dynamics<ENV> in fp64, done = terminal | steps >= max_episode_steps, and on done
//   env_reset_draw<ENV>(seed, i, t); stats / ret_stats as k_env_actor_step keeps them; cur_obs f32
//   [N, LD] (LD = D rounded up to 4 floats, pad 0) holds the observation the env acts on next.
//
// The rollout segment of env i: dense columns [N, cap, .] -- s [.., D] (the observation acted on),
// a int64, r, done, logp f32 -- with fill[i] rows stored, of which the first complete[i] belong to
// finished episodes (complete = fill after a done row is stored).  A step whose env's segment is
// full (fill == cap) stores nothing and counts the row in dropped[i]; the env still steps.
//
// complete is int32 [2, N] with a per-env generation gen[i] (every env its own copy, as t_dev):
// the live slot is gen[i] & 1.  The finish's workgroup i sums the live slot of every env k < i
// while workgroup k zeroes its count -- in the OTHER slot, then gen[k] += 1 -- so the one launch
// reads nothing another workgroup writes.
//
// The finish.  Workgroup i, with m = fill[i] and e = complete[i]; rows [0, e) are whole episodes,
// each ending at its done row.  Per episode (one lane each), backwards with run = 0 in fp64: a done
// row gets d_t = 0, another run = radd(rmul(run, gamma), (double) r_t) and d_t = (float) run; then
// over the episode's fp32 d_t in increasing t, in fp64, mean = (sum d_t) / L and var = (sum (d_t -
// mean)^2) / L, every operation rounded once, and ret_t = (float) ((d_t - mean) / (sqrt(var) +
// 1e-7)): calculate_discount_rewards_with_dones on that episode alone.  The rows (s, a, ret, logp)
// go to the dense batch at offset sum_{k<i} complete[k] in time order -- env-major, then time --
// and n_dev[0] = sum_k complete[k]; batch rows at n and beyond are left as they were.  Then rows
// [e, m) move to [0, m - e) with their old log-probabilities (chunks: read, barrier, write, in
// increasing order, after the batch copy has read the segment), fill[i] = m - e, complete[i] = 0.
//
// The GAE finish (rth_ppo_gae_finish): the other estimator on the same segments -- GAE(lambda) with a
// value bootstrap at the rollout's edge, every stored row of every env, no carry.  Workgroup i, with
// T = fill[i]: the value network staged once (ppo_stage_net), rows 0..T-1 of the segment plus, as row
// T, cur_obs[i] through ppo_forward_rows in tiles of kPpoRows -- the only forward, so v_t is what
// k_ppo_tile computes for that row with those weights, bit for bit -- and v_last = the value of
// cur_obs[i].  Then one lane, backwards over t = T-1 .. 0 in fp64 with run = 0, every operation
// rounded once:
//   nt    = 1 - done_t
//   nv    = (t == T-1) ? v_last : v_{t+1}
//   delta = (r_t + (gamma * nv) * nt) - v_t
//   run   = delta + ((gamma * lam) * nt) * run
//   adv_t = (float) run,  ret_t = (float) (run + (double) v_t)
// A done row is a terminal state (time limit or not): the step has already put the reset draw into
// the next observation, and nt = 0 keeps its value out.  The rows (s, a, ret, adv, v, logp) go to the
// dense batch at offset sum_{k<i} fill[k], env-major then time, n_dev[0] = sum_k fill[k].  Nothing
// in that launch writes fill, so every workgroup sums what the steps left; a second, small launch
// (k_ppo_gae_clear) then sets fill[i] = 0 and both complete slots of env i = 0, and gen[i] += 1.
// One launch would have workgroup k zero fill[k] while workgroup i > k may not have read it yet.
//
// Time-limit ends (rth_ppo_actor_step_tl, rth_ppo_gae_finish_tl): the same two kernels with a
// compile-time flag, on two more columns.  The step also stores, with the row, seg_trunc [N, cap] =
// (steps >= max_episode_steps && !terminal) -- both causes on one step: terminal -- and, on a
// truncated row only, seg_term_s [N, cap, D] = the observation of the post-dynamics state
// (env_store_obs before env_reset_draw); everything else is the step's, bit for bit.  The finish
// lists the truncated rows of its env in increasing t, runs the same forward over that list in
// tiles of kPpoRows (vterm_t = value(seg_term_s[t]); rows with trunc 0 are never read), and the scan
// selects its operands:
//   nt    = 1 - done_t
//   nb    = trunc_t ? 1 : nt
//   nv    = trunc_t ? vterm_t : (t == T-1 ? v_last : v_{t+1})
//   delta = (r_t + (gamma * nv) * nb) - v_t
//   run   = delta + ((gamma * lam) * nt) * run        the lambda-chain is still cut at every done row
// so a truncated row bootstraps from the value of the state its episode ended on, and trunc = 0
// everywhere is the scan above, operation for operation.
#pragma once
#include <type_traits>
#include "env_actor.hpp"
#include "ppo.hpp"

namespace rth {

constexpr int kPpoFinThreads = 256;
constexpr int kPpoMaxCap = 4096;  // the finish keeps a segment's rewards and done flags in LDS: 8 bytes a row

struct PpoActor {
  DenseNet net;
  double *state;
  int32_t *ep_steps;
  int64_t *t_dev, *stats;
  double *ret_stats;
  float *cur_obs;
  const int64_t *action_in;    // NULL: the drawn action (workgroup-uniform)
  const double *uniforms_in;   // NULL: the Philox uniform
  int64_t *action;
  float *logprob;
  float *seg_s;
  int64_t *seg_a;
  float *seg_r, *seg_done, *seg_logp;
  int32_t *fill, *complete, *gen;
  int64_t *dropped;
  uint64_t seed;
  int64_t N;
  int cap, max_steps;
};

// the argument block of the time-limit variants (rth_ppo_actor_step_tl, rth_ppo_gae_finish_tl): two more columns
struct PpoActorTl : PpoActor {
  float *seg_trunc;   // [N, cap]: 1 where the time limit alone ended the row's episode
  float *seg_term_s;  // [N, cap, D]: a truncated row's final observation; other rows are never written or read
};
template <bool TL>
using PpoActorOf = std::conditional_t<TL, PpoActorTl, PpoActor>;

__device__ __forceinline__ int ppo_clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int ENV>
__global__ __launch_bounds__(256) void k_ppo_env_reset(PpoActor a) {
  constexpr int LD = env_ld(EnvSpec<ENV>::D);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  double s[4];
  env_reset_draw<ENV>(a.seed, i, 0, s);
#pragma unroll
  for (int k = 0; k < 4; ++k) a.state[i * 4 + k] = s[k];
  a.ep_steps[i] = 0;
  a.t_dev[i] = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) a.stats[i * 3 + k] = 0, a.ret_stats[i * 3 + k] = 0.0;
  env_store_obs<ENV>(a.cur_obs + i * LD, s);
  a.fill[i] = 0;
  a.complete[i] = 0, a.complete[a.N + i] = 0;
  a.gen[i] = 0;
  a.dropped[i] = 0;
}

// TL: the step of rth_ppo_actor_step_tl -- the same code plus the row's seg_trunc and, on a truncated
// row, seg_term_s (the header's "Time-limit ends").
template <int ENV, bool TL>
__global__ __launch_bounds__(kPpoThreads) void k_ppo_actor_step(PpoActorOf<TL> a) {
  constexpr int D = EnvSpec<ENV>::D, A = EnvSpec<ENV>::A, LD = env_ld(D);
  static_assert(D <= kPpoMaxD && A >= kPpoMinA && A <= kPpoMaxA, "the env's shape is one ppo.hpp builds");
  __shared__ __align__(16) PpoActSmem s;
  const int tid = threadIdx.x;
  const int64_t N = a.N;
  ppo_stage_net(a.net, D, A, s.actor);
  const int64_t tiles = (N + kPpoRows - 1) / kPpoRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kPpoRows;
    ppo_load_tile(a.cur_obs, LD, N, r0, D, s.x);  // the acting observations, zero past N / D
    ppo_forward_rows(s.actor, s.x, D, A, s.ra);
    ppo_log_softmax(s.ra.z, A, s.dist);
    if (tid >= kPpoRows || r0 + tid >= N) continue;
    const int64_t i = r0 + tid;
    // everything the lane reads, before the stores below, which it may alias for all the
    // compiler knows: after them every load's latency would be the lane's own
    const int64_t t = a.t_dev[i] + 1;
    double st[4], run[3];
    int64_t ep[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) st[k] = a.state[i * 4 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) run[k] = a.ret_stats[i * 3 + k], ep[k] = a.stats[i * 3 + k];
    const int steps = a.ep_steps[i] + 1;
    const int f = a.fill[i], slot = a.gen[i] & 1;
    const int64_t drop = a.dropped[i];
    float o0[D];
#pragma unroll
    for (int k = 0; k < D; ++k) o0[k] = s.x[tid][k];  // the forward leaves the tile's observations in place
    const double u = a.uniforms_in ? a.uniforms_in[i] : philox_uniform(a.seed, (uint64_t)t, (uint32_t)i, STREAM_PPO);
    int act = ppo_inverse_cdf(s.dist.p[tid], A, u);
    if (a.action_in) {
      const int64_t v = a.action_in[i];
      act = v < 0 ? 0 : (v >= A ? A - 1 : (int)v);  // (an action outside [0, A) reads in bounds)
    }
    const float lp = s.dist.logp[tid][act];
    float rew;
    const bool terminal = env_dynamics<ENV>(st, act, &rew);
    const bool done = terminal | (steps >= a.max_steps);
    [[maybe_unused]] const bool trunc = !terminal & (steps >= a.max_steps);  // both causes on one step: terminal
    [[maybe_unused]] __align__(16) float term[LD];
    if constexpr (TL) {
      if (trunc) env_store_obs<ENV>(term, st);  // what the episode ended on, before the reset draw replaces it
    }
    const double ret = radd(run[0], (double)rew);
    if (done) {
      env_reset_draw<ENV>(a.seed, i, t, st);
      ep[0] += 1, ep[1] += steps, ep[2] = steps;
      run[1] = radd(run[1], ret), run[2] = ret;
    }
    run[0] = done ? 0.0 : ret;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[i * 4 + k] = st[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.ret_stats[i * 3 + k] = run[k], a.stats[i * 3 + k] = ep[k];
    a.ep_steps[i] = done ? 0 : steps;
    a.t_dev[i] = t;
    env_store_obs<ENV>(a.cur_obs + i * LD, st);  // acted on next: after a done the reset observation
    a.action[i] = act;
    a.logprob[i] = lp;
    if (f >= 0 && f < a.cap) {  // the row (s0, a, r, done, logp) into the env's segment
      const int64_t row = i * a.cap + f;
#pragma unroll
      for (int k = 0; k < D; ++k) a.seg_s[row * D + k] = o0[k];
      a.seg_a[row] = act;
      a.seg_r[row] = rew;
      a.seg_done[row] = done ? 1.0f : 0.0f;
      a.seg_logp[row] = lp;
      if constexpr (TL) {
        a.seg_trunc[row] = trunc ? 1.0f : 0.0f;
        if (trunc) {
#pragma unroll
          for (int k = 0; k < D; ++k) a.seg_term_s[row * D + k] = term[k];
        }
      }
      a.fill[i] = f + 1;
      if (done) a.complete[(int64_t)slot * N + i] = f + 1;
    } else {
      a.dropped[i] = drop + 1;
    }
  }
}

// One workgroup per env (the header's "The finish").  Dynamic LDS: d[cap] (the rewards, then d_t,
// then the returns) and dn[cap] (the done flags).
__global__ __launch_bounds__(kPpoFinThreads) void k_ppo_rollout_finish(PpoActor a, int D, double gamma,
                                                                       float *__restrict__ bs, int64_t *__restrict__ ba,
                                                                       float *__restrict__ bret,
                                                                       float *__restrict__ blogp,
                                                                       int64_t *__restrict__ n_dev) {
  extern __shared__ float fin_rows[];
  __shared__ int64_t red[kPpoFinThreads];
  const int tid = threadIdx.x, cap = a.cap;
  const int64_t i = blockIdx.x, N = a.N, base = i * cap;
  float *d = fin_rows, *dn = fin_rows + cap;
  const int g = a.gen[i];
  const int32_t *comp = a.complete + (int64_t)(g & 1) * N;  // the live slot: no workgroup writes it in this launch
  const int m = ppo_clampi(a.fill[i], 0, cap), e = ppo_clampi(comp[i], 0, m);
  // the batch offset: an integer sum, so its order is free
  int64_t acc = 0;
  for (int64_t k = tid; k < i; k += kPpoFinThreads) acc += ppo_clampi(comp[k], 0, cap);
  red[tid] = acc;
  for (int t = tid; t < e; t += kPpoFinThreads) d[t] = a.seg_r[base + t], dn[t] = a.seg_done[base + t];
  __syncthreads();
  for (int st = kPpoFinThreads / 2; st > 0; st >>= 1) {
    if (tid < st) red[tid] += red[tid + st];
    __syncthreads();
  }
  const int64_t off = red[0];
  // the returns: the lane of an episode's done row takes the episode
  for (int t = tid; t < e; t += kPpoFinThreads) {
    if (dn[t] == 0.0f) continue;
    int t0 = t;
    while (t0 > 0 && dn[t0 - 1] == 0.0f) --t0;
    double run = 0.0;
    for (int q = t; q >= t0; --q) {
      float v = 0.0f;
      if (dn[q] == 0.0f) {
        run = radd(rmul(run, gamma), (double)d[q]);
        v = (float)run;
      }
      d[q] = v;
    }
    const double L = (double)(t - t0 + 1);
    double sum = 0.0, vs = 0.0;
    for (int q = t0; q <= t; ++q) sum = radd(sum, (double)d[q]);
    const double mean = sum / L;
    for (int q = t0; q <= t; ++q) {
      const double c = rsub((double)d[q], mean);
      vs = radd(vs, rmul(c, c));
    }
    const double den = radd(sqrt(vs / L), 1e-7);
    for (int q = t0; q <= t; ++q) d[q] = (float)(rsub((double)d[q], mean) / den);
  }
  __syncthreads();
  for (int t = tid; t < e; t += kPpoFinThreads) {
    ba[off + t] = a.seg_a[base + t];
    blogp[off + t] = a.seg_logp[base + t];
    bret[off + t] = d[t];
  }
  for (int x = tid; x < e * D; x += kPpoFinThreads) bs[off * D + x] = a.seg_s[base * D + x];
  if (i == N - 1 && tid == 0) n_dev[0] = off + e;
  __syncthreads();  // the batch copy has read the segment
  const int keep = m - e;
  if (e > 0) {  // (uniform) the carry: rows [e, m) to [0, keep), source and destination may overlap
    for (int c0 = 0; c0 < keep; c0 += kPpoFinThreads) {
      const int q = c0 + tid;
      const bool on = q < keep;
      const int64_t src = base + e + q;
      int64_t av = 0;
      float rv = 0.0f, dv = 0.0f, lv = 0.0f;
      if (on) av = a.seg_a[src], rv = a.seg_r[src], dv = a.seg_done[src], lv = a.seg_logp[src];
      __syncthreads();
      if (on) a.seg_a[base + q] = av, a.seg_r[base + q] = rv, a.seg_done[base + q] = dv, a.seg_logp[base + q] = lv;
    }
    for (int c0 = 0; c0 < keep * D; c0 += kPpoFinThreads) {  // the observations as flat floats
      const int q = c0 + tid;
      const bool on = q < keep * D;
      float v = 0.0f;
      if (on) v = a.seg_s[base * D + e * D + q];
      __syncthreads();
      if (on) a.seg_s[base * D + q] = v;
    }
  }
  if (tid == 0) {
    a.fill[i] = keep;
    a.complete[(int64_t)((g & 1) ^ 1) * N + i] = 0;
    a.gen[i] = g + 1;
  }
}

// The GAE finish (the header's "The GAE finish"): one workgroup per env.  r holds the rewards, then
// the advantages; dn the done flags, then the returns; v the values of the env's rows and, at [m],
// of cur_obs[i].  With the staged value network that is 98 KB of a CU's 160 KB of LDS at any cap.
struct PpoGaeSmem {
  PpoNetSmem value;
  PpoRows rv;
  float x[kPpoRows][kPpoMaxD];
  float r[kPpoMaxCap], dn[kPpoMaxCap], v[kPpoMaxCap + 4];
  int64_t red[kPpoThreads];
};
// ... and of the time-limit variant: vt[t] the value of truncated row t's final observation, tl the
// truncated rows in increasing t (a row index fits 16 bits: cap <= 4096).  A row's truncation flag is
// the sign bit of its dn (done flags are 0 or 1), so it costs no column: 24 KB more, 122 KB of 160.
struct PpoGaeTlSmem : PpoGaeSmem {
  float vt[kPpoMaxCap];
  uint16_t tl[kPpoMaxCap];
};
static_assert(kPpoMaxCap <= 65536 && sizeof(PpoGaeTlSmem) <= 160 * 1024, "a CU's LDS holds the time-limit finish");

// TL: the finish of rth_ppo_gae_finish_tl (the header's "Time-limit ends").  Without the flag the
// kernel, its LDS and its code are rth_ppo_gae_finish's.
template <bool TL>
__global__ __launch_bounds__(kPpoThreads) void k_ppo_gae_finish(PpoActorOf<TL> a, DenseNet va, int D, int LD,
                                                                double gamma, double lam, float *__restrict__ bs,
                                                                int64_t *__restrict__ ba, float *__restrict__ bret,
                                                                float *__restrict__ badv, float *__restrict__ bv,
                                                                float *__restrict__ blogp,
                                                                int64_t *__restrict__ n_dev) {
  __shared__ __align__(16) std::conditional_t<TL, PpoGaeTlSmem, PpoGaeSmem> s;
  const int tid = threadIdx.x, cap = a.cap;
  const int64_t i = blockIdx.x, N = a.N, base = i * cap;
  const int m = ppo_clampi(a.fill[i], 0, cap);  // no launch of this kernel writes fill: k_ppo_gae_clear does
  int64_t acc = 0;  // the batch offset: an integer sum, so its order is free
  for (int64_t k = tid; k < i; k += kPpoThreads) acc += ppo_clampi(a.fill[k], 0, cap);
  s.red[tid] = acc;
  for (int t = tid; t < m; t += kPpoThreads) {
    s.r[t] = a.seg_r[base + t];
    float dn = a.seg_done[base + t];
    if constexpr (TL) {
      if (a.seg_trunc[base + t] != 0.0f) dn = -fabsf(dn);  // (-0 where done is 0: the sign bit alone is read)
    }
    s.dn[t] = dn;
  }
  if (m > 0) ppo_stage_net(va, D, 1, s.value);  // (uniform)
  __syncthreads();
  for (int st = kPpoThreads / 2; st > 0; st >>= 1) {
    if (tid < st) s.red[tid] += s.red[tid + st];
    __syncthreads();
  }
  const int64_t off = s.red[0];
  if (i == N - 1 && tid == 0) n_dev[0] = off + m;
  if (m == 0) return;  // (uniform)
  // the values of rows 0..m-1 and, as row m, of the observation the env acts on next
  for (int r0 = 0; r0 <= m; r0 += kPpoRows) {
    __syncthreads();
    for (int e = tid; e < kPpoRows * kPpoMaxD; e += kPpoThreads) {
      const int r = e / kPpoMaxD, k = e % kPpoMaxD, q = r0 + r;
      float x = 0.0f;
      if (k < D && q <= m) x = q < m ? a.seg_s[(base + q) * D + k] : a.cur_obs[i * LD + k];
      s.x[r][k] = x;
    }
    ppo_forward_rows(s.value, s.x, D, 1, s.rv);
    if (tid < kPpoRows && r0 + tid <= m) s.v[r0 + tid] = s.rv.z[tid][0];
  }
  if constexpr (TL) {
    // the truncated rows, compacted in increasing t: lane tid counts those of its own run of `per`
    // rows, red becomes the counts' running sum (every lane has read `off`), the lane lists its rows
    const int per = (m + kPpoThreads - 1) / kPpoThreads;
    const int t0 = ppo_clampi(tid * per, 0, m), t1 = ppo_clampi(t0 + per, 0, m);
    int mine = 0;
    for (int t = t0; t < t1; ++t) mine += (int)signbit(s.dn[t]);
    __syncthreads();
    s.red[tid] = mine;
    __syncthreads();
    if (tid == 0) {
      int64_t sum = 0;
      for (int k = 0; k < kPpoThreads; ++k) {
        const int64_t c = s.red[k];
        s.red[k] = sum;
        sum += c;
      }
    }
    __syncthreads();
    int at = (int)s.red[tid];
    for (int t = t0; t < t1; ++t)
      if (signbit(s.dn[t])) s.tl[at++] = (uint16_t)t;
    if (tid == kPpoThreads - 1) s.red[tid] = at;  // the total: the last lane's start plus its count
    __syncthreads();
    const int n_tl = (int)s.red[kPpoThreads - 1];  // 0..m (uniform)
    // their values: the same forward on the final observations, a tile of the list at a time
    for (int c0 = 0; c0 < n_tl; c0 += kPpoRows) {
      __syncthreads();
      for (int e = tid; e < kPpoRows * kPpoMaxD; e += kPpoThreads) {
        const int r = e / kPpoMaxD, k = e % kPpoMaxD, q = c0 + r;
        float x = 0.0f;
        if (k < D && q < n_tl) x = a.seg_term_s[(base + s.tl[q]) * D + k];
        s.x[r][k] = x;
      }
      ppo_forward_rows(s.value, s.x, D, 1, s.rv);
      if (tid < kPpoRows && c0 + tid < n_tl) s.vt[s.tl[c0 + tid]] = s.rv.z[tid][0];
    }
  }
  __syncthreads();
  if (tid == 0) {  // the scan: serial, fp64, every operation rounded once
    const double gl = rmul(gamma, lam);
    double run = 0.0;
    for (int t = m - 1; t >= 0; --t) {
      double nt, vt, delta;
      if constexpr (TL) {  // selects: a row that is not truncated takes the operands of the scan without the flag
        const float dn = s.dn[t];
        const bool tr = signbit(dn);
        nt = rsub(1.0, (double)fabsf(dn)), vt = (double)s.v[t];
        const double nb = tr ? 1.0 : nt, nv = tr ? (double)s.vt[t] : (double)s.v[t + 1];
        delta = rsub(radd((double)s.r[t], rmul(rmul(gamma, nv), nb)), vt);
      } else {
        nt = rsub(1.0, (double)s.dn[t]), vt = (double)s.v[t];
        delta = rsub(radd((double)s.r[t], rmul(rmul(gamma, (double)s.v[t + 1]), nt)), vt);
      }
      run = radd(delta, rmul(rmul(gl, nt), run));
      s.r[t] = (float)run;
      s.dn[t] = (float)radd(run, vt);
    }
  }
  __syncthreads();
  for (int t = tid; t < m; t += kPpoThreads) {
    ba[off + t] = a.seg_a[base + t];
    blogp[off + t] = a.seg_logp[base + t];
    badv[off + t] = s.r[t];
    bret[off + t] = s.dn[t];
    bv[off + t] = s.v[t];
  }
  for (int e = tid; e < m * D; e += kPpoThreads) bs[off * D + e] = a.seg_s[base * D + e];
}

// ... and the segments emptied, after every workgroup above has summed the fills
__global__ __launch_bounds__(256) void k_ppo_gae_clear(PpoActor a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  a.fill[i] = 0;
  a.complete[i] = 0, a.complete[a.N + i] = 0;
  a.gen[i] += 1;
}

enum { kPpoReset = 0, kPpoStep = 1, kPpoFinish = 2, kPpoGae = 3 };

// the argument checks of the three entry points
inline const char *ppo_actor_check(const rth_ppo_actor_args *x, int what, PpoActor *out) {
  if (!x) return "NULL args";
  int D, A;
  if (!env_shape(x->env, &D, &A)) return "unknown env id (RTH_ENV_CARTPOLE, RTH_ENV_ACROBOT, RTH_ENV_MOUNTAINCAR)";
  if (!ppo_shape_ok(x->D, x->H, x->A) || x->D != D || x->A != A)
    return "the network shape is not the env's (H = 64; CartPole D = 4, A = 2; Acrobot D = 6, A = 3; "
           "MountainCar D = 2, A = 3)";
  if (x->N < 1 || x->N >= (int64_t(1) << 31)) return "bad N (1 <= N < 2^31)";
  if (x->cap < 1 || x->cap > kPpoMaxCap) return "bad cap (1 <= cap <= 4096 rows per env)";
  if (x->max_episode_steps < 1) return "bad max_episode_steps (>= 1)";
  if (!x->fill || !x->complete || !x->gen || !x->dropped) return "NULL rollout counter";
  PpoActor a{};
  if (what == kPpoGae) {
    if (!x->cur_obs) return "NULL cur_obs";
  } else if (what != kPpoFinish) {
    if (!x->state || !x->ep_steps || !x->t_dev || !x->stats || !x->ret_stats || !x->cur_obs)
      return "NULL state buffer";
    if (reinterpret_cast<uintptr_t>(x->cur_obs) & 15) return "cur_obs must be 16-byte aligned";
  }
  if (what == kPpoStep) {
    if (!dense_net(x->actor, &a.net)) return "NULL network parameter";
    if (!x->action || !x->logprob) return "NULL step buffer";
  }
  if (what != kPpoReset && (!x->seg_s || !x->seg_a || !x->seg_r || !x->seg_done || !x->seg_logp))
    return "NULL rollout column";
  a.state = x->state, a.ep_steps = x->ep_steps, a.t_dev = x->t_dev, a.stats = x->stats, a.ret_stats = x->ret_stats;
  a.cur_obs = x->cur_obs, a.action_in = x->action_in, a.uniforms_in = x->uniforms_in, a.action = x->action;
  a.logprob = x->logprob, a.seg_s = x->seg_s, a.seg_a = x->seg_a, a.seg_r = x->seg_r, a.seg_done = x->seg_done;
  a.seg_logp = x->seg_logp, a.fill = x->fill, a.complete = x->complete, a.gen = x->gen, a.dropped = x->dropped;
  a.seed = x->seed, a.N = x->N, a.cap = x->cap, a.max_steps = x->max_episode_steps;
  *out = a;
  return nullptr;
}

template <int ENV>
inline void ppo_env_launch(bool step, const PpoActor &a, hipStream_t st) {
  actor_launch<k_ppo_actor_step<ENV, false>, k_ppo_env_reset<ENV>, kPpoThreads>(step, a, st);
}

template <int ENV>
inline void ppo_step_tl_launch(const PpoActorTl &a, hipStream_t st) {
  hipLaunchKernelGGL((k_ppo_actor_step<ENV, true>), dim3(dense_grid(a.N)), dim3(kPpoThreads), 0, st, a);
}

// The body of the reset and the step: the checks, then the env's kernel.
inline int ppo_actor_run(const char *fn, const rth_ppo_actor_args *x, bool step, void *stream) {
  PpoActor a;
  const char *bad = ppo_actor_check(x, step ? kPpoStep : kPpoReset, &a);
  RTH_REQUIRE(!bad, "%s: %s", fn, bad);
  switch (x->env) {
    case RTH_ENV_CARTPOLE: ppo_env_launch<RTH_ENV_CARTPOLE>(step, a, as_stream(stream)); break;
    case RTH_ENV_ACROBOT: ppo_env_launch<RTH_ENV_ACROBOT>(step, a, as_stream(stream)); break;
    default: ppo_env_launch<RTH_ENV_MOUNTAINCAR>(step, a, as_stream(stream));
  }
  RTH_LAUNCHED();
  return RTH_OK;
}

// The body of the two GAE finishes: the checks, the finish (TL: with the time-limit columns), the counters.
template <bool TL>
inline int ppo_gae_run(const char *fn, const rth_ppo_actor_args *args, const float *const *value, double gamma,
                       double lam, float *batch_s_dev, int64_t *batch_a_dev, float *batch_ret_dev,
                       float *batch_adv_dev, float *batch_v_dev, float *batch_logprob_dev, int64_t *n_dev,
                       const float *seg_trunc_dev, const float *seg_term_s_dev, void *stream) {
  PpoActorOf<TL> a{};
  const char *bad = ppo_actor_check(args, kPpoGae, &a);
  RTH_REQUIRE(!bad, "%s: %s", fn, bad);
  DenseNet va;
  RTH_REQUIRE(dense_net(value, &va), "%s: NULL value network parameter", fn);
  RTH_REQUIRE(batch_s_dev && batch_a_dev && batch_ret_dev && batch_adv_dev && batch_v_dev && batch_logprob_dev && n_dev,
              "%s: NULL batch buffer", fn);
  RTH_REQUIRE(gamma >= 0.0 && gamma <= 1.0 && lam >= 0.0 && lam <= 1.0, "%s: bad gamma %g or lambda %g (0..1)", fn,
              gamma, lam);
  if constexpr (TL) {
    RTH_REQUIRE(seg_trunc_dev && seg_term_s_dev, "%s: NULL time-limit column", fn);
    a.seg_trunc = const_cast<float *>(seg_trunc_dev), a.seg_term_s = const_cast<float *>(seg_term_s_dev);  // read only
  }
  const int D = (int)args->D;
  hipLaunchKernelGGL((k_ppo_gae_finish<TL>), dim3((unsigned)a.N), dim3(kPpoThreads), 0, as_stream(stream), a, va, D,
                     env_ld(D), gamma, lam, batch_s_dev, batch_a_dev, batch_ret_dev, batch_adv_dev, batch_v_dev,
                     batch_logprob_dev, n_dev);
  RTH_LAUNCHED();
  hipLaunchKernelGGL(k_ppo_gae_clear, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, as_stream(stream),
                     static_cast<const PpoActor &>(a));
  RTH_LAUNCHED();
  return RTH_OK;
}

}  // namespace rth

extern "C" {

int rth_ppo_env_reset(const rth_ppo_actor_args *args, void *stream) {
  return rth::ppo_actor_run("rth_ppo_env_reset", args, false, stream);
}

int rth_ppo_actor_step(const rth_ppo_actor_args *args, void *stream) {
  return rth::ppo_actor_run("rth_ppo_actor_step", args, true, stream);
}

int rth_ppo_actor_step_tl(const rth_ppo_actor_args *args, float *seg_trunc_dev, float *seg_term_s_dev, void *stream) {
  using namespace rth;
  PpoActorTl a{};
  const char *bad = ppo_actor_check(args, kPpoStep, &a);
  RTH_REQUIRE(!bad, "rth_ppo_actor_step_tl: %s", bad);
  RTH_REQUIRE(seg_trunc_dev && seg_term_s_dev, "rth_ppo_actor_step_tl: NULL time-limit column");
  a.seg_trunc = seg_trunc_dev, a.seg_term_s = seg_term_s_dev;
  switch (args->env) {
    case RTH_ENV_CARTPOLE: ppo_step_tl_launch<RTH_ENV_CARTPOLE>(a, as_stream(stream)); break;
    case RTH_ENV_ACROBOT: ppo_step_tl_launch<RTH_ENV_ACROBOT>(a, as_stream(stream)); break;
    default: ppo_step_tl_launch<RTH_ENV_MOUNTAINCAR>(a, as_stream(stream));
  }
  RTH_LAUNCHED();
  return RTH_OK;
}

int rth_ppo_rollout_finish(const rth_ppo_actor_args *args, double gamma, float *batch_s_dev, int64_t *batch_a_dev,
                           float *batch_ret_dev, float *batch_logprob_dev, int64_t *n_dev, void *stream) {
  using namespace rth;
  PpoActor a;
  const char *bad = ppo_actor_check(args, kPpoFinish, &a);
  RTH_REQUIRE(!bad, "rth_ppo_rollout_finish: %s", bad);
  RTH_REQUIRE(batch_s_dev && batch_a_dev && batch_ret_dev && batch_logprob_dev && n_dev,
              "rth_ppo_rollout_finish: NULL batch buffer");
  RTH_REQUIRE(gamma >= 0.0 && gamma <= 1.0, "rth_ppo_rollout_finish: bad gamma %g (0..1)", gamma);
  hipLaunchKernelGGL(k_ppo_rollout_finish, dim3((unsigned)a.N), dim3(kPpoFinThreads), (size_t)a.cap * 8,
                     as_stream(stream), a, (int)args->D, gamma, batch_s_dev, batch_a_dev, batch_ret_dev,
                     batch_logprob_dev, n_dev);
  RTH_LAUNCHED();
  return RTH_OK;
}

int rth_ppo_gae_finish(const rth_ppo_actor_args *args, const float *const *value, double gamma, double lam,
                       float *batch_s_dev, int64_t *batch_a_dev, float *batch_ret_dev, float *batch_adv_dev,
                       float *batch_v_dev, float *batch_logprob_dev, int64_t *n_dev, void *stream) {
  return rth::ppo_gae_run<false>("rth_ppo_gae_finish", args, value, gamma, lam, batch_s_dev, batch_a_dev, batch_ret_dev,
                                 batch_adv_dev, batch_v_dev, batch_logprob_dev, n_dev, nullptr, nullptr, stream);
}

int rth_ppo_gae_finish_tl(const rth_ppo_actor_args *args, const float *const *value, double gamma, double lam,
                          float *batch_s_dev, int64_t *batch_a_dev, float *batch_ret_dev, float *batch_adv_dev,
                          float *batch_v_dev, float *batch_logprob_dev, int64_t *n_dev, const float *seg_trunc_dev,
                          const float *seg_term_s_dev, void *stream) {
  return rth::ppo_gae_run<true>("rth_ppo_gae_finish_tl", args, value, gamma, lam, batch_s_dev, batch_a_dev,
                                batch_ret_dev, batch_adv_dev, batch_v_dev, batch_logprob_dev, n_dev, seg_trunc_dev,
                                seg_term_s_dev, stream);
}

}  // extern "C"
