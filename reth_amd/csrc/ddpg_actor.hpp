// Device-resident continuous-control actors on DDPG's fused actor (ddpg.hpp): one launch per env
// step for N actors, templated on the env id (one env for now: Pendulum-v0, D = 3, Ad = 1), behind
// two entry points: rth_ddpg_env_reset and rth_ddpg_actor_step.  The counterpart of env_actor.hpp
// for a continuous action.  Per tile of kDdpgRows rows the step runs the acting forward
// (ddpg_actor_forward, the only actor forward: a row's noise-free action equals rth_ddpg_act's bit
// for bit), then one lane per env: Ornstein-Uhlenbeck exploration noise on counter-based normal
// draws, the env's dynamics in fp64 in its host class's operation order (reth_amd/envs.py:
// Pendulum), the time limit, the reset of a finished episode and the transition as a dense row.
// No host synchronisation, no atomics, no grid-wide agreement: everything an env touches is
// private to its lane.
//
// Reference: reth/reth/presets/worker.py:128-155 (Worker.step: exploration.act, env.step, on done
// env.reset and exploration.reset, :66), utils/exploration.py:34-53 (OUNoiseExploration),
// utils/noise.py (OUNoise), utils/schedule.py (Schedule._at); the environment restates gym
// 0.17.3's classic_control/pendulum.py (the reference's pinned dependency).
//
// Environments (include/reth_hip.h: RTH_DDPG_ENV_*), state fp64 [N, 4] with unused columns 0:
//   PENDULUM  D 3, Ad 1  state (theta, theta_dot, 0, 0)  obs = (cos theta, sin theta, theta_dot)
//             u = clip((double) action[0], +-2); cost = angle_normalize(theta)^2 + 0.1 theta_dot^2
//             + 0.001 u^2 of the state BEFORE the step; theta_dot' = theta_dot + (-15 sin(theta +
//             pi) + 3 u) 0.05; theta' = theta + theta_dot' 0.05 from the UNCLIPPED theta_dot', which
//             is clipped to +-8 only then; angle_normalize(x) = ((x + pi) % 2 pi) - pi with Python's
//             % (fmod, plus the divisor when the result is non-zero and negative).  The reward is
//             (float) (-cost).  No terminal state: done = 1 only when the episode's step count
//             reaches max_episode_steps.
//
// Step counter.  t_dev is int64 [N]: every env carries its own act count, t = t_dev[i] + 1, so the
// one launch needs no grid-wide agreement.  A reference worker steps its exploration schedule
// once per act; here every env is its own worker, so the schedule advances once per LAUNCH (per
// env step of each env), not once per transition of the set: N envs reach the schedule's end N
// times sooner in transitions than one reference worker does.
//
// Exploration.  The noise state is fp64 [N, Ad]; every operation is one radd / rmul, rounded once
// and never contracted:
//     x'     = x + (theta * (mu - x) + sigma * z)                          (noise.py)
//     eps    = start + (end - start) * k / max_steps,  k = min(t, max_steps) (Schedule._at's order)
//     action = (float) ((double) act_det + eps * x')                       not clipped: what
//              numpy's in-place float32 += float64 yields (exploration.py:38)
// The noise state advances every step, whether or not action_in overrides the action; an episode
// end sets it back to mu (worker.py:66).
//
// Normal draws: a pure function of (seed, env i, t, component a).  One Philox4x32-10 block per four
// components, b = a / 4,
//     counter = {(uint32) i, (uint32) t, (uint32) (t >> 32), STREAM_OU | (b << 16)}   STREAM_OU = 12
//     key     = {(uint32) seed, (uint32) (seed >> 32)}
// and Box-Muller in fp64 on the word pairs j = 0, 1 of its output c:
//     u1 = ((double) c[2j] + 0.5) / 2^32 in (0, 1),  u2 = (double) c[2j + 1] / 2^32 in [0, 1)
//     r  = sqrt(-2 ln u1),  z[4b + 2j] = r cos(2 pi u2),  z[4b + 2j + 1] = r sin(2 pi u2)
//
// Reset draws (the reset entry point at t = 0, and step t of an env whose episode ended at t): one
// Philox block per (seed, env i, t), counter = {(uint32) i, (uint32) t, (uint32) (t >> 32),
// STREAM_PENDULUM} (11), the same key:
//     theta = -pi + (2 pi * (double) c[0]) / 2^32,  theta_dot = -1 + (2 * (double) c[1]) / 2^32
//
// Outputs.  DDPG has no n-step here, so there is no adder and no ring: the transition IS the row,
// s0 [N, D], a [N, Ad], r [N], s1 [N, D], done [N], dense f32; s1 is the terminal observation when
// done.  cur_obs f32 [N, LD] (LD = D rounded up to 4 floats, pad 0, rows moved as 16-byte pieces)
// holds the observation the env acts on next -- after a done the reset observation.
//
// Statistics.  stats int64 [N, 3]: finished episodes, the sum of their lengths, the last length.
// ret_stats fp64 [N, 3]: the running episode's return, the sum of the finished episodes' returns,
// the last finished return -- sums of the fp64 rewards -cost (the host env's), not of their floats.
#pragma once
#include "ddpg.hpp"
#include "env_actor.hpp"

namespace rth {

constexpr uint32_t STREAM_PENDULUM = 11u, STREAM_OU = 12u;

template <int ENV>
struct DdpgEnvSpec;
template <>
struct DdpgEnvSpec<RTH_DDPG_ENV_PENDULUM> {
  static constexpr int D = 3, Ad = 1;
};

struct DdpgActor {
  DenseNet net;
  DdpgDims dims;
  double *state;
  int32_t *ep_steps;
  int64_t *t_dev, *stats;
  double *ret_stats, *noise;
  float *cur_obs;
  const float *action_in;  // NULL: the noisy action (workgroup-uniform)
  float *act_det;          // NULL: not wanted
  float *row_s0, *row_a, *row_r, *row_s1, *row_done;
  uint64_t seed;
  int64_t N;
  double mu, theta, sigma, eps_start, eps_end;
  int64_t eps_steps;
  int max_steps;
};

// ------------------------------------------------------------------ Pendulum
__device__ inline void pendulum_reset_draw(uint64_t seed, int64_t i, int64_t t, double (&s)[4]) {
  const double pi = 3.141592653589793;
  uint32_t c[4];
  env_philox_block(seed, i, t, STREAM_PENDULUM, c);
  s[0] = radd(-pi, rmul(rmul(2.0, pi), (double)c[0]) / 4294967296.0);
  s[1] = radd(-1.0, rmul(2.0, (double)c[1]) / 4294967296.0);
  s[2] = 0.0, s[3] = 0.0;
}

// envs.Pendulum.step: every product and sum rounded where python rounds it, squares as products;
// advances s and returns the fp64 reward -cost
__device__ inline double pendulum_dynamics(double (&s)[4], const float *action) {
  const double max_speed = 8.0, max_torque = 2.0, dt = 0.05, g = 10.0, m = 1.0, l = 1.0, pi = 3.141592653589793;
  const double two_pi = rmul(2.0, pi);
  const double th = s[0], thdot = s[1];
  double u = (double)action[0];
  u = u < -max_torque ? -max_torque : (u > max_torque ? max_torque : u);
  double md = fmod(radd(th, pi), two_pi);  // python's %: the result takes the divisor's sign
  if (md != 0.0 && md < 0.0) md = radd(md, two_pi);
  const double norm = rsub(md, pi);
  const double cost = radd(radd(rmul(norm, norm), rmul(0.1, rmul(thdot, thdot))), rmul(0.001, rmul(u, u)));
  const double k_sin = rmul(-3.0, g) / rmul(2.0, l), k_u = 3.0 / rmul(m, rmul(l, l));
  double newthdot = radd(thdot, rmul(radd(rmul(k_sin, sin(radd(th, pi))), rmul(k_u, u)), dt));
  const double newth = radd(th, rmul(newthdot, dt));
  newthdot = newthdot < -max_speed ? -max_speed : (newthdot > max_speed ? max_speed : newthdot);
  s[0] = newth, s[1] = newthdot, s[2] = 0.0, s[3] = 0.0;
  return -cost;
}

// ------------------------------------------------------------------ per-env pieces of the step
template <int ENV>
__device__ __forceinline__ void ddpg_env_reset_draw(uint64_t seed, int64_t i, int64_t t, double (&s)[4]) {
  if constexpr (ENV == RTH_DDPG_ENV_PENDULUM) pendulum_reset_draw(seed, i, t, s);
}

template <int ENV>
__device__ __forceinline__ double ddpg_env_dynamics(double (&s)[4], const float *action) {
  static_assert(ENV == RTH_DDPG_ENV_PENDULUM, "a new env adds its rules here");
  return pendulum_dynamics(s, action);
}

// the f32 observation of state s, env_ld(D) floats, pad = 0
template <int ENV>
__device__ __forceinline__ void ddpg_env_obs(const double (&s)[4], float (&o)[env_ld(DdpgEnvSpec<ENV>::D)]) {
  if constexpr (ENV == RTH_DDPG_ENV_PENDULUM) {
    o[0] = (float)cos(s[0]), o[1] = (float)sin(s[0]), o[2] = (float)s[1], o[3] = 0.0f;
  }
}

template <int LD>
__device__ __forceinline__ void ddpg_store_cur_obs(float *__restrict__ row, const float (&o)[LD]) {
#pragma unroll
  for (int k = 0; k < LD / 4; ++k)
    reinterpret_cast<float4 *>(row)[k] = make_float4(o[4 * k], o[4 * k + 1], o[4 * k + 2], o[4 * k + 3]);
}

// the standard normal draws z[0..Ad) of (seed, env i, step t): the header's mapping
template <int Ad>
__device__ inline void ou_normals(uint64_t seed, int64_t i, int64_t t, double (&z)[Ad]) {
  const double two_pi = rmul(2.0, 3.141592653589793);
#pragma unroll
  for (int b = 0; b < (Ad + 3) / 4; ++b) {
    uint32_t c[4];
    env_philox_block(seed, i, t, STREAM_OU | ((uint32_t)b << 16), c);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (4 * b + 2 * j >= Ad) break;
      const double u1 = radd((double)c[2 * j], 0.5) / 4294967296.0, u2 = (double)c[2 * j + 1] / 4294967296.0;
      const double r = sqrt(rmul(-2.0, log(u1))), ang = rmul(two_pi, u2);
      z[4 * b + 2 * j] = rmul(r, cos(ang));
      if (4 * b + 2 * j + 1 < Ad) z[4 * b + 2 * j + 1] = rmul(r, sin(ang));
    }
  }
}

template <int ENV>
__global__ __launch_bounds__(256) void k_ddpg_env_reset(DdpgActor a) {
  constexpr int Ad = DdpgEnvSpec<ENV>::Ad, LD = env_ld(DdpgEnvSpec<ENV>::D);
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  double s[4];
  ddpg_env_reset_draw<ENV>(a.seed, i, 0, s);
#pragma unroll
  for (int k = 0; k < 4; ++k) a.state[i * 4 + k] = s[k];
  a.ep_steps[i] = 0;
  a.t_dev[i] = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) a.stats[i * 3 + k] = 0, a.ret_stats[i * 3 + k] = 0.0;
#pragma unroll
  for (int k = 0; k < Ad; ++k) a.noise[i * Ad + k] = a.mu;
  float o[LD];
  ddpg_env_obs<ENV>(s, o);
  ddpg_store_cur_obs<LD>(a.cur_obs + i * LD, o);
}

template <int ENV>
__global__ __launch_bounds__(kDdpgThreads) void k_ddpg_actor_step(DdpgActor a) {
  constexpr int D = DdpgEnvSpec<ENV>::D, Ad = DdpgEnvSpec<ENV>::Ad, LD = env_ld(D);
  static_assert(D <= kDdpgMaxD && Ad <= kDdpgMaxAd, "the env's shape is one ddpg.hpp builds");
  __shared__ __align__(16) DdpgSmem s;
  const int tid = threadIdx.x;
  const int64_t N = a.N;
  const int64_t tiles = (N + kDdpgRows - 1) / kDdpgRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kDdpgRows;
    __syncthreads();  // the previous tile is done with s
    dense_load_x(a.cur_obs, LD, N, r0, D, s.x);  // the acting observations, zero past N / D
    ddpg_actor_forward(a.net, a.dims, &s.h1[0][0], &s.h2[0][0], s);
    if (tid >= kDdpgRows || r0 + tid >= N) continue;
    const int64_t i = r0 + tid;
    // everything the lane reads, before the stores below, which it may alias for all the
    // compiler knows: after them every load's latency would be the lane's own
    const int64_t t = a.t_dev[i] + 1;
    double st[4], x[Ad], run[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) st[k] = a.state[i * 4 + k];
#pragma unroll
    for (int k = 0; k < Ad; ++k) x[k] = a.noise[i * Ad + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) run[k] = a.ret_stats[i * 3 + k];
    const int steps = a.ep_steps[i] + 1;
    int64_t ep[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) ep[k] = a.stats[i * 3 + k];
    float act[Ad], det[Ad], o0[D];
#pragma unroll
    for (int k = 0; k < Ad; ++k) det[k] = s.act[tid][k], act[k] = a.action_in ? a.action_in[i * Ad + k] : 0.0f;
#pragma unroll
    for (int k = 0; k < D; ++k) o0[k] = s.x[tid][k];  // the forward leaves the tile's observations in place
    // OU noise and the schedule
    double z[Ad];
    ou_normals<Ad>(a.seed, i, t, z);
    const int64_t kk = t < a.eps_steps ? t : a.eps_steps;
    const double eps = radd(a.eps_start, rmul(rsub(a.eps_end, a.eps_start), (double)kk) / (double)a.eps_steps);
#pragma unroll
    for (int k = 0; k < Ad; ++k) {
      x[k] = radd(x[k], radd(rmul(a.theta, rsub(a.mu, x[k])), rmul(a.sigma, z[k])));
      if (!a.action_in) act[k] = (float)radd((double)det[k], rmul(eps, x[k]));
    }
    const double rew = ddpg_env_dynamics<ENV>(st, act);
    const bool done = steps >= a.max_steps;
    float o1[LD], oc[LD];
    ddpg_env_obs<ENV>(st, o1);  // the terminal observation when done
#pragma unroll
    for (int k = 0; k < LD; ++k) oc[k] = o1[k];
    const double ret = radd(run[0], rew);
    if (done) {
      ddpg_env_reset_draw<ENV>(a.seed, i, t, st);
      ddpg_env_obs<ENV>(st, oc);  // acted on next
      ep[0] += 1, ep[1] += steps, ep[2] = steps;
      run[1] = radd(run[1], ret), run[2] = ret;
    }
    run[0] = done ? 0.0 : ret;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[i * 4 + k] = st[k];
#pragma unroll
    for (int k = 0; k < Ad; ++k) a.noise[i * Ad + k] = done ? a.mu : x[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.ret_stats[i * 3 + k] = run[k], a.stats[i * 3 + k] = ep[k];
    a.ep_steps[i] = done ? 0 : steps;
    a.t_dev[i] = t;
    ddpg_store_cur_obs<LD>(a.cur_obs + i * LD, oc);
#pragma unroll
    for (int k = 0; k < D; ++k) a.row_s0[i * D + k] = o0[k], a.row_s1[i * D + k] = o1[k];
#pragma unroll
    for (int k = 0; k < Ad; ++k) {
      a.row_a[i * Ad + k] = act[k];
      if (a.act_det) a.act_det[i * Ad + k] = det[k];
    }
    a.row_r[i] = (float)rew;
    a.row_done[i] = done ? 1.0f : 0.0f;
  }
}

inline bool ddpg_env_shape(int64_t env, int *D, int *Ad) {
  switch (env) {
    case RTH_DDPG_ENV_PENDULUM:
      *D = DdpgEnvSpec<RTH_DDPG_ENV_PENDULUM>::D, *Ad = DdpgEnvSpec<RTH_DDPG_ENV_PENDULUM>::Ad;
      return true;
    default: return false;
  }
}

// the argument checks of the two entry points
inline const char *ddpg_actor_check(const rth_ddpg_actor_args *x, bool step, DdpgActor *out) {
  if (!x) return "NULL args";
  int D, Ad;
  if (!ddpg_env_shape(x->env, &D, &Ad)) return "unknown env id (RTH_DDPG_ENV_PENDULUM)";
  if (x->D != D || x->Ad != Ad || !ddpg_shape_ok(x->D, x->Ad, x->H1, x->H2))
    return "the network shape is not the env's (Pendulum D = 3, Ad = 1) or not one rth_ddpg_supported "
           "builds " RTH_DDPG_LIMITS;
  if (x->N < 1 || x->N >= (int64_t(1) << 31)) return "bad N (1 <= N < 2^31)";
  if (x->max_episode_steps < 1) return "bad max_episode_steps (>= 1)";
  if (!x->state || !x->ep_steps || !x->t_dev || !x->stats || !x->ret_stats || !x->noise || !x->cur_obs)
    return "NULL state buffer";
  if (reinterpret_cast<uintptr_t>(x->cur_obs) & 15) return "cur_obs must be 16-byte aligned";
  DdpgActor a{};
  if (step) {
    if (!dense_net(x->actor, &a.net)) return "NULL network parameter";
    if (!x->row_s0 || !x->row_a || !x->row_r || !x->row_s1 || !x->row_done) return "NULL step buffer";
    if (x->eps_steps < 1) return "bad eps_steps (>= 1)";
  }
  a.dims = DdpgDims{(int)x->D, (int)x->Ad, (int)x->H1, (int)x->H2};
  a.state = x->state, a.ep_steps = x->ep_steps, a.t_dev = x->t_dev, a.stats = x->stats, a.ret_stats = x->ret_stats;
  a.noise = x->noise, a.cur_obs = x->cur_obs, a.action_in = x->action_in, a.act_det = x->act_det;
  a.row_s0 = x->row_s0, a.row_a = x->row_a, a.row_r = x->row_r, a.row_s1 = x->row_s1, a.row_done = x->row_done;
  a.seed = x->seed, a.N = x->N, a.mu = x->mu, a.theta = x->theta, a.sigma = x->sigma;
  a.eps_start = x->eps_start, a.eps_end = x->eps_end, a.eps_steps = x->eps_steps, a.max_steps = x->max_episode_steps;
  *out = a;
  return nullptr;
}

// The body of both entry points: the checks, then the env's step or reset kernel.
inline int ddpg_actor_run(const char *fn, const rth_ddpg_actor_args *x, bool step, void *stream) {
  DdpgActor a;
  const char *bad = ddpg_actor_check(x, step, &a);
  RTH_REQUIRE(!bad, "%s: %s", fn, bad);
  constexpr int ENV = RTH_DDPG_ENV_PENDULUM;  // the one env the check lets through
  actor_launch<k_ddpg_actor_step<ENV>, k_ddpg_env_reset<ENV>, kDdpgThreads>(step, a, as_stream(stream));
  RTH_LAUNCHED();
  return RTH_OK;
}

}  // namespace rth

extern "C" {

int rth_ddpg_env_reset(const rth_ddpg_actor_args *args, void *stream) {
  return rth::ddpg_actor_run("rth_ddpg_env_reset", args, false, stream);
}

int rth_ddpg_actor_step(const rth_ddpg_actor_args *args, void *stream) {
  return rth::ddpg_actor_run("rth_ddpg_actor_step", args, true, stream);
}

}  // extern "C"
