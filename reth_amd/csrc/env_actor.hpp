// Device-resident classic-control actors on the fused MLP kernels: one launch per env step for N
// actors, generic over a small family of environments -- CartPole-v0/v1, Acrobot-v1 and
// MountainCar-v0 -- each at its own network shape (D, A).  ONE step kernel and ONE reset kernel,
// templated on the env id, behind four entry points: rth_env_reset / rth_env_actor_step (any env,
// here) and rth_cartpole_reset / rth_mlp_actor_step (mlp_actor.hpp: adapters that launch the
// CartPole instance without return statistics; same bits, pinned by
// tests/test_classic_actors_gpu.py::test_generic_cartpole_equals_the_cartpole_actors).
// Per tile of kMlpRows rows the step runs the acting forward of mlp.hpp at the env's (D, A)
// (mlp_forward_rows, the only forward: a row's Q equals rth_mlp_q's bit for bit), then one lane per
// env: ε-greedy with the draws of eps_greedy_one, the env's dynamics in fp64 in its host class's
// operation order (reth_amd/envs.py: CartPole, Acrobot, MountainCar), the time limit, the reset of
// a finished episode, the f32 observation into a per-env ring, the n-step push (nstep_push_one on
// an rth_nstep handle) and the emitted row by handle and by value.  No host synchronisation, no
// atomics: everything an env touches is private to its lane.
//
// Reference: reth/reth/presets/worker.py:128-155 (Worker.step: act, env.step, env.reset on done),
// utils/exploration.py:26-31, algorithm/dqn/dqn_solver.py:126-131, utils/nstep_adder.py:11-28; the
// environments restate gym 0.17.3's classic_control definitions (the reference's pinned dependency).
//
// Environments (include/reth_hip.h: RTH_ENV_*), state fp64 [N, 4] with unused columns 0:
//   CARTPOLE     D 4, A 2  state (x, x_dot, theta, theta_dot)   obs = state          reward 1
//   ACROBOT      D 6, A 3  state (th1, th2, w1, w2)             obs = (cos th1, sin th1, cos th2,
//                          sin th2, w1, w2)                     reward -1, 0 on the terminal step
//   MOUNTAINCAR  D 2, A 3  state (p, v, 0, 0)                   obs = (p, v)         reward -1
// The time limit ends an episode without changing its reward.
//
// Step counter.  t_dev is int64 [N]: every env carries the (common) number of env steps taken and
// advances its own copy, t = t_dev[i] + 1, so the one launch needs no grid-wide agreement on who
// increments a scalar.  ε-greedy at step t draws with counter = t, lane = i (eps_explore_draw).
//
// Reset draws (the reset entry points at t = 0, and step t of an env whose episode ended at t): one
// Philox4x32-10 block per (seed, env i, t) -- a pure function of the three --,
//     counter = {(uint32) i, (uint32) t, (uint32) (t >> 32), stream}
//     key     = {(uint32) seed, (uint32) (seed >> 32)}
// with stream = STREAM_CARTPOLE (7), STREAM_ACROBOT (9), STREAM_MOUNTAINCAR (10), and with the
// four output words c[k], in fp64 with each operation rounded once:
//     CartPole     state[k] = -0.05 + (0.1 * (double) c[k]) / 2^32   k = 0..3, in [-0.05, 0.05)
//     Acrobot      state[k] = -0.1  + (0.2 * (double) c[k]) / 2^32   k = 0..3, in [-0.1, 0.1)
//     MountainCar  p        = -0.6  + (0.2 * (double) c[0]) / 2^32   in [-0.6, -0.4);  v = 0
//
// Observation ring.  f32 [N * ring + 1, LD], LD = D rounded up to 4 floats (CartPole 4, Acrobot 8,
// MountainCar 4) so a row moves as 16-byte pieces; the pad floats are written as 0; the last row
// is an all-zero sink the kernel never writes.  Env i's slot s is row i * ring + s = the handle.
// Step t writes the next observation into slot (2t) % ring and, when the episode ended, the reset
// observation into (2t + 1) % ring; cur_slot[i] is the slot of the observation the env acts on
// next.  A done row's s1 is the terminal observation.  An emitted n-step row references slots
// written at most n + 1 steps earlier, so ring >= 2 (n + 2) keeps them intact for the by-value
// copy.  row_obs0 / row_obs1 are dense [N, D] (D is even for every env: 8-byte pieces).
//
// Statistics.  stats int64 [N, 3]: finished episodes, the sum of their lengths, the last length.
// ret_stats fp64 [N, 3], NULL from the CartPole adapters (the return is the length there): the
// running episode's return, the sum of the finished episodes' returns, the last finished return
// (rewards are small integers, so the sums are exact).
#pragma once
#include "actor_shared.hpp"
#include "mlp.hpp"

namespace rth {

constexpr uint32_t STREAM_CARTPOLE = 7u, STREAM_ACROBOT = 9u, STREAM_MOUNTAINCAR = 10u;

template <int ENV>
struct EnvSpec;
template <>
struct EnvSpec<RTH_ENV_CARTPOLE> {
  static constexpr int D = 4, A = 2;
};
template <>
struct EnvSpec<RTH_ENV_ACROBOT> {
  static constexpr int D = 6, A = 3;
};
template <>
struct EnvSpec<RTH_ENV_MOUNTAINCAR> {
  static constexpr int D = 2, A = 3;
};
constexpr int env_ld(int D) { return (D + 3) & ~3; }  // the ring's row stride in floats

struct EnvActor {
  DenseNet net;
  double *state;
  int32_t *ep_steps;
  int64_t *t_dev, *stats;
  double *ret_stats;  // NULL: no return statistics (workgroup-uniform)
  float *obs_ring;
  int64_t *cur_slot;
  const double *eps;
  const int64_t *action_in;
  int64_t *action;
  float *reward, *done;
  int64_t *s0_h, *s1_h;
  int32_t *emit;
  int64_t *row_s0, *row_a, *row_s1;
  float *row_r, *row_done, *row_obs0, *row_obs1, *q_out;
  uint64_t seed;
  int64_t N;
  int ring, max_steps;
  NStepState ns;
  int n;
  double gamma;
  int mode;
};

// ------------------------------------------------------------------ CartPole
__device__ __forceinline__ float4 cartpole_obs(const double (&s)[4]) {
  return make_float4((float)s[0], (float)s[1], (float)s[2], (float)s[3]);
}

// envs.CartPole.step (gym 0.17.3 classic_control/cartpole.py, Euler): every product and sum
// rounded where python rounds it, squares as products; returns the terminal test on x / theta
__device__ inline bool cartpole_dynamics(double (&s)[4], int64_t action) {
  const double gravity = 9.8, masscart = 1.0, masspole = 0.1, length = 0.5, force_mag = 10.0, tau = 0.02;
  const double theta_threshold = 12 * 2 * 3.141592653589793 / 360, x_threshold = 2.4;
  double x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
  const double force = action == 1 ? force_mag : -force_mag;
  const double costheta = cos(theta), sintheta = sin(theta);
  const double total_mass = radd(masspole, masscart);
  const double polemass_length = rmul(masspole, length);
  const double temp = radd(force, rmul(rmul(polemass_length, rmul(theta_dot, theta_dot)), sintheta)) / total_mass;
  const double thetaacc =
      rsub(rmul(gravity, sintheta), rmul(costheta, temp)) /
      rmul(length, rsub(4.0 / 3.0, rmul(masspole, rmul(costheta, costheta)) / total_mass));
  const double xacc = rsub(temp, rmul(rmul(polemass_length, thetaacc), costheta) / total_mass);
  x = radd(x, rmul(tau, x_dot));
  x_dot = radd(x_dot, rmul(tau, xacc));
  theta = radd(theta, rmul(tau, theta_dot));
  theta_dot = radd(theta_dot, rmul(tau, thetaacc));
  s[0] = x, s[1] = x_dot, s[2] = theta, s[3] = theta_dot;
  return x < -x_threshold || x > x_threshold || theta < -theta_threshold || theta > theta_threshold;
}

// ------------------------------------------------------------------ Acrobot
// envs.Acrobot._dsdt (gym 0.17.3 classic_control/acrobot.py, the "book" dynamics): every product
// and sum rounded where python rounds it (left to right), squares as products
__device__ inline void acrobot_dsdt(const double (&y)[4], double tau, double (&d)[4]) {
  const double m1 = 1.0, m2 = 1.0, l1 = 1.0, lc1 = 0.5, lc2 = 0.5, I1 = 1.0, I2 = 1.0, g = 9.8;
  const double half_pi = 3.141592653589793 / 2.0;
  const double t1 = y[0], t2 = y[1], w1 = y[2], w2 = y[3];
  const double c2 = cos(t2), s2 = sin(t2);
  const double d1 = radd(
      radd(radd(rmul(rmul(m1, lc1), lc1),
                rmul(m2, radd(radd(rmul(l1, l1), rmul(lc2, lc2)), rmul(rmul(rmul(2.0, l1), lc2), c2)))),
           I1),
      I2);
  const double d2 = radd(rmul(m2, radd(rmul(lc2, lc2), rmul(rmul(l1, lc2), c2))), I2);
  const double phi2 = rmul(rmul(rmul(m2, lc2), g), cos(rsub(radd(t1, t2), half_pi)));
  const double p1a = rmul(rmul(rmul(rmul(-m2, l1), lc2), rmul(w2, w2)), s2);
  const double p1b = rmul(rmul(rmul(rmul(rmul(rmul(2.0, m2), l1), lc2), w2), w1), s2);
  const double p1c = rmul(rmul(radd(rmul(m1, lc1), rmul(m2, l1)), g), cos(rsub(t1, half_pi)));
  const double phi1 = radd(radd(rsub(p1a, p1b), p1c), phi2);
  const double num =
      rsub(rsub(radd(tau, rmul(d2 / d1, phi1)), rmul(rmul(rmul(rmul(m2, l1), lc2), rmul(w1, w1)), s2)), phi2);
  const double den = rsub(radd(rmul(rmul(m2, lc2), lc2), I2), rmul(d2, d2) / d1);
  const double a2 = num / den;
  const double a1 = -radd(rmul(d2, a2), phi1) / d1;
  d[0] = w1, d[1] = w2, d[2] = a1, d[3] = a2;
}

constexpr int kWrapMax = 8;  // a step moves an angle by < 2 turns (|w| <= 9 pi, dt = 0.2): never reached from a wrapped state

// envs.Acrobot.step: one classical RK4 step of dt = 0.2, the angles wrapped into [-pi, pi], the
// velocities clamped to +-4 pi / +-9 pi; returns the terminal test -cos th1 - cos(th1 + th2) > 1
__device__ inline bool acrobot_dynamics(double (&s)[4], int64_t action) {
  const double dt = 0.2, dt2 = 0.2 / 2.0, dt6 = 0.2 / 6.0, pi = 3.141592653589793;
  const double two_pi = rmul(2.0, pi), max1 = rmul(4.0, pi), max2 = rmul(9.0, pi);
  const double tau = (double)(action - 1);
  double y[4], k[4], acc[4] = {};
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = s[j];
  // k1 = f(y0), k2 = f(y0 + dt/2 k1), k3 = f(y0 + dt/2 k2), k4 = f(y0 + dt k3);
  // y1 = y0 + dt/6 (((k1 + 2 k2) + 2 k3) + k4).  One body for the four stages: code size
#pragma unroll 1
  for (int stage = 0; stage < 4; ++stage) {
    acrobot_dsdt(y, tau, k);
    const double wgt = (stage == 1 || stage == 2) ? 2.0 : 1.0;  // 1.0 * k is k exactly
    const double adv = stage == 2 ? dt : dt2;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      acc[j] = stage == 0 ? k[j] : radd(acc[j], rmul(wgt, k[j]));
      y[j] = radd(s[j], rmul(adv, k[j]));
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) y[j] = radd(s[j], rmul(dt6, acc[j]));
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    double x = y[j];
    for (int it = 0; it < kWrapMax && x > pi; ++it) x = rsub(x, two_pi);
    for (int it = 0; it < kWrapMax && x < -pi; ++it) x = radd(x, two_pi);
    y[j] = x;
  }
  y[2] = y[2] < -max1 ? -max1 : (y[2] > max1 ? max1 : y[2]);
  y[3] = y[3] < -max2 ? -max2 : (y[3] > max2 ? max2 : y[3]);
#pragma unroll
  for (int j = 0; j < 4; ++j) s[j] = y[j];
  return rsub(-cos(y[0]), cos(radd(y[1], y[0]))) > 1.0;
}

// ------------------------------------------------------------------ MountainCar
// envs.MountainCar.step (gym 0.17.3 classic_control/mountain_car.py); returns p >= 0.5 and v >= 0
__device__ inline bool mountaincar_dynamics(double (&s)[4], int64_t action) {
  const double min_p = -1.2, max_p = 0.6, max_v = 0.07, goal_p = 0.5, force = 0.001, gravity = 0.0025;
  double p = s[0], v = s[1];
  v = radd(v, radd(rmul((double)(action - 1), force), rmul(cos(rmul(3.0, p)), -gravity)));
  v = v < -max_v ? -max_v : (v > max_v ? max_v : v);
  p = radd(p, v);
  p = p < min_p ? min_p : (p > max_p ? max_p : p);
  if (p == min_p && v < 0.0) v = 0.0;
  s[0] = p, s[1] = v, s[2] = 0.0, s[3] = 0.0;
  return p >= goal_p && v >= 0.0;
}

// ------------------------------------------------------------------ per-env pieces of the step
__device__ inline void uniform_reset_draw(uint64_t seed, int64_t i, int64_t t, uint32_t stream, double lo,
                                          double width, int n, double (&s)[4]) {
  uint32_t c[4];
  env_philox_block(seed, i, t, stream, c);
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = k < n ? radd(lo, rmul(width, (double)c[k]) / 4294967296.0) : 0.0;
}

template <int ENV>
__device__ __forceinline__ void env_reset_draw(uint64_t seed, int64_t i, int64_t t, double (&s)[4]) {
  if constexpr (ENV == RTH_ENV_CARTPOLE) uniform_reset_draw(seed, i, t, STREAM_CARTPOLE, -0.05, 0.1, 4, s);
  if constexpr (ENV == RTH_ENV_ACROBOT) uniform_reset_draw(seed, i, t, STREAM_ACROBOT, -0.1, 0.2, 4, s);
  if constexpr (ENV == RTH_ENV_MOUNTAINCAR) uniform_reset_draw(seed, i, t, STREAM_MOUNTAINCAR, -0.6, 0.2, 1, s);
}

// the env's rules: advances s, returns the terminal test, *reward = this step's reward
template <int ENV>
__device__ __forceinline__ bool env_dynamics(double (&s)[4], int64_t action, float *reward) {
  if constexpr (ENV == RTH_ENV_CARTPOLE) {
    *reward = 1.0f;
    return cartpole_dynamics(s, action);
  } else if constexpr (ENV == RTH_ENV_ACROBOT) {
    const bool terminal = acrobot_dynamics(s, action);
    *reward = terminal ? 0.0f : -1.0f;
    return terminal;
  } else {
    *reward = -1.0f;
    return mountaincar_dynamics(s, action);
  }
}

// the f32 observation of state s into a ring row (env_ld(D) floats, 16-byte aligned), pad = 0
template <int ENV>
__device__ __forceinline__ void env_store_obs(float *__restrict__ row, const double (&s)[4]) {
  float4 *row4 = reinterpret_cast<float4 *>(row);
  if constexpr (ENV == RTH_ENV_CARTPOLE) row4[0] = cartpole_obs(s);
  if constexpr (ENV == RTH_ENV_ACROBOT) {
    row4[0] = make_float4((float)cos(s[0]), (float)sin(s[0]), (float)cos(s[1]), (float)sin(s[1]));
    row4[1] = make_float4((float)s[2], (float)s[3], 0.0f, 0.0f);
  }
  if constexpr (ENV == RTH_ENV_MOUNTAINCAR) row4[0] = make_float4((float)s[0], (float)s[1], 0.0f, 0.0f);
}

template <int ENV>
__global__ __launch_bounds__(256) void k_env_reset(EnvActor a) {
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
  for (int k = 0; k < 3; ++k) {
    a.stats[i * 3 + k] = 0;
    if (a.ret_stats) a.ret_stats[i * 3 + k] = 0.0;
  }
  env_store_obs<ENV>(a.obs_ring + (i * a.ring + 1) * LD, s);
  a.cur_slot[i] = 1;
}

template <int ENV>
__global__ __launch_bounds__(kMlpThreads) void k_env_actor_step(EnvActor a) {
  constexpr int D = EnvSpec<ENV>::D, A = EnvSpec<ENV>::A, LD = env_ld(D);
  static_assert(D % 2 == 0 && D <= kMlpMaxD && A <= kMlpMaxA, "row_obs moves as 8-byte pieces");
  __shared__ __align__(16) MlpSmem s;
  const int tid = threadIdx.x;
  const int64_t N = a.N;
  const int ring = a.ring;
  mlp_stage_net(a.net, D, A, s);
  const int64_t tiles = (N + kMlpRows - 1) / kMlpRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kMlpRows;
    __syncthreads();  // the previous tile is done with s
    for (int e = tid; e < kMlpRows * kMlpMaxD; e += kMlpThreads) {  // the acting observations, zero past N / D
      const int r = e / kMlpMaxD, k = e % kMlpMaxD;
      float v = 0.0f;
      if (r0 + r < N && k < D) v = a.obs_ring[((r0 + r) * ring + a.cur_slot[r0 + r]) * LD + k];
      s.x[r][k] = v;
    }
    mlp_forward_rows(s.x, D, A, s);
    if (a.q_out) mlp_store_q(s, a.q_out, N, r0, A);
    if (tid >= kMlpRows || r0 + tid >= N) continue;
    const int64_t i = r0 + tid;
    const int64_t t = a.t_dev[i] + 1;
    int64_t act;
    if (a.action_in) {
      act = a.action_in[i];
    } else {
      act = eps_explore_draw(i, A, a.eps[i], nullptr, nullptr, a.seed, (uint64_t)t);
      if (act < 0) act = argmax_first(s.q[tid], A);
    }
    double st[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) st[k] = a.state[i * 4 + k];
    const int steps = a.ep_steps[i] + 1;
    // (the running return is fetched with the state: after the ring stores below, which it may
    // alias for all the compiler knows, its latency would be the lane's own)
    double *rs = a.ret_stats ? a.ret_stats + i * 3 : nullptr;  // NULL for every lane or for none
    const double run = rs ? rs[0] : 0.0;
    float rew;
    const bool done = env_dynamics<ENV>(st, act, &rew) | (steps >= a.max_steps);
    const int64_t cur = a.cur_slot[i];
    const int64_t nxt = (2 * t) % ring, rst = (2 * t + 1) % ring;
    const int64_t s0h = i * ring + cur, s1h = i * ring + nxt;
    env_store_obs<ENV>(a.obs_ring + s1h * LD, st);  // the terminal observation when done
    const double ret = radd(run, (double)rew);
    if (done) {
      env_reset_draw<ENV>(a.seed, i, t, st);
      env_store_obs<ENV>(a.obs_ring + (i * ring + rst) * LD, st);
      a.stats[i * 3 + 0] += 1;
      a.stats[i * 3 + 1] += steps;
      a.stats[i * 3 + 2] = steps;
      if (rs) rs[1] = radd(rs[1], ret), rs[2] = ret;
    }
    if (rs) rs[0] = done ? 0.0 : ret;
#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[i * 4 + k] = st[k];
    a.ep_steps[i] = done ? 0 : steps;
    a.cur_slot[i] = done ? rst : nxt;
    a.t_dev[i] = t;
    a.action[i] = act;
    a.reward[i] = rew;
    a.done[i] = done ? 1.0f : 0.0f;
    a.s0_h[i] = s0h;
    a.s1_h[i] = s1h;
    nstep_push_one(a.ns, i, a.n, a.gamma, a.mode, s0h, act, rew, s1h, done ? 1.0f : 0.0f, a.emit, a.row_s0, a.row_a,
                   a.row_r, a.row_s1, a.row_done);
    if (a.emit[i]) {  // the emitted row by value: its observations out of the ring, dense [N, D]
      const float2 *o0 = reinterpret_cast<const float2 *>(a.obs_ring + a.row_s0[i] * LD);
      const float2 *o1 = reinterpret_cast<const float2 *>(a.obs_ring + a.row_s1[i] * LD);
      float2 v0[D / 2], v1[D / 2];  // every piece fetched before the first is stored: one round trip, not D
#pragma unroll
      for (int k = 0; k < D / 2; ++k) v0[k] = o0[k], v1[k] = o1[k];
#pragma unroll
      for (int k = 0; k < D / 2; ++k) {
        reinterpret_cast<float2 *>(a.row_obs0)[i * (D / 2) + k] = v0[k];
        reinterpret_cast<float2 *>(a.row_obs1)[i * (D / 2) + k] = v1[k];
      }
    }
  }
}

inline bool env_shape(int64_t env, int *D, int *A) {
  switch (env) {
    case RTH_ENV_CARTPOLE: *D = EnvSpec<RTH_ENV_CARTPOLE>::D, *A = EnvSpec<RTH_ENV_CARTPOLE>::A; return true;
    case RTH_ENV_ACROBOT: *D = EnvSpec<RTH_ENV_ACROBOT>::D, *A = EnvSpec<RTH_ENV_ACROBOT>::A; return true;
    case RTH_ENV_MOUNTAINCAR: *D = EnvSpec<RTH_ENV_MOUNTAINCAR>::D, *A = EnvSpec<RTH_ENV_MOUNTAINCAR>::A; return true;
    default: return false;
  }
}

// the argument checks of the entry points; `h`: the adder of a step (NULL for the reset);
// `want_ret`: ret_stats must be there (the CartPole adapters pass none)
inline const char *env_actor_check(const rth_env_actor_args *x, const rth_nstep *h, bool step, bool want_ret,
                                   EnvActor *out) {
  if (!x) return "NULL args";
  int D, A;
  if (!env_shape(x->env, &D, &A)) return "unknown env id (RTH_ENV_CARTPOLE, RTH_ENV_ACROBOT, RTH_ENV_MOUNTAINCAR)";
  if (!mlp_shape_ok(x->D, x->H, x->A) || x->D != D || x->A != A)
    return "the network shape is not the env's (H = 128; CartPole D = 4, A = 2; Acrobot D = 6, A = 3; "
           "MountainCar D = 2, A = 3)";
  if (x->N < 1 || x->N >= (int64_t(1) << 31)) return "bad N (1 <= N < 2^31)";
  if (x->ring < 4) return "bad ring (ring >= 4)";
  if (x->max_episode_steps < 1) return "bad max_episode_steps (>= 1)";
  if (!x->state || !x->ep_steps || !x->t_dev || !x->stats || (want_ret && !x->ret_stats) || !x->obs_ring ||
      !x->cur_slot)
    return "NULL state buffer";
  EnvActor a{};
  if (step) {
    if (!h) return "NULL adder handle";
    if (x->N != h->N) return "N differs from the adder's";
    if (x->ring < 2 * (h->n + 2)) return "bad ring (ring >= 2 (n_step + 2): an emitted row's observations must survive)";
    if (!dense_net(x->params, &a.net)) return "NULL network parameter";
    if (!x->eps || !x->action || !x->reward || !x->done || !x->s0_h || !x->s1_h || !x->emit || !x->row_s0 ||
        !x->row_a || !x->row_s1 || !x->row_r || !x->row_done || !x->row_obs0 || !x->row_obs1)
      return "NULL step buffer";
    if ((reinterpret_cast<uintptr_t>(x->row_obs0) | reinterpret_cast<uintptr_t>(x->row_obs1)) & 15)
      return "row_obs0 / row_obs1 must be 16-byte aligned";
    a.ns = h->st, a.n = h->n, a.gamma = h->gamma, a.mode = h->mode;
  }
  if (reinterpret_cast<uintptr_t>(x->obs_ring) & 15) return "obs_ring must be 16-byte aligned";
  a.state = x->state, a.ep_steps = x->ep_steps, a.t_dev = x->t_dev, a.stats = x->stats, a.ret_stats = x->ret_stats;
  a.obs_ring = x->obs_ring, a.cur_slot = x->cur_slot, a.eps = x->eps, a.action_in = x->action_in;
  a.action = x->action, a.reward = x->reward, a.done = x->done, a.s0_h = x->s0_h, a.s1_h = x->s1_h;
  a.emit = x->emit, a.row_s0 = x->row_s0, a.row_a = x->row_a, a.row_s1 = x->row_s1, a.row_r = x->row_r;
  a.row_done = x->row_done, a.row_obs0 = x->row_obs0, a.row_obs1 = x->row_obs1, a.q_out = x->q_out;
  a.seed = x->seed, a.N = x->N, a.ring = x->ring, a.max_steps = x->max_episode_steps;
  *out = a;
  return nullptr;
}

// the launch of an actor set's step kernel (workgroups of `Threads`, dense_grid over its N envs) or of
// its reset kernel (one lane per env); ddpg_actor.hpp launches through it too
template <auto Step, auto Reset, int Threads, class Actor>
inline void actor_launch(bool step, const Actor &a, hipStream_t st) {
  if (step)
    hipLaunchKernelGGL(Step, dim3(dense_grid(a.N)), dim3(Threads), 0, st, a);
  else
    hipLaunchKernelGGL(Reset, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, st, a);
}

template <int ENV>
inline void env_launch(bool step, const EnvActor &a, hipStream_t st) {
  actor_launch<k_env_actor_step<ENV>, k_env_reset<ENV>, kMlpThreads>(step, a, st);
}

// The body of the four entry points: the checks, then the env's step (with the adder `h`) or reset
// kernel.  `fn`: the entry point that was called, for its error messages.
inline int env_actor_run(const char *fn, const rth_nstep *h, const rth_env_actor_args *x, bool step, bool want_ret,
                         void *stream) {
  EnvActor a;
  const char *bad = env_actor_check(x, h, step, want_ret, &a);
  RTH_REQUIRE(!bad, "%s: %s", fn, bad);
  switch (x->env) {
    case RTH_ENV_CARTPOLE: env_launch<RTH_ENV_CARTPOLE>(step, a, as_stream(stream)); break;
    case RTH_ENV_ACROBOT: env_launch<RTH_ENV_ACROBOT>(step, a, as_stream(stream)); break;
    default: env_launch<RTH_ENV_MOUNTAINCAR>(step, a, as_stream(stream));
  }
  RTH_LAUNCHED();
  return RTH_OK;
}

}  // namespace rth

extern "C" {

int rth_env_reset(const rth_env_actor_args *args, void *stream) {
  return rth::env_actor_run("rth_env_reset", nullptr, args, false, true, stream);
}

int rth_env_actor_step(rth_nstep *h, const rth_env_actor_args *args, void *stream) {
  return rth::env_actor_run("rth_env_actor_step", h, args, true, true, stream);
}

}  // extern "C"
