// Device-resident vectorised CartPole actors on the fused MLP kernels: one launch per env step for
// N actors (rth_mlp_actor_step) -- the acting forward of mlp.hpp (mlp_forward_rows, the only
// forward: a row's Q equals rth_mlp_q's bit for bit), then one lane per env: ε-greedy with the
// draws of eps_greedy_one, gym's CartPole-v0/v1 dynamics in fp64 (envs.CartPole.step's operation
// order), the reset of a finished episode, the f32 observations into a per-env ring and the n-step
// push (nstep_push_one on an rth_nstep handle), the emitted row also by value.  No host
// synchronisation, no atomics: everything an env touches is private to its lane.
//
// Reference: reth/reth/presets/worker.py:128-155 (Worker.step: act, env.step, env.reset on done),
// utils/exploration.py:26-31, algorithm/dqn/dqn_solver.py:126-131,
// utils/nstep_adder.py:11-28.
//
// Step counter.  t_dev is int64 [N]: every env carries the (common) number of env steps taken and
// advances its own copy, t = t_dev[i] + 1, so the one launch needs no grid-wide agreement on who
// increments a scalar.  ε-greedy at step t draws with counter = t, lane = i (eps_explore_draw).
//
// Reset draws (rth_cartpole_reset at t = 0, and step t of an env whose episode ended at t): one
// Philox4x32-10 block per (seed, env i, t),
//     counter = {(uint32) i, (uint32) t, (uint32) (t >> 32), STREAM_CARTPOLE (= 7)}
//     key     = {(uint32) seed, (uint32) (seed >> 32)}
// and with the four output words c[k]:  state[k] = -0.05 + (0.1 * (double) c[k]) / 2^32  in fp64
// (each operation rounded once), a value in [-0.05, 0.05).  A pure function of (seed, i, t).
//
// Observation ring.  f32 [N * ring + 1, 4] (the last row: an all-zero sink the kernel never
// writes), env i's slot s at row i * ring + s = the handle.  Step t writes the next observation
// into slot (2t) % ring and, when the episode ended, the reset observation into (2t + 1) % ring;
// cur_slot[i] is the slot of the observation the env acts on next.  A done row's s1 is the
// terminal observation.  An emitted n-step row references slots written at most n + 1 steps
// earlier, so ring >= 2 (n + 2) keeps them intact for the by-value copy.
#pragma once
#include "actor_shared.hpp"
#include "mlp.hpp"

namespace rth {

constexpr uint32_t STREAM_CARTPOLE = 7u;
constexpr int kCartD = 4, kCartA = 2;

struct MlpActor {
  MlpNet net;
  double *state;
  int32_t *ep_steps;
  int64_t *t_dev, *stats;
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

__device__ inline void cartpole_reset_draw(uint64_t seed, int64_t i, int64_t t, double (&s)[4]) {
  uint32_t c[4] = {(uint32_t)i, (uint32_t)t, (uint32_t)((uint64_t)t >> 32), STREAM_CARTPOLE};
  philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = radd(-0.05, rmul(0.1, (double)c[k]) / 4294967296.0);
}

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

__global__ __launch_bounds__(256) void k_cartpole_reset(MlpActor a) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  double s[4];
  cartpole_reset_draw(a.seed, i, 0, s);
#pragma unroll
  for (int k = 0; k < 4; ++k) a.state[i * 4 + k] = s[k];
  a.ep_steps[i] = 0;
  a.t_dev[i] = 0;
#pragma unroll
  for (int k = 0; k < 3; ++k) a.stats[i * 3 + k] = 0;
  reinterpret_cast<float4 *>(a.obs_ring)[i * a.ring + 1] = cartpole_obs(s);
  a.cur_slot[i] = 1;
}

__global__ __launch_bounds__(kMlpThreads) void k_mlp_actor_step(MlpActor a) {
  __shared__ __align__(16) MlpSmem s;
  const int tid = threadIdx.x;
  const int64_t N = a.N;
  const int ring = a.ring;
  mlp_stage_net(a.net, kCartD, kCartA, s);
  float4 *ring4 = reinterpret_cast<float4 *>(a.obs_ring);
  const int64_t tiles = (N + kMlpRows - 1) / kMlpRows;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const int64_t r0 = tile * kMlpRows;
    __syncthreads();  // the previous tile is done with s
    for (int e = tid; e < kMlpRows * kMlpMaxD; e += kMlpThreads) {  // the acting observations, zero past N / D
      const int r = e / kMlpMaxD, k = e % kMlpMaxD;
      float v = 0.0f;
      if (r0 + r < N && k < kCartD) v = a.obs_ring[((r0 + r) * ring + a.cur_slot[r0 + r]) * kCartD + k];
      s.x[r][k] = v;
    }
    mlp_forward_rows(s.x, kCartD, kCartA, s);
    if (a.q_out) mlp_store_q(s, a.q_out, N, r0, kCartA);
    if (tid >= kMlpRows || r0 + tid >= N) continue;
    const int64_t i = r0 + tid;
    const int64_t t = a.t_dev[i] + 1;
    int64_t act;
    if (a.action_in) {
      act = a.action_in[i];
    } else {
      act = eps_explore_draw(i, kCartA, a.eps[i], nullptr, nullptr, a.seed, (uint64_t)t);
      if (act < 0) act = argmax_first(s.q[tid], kCartA);
    }
    double st[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) st[k] = a.state[i * 4 + k];
    const int steps = a.ep_steps[i] + 1;
    const bool done = cartpole_dynamics(st, act) | (steps >= a.max_steps);
    const int64_t cur = a.cur_slot[i];
    const int64_t nxt = (2 * t) % ring, rst = (2 * t + 1) % ring;
    const int64_t s0h = i * ring + cur, s1h = i * ring + nxt;
    ring4[s1h] = cartpole_obs(st);  // the terminal observation when done
    if (done) {
      cartpole_reset_draw(a.seed, i, t, st);
      ring4[i * ring + rst] = cartpole_obs(st);
      a.stats[i * 3 + 0] += 1;
      a.stats[i * 3 + 1] += steps;
      a.stats[i * 3 + 2] = steps;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a.state[i * 4 + k] = st[k];
    a.ep_steps[i] = done ? 0 : steps;
    a.cur_slot[i] = done ? rst : nxt;
    a.t_dev[i] = t;
    a.action[i] = act;
    a.reward[i] = 1.0f;
    a.done[i] = done ? 1.0f : 0.0f;
    a.s0_h[i] = s0h;
    a.s1_h[i] = s1h;
    nstep_push_one(a.ns, i, a.n, a.gamma, a.mode, s0h, act, 1.0f, s1h, done ? 1.0f : 0.0f, a.emit, a.row_s0, a.row_a,
                   a.row_r, a.row_s1, a.row_done);
    if (a.emit[i]) {  // the emitted row by value: its observations out of the ring
      reinterpret_cast<float4 *>(a.row_obs0)[i] = ring4[a.row_s0[i]];
      reinterpret_cast<float4 *>(a.row_obs1)[i] = ring4[a.row_s1[i]];
    }
  }
}

// the argument checks of both entry points; `h`: the adder of a step (NULL for the reset)
inline const char *mlp_actor_check(const rth_mlp_actor_args *x, const rth_nstep *h, bool step, MlpActor *out) {
  if (!x) return "NULL args";
  if (!mlp_shape_ok(x->D, x->H, x->A) || x->D != kCartD || x->A != kCartA)
    return "unsupported network shape (CartPole: D = 4, H = 128, A = 2)";
  if (x->N < 1 || x->N >= (int64_t(1) << 31)) return "bad N (1 <= N < 2^31)";
  if (x->ring < 4) return "bad ring (ring >= 4)";
  if (x->max_episode_steps < 1) return "bad max_episode_steps (>= 1)";
  if (!x->state || !x->ep_steps || !x->t_dev || !x->stats || !x->obs_ring || !x->cur_slot) return "NULL state buffer";
  MlpActor a{};
  if (step) {
    if (!h) return "NULL adder handle";
    if (x->N != h->N) return "N differs from the adder's";
    if (x->ring < 2 * (h->n + 2)) return "bad ring (ring >= 2 (n_step + 2): an emitted row's observations must survive)";
    if (!mlp_net(x->params, &a.net)) return "NULL network parameter";
    if (!x->eps || !x->action || !x->reward || !x->done || !x->s0_h || !x->s1_h || !x->emit || !x->row_s0 ||
        !x->row_a || !x->row_s1 || !x->row_r || !x->row_done || !x->row_obs0 || !x->row_obs1)
      return "NULL step buffer";
    if ((reinterpret_cast<uintptr_t>(x->row_obs0) | reinterpret_cast<uintptr_t>(x->row_obs1)) & 15)
      return "row_obs0 / row_obs1 must be 16-byte aligned";
    a.ns = h->st, a.n = h->n, a.gamma = h->gamma, a.mode = h->mode;
  }
  if (reinterpret_cast<uintptr_t>(x->obs_ring) & 15) return "obs_ring must be 16-byte aligned";
  a.state = x->state, a.ep_steps = x->ep_steps, a.t_dev = x->t_dev, a.stats = x->stats;
  a.obs_ring = x->obs_ring, a.cur_slot = x->cur_slot, a.eps = x->eps, a.action_in = x->action_in;
  a.action = x->action, a.reward = x->reward, a.done = x->done, a.s0_h = x->s0_h, a.s1_h = x->s1_h;
  a.emit = x->emit, a.row_s0 = x->row_s0, a.row_a = x->row_a, a.row_s1 = x->row_s1, a.row_r = x->row_r;
  a.row_done = x->row_done, a.row_obs0 = x->row_obs0, a.row_obs1 = x->row_obs1, a.q_out = x->q_out;
  a.seed = x->seed, a.N = x->N, a.ring = x->ring, a.max_steps = x->max_episode_steps;
  *out = a;
  return nullptr;
}

}  // namespace rth

extern "C" {

int rth_cartpole_reset(const rth_mlp_actor_args *args, void *stream) {
  using namespace rth;
  MlpActor a;
  const char *bad = mlp_actor_check(args, nullptr, false, &a);
  RTH_REQUIRE(!bad, "rth_cartpole_reset: %s", bad);
  hipLaunchKernelGGL(k_cartpole_reset, dim3((unsigned)((a.N + 255) / 256)), dim3(256), 0, as_stream(stream), a);
  RTH_LAUNCHED();
  return RTH_OK;
}

int rth_mlp_actor_step(rth_nstep *h, const rth_mlp_actor_args *args, void *stream) {
  using namespace rth;
  MlpActor a;
  const char *bad = mlp_actor_check(args, h, true, &a);
  RTH_REQUIRE(!bad, "rth_mlp_actor_step: %s", bad);
  const int64_t tiles = (a.N + kMlpRows - 1) / kMlpRows;
  hipLaunchKernelGGL(k_mlp_actor_step, dim3((unsigned)(tiles < kMlpMaxBlocks ? tiles : kMlpMaxBlocks)),
                     dim3(kMlpThreads), 0, as_stream(stream), a);
  RTH_LAUNCHED();
  return RTH_OK;
}

}  // extern "C"
