// PPO's two networks (ppo_model.py:6-40: actor Linear(D,64) -> tanh -> Linear(64,64) -> tanh ->
// Linear(64,A) -> softmax; value Linear(D,64) -> tanh -> Linear(64,64) -> tanh -> Linear(64,1)) as
// fused fp32 kernels: rth_ppo_act (the actor forward, the log-softmax and one Categorical draw per
// row, one launch) and rth_ppo_grads (one epoch of ppo_solver.py:72-96 for both networks: two
// forwards, ratio, clipped surrogate, entropy, the squared value error and the backward through
// both networks, two launches).
//
// At H = 64 a network is at most 41 KB of fp32 (D = 64, A = 18; 19 KB at CartPole's D = 4): a
// workgroup stages the actor -- rth_ppo_grads: the actor and the value network, side by side -- in
// LDS once, as mlp.hpp does (row stride 68 floats), and walks tiles of kPpoRows rows; a forward's
// only round trip to L2 / HBM is its input rows.  Lane j = tid % 64 owns a hidden unit, tid / 64
// picks 2 of the tile's 8 rows.  Every product is one fmaf, a dot product has dense.hpp's ONE
// summation order, then the bias -- but the last layer's 64 products are summed in fp64 and the logit
// (or value) rounded once; tanh, exp and log are evaluated in fp64 and rounded once
// (ddpg.hpp's precedent).  ppo_forward_rows is the only forward and ppo_log_softmax the only
// log-softmax, so a row's log-probability does not depend on n, on its position, on the row
// stride or on the entry point.  The batch sums (weight and bias gradients, the mean squared
// value error, the loss mean) are the second launch, with dense.hpp's functions in its order
// (gradients: per chunk of 128 rows, the chunks' sums added in fp64 -- ppo_wgrad_tile): no atomics.
// rth_ppo_grads_adv is rth_ppo_grads with the surrogate's advantage as an input (GAE:
// ppo_actor.hpp's rth_ppo_gae_finish) and rth_ppo_adv_normalize normalises such a column in place.
// ppo_shuffle.hpp's rth_ppo_shuffle lays a batch out as K shuffled minibatches, each of which goes
// through rth_ppo_grads_n / rth_ppo_grads_adv as a batch of its own.
#pragma once
#include "dense.hpp"

namespace rth {

constexpr uint32_t STREAM_PPO = 13u;  // the Categorical draw's Philox stream word
constexpr int kPpoH = 64, kPpoMaxD = kDenseMaxD, kPpoMinA = 2, kPpoMaxA = 18;
constexpr int kPpoRows = kDenseRows;        // rows per tile
constexpr int kPpoThreads = kDenseThreads;  // lane j = tid % 64: hidden unit; tid / 64: which 2 of the tile's rows
constexpr int kPpoRpt = kPpoRows / (kPpoThreads / kPpoH);
constexpr int kPpoLdw = kPpoH + 4;     // LDS row stride of a staged weight (layer 1: columns [D, round-up-8(D)) zero)
constexpr int kPpoLdA = kPpoMaxA + 2;  // ... of a tile's per-action rows
static_assert(kPpoRows * kPpoMaxA <= kPpoThreads, "one lane per (row, action)");
static_assert(kPpoMaxD <= kPpoH, "layer 1's staged row stride");

struct PpoNetSmem {  // a staged network
  float w1[kPpoH * kPpoLdw];
  float w2[kPpoH * kPpoLdw];
  float w3[kPpoMaxA * kPpoLdw];
  float b1[kPpoH], b2[kPpoH], b3[kPpoLdA];
};

struct PpoRows {  // a tile's rows through one network
  float h1[kPpoRows][kPpoH];
  float h2[kPpoRows][kPpoH];
  float g2[kPpoRows][kPpoH];  // d(loss)/d(layer 2's pre-activation)
  float z[kPpoRows][kPpoLdA];  // the last layer's output: logits, or the state value in column 0
};

struct PpoDist {  // a tile's Categorical rows
  double e[kPpoRows][kPpoLdA];  // exp(z - max z)
  float logp[kPpoRows][kPpoLdA];
  float p[kPpoRows][kPpoLdA];
  float g3[kPpoRows][kPpoLdA];  // d(loss)/d(logits)
  float k[kPpoRows], ent[kPpoRows], gv[kPpoRows];  // the surrogate's factor, the entropy, d(loss)/d(value)
  int act[kPpoRows];                               // the row's action; -1: a row past B
};

struct PpoActSmem {
  PpoNetSmem actor;
  PpoRows ra;
  PpoDist dist;
  float x[kPpoRows][kPpoMaxD];
};

struct PpoGradSmem {
  PpoNetSmem actor, value;
  PpoRows ra, rv;
  PpoDist dist;
  float x[kPpoRows][kPpoMaxD];
};

// rth_ppo_grads' workspace, in floats from its start: the new log-probabilities first
struct PpoWs {
  float *logp, *le, *se, *gv, *g3, *ah1, *ah2, *ag1, *ag2, *vh1, *vh2, *vg1, *vg2;
  __host__ __device__ PpoWs(float *p, int64_t B, int A) {
    logp = p, le = logp + B, se = le + B, gv = se + B, g3 = gv + B;
    ah1 = g3 + B * A, ah2 = ah1 + B * kPpoH, ag1 = ah2 + B * kPpoH, ag2 = ag1 + B * kPpoH;
    vh1 = ag2 + B * kPpoH, vh2 = vh1 + B * kPpoH, vg1 = vh2 + B * kPpoH, vg2 = vg1 + B * kPpoH;
  }
  static int64_t floats(int64_t B, int64_t A) { return B * (4 + A + 8 * kPpoH); }
};

// the rows of a batch of capacity `cap`: all of them, or the device's count n_dev[0] clamped to [0, cap]
__device__ __forceinline__ int64_t ppo_rows(int64_t cap, const int64_t *__restrict__ n_dev) {
  if (!n_dev) return cap;
  const int64_t n = *n_dev;
  return n < 0 ? 0 : (n < cap ? n : cap);
}

// a network's parameters (N3 rows in its last layer) into LDS; the caller synchronises before they are read
__device__ inline void ppo_stage_net(const DenseNet &p, int D, int N3, PpoNetSmem &s) {
  const int tid = threadIdx.x;
  const int D8 = (D + 7) & ~7;
#pragma unroll 4
  for (int i = tid; i < kPpoH * D8; i += kPpoThreads) {
    const int j = i / D8, k = i - j * D8;
    s.w1[j * kPpoLdw + k] = k < D ? p.w1[j * D + k] : 0.0f;
  }
#pragma unroll 8
  for (int i = tid; i < kPpoH * kPpoH; i += kPpoThreads) s.w2[(i >> 6) * kPpoLdw + (i & (kPpoH - 1))] = p.w2[i];
  for (int i = tid; i < N3 * kPpoH; i += kPpoThreads) s.w3[(i >> 6) * kPpoLdw + (i & (kPpoH - 1))] = p.w3[i];
  if (tid < kPpoH) {
    s.b1[tid] = p.b1[tid];
    s.b2[tid] = p.b2[tid];
  }
  if (tid < N3) s.b3[tid] = p.b3[tid];
}

__device__ __forceinline__ float ppo_tanh(float v) { return (float)tanh((double)v); }  // fp64, rounded once

// The forward of the kPpoRows rows in xs (dense_load_x) through the net staged in w: o.h1 / o.h2 =
// the hidden activations, o.z[r][0..N3) = the last layer.  Starts and ends with a workgroup barrier.
__device__ inline void ppo_forward_rows(const PpoNetSmem &w, const float (*xs)[kPpoMaxD], int D, int N3, PpoRows &o) {
  const int tid = threadIdx.x, j = tid & (kPpoH - 1), rb = (tid >> 6) * kPpoRpt;
  __syncthreads();
  {  // layer 1: hidden unit j of kPpoRpt rows
    float acc[kPpoRpt][8] = {};
    const float *wr = w.w1 + j * kPpoLdw;
    for (int k0 = 0; k0 < D; k0 += 8) {
      const float4 wa = *reinterpret_cast<const float4 *>(wr + k0);
      const float4 wb = *reinterpret_cast<const float4 *>(wr + k0 + 4);
#pragma unroll
      for (int rr = 0; rr < kPpoRpt; ++rr) {
        const float4 xa = *reinterpret_cast<const float4 *>(&xs[rb + rr][k0]);
        const float4 xb = *reinterpret_cast<const float4 *>(&xs[rb + rr][k0 + 4]);
        dense_fma8(xa, xb, wa, wb, acc[rr]);
      }
    }
    const float b = w.b1[j];
#pragma unroll
    for (int rr = 0; rr < kPpoRpt; ++rr) o.h1[rb + rr][j] = ppo_tanh(radd(dense_tree8(acc[rr]), b));
  }
  __syncthreads();
  {  // layer 2
    float acc[kPpoRpt][8] = {};
    const float *wr = w.w2 + j * kPpoLdw;
#pragma unroll 2
    for (int k0 = 0; k0 < kPpoH; k0 += 8) {
      const float4 wa = *reinterpret_cast<const float4 *>(wr + k0);
      const float4 wb = *reinterpret_cast<const float4 *>(wr + k0 + 4);
#pragma unroll
      for (int rr = 0; rr < kPpoRpt; ++rr) {
        const float4 xa = *reinterpret_cast<const float4 *>(&o.h1[rb + rr][k0]);
        const float4 xb = *reinterpret_cast<const float4 *>(&o.h1[rb + rr][k0 + 4]);
        dense_fma8(xa, xb, wa, wb, acc[rr]);
      }
    }
    const float b = w.b2[j];
#pragma unroll
    for (int rr = 0; rr < kPpoRpt; ++rr) o.h2[rb + rr][j] = ppo_tanh(radd(dense_tree8(acc[rr]), b));
  }
  __syncthreads();
  if (tid < kPpoRows * N3) {  // layer 3: one lane per (row, output)
    // A trained policy's last weights are large: its logits reach the hundreds, and what an fp32 sum
    // of the 64 products loses there (a spacing or two of a logit) goes whole into the
    // log-probability and, times rho |adv|, into the loss.  The products are exact in fp64: summed
    // there in increasing k, then the bias, the logit is rounded once.
    const int r = tid / N3, a = tid % N3;
    double acc = 0.0;
    const float *wr = w.w3 + a * kPpoLdw;
#pragma unroll 2
    for (int k0 = 0; k0 < kPpoH; k0 += 4) {
      const float4 wa = *reinterpret_cast<const float4 *>(wr + k0);
      const float4 xa = *reinterpret_cast<const float4 *>(&o.h2[r][k0]);
      acc = fma((double)xa.x, (double)wa.x, acc);
      acc = fma((double)xa.y, (double)wa.y, acc);
      acc = fma((double)xa.z, (double)wa.z, acc);
      acc = fma((double)xa.w, (double)wa.w, acc);
    }
    o.z[r][a] = (float)(acc + (double)w.b3[a]);
  }
  __syncthreads();
}

// The log-softmax of the tile's logits z (behind a barrier): with m = max_j z_j (exact) and, in
// fp64, s = sum_j exp(z_j - m) in increasing j: logp_j = fl32((z_j - m) - log s), p_j =
// fl32(exp(logp_j)).  One lane per (row, action).  Ends with a workgroup barrier.
__device__ inline void ppo_log_softmax(const float (*z)[kPpoLdA], int A, PpoDist &d) {
  const int tid = threadIdx.x, r = tid / A, j = tid % A;
  const bool lane = tid < kPpoRows * A;
  double dz = 0.0;
  if (lane) {
    float m = z[r][0];
    for (int i = 1; i < A; ++i) m = z[r][i] > m ? z[r][i] : m;
    dz = (double)z[r][j] - (double)m;
    d.e[r][j] = exp(dz);
  }
  __syncthreads();
  if (lane) {
    double s = 0.0;
    for (int i = 0; i < A; ++i) s += d.e[r][i];
    const float lp = (float)(dz - log(s));
    d.logp[r][j] = lp;
    d.p[r][j] = (float)exp((double)lp);
  }
  __syncthreads();
}

// dense_load_x into x behind a barrier (the previous tile is done with the LDS rows)
__device__ inline void ppo_load_tile(const float *__restrict__ x, int64_t ldx, int64_t n, int64_t r0, int D,
                                     float (*xs)[kPpoMaxD]) {
  __syncthreads();
  dense_load_x(x, ldx, n, r0, D, xs);
}

// The Categorical draw, the only one: the inverse CDF over the running fp32 sum of a row's
// probabilities -- the first j with c_j > u, c_j = fl32(c_{j-1} + p_j), or A - 1 if there is none
__device__ __forceinline__ int ppo_inverse_cdf(const float *p, int A, double u) {
  float c = 0.0f;
  for (int j = 0; j < A; ++j) {
    c = radd(c, p[j]);
    if ((double)c > u) return j;
  }
  return A - 1;
}

__global__ __launch_bounds__(kPpoThreads) void k_ppo_act(DenseNet p, const float *__restrict__ x, int64_t ldx,
                                                         int64_t n, int D, int A, const double *__restrict__ uniforms,
                                                         uint64_t seed, uint64_t counter, int64_t *__restrict__ action,
                                                         float *__restrict__ logprob, float *__restrict__ probs) {
  __shared__ __align__(16) PpoActSmem s;
  const int tid = threadIdx.x;
  ppo_stage_net(p, D, A, s.actor);
  const int64_t tiles = (n + kPpoRows - 1) / kPpoRows;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * kPpoRows;
    ppo_load_tile(x, ldx, n, r0, D, s.x);
    ppo_forward_rows(s.actor, s.x, D, A, s.ra);
    ppo_log_softmax(s.ra.z, A, s.dist);
    if (tid < kPpoRows && r0 + tid < n) {
      const int64_t row = r0 + tid;
      const double u = uniforms ? uniforms[row] : philox_uniform(seed, counter, (uint32_t)row, STREAM_PPO);
      const int a = ppo_inverse_cdf(s.dist.p[tid], A, u);
      action[row] = a;
      logprob[row] = s.dist.logp[tid][a];
    }
    if (probs && tid < kPpoRows * A) {
      const int r = tid / A, j = tid % A;
      if (r0 + r < n) probs[(r0 + r) * A + j] = s.dist.p[r][j];
    }
  }
}

// layer 2's data gradient of one network down its staged weight's columns, g1 = (1 - h1^2) g2 W2,
// and the tile's activations and pre-activation gradients to the workspace (rows r0 + r < B only)
__device__ inline void ppo_dgrad_store(const PpoNetSmem &w, const PpoRows &o, float *__restrict__ h1,
                                       float *__restrict__ h2, float *__restrict__ g1, float *__restrict__ g2,
                                       int64_t r0, int64_t B) {
  const int tid = threadIdx.x, j = tid & (kPpoH - 1), rb = (tid >> 6) * kPpoRpt;
  float acc[kPpoRpt][8] = {};
#pragma unroll 2
  for (int j0 = 0; j0 < kPpoH; j0 += 8) {
    float wv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) wv[i] = w.w2[(j0 + i) * kPpoLdw + j];
    const float4 wa = make_float4(wv[0], wv[1], wv[2], wv[3]), wb = make_float4(wv[4], wv[5], wv[6], wv[7]);
#pragma unroll
    for (int rr = 0; rr < kPpoRpt; ++rr) {
      const float4 ga = *reinterpret_cast<const float4 *>(&o.g2[rb + rr][j0]);
      const float4 gb = *reinterpret_cast<const float4 *>(&o.g2[rb + rr][j0 + 4]);
      dense_fma8(ga, gb, wa, wb, acc[rr]);
    }
  }
#pragma unroll
  for (int rr = 0; rr < kPpoRpt; ++rr) {
    const int r = rb + rr;
    if (r0 + r < B) {
      const int64_t i = (r0 + r) * kPpoH + j;
      const float h = o.h1[r][j];
      g1[i] = rmul(dense_tree8(acc[rr]), rsub(1.0f, rmul(h, h)));
      g2[i] = o.g2[r][j];
      h2[i] = o.h2[r][j];
      h1[i] = h;
    }
  }
}

// rth_ppo_grads' first launch.  Per tile of rows: the actor's and the value network's forward,
// the log-softmax, then per row ppo_solver.py:79-91 -- ratio, advantage, the clipped surrogate, the
// entropy, the squared value error -- and, backward, d(mean loss)/d(logits), d/d(value) and both
// networks' data gradients; activations and pre-activation gradients go to the workspace for the
// second launch, which also finishes the per-row loss (the mean squared error is a batch scalar).
// `cap` lays the workspace out; the batch is its first ppo_rows(cap, n_dev) rows.
__global__ __launch_bounds__(kPpoThreads) void k_ppo_tile(DenseNet ac, DenseNet va, const float *__restrict__ st,
                                                          int64_t lds, const int64_t *__restrict__ act,
                                                          const float *__restrict__ ret,
                                                          const float *__restrict__ advp,
                                                          const float *__restrict__ old_logp, int64_t cap,
                                                          const int64_t *__restrict__ n_dev, int D, int A,
                                                          float clip_lo, float clip_hi, float vf_coef, float ent_coef,
                                                          int backward, float *__restrict__ wsp) {
  __shared__ __align__(16) PpoGradSmem s;
  const PpoWs ws(wsp, cap, A);
  const int64_t B = ppo_rows(cap, n_dev);
  const int tid = threadIdx.x, j = tid & (kPpoH - 1), rb = (tid >> 6) * kPpoRpt;
  const int64_t tiles = (B + kPpoRows - 1) / kPpoRows;
  if ((int64_t)blockIdx.x >= tiles) return;  // (uniform) no tile: nothing to stage the weights for
  const float invB = 1.0f / (float)B;
  ppo_stage_net(ac, D, A, s.actor);
  ppo_stage_net(va, D, 1, s.value);
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * kPpoRows;
    ppo_load_tile(st, lds, B, r0, D, s.x);
    ppo_forward_rows(s.actor, s.x, D, A, s.ra);
    ppo_forward_rows(s.value, s.x, D, 1, s.rv);
    ppo_log_softmax(s.ra.z, A, s.dist);
    if (tid < kPpoRows) {
      const int64_t b = r0 + tid;
      if (b < B) {
        const int64_t a64 = act[b];
        const int a = a64 < 0 ? 0 : (a64 >= A ? A - 1 : (int)a64);  // (an action outside [0, A) reads in bounds)
        const float lp = s.dist.logp[tid][a];
        const float v = s.rv.z[tid][0], rt = ret[b];
        const float adv = advp ? advp[b] : rsub(rt, v);  // rth_ppo_grads_adv: the advantage as given
        const float rho = (float)exp((double)lp - (double)old_logp[b]);
        const float rc = rho < clip_lo ? clip_lo : (rho > clip_hi ? clip_hi : rho);
        const float s1 = rmul(rho, adv), s2 = rmul(rc, adv);
        const float mn = s2 < s1 ? s2 : s1;
        double h = 0.0;
        for (int i = 0; i < A; ++i) h -= (double)s.dist.p[tid][i] * (double)s.dist.logp[tid][i];
        const float ent = (float)h;
        const float dv = rsub(v, rt);
        ws.logp[b] = lp;
        ws.le[b] = rsub(-mn, rmul(ent_coef, ent));
        ws.se[b] = rmul(dv, dv);
        // autograd through min and clamp: the unclipped term where it is the smaller, or rho is not clipped
        s.dist.k[tid] = (s1 < s2 || (rho >= clip_lo && rho <= clip_hi)) ? -s1 : 0.0f;
        s.dist.ent[tid] = ent;
        s.dist.gv[tid] = rmul(rmul(rmul(2.0f, vf_coef), dv), invB);
        s.dist.act[tid] = a;
      } else {
        s.dist.k[tid] = s.dist.ent[tid] = s.dist.gv[tid] = 0.0f;
        s.dist.act[tid] = -1;
      }
    }
    if (!backward) continue;
    __syncthreads();
    if (tid < kPpoRows * A) {  // d(mean loss)/d(logits) = (1/B) [k (onehot(a) - p) + ent_coef p (logp + H)]
      const int r = tid / A, i = tid % A;
      const float p = s.dist.p[r][i];
      const float t1 = rmul(s.dist.k[r], rsub(i == s.dist.act[r] ? 1.0f : 0.0f, p));
      const float t2 = rmul(rmul(ent_coef, p), radd(s.dist.logp[r][i], s.dist.ent[r]));
      const float g = s.dist.act[r] >= 0 ? rmul(invB, radd(t1, t2)) : 0.0f;
      s.dist.g3[r][i] = g;
      if (r0 + r < B) ws.g3[(r0 + r) * A + i] = g;
    }
    if (tid < kPpoRows && r0 + tid < B) ws.gv[r0 + tid] = s.dist.gv[tid];
    __syncthreads();
    // layer 3's data gradients through tanh: g2 = (1 - h2^2) (g3 W3)
#pragma unroll
    for (int rr = 0; rr < kPpoRpt; ++rr) {
      const int r = rb + rr;
      float acc = 0.0f;
      for (int a = 0; a < A; ++a) acc = fmaf(s.dist.g3[r][a], s.actor.w3[a * kPpoLdw + j], acc);
      const float ha = s.ra.h2[r][j], hv = s.rv.h2[r][j];
      s.ra.g2[r][j] = rmul(acc, rsub(1.0f, rmul(ha, ha)));
      s.rv.g2[r][j] = rmul(rmul(s.dist.gv[r], s.value.w3[j]), rsub(1.0f, rmul(hv, hv)));
    }
    __syncthreads();
    ppo_dgrad_store(s.actor, s.ra, ws.ah1, ws.ah2, ws.ag1, ws.ag2, r0, B);
    ppo_dgrad_store(s.value, s.rv, ws.vh1, ws.vh2, ws.vg1, ws.vg2, r0, B);
  }
}

// The batch sums of the second launch.  PPO's batches are thousands of rows, and dense.hpp's order
// (row b to accumulator b % 4) is a serial fp32 chain of B / 4 additions per accumulator, whose
// rounding error grows with B: at B = 8,200 it is several 1e-6 of the largest gradient element.
// So the batch is summed in chunks of kPpoChunk rows, each chunk by dense.hpp's function in its
// order (a chain of 32), and the chunks' sums are added in increasing order in fp64 and rounded
// once; B <= kPpoChunk is dense.hpp's order itself.  A lane reads back only what it wrote itself
// (the chunk's sum, parked in the gradient element it finally overwrites): no barrier, no atomics.
// B = 0 (a device-counted batch without rows) writes zeros.
constexpr int kPpoChunk = 128;

__device__ inline void ppo_wgrad_tile(const float *__restrict__ G, int64_t ldg, int N, const float *__restrict__ X,
                                      int64_t ldx, int K, int64_t B, int n0, float *gw) {
  const int k = (int)threadIdx.x;
  if (B == 0) return dense_wgrad_tile(G, ldg, N, X, ldx, K, 0, n0, 0, gw);
  double acc[kDenseGradJ] = {};
  for (int64_t c0 = 0; c0 < B; c0 += kPpoChunk) {
    const int64_t nb = B - c0 < kPpoChunk ? B - c0 : kPpoChunk;
    dense_wgrad_tile(G + c0 * ldg, ldg, N, X + c0 * ldx, ldx, K, nb, n0, 0, gw);
    if (B <= kPpoChunk || k >= K) continue;
#pragma unroll
    for (int i = 0; i < kDenseGradJ; ++i)
      if (n0 + i < N) acc[i] += (double)*(volatile const float *)&gw[(int64_t)(n0 + i) * K + k];
  }
  if (B <= kPpoChunk || k >= K) return;
#pragma unroll
  for (int i = 0; i < kDenseGradJ; ++i)
    if (n0 + i < N) gw[(int64_t)(n0 + i) * K + k] = (float)acc[i];
}

__device__ inline void ppo_bgrad(const float *__restrict__ G, int64_t ldg, int N, int64_t B, float *gb) {
  const int n = (int)threadIdx.x;
  if (B == 0) return dense_bgrad(G, ldg, N, 0, 0, gb);
  double acc = 0.0;
  for (int64_t c0 = 0; c0 < B; c0 += kPpoChunk) {
    const int64_t nb = B - c0 < kPpoChunk ? B - c0 : kPpoChunk;
    dense_bgrad(G + c0 * ldg, ldg, N, nb, 0, gb);
    if (B > kPpoChunk && n < N) acc += (double)*(volatile const float *)&gb[n];
  }
  if (B > kPpoChunk && n < N) gb[n] = (float)acc;
}

// the second launch's workgroups per network: 16 for the middle layer's weight gradient, 16 for the
// first layer's, ceil(N3 / 4) for the last layer's and three for the bias gradients; after both
// networks, one workgroup for the losses
constexpr int kPpoWT = kPpoH / kDenseGradJ;
inline __host__ __device__ int ppo_net_blocks(int N3) { return 2 * kPpoWT + (N3 + kDenseGradJ - 1) / kDenseGradJ + 3; }

__device__ inline void ppo_net_wgrad(int blk, const DenseGrads &g, const float *__restrict__ st, int64_t lds, int64_t B,
                                     int D, int N3, const float *h1, const float *h2, const float *g1, const float *g2,
                                     const float *g3) {
  const int n_tiles = (N3 + kDenseGradJ - 1) / kDenseGradJ;
  if (blk < kPpoWT) return ppo_wgrad_tile(g2, kPpoH, kPpoH, h1, kPpoH, kPpoH, B, blk * kDenseGradJ, g.w2);
  blk -= kPpoWT;
  if (blk < kPpoWT) return ppo_wgrad_tile(g1, kPpoH, kPpoH, st, lds, D, B, blk * kDenseGradJ, g.w1);
  blk -= kPpoWT;
  if (blk < n_tiles) return ppo_wgrad_tile(g3, N3, N3, h2, kPpoH, kPpoH, B, blk * kDenseGradJ, g.w3);
  blk -= n_tiles;
  if (blk == 0) return ppo_bgrad(g1, kPpoH, kPpoH, B, g.b1);
  if (blk == 1) return ppo_bgrad(g2, kPpoH, kPpoH, B, g.b2);
  ppo_bgrad(g3, N3, N3, B, g.b3);
}

// rth_ppo_grads' second launch: the batch reductions of both networks, then the loss workgroup:
// mse = (1/B) sum_b (v_b - ret_b)^2, loss_b = le_b + vf_coef mse, |loss_b| and the mean of loss_b
// as (1/B) sum_b le_b + vf_coef mse.  Without gradients only the loss workgroup runs (first = its index).
// B = ppo_rows(cap, n_dev) as in the first launch; B = 0: zero gradients and a zero loss mean.
__global__ __launch_bounds__(kDenseGradThreads) void k_ppo_wgrad(DenseGrads ga, DenseGrads gv,
                                                                const float *__restrict__ st, int64_t lds, int64_t cap,
                                                                const int64_t *__restrict__ n_dev, int D, int A,
                                                                float vf_coef, float *__restrict__ wsp,
                                                                float *__restrict__ loss_abs,
                                                                float *__restrict__ loss_mean, int first) {
  __shared__ float part[kDenseGradThreads];
  const PpoWs ws(wsp, cap, A);
  const int64_t B = ppo_rows(cap, n_dev);
  int blk = (int)blockIdx.x + first;
  const int na = ppo_net_blocks(A), nv = ppo_net_blocks(1);
  if (blk < na) return ppo_net_wgrad(blk, ga, st, lds, B, D, A, ws.ah1, ws.ah2, ws.ag1, ws.ag2, ws.g3);
  blk -= na;
  if (blk < nv) return ppo_net_wgrad(blk, gv, st, lds, B, D, 1, ws.vh1, ws.vh2, ws.vg1, ws.vg2, ws.gv);
  const float invB = B ? 1.0f / (float)B : 0.0f;
  const float vmse = rmul(vf_coef, rmul(dense_loss_sum(ws.se, B, part), invB));
  __syncthreads();  // every lane has read the sum before `part` is used again
  for (int64_t b = threadIdx.x; b < B; b += kDenseGradThreads) loss_abs[b] = fabsf(radd(ws.le[b], vmse));
  const float sum = dense_loss_sum(ws.le, B, part);
  if (threadIdx.x == 0 && loss_mean) loss_mean[0] = radd(rmul(sum, invB), vmse);
}

// rth_ppo_adv_normalize: adv_b = fl32((adv_b - mean) / (std + 1e-8)) over the first ppo_rows(cap, n_dev)
// rows, in place, mean and population std of the fp32 advantages in fp64.  One workgroup; a sum is
// lane t's serial sum over the rows b = t (mod kPpoNormThreads) in increasing b, then a tree over the
// lanes: a fixed order.  Every row is read (twice) before the first is written.
constexpr int kPpoNormThreads = 1024;

__device__ inline double ppo_norm_sum(double acc, double *part) {
  const int tid = threadIdx.x;
  __syncthreads();  // `part` is free again
  part[tid] = acc;
  __syncthreads();
  for (int st = kPpoNormThreads / 2; st > 0; st >>= 1) {
    if (tid < st) part[tid] = radd(part[tid], part[tid + st]);
    __syncthreads();
  }
  return part[0];
}

__global__ __launch_bounds__(kPpoNormThreads) void k_ppo_adv_normalize(float *__restrict__ adv, int64_t cap,
                                                                       const int64_t *__restrict__ n_dev) {
  __shared__ double part[kPpoNormThreads];
  const int64_t n = ppo_rows(cap, n_dev);
  if (n == 0) return;  // (uniform)
  double acc = 0.0;
  for (int64_t b = threadIdx.x; b < n; b += kPpoNormThreads) acc = radd(acc, (double)adv[b]);
  const double mean = ppo_norm_sum(acc, part) / (double)n;
  acc = 0.0;
  for (int64_t b = threadIdx.x; b < n; b += kPpoNormThreads) {
    const double c = rsub((double)adv[b], mean);
    acc = radd(acc, rmul(c, c));
  }
  const double den = radd(sqrt(ppo_norm_sum(acc, part) / (double)n), 1e-8);
  for (int64_t b = threadIdx.x; b < n; b += kPpoNormThreads) adv[b] = (float)(rsub((double)adv[b], mean) / den);
}

inline bool ppo_shape_ok(int64_t D, int64_t H, int64_t A) {
  return H == kPpoH && D >= 1 && D <= kPpoMaxD && A >= kPpoMinA && A <= kPpoMaxA;
}

#define RTH_PPO_LIMITS "(H = 64, D in 1..64, A in 2..18)"
#define RTH_PPO_SHAPE(fn)                                                                              \
  RTH_REQUIRE(ppo_shape_ok(D, H, A), fn ": unsupported shape D=%lld H=%lld A=%lld " RTH_PPO_LIMITS, \
              (long long)D, (long long)H, (long long)A)

// The body of rth_ppo_grads (n_dev = NULL: the batch is B rows) and rth_ppo_grads_n (B is the
// capacity, the batch is the first min(*n_dev, B) rows): one code path.  The workspace is laid out
// for B in both, and the chunks of kPpoChunk rows start at row 0 in both, so n rows out of a larger
// capacity give what B = n gives, bit for bit.  rth_ppo_grads_adv is the same path with adv_dev given:
// the surrogate's advantage is adv_dev[b] instead of ret_b - v_b, nothing else changes.
inline int ppo_grads_run(const char *fn, const float *const *actor, const float *const *value, const float *s_dev,
                         int64_t lds, const int64_t *a_dev, const float *ret_dev, const float *adv_dev,
                         const float *old_logprob_dev, int64_t B, const int64_t *n_dev, int64_t D, int64_t H, int64_t A, float eps_clip,
                         float vf_coef, float ent_coef, float *const *actor_grads, float *const *value_grads,
                         float *loss_abs_dev, float *loss_mean_dev, void *workspace_dev, void *stream) {
  RTH_REQUIRE(ppo_shape_ok(D, H, A), "%s: unsupported shape D=%lld H=%lld A=%lld " RTH_PPO_LIMITS, fn, (long long)D,
              (long long)H, (long long)A);
  RTH_REQUIRE(B >= 1 && B <= (int64_t)1 << 40 && lds >= D, "%s: bad B=%lld or row stride %lld < D=%lld", fn,
              (long long)B, (long long)lds, (long long)D);
  DenseNet ac, va;
  RTH_REQUIRE(dense_net(actor, &ac) && dense_net(value, &va) && s_dev && a_dev && ret_dev && old_logprob_dev &&
                  loss_abs_dev && workspace_dev,
              "%s: NULL argument", fn);
  RTH_REQUIRE((actor_grads == nullptr) == (value_grads == nullptr),
              "%s: both gradient arrays or neither (evaluate only)", fn);
  const bool backward = actor_grads != nullptr;
  DenseGrads ga{}, gv{};
  if (backward) {
    for (int i = 0; i < 6; ++i) RTH_REQUIRE(actor_grads[i] && value_grads[i], "%s: NULL gradient buffer %d", fn, i);
    ga = DenseGrads{actor_grads[0], actor_grads[1], actor_grads[2], actor_grads[3], actor_grads[4], actor_grads[5]};
    gv = DenseGrads{value_grads[0], value_grads[1], value_grads[2], value_grads[3], value_grads[4], value_grads[5]};
  }
  // the clip range as the reference's python floats 1 - eps and 1 + eps, rounded to fp32 once
  const float lo = (float)(1.0 - (double)eps_clip), hi = (float)(1.0 + (double)eps_clip);
  float *ws = static_cast<float *>(workspace_dev);
  hipLaunchKernelGGL(k_ppo_tile, dim3(dense_grid(B)), dim3(kPpoThreads), 0, as_stream(stream), ac, va, s_dev, lds,
                     a_dev, ret_dev, adv_dev, old_logprob_dev, B, n_dev, (int)D, (int)A, lo, hi, vf_coef, ent_coef,
                     (int)backward, ws);
  RTH_LAUNCHED();
  const int grad_blocks = ppo_net_blocks((int)A) + ppo_net_blocks(1);
  hipLaunchKernelGGL(k_ppo_wgrad, dim3(backward ? grad_blocks + 1 : 1), dim3(kDenseGradThreads), 0, as_stream(stream),
                     ga, gv, s_dev, lds, B, n_dev, (int)D, (int)A, vf_coef, ws, loss_abs_dev, loss_mean_dev,
                     backward ? 0 : grad_blocks);
  RTH_LAUNCHED();
  return RTH_OK;
}

}  // namespace rth

extern "C" {

int rth_ppo_supported(int64_t D, int64_t H, int64_t A) { return rth::ppo_shape_ok(D, H, A) ? 1 : 0; }

int64_t rth_ppo_workspace(int64_t B, int64_t D, int64_t H, int64_t A) {
  using namespace rth;
  RTH_REQUIRE(ppo_shape_ok(D, H, A) && B >= 1 && B <= (int64_t)1 << 40,
              "rth_ppo_workspace: unsupported shape B=%lld D=%lld H=%lld A=%lld " RTH_PPO_LIMITS, (long long)B,
              (long long)D, (long long)H, (long long)A);
  return (PpoWs::floats(B, A) * 4 + 15) / 16 * 16;
}

int rth_ppo_act(const float *const *actor, const float *x_dev, int64_t ldx, int64_t n, int64_t D, int64_t H, int64_t A,
                const double *uniforms_dev, uint64_t seed, uint64_t counter, int64_t *action_dev, float *logprob_dev,
                float *probs_dev, void *stream) {
  using namespace rth;
  RTH_PPO_SHAPE("rth_ppo_act");
  RTH_REQUIRE(n >= 1 && n <= (int64_t)1 << 32 && ldx >= D, "rth_ppo_act: bad n=%lld (1..2^32) or ldx=%lld < D=%lld",
              (long long)n, (long long)ldx, (long long)D);
  DenseNet p;
  RTH_REQUIRE(dense_net(actor, &p) && x_dev && action_dev && logprob_dev, "rth_ppo_act: NULL argument");
  hipLaunchKernelGGL(k_ppo_act, dim3(dense_grid(n)), dim3(kPpoThreads), 0, as_stream(stream), p, x_dev, ldx, n, (int)D,
                     (int)A, uniforms_dev, seed, counter, action_dev, logprob_dev, probs_dev);
  RTH_LAUNCHED();
  return RTH_OK;
}

int rth_ppo_grads(const float *const *actor, const float *const *value, const float *s_dev, int64_t lds,
                  const int64_t *a_dev, const float *ret_dev, const float *old_logprob_dev, int64_t B, int64_t D,
                  int64_t H, int64_t A, float eps_clip, float vf_coef, float ent_coef, float *const *actor_grads,
                  float *const *value_grads, float *loss_abs_dev, float *loss_mean_dev, void *workspace_dev,
                  void *stream) {
  return rth::ppo_grads_run("rth_ppo_grads", actor, value, s_dev, lds, a_dev, ret_dev, nullptr, old_logprob_dev, B,
                            nullptr, D, H, A, eps_clip, vf_coef, ent_coef, actor_grads, value_grads, loss_abs_dev, loss_mean_dev,
                            workspace_dev, stream);
}

int rth_ppo_grads_n(const float *const *actor, const float *const *value, const float *s_dev, int64_t lds,
                    const int64_t *a_dev, const float *ret_dev, const float *old_logprob_dev, int64_t B, int64_t D,
                    int64_t H, int64_t A, float eps_clip, float vf_coef, float ent_coef, float *const *actor_grads,
                    float *const *value_grads, float *loss_abs_dev, float *loss_mean_dev, void *workspace_dev,
                    const int64_t *n_dev, void *stream) {
  RTH_REQUIRE(n_dev, "rth_ppo_grads_n: NULL row count");
  return rth::ppo_grads_run("rth_ppo_grads_n", actor, value, s_dev, lds, a_dev, ret_dev, nullptr, old_logprob_dev, B,
                            n_dev, D, H, A, eps_clip, vf_coef, ent_coef, actor_grads, value_grads, loss_abs_dev, loss_mean_dev,
                            workspace_dev, stream);
}

int rth_ppo_grads_adv(const float *const *actor, const float *const *value, const float *s_dev, int64_t lds,
                      const int64_t *a_dev, const float *ret_dev, const float *adv_dev, const float *old_logprob_dev,
                      int64_t B, int64_t D, int64_t H, int64_t A, float eps_clip, float vf_coef, float ent_coef,
                      float *const *actor_grads, float *const *value_grads, float *loss_abs_dev, float *loss_mean_dev,
                      void *workspace_dev, const int64_t *n_dev, void *stream) {
  RTH_REQUIRE(adv_dev, "rth_ppo_grads_adv: NULL advantages");
  return rth::ppo_grads_run("rth_ppo_grads_adv", actor, value, s_dev, lds, a_dev, ret_dev, adv_dev, old_logprob_dev,
                            B, n_dev, D, H, A, eps_clip, vf_coef, ent_coef, actor_grads, value_grads, loss_abs_dev,
                            loss_mean_dev, workspace_dev, stream);
}

int rth_ppo_adv_normalize(float *adv_dev, int64_t B, const int64_t *n_dev, void *stream) {
  using namespace rth;
  RTH_REQUIRE(adv_dev && B >= 1 && B <= (int64_t)1 << 40, "rth_ppo_adv_normalize: NULL advantages or bad B=%lld",
              (long long)B);
  hipLaunchKernelGGL(k_ppo_adv_normalize, dim3(1), dim3(kPpoNormThreads), 0, as_stream(stream), adv_dev, B, n_dev);
  RTH_LAUNCHED();
  return RTH_OK;
}

}  // extern "C"
