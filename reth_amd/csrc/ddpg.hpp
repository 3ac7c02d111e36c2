// DDPG's actor and critic (ddpg_model.py:76-122: actor Linear(D,H1) -> ReLU -> Linear(H1,H2) -> ReLU
// -> Linear(H2,Ad) -> tanh; critic Linear(D,H1) -> ReLU -> Linear(H1+Ad,H2) on cat(h1, a) -> ReLU ->
// Linear(H2,1)) as fused fp32 kernels: rth_ddpg_act (the actor forward, one launch),
// rth_ddpg_critic_grads (ddpg_solver.py:79-94: both target forwards, the critic forward, td, the
// loss and the critic's backward, two launches), rth_ddpg_actor_grads (:98-101: the actor
// forward, the critic forward on its action and the backward through the critic's action
// columns into the actor, two launches) and rth_soft_update (util.py:15-24, one launch).
//
// A 400 x 300 layer is 480 KB: it does not fit in LDS the way mlp.hpp's network does, but the four
// networks (~2 MB) stay in L2 / Infinity Cache across an update.  A workgroup owns a tile of
// kDdpgRows batch rows and walks them through whole networks, the activations in LDS; each layer's
// weights stream through one LDS chunk (128 output units x 32 k, fetched coalesced with scalar
// loads -- the critic's [H2, H1+Ad] rows are not 16-byte aligned --, written with a padded row
// stride, read as float4 after staging; the next chunk's loads are in flight in registers while
// the current one is multiplied).  No grid-wide synchronisation and no launch per layer; the
// alternative, splitting a layer's output columns over workgroups, needs one or the other.
// The data gradient of the middle layer streams the same weights in [32 n x 128 k] chunks and
// walks their columns.  The batch reductions (weight and bias gradients, the loss mean) are the
// second launch, over the activations and pre-activation gradients the first left in the
// workspace.
//
// Every product is one fmaf.  A dot product over k has ONE summation order -- dense.hpp's, which
// ddpg_dense and ddpg_head share --, then the bias; zero padding adds nothing.  A row's result does
// not depend on B, on its position, on the grid or on the entry point.  The batch sums are
// dense.hpp's, in its order: no atomics.
#pragma once
#include "dense.hpp"

namespace rth {

constexpr int kDdpgMaxD = kDenseMaxD, kDdpgMaxAd = 8, kDdpgMaxH = 512;
constexpr int kDdpgRows = kDenseRows;        // rows per tile
constexpr int kDdpgThreads = kDenseThreads;  // lane j = tid % 128: output unit of a pass; tid / 128: which 4 of the tile's rows
constexpr int kDdpgNT = 128, kDdpgRpt = kDdpgRows / (kDdpgThreads / kDdpgNT);
constexpr int kDdpgKT = 32;                // reduction length of one staged chunk
constexpr int kDdpgLdW = kDdpgKT + 4;      // row stride of a forward chunk [128 units][32 k]
constexpr int kDdpgLdT = kDdpgNT + 4;      // ... of a transposed chunk [32 n][128 columns]
constexpr int kDdpgChunk = kDdpgNT * kDdpgLdW;
constexpr int kDdpgPer = kDdpgNT * kDdpgKT / kDdpgThreads;  // chunk elements a lane fetches
constexpr int kDdpgLdH = kDdpgMaxH + kDdpgMaxAd;            // row stride of the activations in LDS
static_assert(kDdpgChunk >= kDdpgKT * kDdpgLdT, "the transposed chunk fits in the staging buffer");
static_assert(kDdpgRows * kDdpgMaxAd <= kDdpgThreads, "one lane per (row, action component)");

// a network (DenseNet): fc1.weight [H1, D], fc1.bias, fc2.weight [H2, H1 (+ Ad)], fc2.bias, fc3.weight [Ad | 1, H2], fc3.bias
struct DdpgDims {
  int D, Ad, H1, H2;
};

struct DdpgSmem {
  float w[kDdpgChunk];  // the staged weight chunk
  float x[kDdpgRows][kDdpgMaxD];
  float h1[kDdpgRows][kDdpgLdH];  // layer 1's activations; the critic's: cat(h1, a)
  float h2[kDdpgRows][kDdpgLdH];
  float ah1[kDdpgRows][kDdpgLdH];  // k_ddpg_actor: the actor's activations beside the critic's
  float ah2[kDdpgRows][kDdpgLdH];
  float g2[kDdpgRows][kDdpgLdH];  // d(loss)/d(layer 2's pre-activation)
  float part[kDdpgRows * kDdpgMaxAd * 8];  // ddpg_head's eight accumulators per output
  float pre[kDdpgRows][kDdpgMaxAd];        // the actor head before tanh; k_ddpg_critic: the batch's actions
  float act[kDdpgRows][kDdpgMaxAd];
  float gpre[kDdpgRows][kDdpgMaxAd];  // d(loss)/d(the actor head's pre-activation)
  float q[kDdpgRows], q1[kDdpgRows], g3[kDdpgRows];
};

// the workspace of the two gradient calls, in floats from its start
struct DdpgWs {
  float *act, *le, *g3, *xc, *h2, *g1, *g2;
  __host__ __device__ DdpgWs(float *p, int64_t B, const DdpgDims &d) {
    act = p, le = act + B * d.Ad, g3 = le + B, xc = g3 + B * d.Ad;
    h2 = xc + B * (d.H1 + d.Ad), g1 = h2 + B * d.H2, g2 = g1 + B * d.H1;
  }
  static int64_t floats(int64_t B, int64_t Ad, int64_t H1, int64_t H2) {
    return B * (2 * Ad + 1 + (H1 + Ad) + 2 * H2 + H1);
  }
};

// out[r][n] = act(sum_k in[r][k] W[n][k] + bias[n]) for the tile's rows: W [N, K] dense in global
// memory (any alignment), in / out LDS rows (strides multiples of 4; in's columns [K, round-up-8(K))
// are zeroed here).  Starts and ends with a workgroup barrier.
__device__ inline void ddpg_dense(const float *__restrict__ W, const float *__restrict__ bias, int N, int K, float *in,
                                  int ldin, float *out, int ldout, bool relu, DdpgSmem &s) {
  const int tid = threadIdx.x, j = tid & (kDdpgNT - 1), rb = (tid >> 7) * kDdpgRpt;
  const int K8 = (K + 7) & ~7;
  const int lrow = tid >> 5, lcol = tid & (kDdpgKT - 1);  // chunk elements (lrow + 8 i, lcol)
  __syncthreads();
  if (tid < kDdpgRows * 8) {
    const int c = K + (tid & 7);
    if (c < K8) in[(tid >> 3) * ldin + c] = 0.0f;
  }
  for (int n0 = 0; n0 < N; n0 += kDdpgNT) {
    float acc[kDdpgRpt][8] = {};
    float v[kDdpgPer];
#pragma unroll
    for (int i = 0; i < kDdpgPer; ++i) {
      const int n = n0 + lrow + 8 * i;
      v[i] = (n < N && lcol < K) ? W[(int64_t)n * K + lcol] : 0.0f;
    }
    for (int k0 = 0; k0 < K; k0 += kDdpgKT) {
      __syncthreads();  // the previous chunk is read
#pragma unroll
      for (int i = 0; i < kDdpgPer; ++i) s.w[(lrow + 8 * i) * kDdpgLdW + lcol] = v[i];
      __syncthreads();
      if (k0 + kDdpgKT < K) {  // the next chunk's loads fly while this one is multiplied
        const int k = k0 + kDdpgKT + lcol;
#pragma unroll
        for (int i = 0; i < kDdpgPer; ++i) {
          const int n = n0 + lrow + 8 * i;
          v[i] = (n < N && k < K) ? W[(int64_t)n * K + k] : 0.0f;
        }
      }
      const int kend = K8 - k0 < kDdpgKT ? K8 - k0 : kDdpgKT;
      const float *w = s.w + j * kDdpgLdW;
      for (int kk = 0; kk < kend; kk += 8) {
        const float4 wa = *reinterpret_cast<const float4 *>(w + kk);
        const float4 wb = *reinterpret_cast<const float4 *>(w + kk + 4);
#pragma unroll
        for (int rr = 0; rr < kDdpgRpt; ++rr) {
          const float *xr = in + (rb + rr) * ldin + k0 + kk;
          const float4 xa = *reinterpret_cast<const float4 *>(xr);
          const float4 xb = *reinterpret_cast<const float4 *>(xr + 4);
          dense_fma8(xa, xb, wa, wb, acc[rr]);
        }
      }
    }
    if (n0 + j < N) {
      const float b = bias[n0 + j];
#pragma unroll
      for (int rr = 0; rr < kDdpgRpt; ++rr) {
        const float val = radd(dense_tree8(acc[rr]), b);
        out[(rb + rr) * ldout + n0 + j] = relu ? dense_relu(val) : val;
      }
    }
  }
  __syncthreads();
}

// The data gradient of a layer down its weight's columns: for k in [0, Kout)
//   out[r0 + r][k] = mask[r][k] > 0 ? sum_n g[r][n] W[n * ldw + k] : 0
// W [N, ldw] in global memory, g / mask LDS rows (g's columns [N, round-up-8(N)) are zeroed here),
// out global rows of stride ldo, stored for r0 + r < B only.  The sum over n in ddpg_dense's order.
// Starts and ends with a workgroup barrier.
__device__ inline void ddpg_dense_t(const float *__restrict__ W, int ldw, int N, int Kout, float *g, int ldg,
                                    const float *mask, int ldm, float *__restrict__ out, int64_t ldo, int64_t r0,
                                    int64_t B, DdpgSmem &s) {
  const int tid = threadIdx.x, j = tid & (kDdpgNT - 1), rb = (tid >> 7) * kDdpgRpt;
  const int N8 = (N + 7) & ~7;
  const int lrow = tid >> 7, lcol = tid & (kDdpgNT - 1);  // chunk elements (lrow + 2 i, lcol)
  __syncthreads();
  if (tid < kDdpgRows * 8) {
    const int c = N + (tid & 7);
    if (c < N8) g[(tid >> 3) * ldg + c] = 0.0f;
  }
  for (int kb = 0; kb < Kout; kb += kDdpgNT) {
    float acc[kDdpgRpt][8] = {};
    float v[kDdpgPer];
    const bool col_ok = kb + lcol < Kout;
#pragma unroll
    for (int i = 0; i < kDdpgPer; ++i) {
      const int n = lrow + 2 * i;
      v[i] = (n < N && col_ok) ? W[(int64_t)n * ldw + kb + lcol] : 0.0f;
    }
    for (int n0 = 0; n0 < N; n0 += kDdpgKT) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < kDdpgPer; ++i) s.w[(lrow + 2 * i) * kDdpgLdT + lcol] = v[i];
      __syncthreads();
      if (n0 + kDdpgKT < N) {
#pragma unroll
        for (int i = 0; i < kDdpgPer; ++i) {
          const int n = n0 + kDdpgKT + lrow + 2 * i;
          v[i] = (n < N && col_ok) ? W[(int64_t)n * ldw + kb + lcol] : 0.0f;
        }
      }
      const int nend = N8 - n0 < kDdpgKT ? N8 - n0 : kDdpgKT;
      for (int nn = 0; nn < nend; nn += 8) {
        float wv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wv[i] = s.w[(nn + i) * kDdpgLdT + j];
        const float4 wa = make_float4(wv[0], wv[1], wv[2], wv[3]), wb = make_float4(wv[4], wv[5], wv[6], wv[7]);
#pragma unroll
        for (int rr = 0; rr < kDdpgRpt; ++rr) {
          const float *gr = g + (rb + rr) * ldg + n0 + nn;
          const float4 ga = *reinterpret_cast<const float4 *>(gr);
          const float4 gb = *reinterpret_cast<const float4 *>(gr + 4);
          dense_fma8(ga, gb, wa, wb, acc[rr]);
        }
      }
    }
    if (kb + j < Kout) {
#pragma unroll
      for (int rr = 0; rr < kDdpgRpt; ++rr) {
        const int r = rb + rr;
        if (r0 + r < B) out[(r0 + r) * ldo + kb + j] = mask[r * ldm + kb + j] > 0.0f ? dense_tree8(acc[rr]) : 0.0f;
      }
    }
  }
  __syncthreads();
}

// A narrow layer (Nout <= kDdpgMaxAd outputs): out[r][a] = sum_k in[r][k] W[a * sa + k * sk] (+ bias[a]).
// Eight lanes per output: lane i sums the terms k = i (mod 8) in increasing k -- accumulator i of
// ddpg_dense's order --, then the same tree and the bias.  (sa, sk) = (K, 1): a weight's rows;
// (1, ld): its columns.  Starts and ends with a workgroup barrier.
__device__ inline void ddpg_head(const float *__restrict__ W, int64_t sa, int64_t sk, const float *__restrict__ bias,
                                 int Nout, int K, const float *in, int ldin, float *out, int ldout, DdpgSmem &s) {
  const int tid = threadIdx.x;
  __syncthreads();
  for (int task = tid; task < kDdpgRows * Nout * 8; task += kDdpgThreads) {
    const int i = task & 7, o = task >> 3, a = o % Nout, r = o / Nout;
    const float *x = in + r * ldin;
    const float *w = W + a * sa;
    float acc = 0.0f;
#pragma unroll 4
    for (int k = i; k < K; k += 8) acc = fmaf(x[k], w[k * sk], acc);
    s.part[task] = acc;
  }
  __syncthreads();
  for (int o = tid; o < kDdpgRows * Nout; o += kDdpgThreads) {
    const int a = o % Nout, r = o / Nout;
    float p[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = s.part[o * 8 + i];
    const float val = dense_tree8(p);
    out[r * ldout + a] = bias ? radd(val, bias[a]) : val;
  }
  __syncthreads();
}

// The actor's forward of the rows in s.x: the hidden activations to h1b / h2b (LDS, stride
// kDdpgLdH), the head to s.pre, its tanh -- in fp64, rounded once -- to s.act.  The only actor forward.
__device__ inline void ddpg_actor_forward(const DenseNet &p, const DdpgDims &d, float *h1b, float *h2b, DdpgSmem &s) {
  ddpg_dense(p.w1, p.b1, d.H1, d.D, &s.x[0][0], kDdpgMaxD, h1b, kDdpgLdH, true, s);
  ddpg_dense(p.w2, p.b2, d.H2, d.H1, h1b, kDdpgLdH, h2b, kDdpgLdH, true, s);
  ddpg_head(p.w3, d.H2, 1, p.b3, d.Ad, d.H2, h2b, kDdpgLdH, &s.pre[0][0], kDdpgMaxAd, s);
  const int tid = threadIdx.x;
  if (tid < kDdpgRows * d.Ad) {
    const int r = tid / d.Ad, a = tid % d.Ad;
    s.act[r][a] = (float)tanh((double)s.pre[r][a]);
  }
  __syncthreads();
}

// The critic's forward of the rows in s.x with the actions a (LDS rows of stride kDdpgMaxAd):
// cat(h1, a) to s.h1, h2 to s.h2, Q to q.
__device__ inline void ddpg_critic_forward(const DenseNet &p, const DdpgDims &d, const float *a, float *q, DdpgSmem &s) {
  ddpg_dense(p.w1, p.b1, d.H1, d.D, &s.x[0][0], kDdpgMaxD, &s.h1[0][0], kDdpgLdH, true, s);
  const int tid = threadIdx.x;
  if (tid < kDdpgRows * d.Ad) {
    const int r = tid / d.Ad, c = tid % d.Ad;
    s.h1[r][d.H1 + c] = a[r * kDdpgMaxAd + c];
  }
  ddpg_dense(p.w2, p.b2, d.H2, d.H1 + d.Ad, &s.h1[0][0], kDdpgLdH, &s.h2[0][0], kDdpgLdH, true, s);
  ddpg_head(p.w3, d.H2, 1, p.b3, 1, d.H2, &s.h2[0][0], kDdpgLdH, q, 1, s);
}

// rows of an LDS activation block to the workspace (rows r0 + r < B only)
__device__ inline void ddpg_store_rows(const float *src, int cols, float *__restrict__ dst, int64_t ldd, int64_t r0,
                                       int64_t B) {
  for (int i = threadIdx.x; i < kDdpgRows * cols; i += kDdpgThreads) {
    const int r = i / cols, k = i - r * cols;
    if (r0 + r < B) dst[(r0 + r) * ldd + k] = src[r * kDdpgLdH + k];
  }
}

__global__ __launch_bounds__(kDdpgThreads) void k_ddpg_act(DenseNet p, const float *__restrict__ x, int64_t ldx,
                                                           int64_t n, DdpgDims d, float *__restrict__ out) {
  __shared__ __align__(16) DdpgSmem s;
  const int64_t tiles = (n + kDdpgRows - 1) / kDdpgRows;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * kDdpgRows;
    __syncthreads();
    dense_load_x(x, ldx, n, r0, d.D, s.x);
    ddpg_actor_forward(p, d, &s.h1[0][0], &s.h2[0][0], s);
    const int tid = threadIdx.x;
    if (tid < kDdpgRows * d.Ad) {
      const int r = tid / d.Ad, a = tid % d.Ad;
      if (r0 + r < n) out[(r0 + r) * d.Ad + a] = s.act[r][a];
    }
  }
}

// rth_ddpg_critic_grads' first launch.  Per tile of rows: a1 = actor_tgt(s1), critic_tgt(s1, a1),
// critic(s0, a), the td arithmetic of ddpg_solver.py:81-91 in its operation order (|td|, the loss
// element, dQ) and -- backward -- the critic's data gradients; cat(h1, a), h2 and the
// pre-activation gradients go to the workspace for the second launch.
__global__ __launch_bounds__(kDdpgThreads) void k_ddpg_critic(
    DenseNet cr, DenseNet at, DenseNet ct, const float *__restrict__ s0, int64_t lds0, const float *__restrict__ a,
    int64_t lda, const float *__restrict__ rew, const float *__restrict__ done, const float *__restrict__ s1,
    int64_t lds1, const float *__restrict__ isw, int64_t B, DdpgDims d, float gamma, int backward,
    float *__restrict__ wsp, float *__restrict__ td_abs) {
  __shared__ __align__(16) DdpgSmem s;
  const DdpgWs ws(wsp, B, d);
  const int tid = threadIdx.x;
  const int64_t tiles = (B + kDdpgRows - 1) / kDdpgRows;
  const float invB = 1.0f / (float)B;
  const int K2 = d.H1 + d.Ad;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * kDdpgRows;
    __syncthreads();
    dense_load_x(s1, lds1, B, r0, d.D, s.x);
    ddpg_actor_forward(at, d, &s.h1[0][0], &s.h2[0][0], s);
    ddpg_critic_forward(ct, d, &s.act[0][0], s.q1, s);
    dense_load_x(s0, lds0, B, r0, d.D, s.x);
    if (tid < kDdpgRows * d.Ad) {
      const int r = tid / d.Ad, c = tid % d.Ad;
      s.pre[r][c] = r0 + r < B ? a[(r0 + r) * lda + c] : 0.0f;
    }
    ddpg_critic_forward(cr, d, &s.pre[0][0], s.q, s);
    if (tid < kDdpgRows) {
      const int64_t b = r0 + tid;
      if (b < B) {
        // y = r + ((1 - done) * gamma) * Q'(s1, a1); td = Q(s0, a) - y; loss element td^2 (* w)
        const float y = radd(rew[b], rmul(rmul(rsub(1.0f, done[b]), gamma), s.q1[tid]));
        const float td = rsub(s.q[tid], y);
        float l = rmul(td, td);
        float g = invB;  // autograd: mean -> mul(w) -> pow(2)
        if (isw) {
          l = rmul(l, isw[b]);
          g = rmul(g, isw[b]);
        }
        s.g3[tid] = rmul(g, rmul(2.0f, td));
        ws.le[b] = l;
        if (td_abs) td_abs[b] = fabsf(td);
      } else {
        s.g3[tid] = 0.0f;
      }
    }
    if (!backward) continue;
    __syncthreads();
    // layer 3's data gradient, ReLU mask: g2 = (h2 > 0) ? g3 W3 : 0
    for (int i = tid; i < kDdpgRows * d.H2; i += kDdpgThreads) {
      const int r = i / d.H2, n = i - r * d.H2;
      s.g2[r][n] = s.h2[r][n] > 0.0f ? rmul(s.g3[r], cr.w3[n]) : 0.0f;
    }
    // layer 2's: g1 = (h1 > 0) ? g2 W2[:, :H1] : 0 (the action columns carry no gradient here)
    ddpg_dense_t(cr.w2, K2, d.H2, d.H1, &s.g2[0][0], kDdpgLdH, &s.h1[0][0], kDdpgLdH, ws.g1, d.H1, r0, B, s);
    ddpg_store_rows(&s.h1[0][0], K2, ws.xc, K2, r0, B);
    ddpg_store_rows(&s.h2[0][0], d.H2, ws.h2, d.H2, r0, B);
    ddpg_store_rows(&s.g2[0][0], d.H2, ws.g2, d.H2, r0, B);
    if (tid < kDdpgRows && r0 + tid < B) ws.g3[r0 + tid] = s.g3[tid];
  }
}

// rth_ddpg_actor_grads' first launch.  Per tile of rows: a = actor(s0) (ddpg_actor_forward, so
// rth_ddpg_act's values), Q = critic(s0, a), the loss element -Q, and the backward of -mean(Q):
// through the critic's last layer, its middle layer's ReLU and the action columns [H1, H1 + Ad) of
// its middle weight, through 1 - tanh^2, then the actor's data gradients.  The action, the actor's
// activations and pre-activation gradients go to the workspace for the second launch.
__global__ __launch_bounds__(kDdpgThreads) void k_ddpg_actor(DenseNet ac, DenseNet cr, const float *__restrict__ s0,
                                                             int64_t lds0, int64_t B, DdpgDims d,
                                                             float *__restrict__ wsp) {
  __shared__ __align__(16) DdpgSmem s;
  const DdpgWs ws(wsp, B, d);
  const int tid = threadIdx.x;
  const int64_t tiles = (B + kDdpgRows - 1) / kDdpgRows;
  const float ginv = -(1.0f / (float)B);  // d(-mean Q)/dQ
  const int K2 = d.H1 + d.Ad;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * kDdpgRows;
    __syncthreads();
    dense_load_x(s0, lds0, B, r0, d.D, s.x);
    ddpg_actor_forward(ac, d, &s.ah1[0][0], &s.ah2[0][0], s);
    ddpg_critic_forward(cr, d, &s.act[0][0], s.q, s);
    // the critic's layer 3 and ReLU: g2 = (h2 > 0) ? -1/B W3 : 0
    for (int i = tid; i < kDdpgRows * d.H2; i += kDdpgThreads) {
      const int r = i / d.H2, n = i - r * d.H2;
      s.g2[r][n] = (s.h2[r][n] > 0.0f && r0 + r < B) ? rmul(ginv, cr.w3[n]) : 0.0f;
    }
    // d(loss)/da = g2 W2[:, H1:H1+Ad], then tanh's derivative 1 - a^2
    ddpg_head(cr.w2 + d.H1, 1, K2, nullptr, d.Ad, d.H2, &s.g2[0][0], kDdpgLdH, &s.gpre[0][0], kDdpgMaxAd, s);
    if (tid < kDdpgRows * d.Ad) {
      const int r = tid / d.Ad, c = tid % d.Ad;
      const float y = s.act[r][c];
      s.gpre[r][c] = rmul(s.gpre[r][c], rsub(1.0f, rmul(y, y)));
    }
    __syncthreads();
    // the actor's layer 3 and ReLU: g2 = (h2 > 0) ? gpre W3 : 0
    for (int i = tid; i < kDdpgRows * d.H2; i += kDdpgThreads) {
      const int r = i / d.H2, n = i - r * d.H2;
      float acc = 0.0f;
      for (int c = 0; c < d.Ad; ++c) acc = fmaf(s.gpre[r][c], ac.w3[c * d.H2 + n], acc);
      s.g2[r][n] = s.ah2[r][n] > 0.0f ? acc : 0.0f;
    }
    ddpg_dense_t(ac.w2, d.H1, d.H2, d.H1, &s.g2[0][0], kDdpgLdH, &s.ah1[0][0], kDdpgLdH, ws.g1, d.H1, r0, B, s);
    ddpg_store_rows(&s.ah1[0][0], d.H1, ws.xc, K2, r0, B);
    ddpg_store_rows(&s.ah2[0][0], d.H2, ws.h2, d.H2, r0, B);
    ddpg_store_rows(&s.g2[0][0], d.H2, ws.g2, d.H2, r0, B);
    if (tid < kDdpgRows * d.Ad) {
      const int r = tid / d.Ad, c = tid % d.Ad;
      if (r0 + r < B) {
        ws.act[(r0 + r) * d.Ad + c] = s.act[r][c];
        ws.g3[(r0 + r) * d.Ad + c] = s.gpre[r][c];
      }
    }
    if (tid < kDdpgRows && r0 + tid < B) ws.le[r0 + tid] = -s.q[tid];
  }
}

// the second launch's workgroups: the middle layer's weight gradient ([H2, Kw2], Kw2 = H1 + Ad for
// the critic, H1 for the actor), the first layer's, the last layer's ([N3, H2]), the three bias
// gradients, then one workgroup for the loss mean
struct DdpgWgradPlan {
  int kt2, t2, t1, kt3, t3, nb1, nb2;
  __host__ __device__ DdpgWgradPlan(const DdpgDims &d, int Kw2, int N3) {
    kt2 = (Kw2 + kDenseGradThreads - 1) / kDenseGradThreads;
    t2 = (d.H2 + kDenseGradJ - 1) / kDenseGradJ * kt2;
    t1 = (d.H1 + kDenseGradJ - 1) / kDenseGradJ;
    kt3 = (d.H2 + kDenseGradThreads - 1) / kDenseGradThreads;
    t3 = (N3 + kDenseGradJ - 1) / kDenseGradJ * kt3;
    nb1 = (d.H1 + kDenseGradThreads - 1) / kDenseGradThreads;
    nb2 = (d.H2 + kDenseGradThreads - 1) / kDenseGradThreads;
  }
  __host__ __device__ int grad_blocks() const { return t2 + t1 + t3 + nb1 + nb2 + 1; }
};

__global__ __launch_bounds__(kDenseGradThreads) void k_ddpg_wgrad(DenseGrads g, const float *__restrict__ s0,
                                                                 int64_t lds0, int64_t B, DdpgDims d, int Kw2, int N3,
                                                                 float *__restrict__ wsp, float *__restrict__ loss,
                                                                 int first) {
  __shared__ float part[kDenseGradThreads];
  const DdpgWs ws(wsp, B, d);
  const DdpgWgradPlan pl(d, Kw2, N3);
  const int K2 = d.H1 + d.Ad;
  int blk = (int)blockIdx.x + first;
  if (blk < pl.t2)
    return dense_wgrad_tile(ws.g2, d.H2, d.H2, ws.xc, K2, Kw2, B, blk / pl.kt2 * kDenseGradJ,
                           blk % pl.kt2 * kDenseGradThreads, g.w2);
  blk -= pl.t2;
  if (blk < pl.t1) return dense_wgrad_tile(ws.g1, d.H1, d.H1, s0, lds0, d.D, B, blk * kDenseGradJ, 0, g.w1);
  blk -= pl.t1;
  if (blk < pl.t3)
    return dense_wgrad_tile(ws.g3, N3, N3, ws.h2, d.H2, d.H2, B, blk / pl.kt3 * kDenseGradJ,
                           blk % pl.kt3 * kDenseGradThreads, g.w3);
  blk -= pl.t3;
  if (blk < pl.nb1) return dense_bgrad(ws.g1, d.H1, d.H1, B, blk * kDenseGradThreads, g.b1);
  blk -= pl.nb1;
  if (blk < pl.nb2) return dense_bgrad(ws.g2, d.H2, d.H2, B, blk * kDenseGradThreads, g.b2);
  blk -= pl.nb2;
  if (blk == 0) return dense_bgrad(ws.g3, N3, N3, B, 0, g.b3);
  const float sum = dense_loss_sum(ws.le, B, part);
  if (threadIdx.x == 0 && loss) loss[0] = sum / (float)B;
}

// rth_soft_update: every tensor of a network in one launch, kSoftPer elements per workgroup
constexpr int kSoftMaxTensors = 16, kSoftThreads = 256, kSoftPer = 1024;
struct SoftArgs {
  float *t[kSoftMaxTensors];
  const float *p[kSoftMaxTensors];
  int64_t n[kSoftMaxTensors];
  int64_t first[kSoftMaxTensors + 1];  // the tensors' first workgroups
  int count;
};

__global__ __launch_bounds__(kSoftThreads) void k_soft_update(SoftArgs a, float one_minus_tau, float tau) {
  const int64_t blk = blockIdx.x;
  int i = 0;
  while (i + 1 < a.count && blk >= a.first[i + 1]) ++i;
  float *__restrict__ t = a.t[i];
  const float *__restrict__ p = a.p[i];
  const int64_t base = (blk - a.first[i]) * kSoftPer;
#pragma unroll
  for (int u = 0; u < kSoftPer / kSoftThreads; ++u) {
    const int64_t e = base + threadIdx.x + u * kSoftThreads;
    // target * (1 - tau) + param * tau (util.py:24): two products, one sum, each rounded once
    if (e < a.n[i]) t[e] = radd(rmul(t[e], one_minus_tau), rmul(p[e], tau));
  }
}

inline bool ddpg_shape_ok(int64_t D, int64_t Ad, int64_t H1, int64_t H2) {
  return D >= 1 && D <= kDdpgMaxD && Ad >= 1 && Ad <= kDdpgMaxAd && H1 >= 4 && H1 <= kDdpgMaxH && H1 % 4 == 0 &&
         H2 >= 4 && H2 <= kDdpgMaxH && H2 % 4 == 0;
}

#define RTH_DDPG_LIMITS "(D in 1..64, Ad in 1..8, H1 and H2 multiples of 4 in 4..512)"
#define RTH_DDPG_SHAPE(fn)                                                                                    \
  RTH_REQUIRE(ddpg_shape_ok(D, Ad, H1, H2), fn ": unsupported shape D=%lld Ad=%lld H1=%lld H2=%lld " RTH_DDPG_LIMITS, \
              (long long)D, (long long)Ad, (long long)H1, (long long)H2)

}  // namespace rth

extern "C" {

int rth_ddpg_supported(int64_t D, int64_t Ad, int64_t H1, int64_t H2) {
  return rth::ddpg_shape_ok(D, Ad, H1, H2) ? 1 : 0;
}

int64_t rth_ddpg_workspace(int64_t B, int64_t D, int64_t Ad, int64_t H1, int64_t H2) {
  using namespace rth;
  RTH_REQUIRE(ddpg_shape_ok(D, Ad, H1, H2) && B >= 1 && B <= (int64_t)1 << 40,
              "rth_ddpg_workspace: unsupported shape B=%lld D=%lld Ad=%lld H1=%lld H2=%lld " RTH_DDPG_LIMITS,
              (long long)B, (long long)D, (long long)Ad, (long long)H1, (long long)H2);
  return (DdpgWs::floats(B, Ad, H1, H2) * 4 + 15) / 16 * 16;
}

int rth_ddpg_act(const float *const *actor, const float *x_dev, int64_t ldx, int64_t n, int64_t D, int64_t Ad,
                 int64_t H1, int64_t H2, float *act_out_dev, void *stream) {
  using namespace rth;
  RTH_DDPG_SHAPE("rth_ddpg_act");
  RTH_REQUIRE(n >= 1 && n <= (int64_t)1 << 40 && ldx >= D, "rth_ddpg_act: bad n=%lld or ldx=%lld < D=%lld",
              (long long)n, (long long)ldx, (long long)D);
  DenseNet p;
  RTH_REQUIRE(dense_net(actor, &p) && x_dev && act_out_dev, "rth_ddpg_act: NULL argument");
  const DdpgDims d{(int)D, (int)Ad, (int)H1, (int)H2};
  hipLaunchKernelGGL(k_ddpg_act, dim3(dense_grid(n)), dim3(kDdpgThreads), 0, as_stream(stream), p, x_dev, ldx, n, d,
                     act_out_dev);
  RTH_LAUNCHED();
  return RTH_OK;
}

int rth_ddpg_critic_grads(const float *const *critic, const float *const *actor_target,
                          const float *const *critic_target, const float *s0_dev, int64_t lds0, const float *a_dev,
                          int64_t lda, const float *r_dev, const float *done_dev, const float *s1_dev, int64_t lds1,
                          const float *isw_dev, int64_t B, int64_t D, int64_t Ad, int64_t H1, int64_t H2, float gamma,
                          float *const *grads, float *td_abs_dev, float *loss_dev, void *workspace_dev, void *stream) {
  using namespace rth;
  RTH_DDPG_SHAPE("rth_ddpg_critic_grads");
  RTH_REQUIRE(B >= 1 && B <= (int64_t)1 << 40 && lds0 >= D && lds1 >= D && lda >= Ad,
              "rth_ddpg_critic_grads: bad B=%lld or row stride (%lld, %lld) < D=%lld, %lld < Ad=%lld", (long long)B,
              (long long)lds0, (long long)lds1, (long long)D, (long long)lda, (long long)Ad);
  DenseNet cr, at, ct;
  RTH_REQUIRE(dense_net(critic, &cr) && dense_net(actor_target, &at) && dense_net(critic_target, &ct) && s0_dev &&
                  a_dev && r_dev && done_dev && s1_dev && workspace_dev,
              "rth_ddpg_critic_grads: NULL argument");
  DenseGrads g{};
  if (grads) {
    for (int i = 0; i < 6; ++i) RTH_REQUIRE(grads[i], "rth_ddpg_critic_grads: NULL gradient buffer %d", i);
    g = DenseGrads{grads[0], grads[1], grads[2], grads[3], grads[4], grads[5]};
  }
  const DdpgDims d{(int)D, (int)Ad, (int)H1, (int)H2};
  float *ws = static_cast<float *>(workspace_dev);
  hipLaunchKernelGGL(k_ddpg_critic, dim3(dense_grid(B)), dim3(kDdpgThreads), 0, as_stream(stream), cr, at, ct, s0_dev,
                     lds0, a_dev, lda, r_dev, done_dev, s1_dev, lds1, isw_dev, B, d, gamma, (int)(grads != nullptr), ws,
                     td_abs_dev);
  RTH_LAUNCHED();
  const int Kw2 = (int)(H1 + Ad);
  const int grad_blocks = DdpgWgradPlan(d, Kw2, 1).grad_blocks();
  if (grads) {  // every gradient element, then the loss mean
    hipLaunchKernelGGL(k_ddpg_wgrad, dim3(grad_blocks + 1), dim3(kDenseGradThreads), 0, as_stream(stream), g, s0_dev,
                       lds0, B, d, Kw2, 1, ws, loss_dev, 0);
    RTH_LAUNCHED();
  } else if (loss_dev) {
    hipLaunchKernelGGL(k_ddpg_wgrad, dim3(1), dim3(kDenseGradThreads), 0, as_stream(stream), g, s0_dev, lds0, B, d, Kw2,
                       1, ws, loss_dev, grad_blocks);
    RTH_LAUNCHED();
  }
  return RTH_OK;
}

int rth_ddpg_actor_grads(const float *const *actor, const float *const *critic, const float *s0_dev, int64_t lds0,
                         int64_t B, int64_t D, int64_t Ad, int64_t H1, int64_t H2, float *const *grads,
                         float *loss_dev, void *workspace_dev, void *stream) {
  using namespace rth;
  RTH_DDPG_SHAPE("rth_ddpg_actor_grads");
  RTH_REQUIRE(B >= 1 && B <= (int64_t)1 << 40 && lds0 >= D, "rth_ddpg_actor_grads: bad B=%lld or row stride %lld < D=%lld",
              (long long)B, (long long)lds0, (long long)D);
  DenseNet ac, cr;
  RTH_REQUIRE(dense_net(actor, &ac) && dense_net(critic, &cr) && s0_dev && workspace_dev && grads,
              "rth_ddpg_actor_grads: NULL argument");
  for (int i = 0; i < 6; ++i) RTH_REQUIRE(grads[i], "rth_ddpg_actor_grads: NULL gradient buffer %d", i);
  const DenseGrads g{grads[0], grads[1], grads[2], grads[3], grads[4], grads[5]};
  const DdpgDims d{(int)D, (int)Ad, (int)H1, (int)H2};
  float *ws = static_cast<float *>(workspace_dev);
  hipLaunchKernelGGL(k_ddpg_actor, dim3(dense_grid(B)), dim3(kDdpgThreads), 0, as_stream(stream), ac, cr, s0_dev, lds0,
                     B, d, ws);
  RTH_LAUNCHED();
  const int grad_blocks = DdpgWgradPlan(d, (int)H1, (int)Ad).grad_blocks();
  hipLaunchKernelGGL(k_ddpg_wgrad, dim3(grad_blocks + 1), dim3(kDenseGradThreads), 0, as_stream(stream), g, s0_dev, lds0,
                     B, d, (int)H1, (int)Ad, ws, loss_dev, 0);
  RTH_LAUNCHED();
  return RTH_OK;
}

int rth_soft_update(float *const *target, const float *const *source, const int64_t *numel, int32_t n_tensors,
                    double tau, void *stream) {
  using namespace rth;
  RTH_REQUIRE(target && source && numel && n_tensors >= 1 && n_tensors <= kSoftMaxTensors,
              "rth_soft_update: NULL argument or n_tensors=%d outside 1..%d", (int)n_tensors, kSoftMaxTensors);
  SoftArgs a{};
  a.count = n_tensors;
  int64_t blocks = 0;
  for (int i = 0; i < n_tensors; ++i) {
    RTH_REQUIRE(target[i] && source[i] && numel[i] >= 1 && numel[i] <= (int64_t)1 << 40,
                "rth_soft_update: tensor %d is NULL or has numel=%lld outside 1..2^40", i, (long long)numel[i]);
    a.t[i] = target[i], a.p[i] = source[i], a.n[i] = numel[i];
    a.first[i] = blocks;
    blocks += (numel[i] + kSoftPer - 1) / kSoftPer;
  }
  a.first[n_tensors] = blocks;
  RTH_REQUIRE(blocks <= 0x7fffffff, "rth_soft_update: %lld workgroups exceed one grid", (long long)blocks);
  hipLaunchKernelGGL(k_soft_update, dim3((unsigned)blocks), dim3(kSoftThreads), 0, as_stream(stream), a,
                     (float)(1.0 - tau), (float)tau);
  RTH_LAUNCHED();
  return RTH_OK;
}

}  // extern "C"
