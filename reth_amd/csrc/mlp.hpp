// The MLP Q-network (dqn_model.py:59-71: Linear(D,128) -> ReLU -> Linear(128,128) -> ReLU ->
// Linear(128,A), the CartPole configuration) as fused fp32 kernels: rth_mlp_q (the forward +
// argmax, one launch) and rth_mlp_dqn_grads (dqn_solver.py:68-117: three forwards, the TD / Huber
// arithmetic of k_td_huber and the backward through the online net, two launches).
//
// The whole network is ~70 KB of fp32 weights: a workgroup stages all of it in LDS once (the
// 128 x 128 middle layer with a row stride of 132 floats: ds_read_b128 down a row and ds_read_b32
// down a column are both conflict-free) and walks tiles of kMlpRows rows, so a forward's only HBM
// / L2 round trip is its input rows.  Every product is one fmaf (VALU, one rounding).  A dot
// product over k has ONE summation order -- dense.hpp's; mlp_forward_tile is the only forward --,
// then the bias: a row's Q does not depend on n, on its position or on the entry point.  The weight
// and bias gradients and the loss sum over the batch in dense.hpp's order, with its functions.
#pragma once
#include "dense.hpp"

namespace rth {

constexpr int kMlpH = 128, kMlpMaxD = kDenseMaxD, kMlpMaxA = 18;
constexpr int kMlpRows = kDenseRows;        // rows per tile
constexpr int kMlpThreads = kDenseThreads;  // lane j = tid % 128: hidden unit; tid / 128: which 4 of the tile's rows
constexpr int kMlpRpt = kMlpRows / (kMlpThreads / kMlpH);
constexpr int kMlpLdw = kMlpH + 4;  // LDS row stride of the staged middle and last layer
constexpr int kMlpLd1 = kMlpMaxD + 4;  // ... of the first layer (columns [D, round-up-8(D)) zero)
static_assert(kMlpRows * kMlpMaxA <= kMlpThreads && kMlpMaxA <= kMaxActions, "one lane per (row, action)");

struct MlpSmem {
  float w2[kMlpH * kMlpLdw];
  float w1[kMlpH * kMlpLd1];
  float w3[kMlpMaxA * kMlpLdw];
  float b1[kMlpH], b2[kMlpH], b3[kMlpMaxA + 2];
  float x[kMlpRows][kMlpMaxD];
  float x1[kMlpRows][kMlpMaxD];  // k_mlp_td: the tile's s1 rows beside its s0 rows
  // k_mlp_td: the tile's batch columns and its three Q row blocks (row stride A) for td_huber_row
  double isw[kMlpRows];
  int64_t act[kMlpRows];
  float rew[kMlpRows], done[kMlpRows];
  float tq0[kMlpRows * kMlpMaxA], tq1o[kMlpRows * kMlpMaxA], tq1t[kMlpRows * kMlpMaxA];
  float h1[kMlpRows][kMlpH];
  float h2[kMlpRows][kMlpH];
  float g2[kMlpRows][kMlpH];  // d(loss)/d(layer 2's pre-activation)
  float q[kMlpRows][kMlpMaxA + 2];
  float g3[kMlpRows][kMlpMaxA + 2];  // d(loss)/dQ
};

// rth_mlp_dqn_grads' workspace, in floats from its start
struct MlpWs {
  float *q1t, *g3, *le, *h1, *h2, *g1, *g2;
  __host__ __device__ MlpWs(float *p, int64_t B, int A) {
    q1t = p, g3 = q1t + B * A, le = g3 + B * A;
    h1 = le + B, h2 = h1 + B * kMlpH, g1 = h2 + B * kMlpH, g2 = g1 + B * kMlpH;
  }
  static int64_t floats(int64_t B, int64_t A) { return 2 * B * A + B + 4 * B * kMlpH; }
};

// the network's parameters into LDS; the caller synchronises before they are read
__device__ inline void mlp_stage_net(const DenseNet &p, int D, int A, MlpSmem &s) {
  const int tid = threadIdx.x;
  if ((reinterpret_cast<uintptr_t>(p.w2) & 15) == 0) {  // every load of the middle layer in flight at once
    constexpr int N4 = kMlpH * kMlpH / 4 / kMlpThreads;
    const float4 *__restrict__ w4 = reinterpret_cast<const float4 *>(p.w2);
    float4 v[N4];
#pragma unroll
    for (int i = 0; i < N4; ++i) v[i] = w4[tid + i * kMlpThreads];
#pragma unroll
    for (int i = 0; i < N4; ++i) {
      const int e = (tid + i * kMlpThreads) * 4;
      *reinterpret_cast<float4 *>(&s.w2[(e >> 7) * kMlpLdw + (e & (kMlpH - 1))]) = v[i];
    }
  } else {
#pragma unroll 8
    for (int i = tid; i < kMlpH * kMlpH; i += kMlpThreads) s.w2[(i >> 7) * kMlpLdw + (i & (kMlpH - 1))] = p.w2[i];
  }
  const int D8 = (D + 7) & ~7;
#pragma unroll 4
  for (int i = tid; i < kMlpH * D8; i += kMlpThreads) {
    const int j = i / D8, k = i - j * D8;
    s.w1[j * kMlpLd1 + k] = k < D ? p.w1[j * D + k] : 0.0f;
  }
#pragma unroll 4
  for (int i = tid; i < A * kMlpH; i += kMlpThreads) s.w3[(i >> 7) * kMlpLdw + (i & (kMlpH - 1))] = p.w3[i];
  if (tid < kMlpH) {
    s.b1[tid] = p.b1[tid];
    s.b2[tid] = p.b2[tid];
  }
  if (tid < A) s.b3[tid] = p.b3[tid];
}

// The forward of the kMlpRows rows in xs (dense_load_x) through the net staged in s (mlp_stage_net):
// s.h1 / s.h2 = the hidden activations, s.q = Q.  Starts and ends with a workgroup barrier.
__device__ inline void mlp_forward_rows(const float (*xs)[kMlpMaxD], int D, int A, MlpSmem &s) {
  const int tid = threadIdx.x, j = tid & (kMlpH - 1), rb = (tid >> 7) * kMlpRpt;
  __syncthreads();
  {  // layer 1: hidden unit j of kMlpRpt rows
    float acc[kMlpRpt][8] = {};
    const float *w = s.w1 + j * kMlpLd1;
    for (int k0 = 0; k0 < D; k0 += 8) {
      const float4 wa = *reinterpret_cast<const float4 *>(w + k0);
      const float4 wb = *reinterpret_cast<const float4 *>(w + k0 + 4);
#pragma unroll
      for (int rr = 0; rr < kMlpRpt; ++rr) {
        const float4 xa = *reinterpret_cast<const float4 *>(&xs[rb + rr][k0]);
        const float4 xb = *reinterpret_cast<const float4 *>(&xs[rb + rr][k0 + 4]);
        dense_fma8(xa, xb, wa, wb, acc[rr]);
      }
    }
    const float b = s.b1[j];
#pragma unroll
    for (int rr = 0; rr < kMlpRpt; ++rr) s.h1[rb + rr][j] = dense_relu(radd(dense_tree8(acc[rr]), b));
  }
  __syncthreads();
  {  // layer 2 from LDS
    float acc[kMlpRpt][8] = {};
    const float *w = s.w2 + j * kMlpLdw;
#pragma unroll 2
    for (int k0 = 0; k0 < kMlpH; k0 += 8) {
      const float4 wa = *reinterpret_cast<const float4 *>(w + k0);
      const float4 wb = *reinterpret_cast<const float4 *>(w + k0 + 4);
#pragma unroll
      for (int rr = 0; rr < kMlpRpt; ++rr) {
        const float4 xa = *reinterpret_cast<const float4 *>(&s.h1[rb + rr][k0]);
        const float4 xb = *reinterpret_cast<const float4 *>(&s.h1[rb + rr][k0 + 4]);
        dense_fma8(xa, xb, wa, wb, acc[rr]);
      }
    }
    const float b = s.b2[j];
#pragma unroll
    for (int rr = 0; rr < kMlpRpt; ++rr) s.h2[rb + rr][j] = dense_relu(radd(dense_tree8(acc[rr]), b));
  }
  __syncthreads();
  if (tid < kMlpRows * A) {  // layer 3: one lane per (row, action)
    const int r = tid / A, a = tid % A;
    float acc[8] = {};
    const float *w = s.w3 + a * kMlpLdw;
#pragma unroll 2
    for (int k0 = 0; k0 < kMlpH; k0 += 8) {
      const float4 wa = *reinterpret_cast<const float4 *>(w + k0);
      const float4 wb = *reinterpret_cast<const float4 *>(w + k0 + 4);
      const float4 xa = *reinterpret_cast<const float4 *>(&s.h2[r][k0]);
      const float4 xb = *reinterpret_cast<const float4 *>(&s.h2[r][k0 + 4]);
      dense_fma8(xa, xb, wa, wb, acc);
    }
    s.q[r][a] = radd(dense_tree8(acc), s.b3[a]);
  }
  __syncthreads();
}

// dense_load_x into s.x behind a barrier (the previous tile is done with s), then the forward
__device__ inline void mlp_forward_tile(const float *__restrict__ x, int64_t ldx, int64_t n, int64_t r0, int D, int A,
                                        MlpSmem &s) {
  __syncthreads();
  dense_load_x(x, ldx, n, r0, D, s.x);
  mlp_forward_rows(s.x, D, A, s);
}

// s.q's rows of this tile to q [n, A]
__device__ inline void mlp_store_q(const MlpSmem &s, float *__restrict__ q, int64_t n, int64_t r0, int A) {
  const int tid = threadIdx.x;
  if (tid < kMlpRows * A) {
    const int r = tid / A, a = tid % A;
    if (r0 + r < n) q[(r0 + r) * A + a] = s.q[r][a];
  }
}

__global__ __launch_bounds__(kMlpThreads) void k_mlp_q(DenseNet p, const float *__restrict__ x, int64_t ldx, int64_t n,
                                                       int D, int A, float *__restrict__ q,
                                                       int32_t *__restrict__ amax) {
  __shared__ __align__(16) MlpSmem s;
  mlp_stage_net(p, D, A, s);
  const int64_t tiles = (n + kMlpRows - 1) / kMlpRows;
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * kMlpRows;
    mlp_forward_tile(x, ldx, n, r0, D, A, s);
    mlp_store_q(s, q, n, r0, A);
    if (amax && threadIdx.x < kMlpRows && r0 + threadIdx.x < n)
      amax[r0 + threadIdx.x] = argmax_first(s.q[threadIdx.x], A);  // torch.argmax: the first maximum
  }
}

// rth_mlp_dqn_grads' first launch.  Per tile of rows: Q_tgt(s1) with the target weights staged (to
// the workspace), then with the online weights staged -- the tile's s0 / s1 rows, batch columns and
// Q_tgt rows fetched in one round trip -- Q(s1) (double_q), Q(s0), the TD / Huber row arithmetic
// (td_huber_row on the three Q row blocks in LDS: |td|, the loss element, dQ) and -- backward -- the
// data gradients of the online net's three layers; the activations and pre-activation gradients
// go to the workspace for the second launch, stored at the tile's end (no barrier waits on them).
__global__ __launch_bounds__(kMlpThreads) void k_mlp_td(
    DenseNet on, DenseNet tg, const float *__restrict__ s0, int64_t lds0, const float *__restrict__ s1, int64_t lds1,
    const int64_t *__restrict__ act, const float *__restrict__ rew, const float *__restrict__ done,
    const double *__restrict__ isw, int64_t B, int D, int A, float gamma_n, int double_q, int backward,
    float *__restrict__ wsp, float *__restrict__ td_abs) {
  __shared__ __align__(16) MlpSmem s;
  const MlpWs ws(wsp, B, A);
  const int tid = threadIdx.x, j = tid & (kMlpH - 1), rb = (tid >> 7) * kMlpRpt;
  const int64_t tiles = (B + kMlpRows - 1) / kMlpRows;
  const float invB = 1.0f / (float)B;
  mlp_stage_net(tg, D, A, s);
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    mlp_forward_tile(s1, lds1, B, t * kMlpRows, D, A, s);
    mlp_store_q(s, ws.q1t, B, t * kMlpRows, A);
  }
  __syncthreads();
  mlp_stage_net(on, D, A, s);
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int64_t r0 = t * kMlpRows;
    const bool qlane = tid < kMlpRows * A;  // lane (r, a) = tid of the tile's Q row blocks
    const int qr = tid / A, qa = tid % A;
    __syncthreads();
    dense_load_x(s0, lds0, B, r0, D, s.x);
    if (double_q) dense_load_x(s1, lds1, B, r0, D, s.x1);
    if (qlane) s.tq1t[tid] = r0 + qr < B ? ws.q1t[(r0 + qr) * A + qa] : 0.0f;  // written by this workgroup above
    if (tid >= kMlpH && tid < kMlpH + kMlpRows && r0 + (tid - kMlpH) < B) {
      const int r = tid - kMlpH;
      s.act[r] = act[r0 + r];
      s.rew[r] = rew[r0 + r];
      s.done[r] = done[r0 + r];
      if (isw) s.isw[r] = isw[r0 + r];
    }
    if (double_q) {
      mlp_forward_rows(s.x1, D, A, s);
      if (qlane) s.tq1o[tid] = s.q[qr][qa];
    }
    mlp_forward_rows(s.x, D, A, s);
    if (qlane) s.tq0[tid] = s.q[qr][qa];
    __syncthreads();
    if (tid < kMlpRows) {
      if (r0 + tid < B) {
        float l;
        const float td = td_huber_row(s.tq0, s.tq1o, s.tq1t, s.act, s.rew, s.done, isw ? s.isw : nullptr, tid, A, 0,
                                      gamma_n, double_q, invB, &l, backward ? s.g3[tid] : nullptr);
        ws.le[r0 + tid] = l;
        if (td_abs) td_abs[r0 + tid] = fabsf(td);
      } else {
        for (int a = 0; a < A; ++a) s.g3[tid][a] = 0.0f;
      }
    }
    if (!backward) continue;
    __syncthreads();
    // layer 3's data gradient, ReLU mask: g2 = (h2 > 0) ? g3 W3 : 0
#pragma unroll
    for (int rr = 0; rr < kMlpRpt; ++rr) {
      const int r = rb + rr;
      float acc = 0.0f;
      for (int a = 0; a < A; ++a) acc = fmaf(s.g3[r][a], s.w3[a * kMlpLdw + j], acc);
      s.g2[r][j] = s.h2[r][j] > 0.0f ? acc : 0.0f;
    }
    __syncthreads();
    {  // layer 2's data gradient down the staged weight's columns: g1 = (h1 > 0) ? g2 W2 : 0
      float acc[kMlpRpt][8] = {};
#pragma unroll 2
      for (int j0 = 0; j0 < kMlpH; j0 += 8) {
        float wv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) wv[i] = s.w2[(j0 + i) * kMlpLdw + j];
        const float4 wa = make_float4(wv[0], wv[1], wv[2], wv[3]), wb = make_float4(wv[4], wv[5], wv[6], wv[7]);
#pragma unroll
        for (int rr = 0; rr < kMlpRpt; ++rr) {
          const float4 ga = *reinterpret_cast<const float4 *>(&s.g2[rb + rr][j0]);
          const float4 gb = *reinterpret_cast<const float4 *>(&s.g2[rb + rr][j0 + 4]);
          dense_fma8(ga, gb, wa, wb, acc[rr]);
        }
      }
#pragma unroll
      for (int rr = 0; rr < kMlpRpt; ++rr) {
        const int r = rb + rr;
        if (r0 + r < B) {
          const int64_t o = (r0 + r) * kMlpH + j;
          ws.g1[o] = s.h1[r][j] > 0.0f ? dense_tree8(acc[rr]) : 0.0f;
          ws.g2[o] = s.g2[r][j];
          ws.h2[o] = s.h2[r][j];
          ws.h1[o] = s.h1[r][j];
        }
      }
    }
    if (qlane && r0 + qr < B) ws.g3[(r0 + qr) * A + qa] = s.g3[qr][qa];
  }
}

// rth_mlp_dqn_grads' second launch: workgroups [0, 32) the middle layer's weight gradient, [32, 64)
// the first layer's, then ceil(A / 4) for the last layer's, three for the bias gradients and the
// last one the loss mean (k_td_huber's per-lane sums and LDS tree); without gradients only the mean
__global__ __launch_bounds__(kDenseGradThreads) void k_mlp_wgrad(DenseGrads g, const float *__restrict__ s0,
                                                                 int64_t lds0, int64_t B, int D, int A,
                                                                 float *__restrict__ wsp, float *__restrict__ loss,
                                                                 int first) {
  __shared__ float part[kDenseGradThreads];
  const MlpWs ws(wsp, B, A);
  constexpr int T = kMlpH / kDenseGradJ;
  const int a_tiles = (A + kDenseGradJ - 1) / kDenseGradJ;
  int blk = (int)blockIdx.x + first;
  if (blk < T) return dense_wgrad_tile(ws.g2, kMlpH, kMlpH, ws.h1, kMlpH, kMlpH, B, blk * kDenseGradJ, 0, g.w2);
  blk -= T;
  if (blk < T) return dense_wgrad_tile(ws.g1, kMlpH, kMlpH, s0, lds0, D, B, blk * kDenseGradJ, 0, g.w1);
  blk -= T;
  if (blk < a_tiles) return dense_wgrad_tile(ws.g3, A, A, ws.h2, kMlpH, kMlpH, B, blk * kDenseGradJ, 0, g.w3);
  blk -= a_tiles;
  if (blk == 0) return dense_bgrad(ws.g1, kMlpH, kMlpH, B, 0, g.b1);
  if (blk == 1) return dense_bgrad(ws.g2, kMlpH, kMlpH, B, 0, g.b2);
  if (blk == 2) return dense_bgrad(ws.g3, A, A, B, 0, g.b3);
  const float sum = dense_loss_sum(ws.le, B, part);
  if (threadIdx.x == 0 && loss) loss[0] = sum * (1.0f / (float)B);
}

inline bool mlp_shape_ok(int64_t D, int64_t H, int64_t A) {
  return H == kMlpH && D >= 1 && D <= kMlpMaxD && A >= 1 && A <= kMlpMaxA;
}

}  // namespace rth

extern "C" {

int rth_mlp_supported(int64_t D, int64_t H, int64_t A) { return rth::mlp_shape_ok(D, H, A) ? 1 : 0; }

int64_t rth_mlp_workspace(int64_t B, int64_t D, int64_t H, int64_t A) {
  using namespace rth;
  RTH_REQUIRE(mlp_shape_ok(D, H, A) && B >= 1 && B <= (int64_t)1 << 40,
              "rth_mlp_workspace: unsupported shape B=%lld D=%lld H=%lld A=%lld (H = 128, D in 1..64, A in 1..18)",
              (long long)B, (long long)D, (long long)H, (long long)A);
  return (MlpWs::floats(B, A) * 4 + 15) / 16 * 16;
}

int rth_mlp_q(const float *const *params, const float *x_dev, int64_t ldx, int64_t n, int64_t D, int64_t H, int64_t A,
              float *q_dev, int32_t *argmax_dev, void *stream) {
  using namespace rth;
  RTH_REQUIRE(mlp_shape_ok(D, H, A), "rth_mlp_q: unsupported shape D=%lld H=%lld A=%lld (H = 128, D in 1..64, A in 1..18)",
              (long long)D, (long long)H, (long long)A);
  RTH_REQUIRE(n >= 1 && ldx >= D, "rth_mlp_q: bad n=%lld or ldx=%lld < D=%lld", (long long)n, (long long)ldx,
              (long long)D);
  DenseNet p;
  RTH_REQUIRE(dense_net(params, &p) && x_dev && q_dev, "rth_mlp_q: NULL argument");
  hipLaunchKernelGGL(k_mlp_q, dim3(dense_grid(n)), dim3(kMlpThreads), 0, as_stream(stream), p, x_dev, ldx, n, (int)D,
                     (int)A, q_dev, argmax_dev);
  RTH_LAUNCHED();
  return RTH_OK;
}

int rth_mlp_dqn_grads(const float *const *online, const float *const *target, const float *s0_dev, int64_t lds0,
                      const float *s1_dev, int64_t lds1, const int64_t *a_dev, const float *r_dev,
                      const float *done_dev, const double *isw_dev, int64_t B, int64_t D, int64_t H, int64_t A,
                      float gamma_n, int32_t double_q, float *const *grads, float *td_abs_dev, float *loss_dev,
                      void *workspace_dev, void *stream) {
  using namespace rth;
  RTH_REQUIRE(mlp_shape_ok(D, H, A),
              "rth_mlp_dqn_grads: unsupported shape D=%lld H=%lld A=%lld (H = 128, D in 1..64, A in 1..18)",
              (long long)D, (long long)H, (long long)A);
  RTH_REQUIRE(B >= 1 && B <= (int64_t)1 << 40 && lds0 >= D && lds1 >= D,
              "rth_mlp_dqn_grads: bad B=%lld or row stride (%lld, %lld) < D=%lld", (long long)B, (long long)lds0,
              (long long)lds1, (long long)D);
  DenseNet on, tg;
  RTH_REQUIRE(dense_net(online, &on) && dense_net(target, &tg) && s0_dev && s1_dev && a_dev && r_dev && done_dev &&
                  workspace_dev,
              "rth_mlp_dqn_grads: NULL argument");
  DenseGrads g{};
  if (grads) {
    for (int i = 0; i < 6; ++i) RTH_REQUIRE(grads[i], "rth_mlp_dqn_grads: NULL gradient buffer %d", i);
    g = DenseGrads{grads[0], grads[1], grads[2], grads[3], grads[4], grads[5]};
  }
  float *ws = static_cast<float *>(workspace_dev);
  hipLaunchKernelGGL(k_mlp_td, dim3(dense_grid(B)), dim3(kMlpThreads), 0, as_stream(stream), on, tg, s0_dev, lds0,
                     s1_dev, lds1, a_dev, r_dev, done_dev, isw_dev, B, (int)D, (int)A, gamma_n, (int)(double_q != 0),
                     (int)(grads != nullptr), ws, td_abs_dev);
  RTH_LAUNCHED();
  const int grad_blocks = 2 * (kMlpH / kDenseGradJ) + (int)((A + kDenseGradJ - 1) / kDenseGradJ) + 3;
  if (grads) {  // every gradient element, then the loss mean
    hipLaunchKernelGGL(k_mlp_wgrad, dim3(grad_blocks + 1), dim3(kDenseGradThreads), 0, as_stream(stream), g, s0_dev, lds0,
                       B, (int)D, (int)A, ws, loss_dev, 0);
    RTH_LAUNCHED();
  } else if (loss_dev) {
    hipLaunchKernelGGL(k_mlp_wgrad, dim3(1), dim3(kDenseGradThreads), 0, as_stream(stream), g, s0_dev, lds0, B, (int)D,
                       (int)A, ws, loss_dev, grad_blocks);
    RTH_LAUNCHED();
  }
  return RTH_OK;
}

}  // extern "C"
