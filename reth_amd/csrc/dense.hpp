// What the fused fp32 dense families (mlp.hpp, ddpg.hpp) share: a network of three Linear layers
// as six pointers, the row loader of a tile, the fmaf / tree primitives of the ONE summation order
// of a dot product (term k to accumulator k % 8 in increasing k, the eight added as
// ((0+1)+(2+3))+((4+5)+(6+7))) and the batch reductions of the second launch (row b to accumulator
// b % 4 in increasing b, then (0+1)+(2+3), per output element; the loss: per-lane strided sums,
// then an LDS tree): no atomics, identical run to run, whatever the grid.  How a layer's weights
// reach the multiply (resident in LDS, or streamed in chunks) is each family's own.
#pragma once
#include "common.hpp"

namespace rth {

constexpr int kDenseRows = 8, kDenseMaxD = 64;  // a tile: rows per workgroup pass x the widest input row
constexpr int kDenseThreads = 256;
constexpr int kDenseMaxBlocks = 1024;
constexpr int kDenseGradThreads = 128, kDenseGradJ = 4;  // second launch: 4 output rows x 128 columns per workgroup

struct DenseNet {  // weight [H1, D], bias, weight [H2, K2], bias, weight [N3, H2], bias (torch layout)
  const float *w1, *b1, *w2, *b2, *w3, *b3;
};

struct DenseGrads {
  float *w1, *b1, *w2, *b2, *w3, *b3;
};

// a host array of six non-NULL device pointers into a DenseNet
inline bool dense_net(const float *const *params, DenseNet *out) {
  if (!params) return false;
  for (int i = 0; i < 6; ++i)
    if (!params[i]) return false;
  *out = DenseNet{params[0], params[1], params[2], params[3], params[4], params[5]};
  return true;
}

// workgroups for `rows` rows walked in tiles of kDenseRows: one per tile, capped
inline unsigned dense_grid(int64_t rows) {
  const int64_t tiles = (rows + kDenseRows - 1) / kDenseRows;
  return (unsigned)(tiles < kDenseMaxBlocks ? tiles : kDenseMaxBlocks);
}

__device__ __forceinline__ float dense_relu(float v) { return v < 0.0f ? 0.0f : v; }  // NaN passes, like torch
__device__ __forceinline__ float dense_tree8(const float (&a)[8]) {
  return radd(radd(radd(a[0], a[1]), radd(a[2], a[3])), radd(radd(a[4], a[5]), radd(a[6], a[7])));
}
__device__ __forceinline__ void dense_fma8(const float4 &xa, const float4 &xb, const float4 &wa, const float4 &wb,
                                           float (&acc)[8]) {
  acc[0] = fmaf(xa.x, wa.x, acc[0]);
  acc[1] = fmaf(xa.y, wa.y, acc[1]);
  acc[2] = fmaf(xa.z, wa.z, acc[2]);
  acc[3] = fmaf(xa.w, wa.w, acc[3]);
  acc[4] = fmaf(xb.x, wb.x, acc[4]);
  acc[5] = fmaf(xb.y, wb.y, acc[5]);
  acc[6] = fmaf(xb.z, wb.z, acc[6]);
  acc[7] = fmaf(xb.w, wb.w, acc[7]);
}

// rows [r0, r0 + kDenseRows) of x [n, D] (row stride ldx) into xs, zero past n and past D: nothing
// outside [0, n) x [0, D) is read.  No barrier.
__device__ inline void dense_load_x(const float *__restrict__ x, int64_t ldx, int64_t n, int64_t r0, int D,
                                    float (*xs)[kDenseMaxD]) {
  for (int i = threadIdx.x; i < kDenseRows * kDenseMaxD; i += kDenseThreads) {
    const int r = i / kDenseMaxD, k = i % kDenseMaxD;
    xs[r][k] = (r0 + r < n && k < D) ? x[(r0 + r) * ldx + k] : 0.0f;
  }
}

// gw[n][k] = sum_b G[b][n] X[b][k] for the rows n in [n0, n0 + kDenseGradJ) and the columns
// k = k0 + lane of one layer: row b to accumulator b % 4
__device__ inline void dense_wgrad_tile(const float *__restrict__ G, int64_t ldg, int N, const float *__restrict__ X,
                                        int64_t ldx, int K, int64_t B, int n0, int k0, float *__restrict__ gw) {
  const int k = k0 + (int)threadIdx.x;
  if (k >= K) return;
  float acc[kDenseGradJ][4] = {};
  int nn[kDenseGradJ];
#pragma unroll
  for (int i = 0; i < kDenseGradJ; ++i) nn[i] = n0 + i < N ? n0 + i : N - 1;  // clamped: read in bounds, not stored
  int64_t b = 0;
#pragma unroll 4
  for (; b + 4 <= B; b += 4) {  // (unrolled: 16 rows' loads in flight; the order of the sums is unchanged)
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float x = X[(b + u) * ldx + k];
#pragma unroll
      for (int i = 0; i < kDenseGradJ; ++i) acc[i][u] = fmaf(G[(b + u) * ldg + nn[i]], x, acc[i][u]);
    }
  }
#pragma unroll
  for (int u = 0; u < 3; ++u) {
    if (b + u < B) {
      const float x = X[(b + u) * ldx + k];
#pragma unroll
      for (int i = 0; i < kDenseGradJ; ++i) acc[i][u] = fmaf(G[(b + u) * ldg + nn[i]], x, acc[i][u]);
    }
  }
#pragma unroll
  for (int i = 0; i < kDenseGradJ; ++i)
    if (n0 + i < N) gw[(int64_t)(n0 + i) * K + k] = radd(radd(acc[i][0], acc[i][1]), radd(acc[i][2], acc[i][3]));
}

// gb[n] = sum_b G[b][n], n = n0 + lane, the same order over b
__device__ inline void dense_bgrad(const float *__restrict__ G, int64_t ldg, int N, int64_t B, int n0,
                                   float *__restrict__ gb) {
  const int n = n0 + (int)threadIdx.x;
  if (n >= N) return;
  float acc[4] = {};
  int64_t b = 0;
#pragma unroll 4
  for (; b + 4 <= B; b += 4) {
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = radd(acc[u], G[(b + u) * ldg + n]);
  }
#pragma unroll
  for (int u = 0; u < 3; ++u)
    if (b + u < B) acc[u] = radd(acc[u], G[(b + u) * ldg + n]);
  gb[n] = radd(radd(acc[0], acc[1]), radd(acc[2], acc[3]));
}

// sum_b le[b] by one workgroup of kDenseGradThreads lanes: lane l sums b = l (mod 128) in increasing
// b, then a tree over `part` (LDS).  The sum is lane 0's return value; the caller scales it.
__device__ inline float dense_loss_sum(const float *__restrict__ le, int64_t B, float (&part)[kDenseGradThreads]) {
  float acc = 0.0f;
  for (int64_t b = threadIdx.x; b < B; b += kDenseGradThreads) acc = radd(acc, le[b]);
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int st = kDenseGradThreads / 2; st > 0; st >>= 1) {
    if ((int)threadIdx.x < st) part[threadIdx.x] = radd(part[threadIdx.x], part[threadIdx.x + st]);
    __syncthreads();
  }
  return part[0];
}

}  // namespace rth
