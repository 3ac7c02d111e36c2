// PPO's shuffled minibatch epochs: rth_ppo_shuffle draws a counter-based permutation of a batch's
// first n rows on the device (n is known only there) and lays the batch out as K dense minibatches
// of pitch Mcap = ceil(B / K) rows, each of which rth_ppo_grads_n / rth_ppo_grads_adv then takes
// through a pointer into the copy with its own device row count mb_n[m].  The gradient kernels do
// not change.
//
// Keys.  key_i = keys_in[i] where given, else all 64 bits c[0] | c[1] << 32 of Philox4x32-10 on the
// block {lane = i, (uint32) c, (uint32) (c >> 32), STREAM_PPO_SHUFFLE} with c = counter[0] and the
// key (seed lo, seed hi).  perm is the STABLE argsort of key[0..n): position q of row i is the
// number of rows j < n with key_j < key_i, or key_j == key_i and j < i -- a total order, so q is a
// bijection onto [0, n) and every destination has exactly one writer: no atomics.
//
// Two launches.  k_ppo_shuffle_keys reads the counter and writes the n keys to the workspace;
// k_ppo_shuffle_rank counts every row's position against all keys, which the workgroup walks in LDS
// tiles of kShufTile, writes perm, gathers the rows and, in workgroup 0, writes mb_n and advances the
// counter -- in a later launch than the one that read it (k_ppo_gae_clear's rule).  Counting is n^2 comparisons: 4 M at the loop's
// 2,048 rows, 4 G at the entry point's limit of 65,536.
#pragma once
#include "ppo.hpp"

namespace rth {

constexpr uint32_t STREAM_PPO_SHUFFLE = 14u;  // the shuffle keys' Philox stream word
constexpr int kShufThreads = 256;
constexpr int kShufTile = 1024;  // keys per LDS tile (8 KB)
constexpr int64_t kShufMaxB = 65536, kShufMaxK = 64;

__global__ __launch_bounds__(kShufThreads) void k_ppo_shuffle_keys(int64_t cap, const int64_t *__restrict__ n_dev,
                                                                   uint64_t seed,
                                                                   const int64_t *__restrict__ counter,
                                                                   const uint64_t *__restrict__ keys_in,
                                                                   uint64_t *__restrict__ keys) {
  const int64_t n = ppo_rows(cap, n_dev);
  const int64_t i = (int64_t)blockIdx.x * kShufThreads + threadIdx.x;
  if (i >= n) return;
  if (keys_in) {
    keys[i] = keys_in[i];
    return;
  }
  const uint64_t ctr = (uint64_t)counter[0];
  uint32_t c[4] = {(uint32_t)i, (uint32_t)ctr, (uint32_t)(ctr >> 32), STREAM_PPO_SHUFFLE};
  philox4x32(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  keys[i] = (uint64_t)c[0] | ((uint64_t)c[1] << 32);
}

struct PpoShuffleCols {  // the batch's columns and their minibatch copies (adv / mb_adv: both or neither)
  const uint32_t *s;
  const int64_t *a;
  const uint32_t *ret, *adv, *logp;
  uint32_t *mb_s;
  int64_t *mb_a;
  uint32_t *mb_ret, *mb_adv, *mb_logp;
};

// kShufSplit lanes share a row: lanes 16 r .. 16 r + 15 of workgroup g own row i = g * kShufRows + r, lane
// u of them counts the keys j = u (mod 16), and a butterfly over the 16 lanes adds the counts (integers:
// the order is free).  Sixteen neighbouring lanes read sixteen neighbouring keys of the LDS tile and
// the wave's four rows read the same ones: no bank conflict.  At the loop's 2,048 rows that is 128
// workgroups of 128 comparisons a lane, where one lane a row would leave 8 workgroups walking 2,048
// each.  Rows are copied as 32-bit words, so a NaN's payload and a zero's sign arrive as they were.
constexpr int kShufSplit = 16, kShufRows = kShufThreads / kShufSplit;
static_assert(kShufTile % kShufSplit == 0 && 64 % kShufSplit == 0, "a row's lanes sit in one wave");

__global__ __launch_bounds__(kShufThreads) void k_ppo_shuffle_rank(PpoShuffleCols c, int64_t lds, int64_t cap,
                                                                   const int64_t *__restrict__ n_dev, int D, int K,
                                                                   const uint64_t *__restrict__ keys,
                                                                   int64_t *__restrict__ counter,
                                                                   int64_t *__restrict__ mb_n,
                                                                   int32_t *__restrict__ perm) {
  __shared__ __align__(16) uint64_t tile[kShufTile];
  __shared__ int64_t dst[kShufRows];
  const int tid = threadIdx.x, u = tid & (kShufSplit - 1), r = tid / kShufSplit;
  const int64_t n = ppo_rows(cap, n_dev);
  const int64_t M = (n + K - 1) / K, Mcap = (cap + K - 1) / K;
  if (blockIdx.x == 0) {  // every workgroup has its own copy of n: nothing below reads these
    if (tid < K) {
      const int64_t left = n - (int64_t)tid * M;
      mb_n[tid] = left < 0 ? 0 : (left < M ? left : M);
    }
    if (tid == 0) counter[0] += 1;
  }
  const int64_t i0 = (int64_t)blockIdx.x * kShufRows;
  if (i0 >= n) return;  // (uniform)
  const int64_t i = i0 + r;
  const bool live = i < n;
  const uint64_t mine = live ? keys[i] : 0;
  const int ii = (int)i, nn = (int)n;  // (n <= 65,536)
  int q = 0;
  for (int j0 = 0; j0 < nn; j0 += kShufTile) {
    const int nt = nn - j0 < kShufTile ? nn - j0 : kShufTile;
    __syncthreads();  // the previous tile has been read
    for (int t = tid; t < nt; t += kShufThreads) tile[t] = keys[j0 + t];
    __syncthreads();
    // row j comes first where its key is smaller, or equal and j < i
#pragma unroll 4
    for (int t = u; t < nt; t += kShufSplit) {
      const uint64_t k = tile[t];
      q += (k < mine) | ((k == mine) & (j0 + t < ii)) ? 1 : 0;
    }
  }
#pragma unroll
  for (int o = kShufSplit / 2; o > 0; o >>= 1) q += __shfl_xor(q, o, kShufSplit);  // (every lane of the wave is here)
  if (live && u == 0) {
    const int m = q / (int)M, j = q - m * (int)M;  // (n >= 1 here, so M >= 1)
    const int64_t d = (int64_t)m * Mcap + j;
    dst[r] = d;
    perm[q] = (int32_t)i;
    c.mb_a[d] = c.a[i];
    c.mb_ret[d] = c.ret[i];
    c.mb_logp[d] = c.logp[i];
    if (c.adv) c.mb_adv[d] = c.adv[i];
  }
  __syncthreads();
  const int rows = (int)(n - i0 < kShufRows ? n - i0 : kShufRows);
  for (int e = tid; e < rows * D; e += kShufThreads) {
    const int rr = e / D, k = e - rr * D;
    c.mb_s[dst[rr] * D + k] = c.s[(i0 + rr) * lds + k];
  }
}

}  // namespace rth

extern "C" {

int64_t rth_ppo_shuffle_workspace(int64_t B) {
  using namespace rth;
  RTH_REQUIRE(B >= 1 && B <= kShufMaxB, "rth_ppo_shuffle_workspace: bad B=%lld (1..65536)", (long long)B);
  return (B * 8 + 15) / 16 * 16;
}

int rth_ppo_shuffle(const float *s_dev, int64_t lds, const int64_t *a_dev, const float *ret_dev, const float *adv_dev,
                    const float *old_logprob_dev, int64_t B, const int64_t *n_dev, int64_t D, int64_t K, uint64_t seed,
                    int64_t *counter_dev, const uint64_t *keys_in, float *mb_s_dev, int64_t *mb_a_dev,
                    float *mb_ret_dev, float *mb_adv_dev, float *mb_logprob_dev, int64_t *mb_n_dev, int32_t *perm_dev,
                    void *workspace_dev, void *stream) {
  using namespace rth;
  RTH_REQUIRE(B >= 1 && B <= kShufMaxB && D >= 1 && D <= kPpoMaxD && K >= 1 && K <= kShufMaxK && K <= B && lds >= D,
              "rth_ppo_shuffle: bad B=%lld (1..65536), D=%lld (1..64), K=%lld (1..64, <= B) or row stride %lld < D",
              (long long)B, (long long)D, (long long)K, (long long)lds);
  RTH_REQUIRE(s_dev && a_dev && ret_dev && old_logprob_dev && counter_dev && mb_s_dev && mb_a_dev && mb_ret_dev &&
                  mb_logprob_dev && mb_n_dev && perm_dev && workspace_dev,
              "rth_ppo_shuffle: NULL argument");
  RTH_REQUIRE((adv_dev == nullptr) == (mb_adv_dev == nullptr),
              "rth_ppo_shuffle: adv_dev and mb_adv_dev are given together or not at all");
  auto w = [](const float *p) { return reinterpret_cast<const uint32_t *>(p); };
  auto wm = [](float *p) { return reinterpret_cast<uint32_t *>(p); };
  const PpoShuffleCols c{w(s_dev),     a_dev,    w(ret_dev),     w(adv_dev),     w(old_logprob_dev),
                         wm(mb_s_dev), mb_a_dev, wm(mb_ret_dev), wm(mb_adv_dev), wm(mb_logprob_dev)};
  uint64_t *keys = static_cast<uint64_t *>(workspace_dev);
  const unsigned grid = (unsigned)((B + kShufThreads - 1) / kShufThreads);
  const unsigned rank_grid = (unsigned)((B + kShufRows - 1) / kShufRows);
  hipLaunchKernelGGL(k_ppo_shuffle_keys, dim3(grid), dim3(kShufThreads), 0, as_stream(stream), B, n_dev, seed,
                     counter_dev, keys_in, keys);
  RTH_LAUNCHED();
  hipLaunchKernelGGL(k_ppo_shuffle_rank, dim3(rank_grid), dim3(kShufThreads), 0, as_stream(stream), c, lds, B, n_dev,
                     (int)D, (int)K, keys, counter_dev, mb_n_dev, perm_dev);
  RTH_LAUNCHED();
  return RTH_OK;
}

}  // extern "C"
