// Nature-DQN convolution torso forward on gfx950: relu(conv2d(x, W) + b) as an implicit GEMM
// on the fp32 MFMA (v_mfma_f32_16x16x4_f32), bias and ReLU applied to the accumulators, NHWC
// fp32 output.  Reference: reth/reth/algorithm/dqn/dqn_model.py:14-20 (Conv2d(4,32,8,4) ->
// ReLU -> Conv2d(32,64,4,2) -> ReLU -> Conv2d(64,64,3,1) -> ReLU).
//
// GEMM view: rows = output pixels (n, oy, ox), columns = output channels, K = (kh, kw, ci).
//   * one wave owns a tile of 16 output pixels x all COUT channels (COUT/16 accumulators of
//     4 registers); the A operand (input window) is read straight from global memory into
//     registers, the B operand (weights) from LDS;
//   * the whole weight tensor is staged once per workgroup in LDS in MFMA fragment order
//     [chunk g][channel block nb][lane][t], so every B read is one conflict-free ds_read_b128
//     feeding four k-steps;
//   * K is walked in chunks of 16 values: lane (m = lane & 15, q = lane >> 4) holds 4
//     consecutive values of the input window (one float4), k-step t of the chunk multiplies
//     value t -- the k order is a permutation of (kh, kw, ci), the weights are staged in the
//     same permutation.
//
// Input: x = [n, HIN, WIN, CIN] fp32 (RTH_CONV_F32_NHWC: the previous layer's output, or a
// channels-last batch); K runs are kh rows of KW*CIN contiguous floats.  (uint8 frame stacks,
// RTH_CONV_U8_CHW, are conv1's alone and run on the bf16 MFMA: conv1_u8.hpp.)
//
// Numerics: each output is an fp32 fma chain over K in the permuted order above (MFMA f32 is
// a k-ordered fmaf chain), then + bias, then ReLU -- the same operations as conv -> bias ->
// relu, summed in a different order than MIOpen's or the reference's CPU convolution.
#pragma once

#include <type_traits>

#include "common.hpp"

namespace rth {

using f32x4 = __attribute__((ext_vector_type(4))) float;
using f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ float relu_c(float v) { return v < 0.0f ? 0.0f : v; }  // NaN passes, like torch

template <int KH, int KW, int S, int CIN, int COUT, int HIN, int WIN>
struct ConvGeom {
  static constexpr int HOUT = (HIN - KH) / S + 1, WOUT = (WIN - KW) / S + 1, PIX = HOUT * WOUT;
  static constexpr int K = KH * KW * CIN, G = K / 16, NB = COUT / 16;
  static constexpr int LDS_F4 = G * NB * 64;  // float4 slots of the staged weights
  // input chunks in flight per wave: a divisor of G, at most 8 / MB
  static constexpr int prefetch(int mb) {
    for (int d = 8 / mb; d > 1; --d)
      if (G % d == 0) return d;
    return 1;
  }
  static_assert(K % 16 == 0 && COUT % 16 == 0, "K and COUT must be multiples of 16");
  static_assert((KW * CIN) % 16 == 0, "unsupported window");

  // the 4 weights of LDS float4 slot sl = (g * NB + nb) * 64 + lane (t = 0..3) from W in
  // OHWI storage: 4 consecutive ci (one 16-byte read)
  __device__ static f32x4 load_slot(const float *__restrict__ w, int sl) {
    const int lane = sl % 64, gn = sl / 64, nb = gn % NB, g = gn / NB;
    const int q = lane >> 4, o = nb * 16 + (lane & 15);
    constexpr int RC = KW * CIN / 16;
    const int kh = g / RC, r = (g % RC) * 16 + 4 * q;  // r = kw * CIN + ci, ci % 4 == 0
    const float4 v = *reinterpret_cast<const float4 *>(w + (int64_t)o * K + kh * KW * CIN + r);
    return f32x4{v.x, v.y, v.z, v.w};
  }
};

// A wave tile is MB blocks of 16 output pixels x all COUT channels.  Every built instantiation
// has MB = 1 (the launcher counts 16-pixel tiles); the axis and its one-trip loops stay because
// the compiler schedules the kernels differently without them (profiles/r18/asm_identity.txt).
// (Measured and removed, DESIGN.md and profiles/history/DESIGN_r01_r05.md: channel-part tiles
// with the part fixed per wave or per workgroup, and a dynamic schedule -- waves claiming tiles
// from a launch-wide atomic counter, r05: 2x slower alone, 108 vs 57 us at 1,024 samples, since
// every claim is an agent-scope atomic on one address from all 8 XCDs.)  rows is unused: uint8
// stacks, which a row index may address, are conv1_u8.hpp's; the forward launcher passes the
// same leading arguments to both.
template <int KH, int KW, int S, int CIN, int COUT, int HIN, int WIN, int WAVES, int MB, int TS = 1>
__global__ __launch_bounds__(WAVES * 64) void k_conv_bias_relu(const void *__restrict__ x,
                                                              const int64_t *__restrict__ rows, int64_t n,
                                                              const int64_t *__restrict__ n_dev,
                                                              const float *__restrict__ w,
                                                              const float *__restrict__ bias,
                                                              float *__restrict__ y, int out_nchw) {
  using Gm = ConvGeom<KH, KW, S, CIN, COUT, HIN, WIN>;
  constexpr int G = Gm::G, NB = Gm::NB, T = WAVES * 64;
  constexpr int TP = 16 * MB;            // output pixels per wave tile
  constexpr int D = Gm::prefetch(MB);  // input chunks in flight per wave
  static_assert(NB % TS == 0, "a split last round needs whole channel blocks per part");
  __shared__ f32x4 wl[Gm::LDS_F4];
  const int64_t wgs = gridDim.x, wgi = blockIdx.x;

  const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int q = lane >> 4, mr = lane & 15;
  if (n_dev) {  // a device-side sample count (<= n): rows past it are neither read nor written
    const int64_t m = *n_dev;
    n = m < n ? (m > 0 ? m : 0) : n;
  }
  const int64_t P = n * Gm::PIX, tiles = (P + TP - 1) / TP, tstride = wgs * WAVES;

  // this lane's window origin in tile t, per M-block (tail lanes read a duplicate pixel)
  auto bases = [&](int64_t t, const uint8_t *(&out)[MB]) {
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
      int64_t p = t * TP + mb * 16 + mr;
      if (p >= P) p = P - 1;
      const int64_t b = p / Gm::PIX;
      const int pp = (int)(p % Gm::PIX), oy = pp / Gm::WOUT, ox = pp % Gm::WOUT;
      out[mb] = reinterpret_cast<const uint8_t *>(static_cast<const float *>(x) +
                                                  ((b * HIN + S * oy) * WIN + S * ox) * CIN + 4 * q);
    }
  };
  // byte offset of chunk g inside the window: kh rows of KW*CIN floats in 16-float chunks
  auto chunk_off = [](int g) -> int {
    constexpr int RC = KW * CIN / 16;
    return 4 * ((g / RC) * WIN * CIN + (g % RC) * 16);
  };
  auto ld = [](const uint8_t *p) { return *reinterpret_cast<const f32x4 *>(p); };

  // wave slots are numbered SIMD-major (waves w and w + 4 of a workgroup share a SIMD): the
  // first gridDim.x * 4 slots put one wave on every SIMD, so a partial last round of tiles
  // lands on distinct SIMDs and no SIMD runs more than ceil(tiles / SIMDs) tiles
  const int64_t slot = WAVES % 4 == 0 ? (int64_t)(wave / 4) * wgs * 4 + wgi * 4 + wave % 4 : wgi * WAVES + wave;
  // Units (r05, TS > 1): the pixel tiles of the whole rounds -- as many as
  // give every SIMD the same count -- run full-width; each pixel tile of the ragged last round
  // is split into TS channel parts (NB / TS blocks each), which the slots continue to take in
  // the same order, so they land on the SIMDs with one tile less: at 1,024 samples the 5,184
  // tiles were 5 or 6 per SIMD, now 5 + at most one quarter.  Same MFMA chain per output.
  const int64_t ptiles = (P + TP - 1) / TP;
  const int64_t per_round = WAVES % 4 == 0 ? wgs * 4 : tstride;  // one slot per SIMD
  const int64_t full = TS > 1 ? ptiles / per_round * per_round : tiles;
  const int64_t total = TS > 1 ? full + (ptiles - full) * TS : tiles;
  auto unit_ptile = [&](int64_t v) -> int64_t { return TS > 1 ? (v < full ? v : full + (v - full) / TS) : v; };
  auto unit_nb0 = [&](int64_t v) -> int {
    if constexpr (TS > 1) return v < full ? 0 : (int)((v - full) % TS) * (NB / TS);
    return 0;
  };
  // the first tile's leading input chunks are requested before the weights are staged
  int64_t v = slot;
  const uint8_t *cur[MB], *nxt[MB];
  bases(unit_ptile(v < total ? v : total - 1), cur);
  f32x4 ar[D][MB];
#pragma unroll
  for (int d = 0; d < D; ++d)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) ar[d][mb] = ld(cur[mb] + chunk_off(d));

  // stage the packed weights (rth_conv_pack: already in fragment order): a coalesced copy,
  // consecutive threads -> consecutive 16-byte LDS slots; all loads first
  {
    constexpr int PER = (Gm::LDS_F4 + T - 1) / T;
    const f32x4 *wp = reinterpret_cast<const f32x4 *>(w);
    f32x4 tmp[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int sl = threadIdx.x + j * T;
      if (sl < Gm::LDS_F4) tmp[j] = wp[sl];
    }
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int sl = threadIdx.x + j * T;
      if (sl < Gm::LDS_F4) wl[sl] = tmp[j];
    }
  }
  __syncthreads();

  float bl[NB];  // the full-width units' bias (nb_first: 0 unless the wave has split units only)
  const int nb_first = unit_nb0(v);
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) bl[nb] = bias[(nb_first + nb) * 16 + mr];
  const f32x4 *wlane = wl + lane;  // this lane's B fragments

  // one unit: NBT channel blocks from nb0 of pixel tile ptile (nxt: the next unit's window)
  auto run = [&](auto nbt, int64_t ptile, int nb0) __attribute__((always_inline)) {
    constexpr int NBT = decltype(nbt)::value;
    float bt[NBT];
    if constexpr (NBT != NB) {
#pragma unroll
      for (int nb = 0; nb < NBT; ++nb) bt[nb] = bias[(nb0 + nb) * 16 + mr];
    } else {
#pragma unroll
      for (int nb = 0; nb < NBT; ++nb) bt[nb] = bl[nb];
    }
    f32x4 acc[MB][NBT];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int nb = 0; nb < NBT; ++nb) acc[mb][nb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    f32x4 bcur[NBT], bnxt[NBT];  // B fragments, one chunk ahead
#pragma unroll
    for (int nb = 0; nb < NBT; ++nb) bcur[nb] = wlane[(nb0 + nb) * 64];

#pragma unroll 1
    for (int g0 = 0; g0 < G; g0 += D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int g = g0 + d;
        const int gb = g + 1 < G ? g + 1 : G - 1;
#pragma unroll
        for (int nb = 0; nb < NBT; ++nb) bnxt[nb] = wlane[(gb * NB + nb0 + nb) * 64];
        // keep the next chunk's B reads here, a whole chunk of MFMAs ahead of their use
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int mb = 0; mb < MB; ++mb) {
            const float a = ar[d][mb][t];
#pragma unroll
            for (int nb = 0; nb < NBT; ++nb)
              acc[mb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bcur[nb][t], acc[mb][nb], 0, 0, 0);
          }
        const int ga = g + D;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
          ar[d][mb] = ld(ga < G ? cur[mb] + chunk_off(ga) : nxt[mb] + chunk_off(ga - G));
#pragma unroll
        for (int nb = 0; nb < NBT; ++nb) bcur[nb] = bnxt[nb];
      }
    }
    // C/D: lane holds column mr of rows 4q .. 4q+3 of each M-block; y is NHWC, or NCHW when
    // out_nchw (the last conv feeding FC1 in the reference's (C, H, W) flatten order)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t po = ptile * TP + mb * 16 + 4 * q + i;
        if (po < P) {
          if (out_nchw) {
            const int64_t b = po / Gm::PIX, pp = po - b * Gm::PIX;
#pragma unroll
            for (int nb = 0; nb < NBT; ++nb)
              y[(b * COUT + (nb0 + nb) * 16 + mr) * Gm::PIX + pp] = relu_c(radd(acc[mb][nb][i], bt[nb]));
          } else {
#pragma unroll
            for (int nb = 0; nb < NBT; ++nb)
              y[po * COUT + (nb0 + nb) * 16 + mr] = relu_c(radd(acc[mb][nb][i], bt[nb]));
          }
        }
      }
  };

  for (; v < total;) {
    const int64_t vn = v + tstride;
    // the chunks past the end of this unit are the next unit's leading chunks
    bases(unit_ptile(vn < total ? vn : v), nxt);
    if (TS > 1 && v >= full)
      run(std::integral_constant<int, NB / TS>{}, unit_ptile(v), unit_nb0(v));
    else
      run(std::integral_constant<int, NB>{}, unit_ptile(v), unit_nb0(v));
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) cur[mb] = nxt[mb];
    v = vn;
  }
}

// OHWI weights -> MFMA fragment order (the LDS image the conv kernel copies)
template <int KH, int KW, int S, int CIN, int COUT, int HIN, int WIN>
__device__ __forceinline__ void pack_one(const float *w, f32x4 *packed, int sl) {
  using Gm = ConvGeom<KH, KW, S, CIN, COUT, HIN, WIN>;
  if (sl < Gm::LDS_F4) packed[sl] = Gm::load_slot(w, sl);
}

template <int KH, int KW, int S, int CIN, int COUT, int HIN, int WIN>
__global__ __launch_bounds__(256) void k_conv_pack(const float *__restrict__ w, f32x4 *__restrict__ packed) {
  using Gm = ConvGeom<KH, KW, S, CIN, COUT, HIN, WIN>;
  const int sl = blockIdx.x * 256 + threadIdx.x;
  if (sl < Gm::LDS_F4) packed[sl] = Gm::load_slot(w, sl);
}

}  // namespace rth
