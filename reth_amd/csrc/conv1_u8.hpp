// conv1 on uint8 frame stacks (RTH_CONV_U8_CHW: x = [CIN, HIN, WIN] bytes per sample -- replay
// rows / an actor frame ring, optionally addressed through a row index, or a replay's frame
// store through frame ids): forward and weight gradient on the bf16 MFMA with exact three-term
// splits, and the reduce launch that finishes the backward's deferred sums.  The u8 -> bf16
// cast happens in registers: no f32 copy of the observation ever exists.
#pragma once

#include "common.hpp"
#include "conv_f32.hpp"
#include "optim.hpp"
#include "wgrad.hpp"

namespace rth {

// ---------------------------------------------------------------------------------------
// conv1 on uint8 stacks on the bf16 MFMA with an exact three-term weight split.
// A byte is exact in bf16, and every fp32 weight is the exact sum w1 + w2 + w3 of three
// bf16 values (w1 = bf16(w), w2 = bf16(w - w1), w3 = w - w1 - w2: 8 + 8 + 8 of the 24
// significand bits), so every product x * wi is exact in fp32 and
//     y = sum_k x_k * w_k = sum_k x_k * w1_k + x_k * w2_k + x_k * w3_k
// is the same sum of exact products as the fp32 path, accumulated in fp32 in a different
// order (3 x K terms instead of K).  Nothing is computed at reduced precision; the rate is
// three bf16 MFMAs per fp32 MFMA's work at 16x the per-clock rate.
// Tile: v_mfma_f32_32x32x16_bf16 with A = the weights (32 output channels x 16 k), B = 32
// output pixels' input windows: lane (r, h) = (lane & 31, lane >> 5) holds k = 8h .. 8h+7 of
// chunk c = run (ci, kh) = 2c + h of pixel r -- 8 consecutive bytes of one stack row -- and
// the same k of output channel r's weights.  A wave keeps all of W (16 chunks x 3 terms,
// 192 VGPRs) in registers for its whole life, so the kernel uses no LDS and leaves the CU's
// LDS to the learner's kernels; it loads the next tile's windows while it multiplies this one.
constexpr int kC1Chunks = 16;                       // K = 256 = 16 chunks of 16
constexpr int kC1PackedBytes = kC1Chunks * 3 * 64 * 16;  // [chunk][term][lane] x 8 bf16

// term t (0, 1, 2) of the exact split of w
__device__ __forceinline__ uint32_t bf16x3_term(float w, int t) {
  const uint32_t h1 = bf16_rne_bits(w);
  const float r1 = rsub(w, bf16_bits_f(h1));
  const uint32_t h2 = bf16_rne_bits(r1);
  const float r2 = rsub(r1, bf16_bits_f(h2));
  return t == 0 ? h1 : (t == 1 ? h2 : bf16_rne_bits(r2));
}

// packed slot sl = (c * 3 + t) * 64 + lane: the 8 bf16 of lane (r, h) for chunk c, term t
// from W in OHWI storage: k = 8h + j of chunk c is (ci, kh) = run 2c + h, kw = j
__device__ __forceinline__ void pack_conv1_bf16x3(const float *__restrict__ w, u32x4 *__restrict__ packed, int sl) {
  if (sl >= kC1PackedBytes / 16) return;
  const int lane = sl % 64, t = (sl / 64) % 3, c = sl / 192;
  const int co = lane & 31, rho = 2 * c + (lane >> 5), ci = rho >> 3, kh = rho & 7;
  float wv[8];  // every load before the first split (the split's branches kept them one at a time)
#pragma unroll
  for (int j = 0; j < 8; ++j) wv[j] = w[((co * 8 + kh) * 8 + j) * 4 + ci];
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = bf16x3_term(wv[j], t);
  packed[sl] = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
}

// conv1 with each stack byte converted once per horizontal window pair (r05).  Horizontally
// adjacent output pixels' windows overlap by half (kernel 8, stride 4): kw 4..7 of pixel ox are
// kw 0..3 of pixel ox + 1.  So a lane loads and converts only the first half (4 bytes) of each
// of its 16 runs and takes the second half, already converted, from the next lane (DPP
// wave_shl:1).  For that the lanes walk VIRTUAL pixels: 21 per output row, the 21st (ox = 20,
// input columns 80..83: inside the 84-wide row) exists only to hand its first halves to ox = 19,
// and each 32-lane tile covers 31 virtual pixels, its lane 31 being the next one, a helper for
// lane 30 (wave_shl:1 moves lane 32 into lane 31: the helper's own second half is garbage, and it
// stores nothing).  Same packed weights, same k order (kw 0..7 of run (ci, kh)), same MFMA
// chain per output as r04's kernel, in which every lane converted its whole window: the outputs
// are bit-identical.  Half the byte loads and conversions per tile; 29.5 of 32 lanes produce an
// output (20 / 21 x 31 / 32).
constexpr int kC1VPix = 21;       // virtual pixels per output row
constexpr int kC1VPerTile = 31;   // virtual pixels a 32-lane tile outputs
// tiles in flight (16 dwords each); r05 A/B: 2 tiles 26.0 us alone at 1,024 samples, 3: 27.3, 1: 30.7
constexpr int kC1BufShare = 2;

// 4 bytes (kw 0..3 of one stack row) -> 4 bf16 in two dwords (exact)
__device__ __forceinline__ void u8x4_to_bf16(uint32_t v, uint32_t &lo, uint32_t &hi) {
  const uint32_t a = __float_as_uint((float)(v & 0xffu)), b = __float_as_uint((float)((v >> 8) & 0xffu));
  const uint32_t c = __float_as_uint((float)((v >> 16) & 0xffu)), d = __float_as_uint((float)(v >> 24));
  lo = __builtin_amdgcn_perm(b, a, 0x07060302u);
  hi = __builtin_amdgcn_perm(d, c, 0x07060302u);
}

__device__ __forceinline__ uint32_t from_next_lane(uint32_t v) {  // lane i <- lane i + 1
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}

__device__ unsigned char g_conv1_sink[64 * 128];  // stores of lanes without an output (never read)

// FRM (r05): x is a replay's frame store (84 x 84-byte frames) and fids[b] the 4 frame ids of
// sample b's stack (the sampled rows' id tuples, rth_replay_sample_frame_ids): each run
// (ci, kh) is read from frame fids[b][ci] -- the bytes the gather would have assembled, so the
// outputs are bit-identical, without the batch copy of the stacks
constexpr int64_t kC1FrameBytes = 84 * 84;
template <bool FRM = false>
__global__ __launch_bounds__(256) void k_conv1_u8_share(const void *__restrict__ x, const int64_t *__restrict__ rows,
                                                      int64_t n, const int64_t *__restrict__ n_dev,
                                                      const float *__restrict__ w, const float *__restrict__ bias,
                                                      float *__restrict__ y, const int32_t *__restrict__ fids) {
  constexpr int HIN = 84, WIN = 84, WOUT = 20, PIX = 400, S = 4, COUT = 32;
  constexpr int VPS = WOUT * kC1VPix;  // 420 virtual pixels per sample
  constexpr int64_t STACK = 4 * HIN * WIN;
  using f32x16 = __attribute__((ext_vector_type(16))) float;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int r = lane & 31, h = lane >> 5;
  if (n_dev) {
    const int64_t m = *n_dev;
    n = m < n ? (m > 0 ? m : 0) : n;
  }
  // 32-bit pixel arithmetic: the launcher requires n * 420 < 2^31
  const int VP = (int)n * VPS, tiles = (VP + kC1VPerTile - 1) / kC1VPerTile, tstride = (int)gridDim.x * 4;
  int tile = (int)blockIdx.x * 4 + wave;
  if (tile >= tiles) return;  // no barriers below
  const uint8_t *xb = static_cast<const uint8_t *>(x);
  // virtual pixel r of tile t: (sample, oy, ox in 0..20); past the end: the last one
  auto vpix = [&](int t, int &b, int &oy, int &ox) {
    int v = t * kC1VPerTile + r;
    if (v >= VP) v = VP - 1;
    b = (int)((unsigned)v / (unsigned)VPS);
    const int rem = v - b * VPS;
    oy = rem / kC1VPix;
    ox = rem - oy * kC1VPix;
  };
  auto window = [&](int t) -> const uint8_t * {
    int b, oy, ox;
    vpix(t, b, oy, ox);
    const int64_t row = rows ? rows[b] : b;
    return xb + row * STACK + ((S * oy) * WIN + S * ox);
  };
  auto run_off = [&](int c) -> int {
    const int rho = 2 * c + h;
    return (rho >> 3) * HIN * WIN + (rho & 7) * WIN;
  };
  const u32x4 *wp = reinterpret_cast<const u32x4 *>(w);
  bf16x8 wf[kC1Chunks][3];
#pragma unroll
  for (int c = 0; c < kC1Chunks; ++c)
#pragma unroll
    for (int t = 0; t < 3; ++t) wf[c][t] = __builtin_bit_cast(bf16x8, wp[(c * 3 + t) * 64 + lane]);
  // (the bias is re-read per tile from L1 / L2 in the epilogue: 16 registers fewer than
  // r04's kernel keeps, which spilled its weights into AGPRs)
  const float4 *bias4 = reinterpret_cast<const float4 *>(bias) + h;

  constexpr int NB = kC1BufShare;
  uint32_t raw[NB][kC1Chunks];  // the first halves of the runs, a ring of tiles in flight
  auto load = [&](uint32_t (&dst)[kC1Chunks], int t) {
    if constexpr (FRM) {
      int b, oy, ox;
      vpix(t, b, oy, ox);
      // a tile's 32 virtual pixels span at most two samples (420 per sample): their id tuples
      // are wave-uniform scalar loads (lgkmcnt: a vector load here would be the newest in the
      // vmcnt queue, and waiting for it would drain the ring of tiles in flight)
      const int tu = __builtin_amdgcn_readfirstlane(t);
      const int v0 = tu * kC1VPerTile, v1 = v0 + kC1VPerTile - 1 < VP ? v0 + kC1VPerTile - 1 : VP - 1;
      const int b0 = (int)((unsigned)v0 / (unsigned)VPS), b1 = (int)((unsigned)v1 / (unsigned)VPS);
      const int4 i0 = reinterpret_cast<const int4 *>(fids)[b0], i1 = reinterpret_cast<const int4 *>(fids)[b1];
      const bool second = b != b0;
      const int4 id = {second ? i1.x : i0.x, second ? i1.y : i0.y, second ? i1.z : i0.z, second ? i1.w : i0.w};
      const int off = (S * oy) * WIN + S * ox;
      const uint8_t *fb[4] = {xb + (int64_t)id.x * kC1FrameBytes + off, xb + (int64_t)id.y * kC1FrameBytes + off,
                              xb + (int64_t)id.z * kC1FrameBytes + off, xb + (int64_t)id.w * kC1FrameBytes + off};
#pragma unroll
      for (int c = 0; c < kC1Chunks; ++c) {
        const int rho = 2 * c + h;  // run (ci, kh) = (rho / 8, rho % 8): h picks the odd / even runs
        dst[c] = *reinterpret_cast<const uint32_t *>(fb[(2 * c) >> 3] + (rho & 7) * WIN);
      }
    } else {
      const uint8_t *p = window(t);
#pragma unroll
      for (int c = 0; c < kC1Chunks; ++c) dst[c] = *reinterpret_cast<const uint32_t *>(p + run_off(c));
    }
  };
  auto compute = [&](const uint32_t (&src)[kC1Chunks], int t) {
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.0f;
#pragma unroll
    for (int c = 0; c < kC1Chunks; ++c) {
      uint32_t lo, hi;
      u8x4_to_bf16(src[c], lo, hi);
      const uint32_t lo2 = from_next_lane(lo), hi2 = from_next_lane(hi);  // kw 4..7 = the next pixel's kw 0..3
      const bf16x8 xf = __builtin_bit_cast(bf16x8, (u32x4{lo, hi, lo2, hi2}));
#pragma unroll
      for (int tm = 0; tm < 3; ++tm) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wf[c][tm], xf, acc, 0, 0, 0);
    }
    // lane r holds virtual pixel r's outputs; virtual column 20, the helper lane 31 and lanes
    // past the end store into the sink (no branch around the stores)
    int b, oy, ox;
    vpix(t, b, oy, ox);
    const bool out = r < kC1VPerTile && ox < WOUT && t * kC1VPerTile + r < VP;
    float *dst = out ? y + ((int64_t)b * PIX + oy * WOUT + ox) * COUT
                     : reinterpret_cast<float *>(g_conv1_sink) + lane * 32;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 bv = bias4[2 * g];  // channels 8g + 4h .. + 3
      float4 o;
      o.x = relu_c(radd(acc[4 * g + 0], bv.x));
      o.y = relu_c(radd(acc[4 * g + 1], bv.y));
      o.z = relu_c(radd(acc[4 * g + 2], bv.z));
      o.w = relu_c(radd(acc[4 * g + 3], bv.w));
      *reinterpret_cast<float4 *>(dst + 8 * g + 4 * h) = o;
    }
  };
#pragma unroll
  for (int i = 0; i + 1 < NB; ++i) load(raw[i], tile + i * tstride < tiles ? tile + i * tstride : tiles - 1);
  for (;;) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int ahead = tile + (NB - 1) * tstride;
      load(raw[(i + NB - 1) % NB], ahead < tiles ? ahead : tiles - 1);
      compute(raw[i], tile);
      tile += tstride;
      if (tile >= tiles) return;
    }
  }
}

__global__ __launch_bounds__(256) void k_conv1_pack_bf16x3(const float *__restrict__ w, u32x4 *__restrict__ packed) {
  pack_conv1_bf16x3(w, packed, blockIdx.x * 256 + threadIdx.x);
}

// ---------------------------------------------------------------------------------------
// conv1 backward on uint8 stacks: gy = (y > 0) ? g : 0 (ReLU backward), gw = sum over output
// pixels of gy (x) im2col(x), gb = sum of gy -- one pass over g, y and the stacks.  The 32 x 256
// weight gradient is held as KW = 8 accumulator tiles per wave: tile kw, column j = (ci, kh)
// (32 of them).  Workgroup w sums a contiguous pixel range and writes its partial
// [co][kk = kw * 32 + (ci, kh)], then its bias sums; k_wgrad_reduce adds the partials in
// workgroup order (deterministic).
constexpr int kWgWaves = 8, kWgBlocks = 256;

// The weight gradient on the bf16 MFMA, the upstream gradient split into three exact bf16
// terms (truncation split: a = hi + mid + lo, 8 significand bits each, so every product with a
// byte is exact in fp32): D[co][(ci, kh)] per kw over this workgroup's pixels -- the exact products an
// fp32 MFMA over the same pixels would sum, accumulated in fp32 in a different order.
// One v_mfma_f32_32x32x16_bf16 takes 16 pixels as two "slots" of 8 consecutive output
// pixels of one output row (ox 0-7, 8-15, 16-19 + 4 masked: 3 slots per row, 60 per
// stack); lane (r, h) holds slot h: as A the masked gradient of channel r (3 terms), as B
// byte kw of run (ci, kh) = r of each pixel's window.  The 8 windows of a slot overlap: run r
// of all of them is one 36-byte span of stack row (ci, 4 oy + kh) (20 bytes for the last
// slot of a row), loaded as 2 x dwordx4 + dword; v_cvt_f32_ubyteN picks byte kw of pixel j
// (byte 4j + kw of the span), so the 8x8 byte transpose is free.  The waves'
// tiles are summed through LDS in wave order.
__device__ __forceinline__ void split3_trunc(float a, uint32_t &t0, uint32_t &t1, uint32_t &t2) {
  const uint32_t u = __float_as_uint(a);
  t0 = u & 0xffff0000u;
  const float r1 = rsub(a, __uint_as_float(t0));
  t1 = __float_as_uint(r1) & 0xffff0000u;
  t2 = __float_as_uint(rsub(r1, __uint_as_float(t1)));  // <= 8 significand bits: exact in bf16
}

// MODE 0: x holds the n stacks; 1: rows[b] indexes x's stacks; 2 (r05): x is a replay's frame
// store and rows the int32 [n][4] frame ids of the stacks (k_conv1_u8_share<true>'s input)
template <int MODE>
__global__ __launch_bounds__(kWgWaves * 64) void k_conv1_wgrad_bf16x3(const uint8_t *__restrict__ x,
                                                                     const int64_t *__restrict__ rows, int64_t n,
                                                                     const float *__restrict__ g,
                                                                     const float *__restrict__ y,
                                                                     float *__restrict__ partial) {
  constexpr int HIN = 84, WIN = 84, WOUT = 20, PIX = 400, KH = 8, KW = 8, S = 4, COUT = 32;
  constexpr int K = 4 * KH * KW, STACK = 4 * HIN * WIN, SLOTS = 3 * 20;  // slots per stack
  using f32x16 = __attribute__((ext_vector_type(16))) float;
  __shared__ float red[kWgWaves][32];
  __shared__ float tile[kWgWaves][32 * 32];
  const int lane = threadIdx.x % 64, o = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
  const int64_t NS = n * SLOTS, NG = (NS + 1) / 2;  // slots, 2-slot groups
  const int64_t chunk = ((NG + gridDim.x - 1) / gridDim.x + kWgWaves - 1) / kWgWaves * kWgWaves;
  const int64_t g_begin = (int64_t)blockIdx.x * chunk, g_end = g_begin + chunk < NG ? g_begin + chunk : NG;
  const int row_off = (o / KH) * HIN * WIN + (o % KH) * WIN;  // run (ci, kh) = o
  struct Raw {
    float gv[8], yv[8];
    uint32_t sp[9];  // the 36-byte span
    int nv;          // valid pixels of the slot (0: past the end)
  };
  // no branches around loads (the compiler then counts the loads in flight exactly instead of
  // waiting for all of them): the two slots' samples and row indices are scalar
  auto load = [&](int64_t gq, Raw &rw) {
    const bool live = gq < g_end;
    const int64_t gi = live ? gq : g_end - 1;
    const int64_t s0 = 2 * gi, s1 = s0 + 1 < NS ? s0 + 1 : NS - 1;  // wave-uniform
    const int64_t b0 = s0 / SLOTS, b1 = s1 / SLOTS;
    const int64_t rw0 = MODE == 1 ? rows[b0] : b0, rw1 = MODE == 1 ? rows[b1] : b1;
    const int64_t sl = h ? s1 : s0, b = h ? b1 : b0, row = h ? rw1 : rw0;
    const int rem = (int)(sl - b * SLOTS), oy = rem / 3, seg = rem % 3;
    rw.nv = live && 2 * gi + h < NS ? (seg == 2 ? 4 : 8) : 0;
    const uint8_t *src;
    if constexpr (MODE == 2) {  // run (ci, kh) = (o / KH, o % KH) from frame ids[b][ci]
      // the two slots' id tuples as wave-uniform scalar loads (not in the vmcnt queue)
      const int4 i0 = reinterpret_cast<const int4 *>(rows)[b0], i1 = reinterpret_cast<const int4 *>(rows)[b1];
      const int4 iv = h ? i1 : i0;
      const int ci = o / KH;
      const int64_t fid = ci == 0 ? iv.x : ci == 1 ? iv.y : ci == 2 ? iv.z : iv.w;
      src = x + fid * (int64_t)(HIN * WIN) + (o % KH) * WIN + (S * oy) * WIN + S * 8 * seg;
    } else {
      src = x + row * (int64_t)STACK + row_off + (S * oy) * WIN + S * 8 * seg;
    }
    const u32x4 v0 = *reinterpret_cast<const u32x4 *>(src);
    const uint32_t v4 = *reinterpret_cast<const uint32_t *>(src + 16);
    // the last slot's span ends the row: its unused upper part re-reads the lower
    const u32x4 v1 = *reinterpret_cast<const u32x4 *>(src + (seg < 2 ? 20 : 0));
    rw.sp[0] = v0[0], rw.sp[1] = v0[1], rw.sp[2] = v0[2], rw.sp[3] = v0[3], rw.sp[4] = v4;
    rw.sp[5] = v1[0], rw.sp[6] = v1[1], rw.sp[7] = v1[2], rw.sp[8] = v1[3];
    const int64_t q0 = b * PIX + oy * WOUT + 8 * seg;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t q = q0 + (j < 4 || seg < 2 ? j : 0);  // masked pixels re-read pixel 0
      rw.gv[j] = g[q * COUT + o];
      rw.yv[j] = y[q * COUT + o];
    }
  };
  f32x16 acc[KW];
#pragma unroll
  for (int t = 0; t < KW; ++t) acc[t] = f32x16{};
  float db = 0.0f;
  auto compute = [&](const Raw &rw) {
    uint32_t tm[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float a = (j < rw.nv && rw.yv[j] > 0.0f) ? rw.gv[j] : 0.0f;
      db = radd(db, a);
      split3_trunc(a, tm[0][j], tm[1][j], tm[2][j]);
    }
    bf16x8 af[3];
#pragma unroll
    for (int t = 0; t < 3; ++t)
      af[t] = __builtin_bit_cast(bf16x8, (u32x4{__builtin_amdgcn_perm(tm[t][1], tm[t][0], 0x07060302u),
                                                 __builtin_amdgcn_perm(tm[t][3], tm[t][2], 0x07060302u),
                                                 __builtin_amdgcn_perm(tm[t][5], tm[t][4], 0x07060302u),
                                                 __builtin_amdgcn_perm(tm[t][7], tm[t][6], 0x07060302u)}));
#pragma unroll
    for (int kw = 0; kw < KW; ++kw) {
      uint32_t f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {  // byte 4j + kw of the span
        const uint32_t wv = rw.sp[j + kw / 4];
        f[j] = __float_as_uint((float)((wv >> (8 * (kw % 4))) & 0xffu));
      }
      const bf16x8 bf = __builtin_bit_cast(bf16x8, (u32x4{__builtin_amdgcn_perm(f[1], f[0], 0x07060302u),
                                                         __builtin_amdgcn_perm(f[3], f[2], 0x07060302u),
                                                         __builtin_amdgcn_perm(f[5], f[4], 0x07060302u),
                                                         __builtin_amdgcn_perm(f[7], f[6], 0x07060302u)}));
#pragma unroll
      for (int t = 0; t < 3; ++t) acc[kw] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[t], bf, acc[kw], 0, 0, 0);
    }
  };
  // this wave's groups g_begin + wave + k * waves, k < ng, two per trip (a group past the end
  // loads a valid one, masked): no branch but the loop's own, and the next group's loads are
  // issued before this group's math
  const int64_t gi0 = g_begin + wave;
  const int64_t ng = gi0 < g_end ? (g_end - gi0 + kWgWaves - 1) / kWgWaves : 0;
  if (ng > 0) {
    Raw ra, rb;
    load(gi0, ra);
    for (int64_t k = 0; k < ng; k += 2) {
      load(gi0 + (k + 1) * kWgWaves, rb);
      __builtin_amdgcn_sched_barrier(0);
      compute(ra);
      load(gi0 + (k + 2) * kWgWaves, ra);
      __builtin_amdgcn_sched_barrier(0);
      compute(rb);
    }
  }
  // bias: lanes o and o + 32 of every wave
  db = radd(db, __shfl_down(db, 32));
  if (h == 0) red[wave][o] = db;
  // the weight tiles: sum the waves through LDS, tile by tile (C/D: lane -> column o of the
  // tile, register r -> row i = 8 (r / 4) + 4 h + r % 4 = output channel)
  float *out = partial + (int64_t)blockIdx.x * (COUT * K + COUT);
#pragma unroll
  for (int t = 0; t < KW; ++t) {
#pragma unroll
    for (int r = 0; r < 16; ++r) tile[wave][(8 * (r / 4) + 4 * h + r % 4) * 32 + o] = acc[t][r];
    __syncthreads();
    for (int e = threadIdx.x; e < 32 * 32; e += kWgWaves * 64) {
      float v = tile[0][e];
#pragma unroll
      for (int w = 1; w < kWgWaves; ++w) v = radd(v, tile[w][e]);
      out[(e / 32) * K + t * 32 + e % 32] = v;  // [o][kk = kw * 32 + (ci, kh)]
    }
    __syncthreads();
  }
  if (threadIdx.x < 32) {
    float v = red[0][threadIdx.x];
    for (int w = 1; w < kWgWaves; ++w) v = radd(v, red[w][threadIdx.x]);
    out[COUT * K + threadIdx.x] = v;
  }
}

// partials [blocks][COUT * K + COUT] (kk = kw * 32 + ci * KH + kh) -> gw OHWI, gb: 64
// elements per workgroup, 4 groups of 64 lanes each summing a quarter of the partials
// (coalesced rows), then the 4 group sums in fixed order
// deferred bias gradients (rth_relu_bias_grad with db = NULL) finished by the extra
// workgroups of this launch, in exactly k_bias_grad_combine's order (qnet.hip: 1024 lanes,
// G = 1024 / C lanes per channel striding the slabs, then a fixed LDS tree): each of the 256
// threads plays 4 of those virtual lanes, so the result is bit-identical to the two-launch form
constexpr int kBiasJobsMax = 4;
constexpr int kBiasVLanes = 1024;  // = qnet.hip's kCombThreads
struct BiasJobs {
  const float *part[kBiasJobsMax];
  float *db[kBiasJobsMax];
  int slabs[kBiasJobsMax], C[kBiasJobsMax];
  int n;
};

// sq (nullable): the fp64 sum of squares of the finished db (clip_grad_norm_'s partial, r06)
__device__ void bias_job(const BiasJobs &bj, int j, double *sq = nullptr) {
  __shared__ float red[kBiasVLanes];
  constexpr int Q = kBiasVLanes / 256, U = 16;
  const int C = bj.C[j], G = kBiasVLanes / C, tid = threadIdx.x, slabs = bj.slabs[j];
  const float *part = bj.part[j];
  // virtual lane vt = tid + 256 q sums slabs vt / C, + G, + 2 G, ... in that order (the order of
  // k_bias_grad_combine's lane vt); the loads of all Q lanes, U slabs each, are in flight together
  // (one round trip per U * G slabs -- 2 for conv2's 324 slabs, where a lane-by-lane loop of
  // 8-load batches took 12); the slabs past the end add +0 (the clamped load is replaced), which
  // leaves every sum unchanged
  float acc[Q];
#pragma unroll
  for (int q = 0; q < Q; ++q) acc[q] = 0.0f;
  for (int base = 0; base < slabs; base += U * G) {
    float v[Q][U];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int vt = tid + 256 * q, c = vt % C, k0 = vt / C + base;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int kk = k0 + u * G;
        v[q][u] = part[(int64_t)(kk < slabs ? kk : slabs - 1) * C + c];
      }
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const int k0 = (tid + 256 * q) / C + base;
#pragma unroll
      for (int u = 0; u < U; ++u) acc[q] = radd(acc[q], k0 + u * G < slabs ? v[q][u] : 0.0f);
    }
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) red[tid + 256 * q] = acc[q];
  __syncthreads();
  for (int st = kBiasVLanes / 2; st >= C; st >>= 1) {
    for (int i = tid; i < st; i += 256) red[i] = radd(red[i], red[i + st]);
    __syncthreads();
  }
  if (tid < C) bj.db[j][tid] = red[tid];
  if (sq) {
    __shared__ double red4[4];
    const double d = tid < C ? (double)red[tid] : 0.0;
    const double t = block_sum(rmul(d, d), red4);
    if (tid == 0) *sq = t;
  }
}

// deferred conv2 / conv3 weight gradients (rth_conv_wgrad_f32_partials): their reduce
// workgroups follow the bias jobs' (r06)
constexpr int kWgradJobsMax = 2;
struct WgradJobs {
  WgfJob j[kWgradJobsMax];
  int n;
};

// workgroup blk of conv1's weight-gradient reduce: 64 of its E outputs, or (blk >= RB) a
// deferred bias gradient, or (past those) a reduce workgroup of a deferred weight gradient.
// sq (nullable): the fp64 sum of squares of what the workgroup finished goes to sq[blk] (r06:
// clip_grad_norm_'s partials from the backward)
template <int KH, int KW, int CIN, int COUT>
__device__ __forceinline__ void wgrad_reduce_wg(int blk, const float *__restrict__ partial, int blocks,
                                                float *__restrict__ gw, float *__restrict__ gb, const BiasJobs &bj,
                                                const WgradJobs &wj, double *__restrict__ sq) {
  constexpr int K = CIN * KH * KW, E = COUT * K + COUT, RB = (E + 63) / 64;
  __shared__ float part[4][64];
  if (blk >= RB + bj.n) {  // a deferred weight gradient
    int b = blk - RB - bj.n, j = 0;
    while (j + 1 < wj.n && b >= wgf_reduce_blocks(wj.j[j])) b -= wgf_reduce_blocks(wj.j[j++]);
    const float v = wgf_reduce_wg(wj.j[j], b);
    if (sq) {
      __shared__ double red4[4];
      const double t = block_sum(rmul((double)v, (double)v), red4);
      if (threadIdx.x == 0) sq[blk] = t;
    }
    return;
  }
  if (blk >= RB) {  // a deferred bias gradient
    bias_job(bj, blk - RB, sq ? sq + blk : nullptr);
    return;
  }
  const int grp = threadIdx.x / 64, l = threadIdx.x % 64;
  const int e = blk * 64 + l;
  const int per = (blocks + 3) / 4, w0 = grp * per, w1 = w0 + per < blocks ? w0 + per : blocks;
  float v = 0.0f;
  if (e < E) {
    int w = w0;
    for (; w + 32 <= w1; w += 32) {  // 32 loads in flight per round trip; the sum stays in w order
      float t[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) t[u] = partial[(int64_t)(w + u) * E + e];
#pragma unroll
      for (int u = 0; u < 32; ++u) v = radd(v, t[u]);
    }
    for (; w + 16 <= w1; w += 16) {
      float t[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) t[u] = partial[(int64_t)(w + u) * E + e];
#pragma unroll
      for (int u = 0; u < 16; ++u) v = radd(v, t[u]);
    }
    for (; w + 8 <= w1; w += 8) {
      float t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = partial[(int64_t)(w + u) * E + e];
#pragma unroll
      for (int u = 0; u < 8; ++u) v = radd(v, t[u]);
    }
    for (; w < w1; ++w) v = radd(v, partial[(int64_t)w * E + e]);
  }
  part[grp][l] = v;
  __syncthreads();
  if (grp != 0) return;  // (wave-uniform)
  v = radd(radd(radd(part[0][l], part[1][l]), part[2][l]), part[3][l]);
  if (sq) {  // wave 0's 64 outputs, a fixed shuffle tree
    double d = e < E ? rmul((double)v, (double)v) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d = radd(d, __shfl_down(d, o, 64));
    if (l == 0) sq[blk] = d;
  }
  if (e >= E) return;
  if (e >= COUT * K) {
    gb[e - COUT * K] = v;
    return;
  }
  const int oi = e / K, kk = e % K, kw = kk / 32, ci = (kk % 32) / KH, kh = kk % KH;
  gw[((oi * KH + kh) * KW + kw) * CIN + ci] = v;
}

template <int KH, int KW, int CIN, int COUT>
__global__ __launch_bounds__(256) void k_wgrad_reduce(const float *__restrict__ partial, int blocks,
                                                      float *__restrict__ gw, float *__restrict__ gb, BiasJobs bj,
                                                      WgradJobs wj) {
  wgrad_reduce_wg<KH, KW, CIN, COUT>(blockIdx.x, partial, blocks, gw, gb, bj, wj, nullptr);
}

// the same reduce launch with clip_grad_norm_'s partials (r06, one rank): workgroups [0, nsq)
// are norm-partial workgroups over the gradients final before it (optim.hpp's grad_sqsum_wg,
// workgroup 0 advancing Adam's step count), the rest the reduce's, each writing the sum of
// squares of the gradients it finishes -- conv1's weight and bias, the deferred bias and weight
// gradients -- right behind them: rth_adam_prenormed then runs the update alone
template <int KH, int KW, int CIN, int COUT>
__global__ __launch_bounds__(256) void k_wgrad_reduce_norm(const float *__restrict__ partial, int blocks,
                                                           float *__restrict__ gw, float *__restrict__ gb, BiasJobs bj,
                                                           WgradJobs wj, OptArgs na, int nsq, double *__restrict__ npart,
                                                           SqStep st, int nlong) {
  // dispatch order (r06): the long workgroups first -- the deferred bias and weight-gradient
  // reduces (nlong of them: hundreds of dependent-ish loads each) -- then conv1's reduce, then the
  // norm partials of the finished gradients; every workgroup keeps its partial slot (nsq + the
  // reduce's block, or the norm block), so the sums are the same (0.504 vs 0.506 ms/step with the
  // norm workgroups first, interleaved)
  constexpr int RB = (COUT * CIN * KH * KW + COUT + 63) / 64;
  const int b = (int)blockIdx.x;
  if (b < nlong) {
    wgrad_reduce_wg<KH, KW, CIN, COUT>(RB + b, partial, blocks, gw, gb, bj, wj, npart + nsq);
  } else if (b < nlong + RB) {
    wgrad_reduce_wg<KH, KW, CIN, COUT>(b - nlong, partial, blocks, gw, gb, bj, wj, npart + nsq);
  } else {
    grad_sqsum_wg(na, b - nlong - RB, npart, st);
  }
}

}  // namespace rth
