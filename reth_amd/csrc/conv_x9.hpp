// The exact-split bf16 MFMA convolution (k_conv_x9): conv3's forward and the data gradients of
// conv3 and conv2, with their weight packs and conv3's bias-gradient slabs.
#pragma once

#include "common.hpp"
#include "conv1_u8.hpp"  // bf16x3_term
#include "conv_f32.hpp"

namespace rth {

// ---------------------------------------------------------------------------------------
// A convolution of f32 NHWC input (conv3's forward; the data gradients below) on the bf16 MFMA
// with an exact 3 x 3-term split of BOTH operands.  (conv2's forward ran on it too until r05:
// slower in the loop than the fp32 MFMA kernel, DESIGN.md.)  Every fp32 value v is the exact sum v1 + v2 + v3 of three bf16 values (the
// round-to-nearest split of bf16x3_term: 8 + 8 + 8 of the 24 significand bits, each residual
// exact), so for an input x and a weight w
//     x * w = sum_{i,j in 1..3} xi * wj
// and every partial product xi * wj has at most 16 significant bits: it is exact in the fp32
// accumulator.  The nine bf16 MFMAs per fp32 product therefore sum exactly the same real
// products as the fp32 MFMA's fmaf chain, accumulated in fp32 in a different order (9K terms
// instead of K) -- the difference is summation order, as between any two fp32 GEMM tilings,
// not precision.  (Exponent domain, measured -- tests/test_exact_split_gpu.py, DESIGN.md: exact
// for values from 2^-110 up; below, the third term's last bits fall under the smallest bf16
// subnormal, 2^-133 -- the MFMA honours bf16 subnormal operands -- and from (2 - 2^-8) 2^127 the
// first term rounds to infinity.  The DQN's values are many orders of magnitude inside.)  Rate: 9
// v_mfma_f32_16x16x32_bf16 (16 cycles each) do the work of 8 v_mfma_f32_16x16x4_f32 (32
// cycles each): 144 vs 256 matrix-pipe cycles per 16 x 16 x 32 block, 1.78x.
//
// Workgroup = 8 waves over NSAMP (runtime nsamp <= NSAMP) samples: the samples' input is
// split once into the three bf16 planes in LDS ([term][ci / 8][pixel] 16-byte units, pixel
// rows rotated within 16-row blocks against bank conflicts); wave w owns output channels
// 16 (w & 3) .. +15 and K half w >> 2 (its B fragments -- all three weight terms of its K half,
// NCH / 2 chunks x 3 x 8 bf16 -- live in registers for the whole launch); every wave walks all
// M-tiles of 16 output pixels of the workgroup's samples.  The two K halves meet in LDS
// (fixed order: first half + second half, then + bias, ReLU), and the output leaves as one
// contiguous run per workgroup (NHWC, or NCHW for FC1) in 16-byte stores.
template <int KH, int KW, int S, int CIN, int HIN, int WIN, int NSAMP, int ROT, int KS, int COUT_ = 64>
struct X9Geom {
  static constexpr int COUT = COUT_, HOUT = (HIN - KH) / S + 1, WOUT = (WIN - KW) / S + 1, PIX = HOUT * WOUT;
  static constexpr int NCB = COUT / 16;                                   // channel blocks (waves per K part)
  static constexpr int K = KH * KW * CIN, NCH = K / 32, NCHP = NCH / KS;  // 32-deep chunks, per K part
  static constexpr int NT = 64 * NCB * KS;                                // threads: NCB channel blocks x KS
  static constexpr int TILES = (NSAMP * PIX + 15) / 16;                  // 16-pixel M-tiles
  static constexpr int NG = CIN / 8;                                     // 16-byte ci groups
  static constexpr int ROWS = NSAMP * HIN * WIN;                         // staged input pixels
  // ROT = rotation | (shift << 4) | (pad << 8): the staged row r goes to unit (r & ~15) |
  // ((r + (r >> shift) * rotation) & 15) of its plane (shift 0 = 5), planes padded by `pad`
  // units (0 = the r03 rule: 1 at rotation 10) -- scripts/x9_lds_sim.py searches these
  static constexpr int ROTV = ROT & 15, SHV = ((ROT >> 4) & 15) ? ((ROT >> 4) & 15) : 5;
  static constexpr int PADV = (ROT >> 8) ? (ROT >> 8) : (ROT == 10 ? 1 : 0);
  static constexpr int PLANE = (ROWS + 15) / 16 * 16 + PADV;  // 16-B units per (term, cg)
  static_assert(SHV >= 4, "the rotation must be constant over each aligned 16-row block (a permutation)");
  static constexpr int LDS_U4 = 3 * NG * PLANE;                          // LDS in 16-B units
  static constexpr int OUT_F = NSAMP * COUT * PIX;                       // output staging floats
  static constexpr int PACKED_U4 = (COUT / 16) * NCH * 3 * 64;           // packed weight fragments
  static_assert(CIN % 32 == 0 || 32 % CIN == 0, "a 32-deep chunk must stay inside one tap");
  static_assert(CIN % 8 == 0 && NCH % KS == 0 && KS >= 1 && KS <= 4, "K must split into KS parts of 32-deep chunks");
  static_assert(COUT % 16 == 0 && NT <= 1024, "16-channel blocks, at most 16 waves");
  static_assert(OUT_F * 4 <= LDS_U4 * 16, "output staging must fit the input image");
  static_assert(LDS_U4 * 16 <= 163840, "LDS image too large");
  __device__ static int swz(int r) { return (r & ~15) | ((r + (r >> SHV) * ROTV) & 15); }
};

// PAD > 0 (the data gradient, rth_conv_dgrad): the staged HIN x WIN image is the input
// zero-padded by PAD on every side -- x is [n, HIN - 2 PAD, WIN - 2 PAD, CIN], the border reads
// zero through the buffer resource's range check --, and bias == NULL writes the raw sums (no
// bias, no ReLU).  CLS (conv2's data gradient, one launch for the 4 stride-parity classes):
// blockIdx.y = class (py, px), its packed kernel at wpk + class * PACKED_U4, and output pixel
// (jy, jx) of the class goes to pixel (2 jy + py, 2 jx + px) of the [n, 2 HOUT, 2 WOUT, COUT]
// NHWC gradient.
// MASK (r05, the data gradient of conv3 only: PAD > 0, no CLS): the output is the gradient of
// the layer below's ReLU output, passed through that ReLU at once -- y = 0 where ymask (the
// layer below's output, same NHWC index space) is <= 0, threshold_backward -- and each
// workgroup writes the layer below's bias-gradient partial sums (slab blockIdx.x: float4 of
// channels 4q.. per quad q, each lane's float4s in order, then a fixed LDS tree over the lanes of
// a quad -- k_relu_bias_grad's slab layout, finished by the same deferred bias job).  This
// replaces rth_relu_bias_grad's launch between the two data gradients.
// NCHW (r15, with MASK: conv3's data gradient straight from FC1's gradient): x is the gradient
// of this layer's own ReLU output where FC1 left it, NCHW [n, CIN, HS, WS], and xmask that
// output.  The staging applies the mask in registers -- threshold_backward(x, xmask, 0) --,
// stores the masked gradient channels-last to xmasked (what the weight gradient reads; the
// bits of rth_relu_bias_grad_nchw's) and splits the same registers into LDS.  A lane's four
// channels are four dwords 4 HS WS bytes apart in each tensor; a wave instruction still covers 16
// consecutive pixels of a channel (64 contiguous bytes).  This replaces rth_relu_bias_grad_nchw's
// pass ahead of conv3's backward; this layer's bias-gradient slabs are summed from xmasked by
// k_bias_slabs_nhwc in that pass's order (a slab's chain runs across samples, which no
// per-workgroup sum can reproduce bit for bit).
template <int KH, int KW, int S, int CIN, int HIN, int WIN, int NSAMP, int ROT, int KS, int PAD = 0, int COUT_ = 64,
          int CLS = 0, int MASK = 0, int NCHW = 0>
__global__ __launch_bounds__(64 * (COUT_ / 16) * KS) void k_conv_x9(const float *__restrict__ x, int64_t n,
                                                                  const int64_t *__restrict__ n_dev, int nsamp,
                                                                  const u32x4 *__restrict__ wpk,
                                                                  const float *__restrict__ bias,
                                                                  float *__restrict__ y, int out_nchw,
                                                                  const float *__restrict__ ymask,
                                                                  float *__restrict__ bpart,
                                                                  const float *__restrict__ xmask,
                                                                  float *__restrict__ xmasked) {
  static_assert(!MASK || (PAD > 0 && !CLS && (64 * (COUT_ / 16) * KS) % (COUT_ / 4) == 0),
                "the masked epilogue is the NHWC data gradient's; every lane keeps one channel quad");
  static_assert(!NCHW || MASK, "the NCHW staging is the masked data gradient's");
  using G = X9Geom<KH, KW, S, CIN, HIN, WIN, NSAMP, ROT, KS, COUT_>;
  if constexpr (CLS) wpk += (size_t)blockIdx.y * G::PACKED_U4;
  constexpr int HS = HIN - 2 * PAD, WS = WIN - 2 * PAD;  // the source image
  constexpr int PIX = G::PIX, NCH2 = G::NCHP, NG = G::NG, PLANE = G::PLANE, COUT = G::COUT, NT = G::NT;
  __shared__ uint4 lds[G::LDS_U4];
  if (n_dev) {
    const int64_t m = *n_dev;
    n = m < n ? (m > 0 ? m : 0) : n;
  }
  (void)nsamp;  // == NSAMP: the host launches the instantiation for the samples per workgroup
  const int64_t b0 = (int64_t)blockIdx.x * NSAMP;
  if (b0 >= n) return;  // the whole workgroup leaves: no barrier is reached
  const int ns = (int)(n - b0 < NSAMP ? n - b0 : NSAMP);
  const int nv = ns * PIX;  // valid output pixels
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cb = wave % G::NCB, half = wave / G::NCB;  // channel block, K part

  // this wave's B fragments: channels 16 cb + (lane & 15), chunks [half * NCH2, +NCH2), 3 terms
  bf16x8 wf[NCH2][3];
  {
    const u32x4 *wp = wpk + ((size_t)(cb * G::NCH + half * NCH2) * 3) * 64 + lane;
#pragma unroll
    for (int c = 0; c < NCH2; ++c)
#pragma unroll
      for (int t = 0; t < 3; ++t) wf[c][t] = __builtin_bit_cast(bf16x8, wp[(c * 3 + t) * 64]);
  }
  // Staging: the samples' input split into the three bf16 planes, float4 (4 ci of one pixel)
  // -> 8 bytes in each plane, unit (t * NG + ci / 8) * PLANE + swz(pixel), half (ci % 8) / 4.
  // Lane l of a wave-instruction takes pixel 16 k + (l & 15), ci group 4 j + (l >> 4): each
  // 16-lane LDS write group spans 16 pixels of one ci group (distinct banks); each pixel's 64
  // loaded bytes are contiguous in global memory.  Two phases: the first half of the samples is
  // staged, then the second half's loads are issued and the tiles of the first half computed
  // while they are in flight; the second half is written to LDS after them.
  constexpr int CB = CIN / 16;                       // 4-ci groups per lane quarter
  constexpr int NA = NSAMP > 1 ? NSAMP / 2 : NSAMP;  // samples in phase A
  constexpr int RA = NA * HIN * WIN;                 // staged pixels of phase A
  constexpr int SA = (RA + 15) / 16 * CB * 64;       // lane slots of phase A
  constexpr int RB_ = (NSAMP - NA) * HIN * WIN;      // ... of phase B
  constexpr int SB = (RB_ + 15) / 16 * CB * 64;
  constexpr int UA = (SA + NT - 1) / NT, UB = SB > 0 ? (SB + NT - 1) / NT : 1;
  const int rows = ns * HIN * WIN;
  auto slot_of = [&](int i, int r0, int &rr, int &c4) {
    const int l = i & 63, blk = i >> 6;
    rr = r0 + (blk / CB) * 16 + (l & 15);
    c4 = (blk % CB) * 4 + (l >> 4);
  };
  // the staging loads go through a buffer resource over the n samples: a slot past the staged
  // rows gets an offset beyond its range and reads zeros, so no load sits under a branch (a
  // "cond ? load : 0" made the compiler wait for each load before issuing the next: the
  // phase-B loads went out one at a time)
  const __amdgpu_buffer_rsrc_t x_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(x), 0, (int)(n * (int64_t)(HS * WS * CIN) * 4), 0x00020000);
  const uint32_t xb0 = (uint32_t)(b0 * (int64_t)(HS * WS * CIN) * 4);
  // (NCHW: xmask through a resource of the same range; m = the slot's mask values)
  const __amdgpu_buffer_rsrc_t m_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float *>(NCHW ? xmask : x), 0, (int)(n * (int64_t)(HS * WS * CIN) * 4), 0x00020000);
  auto fetch = [&](int i, int r0, int rend, float4 &m) -> float4 {
    int rr, c4;
    slot_of(i, r0, rr, c4);
    bool ok = rr < rend && rr < rows;
    int src = rr;
    if constexpr (PAD > 0) {  // staged pixel -> source pixel; the border reads zero
      const int s = rr / (HIN * WIN), rem = rr - s * (HIN * WIN), yy = rem / WIN - PAD, xx = rem % WIN - PAD;
      ok = ok && yy >= 0 && yy < HS && xx >= 0 && xx < WS;
      src = (s * HS + yy) * WS + xx;
      if constexpr (NCHW) src = (s * CIN + 4 * c4) * (HS * WS) + yy * WS + xx;  // channel 4 c4's dword
    }
    if constexpr (NCHW) {  // four channels HS * WS floats apart (past the range they all read zero)
      const uint32_t off = ok ? xb0 + (uint32_t)(src * 4) : 0x80000000u;
      float4 v;
      auto ld = [&](__amdgpu_buffer_rsrc_t r, int k) {
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off + k * (HS * WS * 4), 0, 0));
      };
      v.x = ld(x_rsrc, 0), v.y = ld(x_rsrc, 1), v.z = ld(x_rsrc, 2), v.w = ld(x_rsrc, 3);
      m.x = ld(m_rsrc, 0), m.y = ld(m_rsrc, 1), m.z = ld(m_rsrc, 2), m.w = ld(m_rsrc, 3);
      return v;
    }
    const uint32_t off = ok ? xb0 + (uint32_t)((src * (CIN / 4) + c4) * 16) : 0x80000000u;
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(x_rsrc, off, 0, 0));
  };
  auto commit = [&](float4 v, float4 m, int i, int r0, int rend) {
    int rr, c4;
    slot_of(i, r0, rr, c4);
    if (rr >= rend || rr >= rows) return;
    if constexpr (NCHW) {
      v.x = m.x > 0.0f ? v.x : 0.0f;  // threshold_backward(g, y, 0); a border slot stays zero
      v.y = m.y > 0.0f ? v.y : 0.0f;
      v.z = m.z > 0.0f ? v.z : 0.0f;
      v.w = m.w > 0.0f ? v.w : 0.0f;
      const int s = rr / (HIN * WIN), rem = rr - s * (HIN * WIN), yy = rem / WIN - PAD, xx = rem % WIN - PAD;
      if (yy >= 0 && yy < HS && xx >= 0 && xx < WS)
        *reinterpret_cast<float4 *>(xmasked + (((b0 + s) * HS + yy) * WS + xx) * (int64_t)CIN + 4 * c4) = v;
    }
    uint2 tr[3];
    split3_x4(v, tr);
    uint2 *l2 = reinterpret_cast<uint2 *>(lds);
    const int unit = (c4 >> 1) * PLANE + G::swz(rr);
#pragma unroll
    for (int t = 0; t < 3; ++t) l2[(t * NG * PLANE + unit) * 2 + (c4 & 1)] = tr[t];
  };
  {
    float4 va[UA], ma[NCHW ? UA : 1];
#pragma unroll
    for (int u = 0; u < UA; ++u) va[u] = fetch(tid + u * NT, 0, tid + u * NT < SA ? RA : 0, ma[NCHW ? u : 0]);
#pragma unroll
    for (int u = 0; u < UA; ++u)
      if (tid + u * NT < SA) commit(va[u], ma[NCHW ? u : 0], tid + u * NT, 0, RA);
  }
  float4 vb[UB], mb[NCHW ? UB : 1];
  if constexpr (SB > 0) {
#pragma unroll
    for (int u = 0; u < UB; ++u)
      vb[u] = fetch(tid + u * NT, RA, tid + u * NT < SB ? RA + RB_ : 0, mb[NCHW ? u : 0]);
  }
  const float bl = bias ? bias[cb * 16 + (lane & 15)] : 0.0f;
  __syncthreads();

  // per chunk of this wave's K half (wave-uniform): the tap's pixel offset and the ci group's
  // plane offset; per tile (per lane): the window origin's staged pixel
  int toff[NCH2], coff[NCH2], rbv[G::TILES];
#pragma unroll
  for (int c = 0; c < NCH2; ++c) {
    const int k0 = (half * NCH2 + c) * 32, tap = k0 / CIN;
    toff[c] = (tap / KW) * WIN + tap % KW;
    coff[c] = ((k0 % CIN) / 8) * PLANE;
  }
  const int g = lane >> 4;
#pragma unroll
  for (int tile = 0; tile < G::TILES; ++tile) {
    int p = tile * 16 + (lane & 15);
    if (p >= nv) p = nv - 1;
    const int s = p / PIX, pp = p - s * PIX, oy = pp / G::WOUT, ox = pp - oy * G::WOUT;
    rbv[tile] = s * (HIN * WIN) + S * oy * WIN + S * ox;
  }
  const uint4 *const lt = lds;
  // the A fragments of step q = tile * NCH2 + c, three LDS buffers: step q + 2 is requested
  // while step q multiplies (a sched barrier keeps the compiler from sinking the reads);
  // phase A's tiles [0, TA) read only phase A's samples
  constexpr int TA = NSAMP > 1 ? (NA * PIX) / 16 : G::TILES;
  auto addr = [&](int q) -> int {
    const int tile = q / NCH2, c = q % NCH2;
    return coff[c] + g * PLANE + G::swz(rbv[tile] + toff[c]);
  };
  constexpr int NQ = G::TILES * NCH2, QA = TA * NCH2;
  bf16x8 xf[3][3];
  auto load = [&](int q) {
    const int u = addr(q);
#pragma unroll
    for (int t = 0; t < 3; ++t) xf[q % 3][t] = __builtin_bit_cast(bf16x8, lt[t * NG * PLANE + u]);
  };
  f32x4 acc[G::TILES];  // every tile's accumulator stays in registers (all loops unrolled)
  auto step = [&](int q, int qend) {
    const int tile = q / NCH2, c = q % NCH2;
    if (q + 2 < qend) load(q + 2);
    __builtin_amdgcn_sched_barrier(0);
    const bf16x8(&xc)[3] = xf[q % 3];
    f32x4 a = c == 0 ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[tile];
    // smallest terms first: (3,3) (3,2) (2,3) (3,1) (2,2) (1,3) (2,1) (1,2) (1,1)
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[2], wf[c][2], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[2], wf[c][1], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[1], wf[c][2], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[2], wf[c][0], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[1], wf[c][1], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[0], wf[c][2], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[1], wf[c][0], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[0], wf[c][1], a, 0, 0, 0);
    a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xc[0], wf[c][0], a, 0, 0, 0);
    acc[tile] = a;
    __builtin_amdgcn_sched_barrier(0);
  };
  load(0);
  if (QA > 1) load(1);
#pragma unroll
  for (int q = 0; q < QA; ++q) step(q, QA);
  if constexpr (QA < NQ) {  // phase B: write the second half's samples, then compute its tiles
    if constexpr (SB > 0) {
#pragma unroll
      for (int u = 0; u < UB; ++u)
        if (tid + u * NT < SB) commit(vb[u], mb[NCHW ? u : 0], tid + u * NT, RA, RA + RB_);
    }
    __syncthreads();
    load(QA);
    if (QA + 1 < NQ) load(QA + 1);
#pragma unroll
    for (int q = QA; q < NQ; ++q) step(q, NQ);
  }
  // the K halves meet in the (now free) LDS: half 1 stores its partial sums, half 0 adds its
  // own first, then the bias, ReLU; the workgroup's output run leaves in 16-byte stores.
  // C/D: lane holds channel 16 cb + (lane & 15) of pixels 4 (lane >> 4) + i of each tile
  float *F = reinterpret_cast<float *>(lds);
  const int co = cb * 16 + (lane & 15);
  auto fidx = [&](int p) -> int {
    const int s = p / PIX;
    return out_nchw ? (s * COUT + co) * PIX + (p - s * PIX) : p * COUT + co;
  };
  __syncthreads();  // every wave is done reading the input image
  // parts KS-1 .. 1 in turn: the last stores, each earlier one adds its own first
#pragma unroll
  for (int pt = KS - 1; pt >= 1; --pt) {
    if (half == pt) {
#pragma unroll
      for (int tile = 0; tile < G::TILES; ++tile)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int p = tile * 16 + 4 * g + i;
          if (p < nv) {
            const int f = fidx(p);
            F[f] = pt == KS - 1 ? acc[tile][i] : radd(acc[tile][i], F[f]);
          }
        }
    }
    __syncthreads();
  }
  if (half == 0) {
#pragma unroll
    for (int tile = 0; tile < G::TILES; ++tile)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int p = tile * 16 + 4 * g + i;
        if (p < nv) {
          const int f = fidx(p);
          F[f] = bias ? relu_c(radd(radd(acc[tile][i], F[f]), bl)) : radd(acc[tile][i], F[f]);
        }
      }
  }
  __syncthreads();
  if constexpr (CLS) {  // the class's pixels scattered into the full gradient, 16-byte stores
    const int py = blockIdx.y >> 1, px = blockIdx.y & 1, total4 = nv * COUT / 4;
    const float4 *Fs = reinterpret_cast<const float4 *>(F);
    for (int i = tid; i < total4; i += NT) {
      const int p = i / (COUT / 4), c4 = i - p * (COUT / 4), s = p / PIX, pp = p - s * PIX;
      const int jy = pp / G::WOUT, jx = pp - jy * G::WOUT;
      const int64_t o = (((b0 + s) * (2 * G::HOUT) + 2 * jy + py) * (2 * G::WOUT) + 2 * jx + px) * COUT + 4 * c4;
      *reinterpret_cast<float4 *>(y + o) = Fs[i];
    }
  } else if constexpr (MASK) {
    const int total4 = nv * COUT / 4;
    float4 *yo = reinterpret_cast<float4 *>(y + b0 * (int64_t)(COUT * PIX));
    const float4 *ym = reinterpret_cast<const float4 *>(ymask + b0 * (int64_t)(COUT * PIX));
    const float4 *Fs = reinterpret_cast<const float4 *>(F);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);  // channel quad tid % (COUT / 4), in i order
    // every mask load of the lane issued before the first use (clamped indices, no load under a
    // branch): the one-at-a-time loop waited for each in turn, ~5 round trips per workgroup
    constexpr int UM = (NSAMP * PIX * (COUT / 4) + NT - 1) / NT;
    float4 mk[UM];
#pragma unroll
    for (int u = 0; u < UM; ++u) {
      const int i = tid + u * NT;
      mk[u] = ym[i < total4 ? i : 0];
    }
#pragma unroll
    for (int u = 0; u < UM; ++u) {
      const int i = tid + u * NT;
      if (i < total4) {
        const float4 g = Fs[i], m = mk[u];
        float4 o;
        o.x = m.x > 0.0f ? g.x : 0.0f;  // threshold_backward(g, y, 0)
        o.y = m.y > 0.0f ? g.y : 0.0f;
        o.z = m.z > 0.0f ? g.z : 0.0f;
        o.w = m.w > 0.0f ? g.w : 0.0f;
        yo[i] = o;
        acc.x = radd(acc.x, o.x);
        acc.y = radd(acc.y, o.y);
        acc.z = radd(acc.z, o.z);
        acc.w = radd(acc.w, o.w);
      }
    }
    __syncthreads();  // every lane is done reading F: its first NT float4 hold the lane sums
    float4 *red = reinterpret_cast<float4 *>(F);
    red[tid] = acc;
    __syncthreads();
    constexpr int Q = COUT / 4;
    for (int st = NT / 2; st >= Q; st >>= 1) {  // lanes tid and tid + st share a quad
      if (tid < st) {
        float4 a = red[tid];
        const float4 o = red[tid + st];
        a.x = radd(a.x, o.x);
        a.y = radd(a.y, o.y);
        a.z = radd(a.z, o.z);
        a.w = radd(a.w, o.w);
        red[tid] = a;
      }
      __syncthreads();
    }
    if (tid < Q) reinterpret_cast<float4 *>(bpart)[(int64_t)blockIdx.x * Q + tid] = red[tid];
  } else {
    const int total4 = nv * COUT / 4;  // the run [b0, b0 + ns) of y is contiguous in both layouts
    float4 *yo = reinterpret_cast<float4 *>(y + b0 * (int64_t)(COUT * PIX));
    const float4 *Fs = reinterpret_cast<const float4 *>(F);
    for (int i = tid; i < total4; i += NT) yo[i] = Fs[i];
  }
}

// The bias-gradient slabs of rth_relu_bias_grad_nchw from the masked gradient it would have
// written (gy, channels-last [n, P, C], C = 64, P = 49: k_conv_x9's NCHW staging stores it), bit
// for bit: gridDim.x = bias_grad_slabs(n * P, C) slabs, slab s owns samples [s n / S, (s + 1) n / S),
// lane t sums channel t / 4 over the positions of quarter t % 4 (13, 13, 13, 10) across the
// slab's samples in (sample, position) order, then the four quarter sums in quarter order --
// k_relu_bias_grad_nchw's chain, so a deferred job with slabs = 0 finishes the same db.  The loads
// of up to UB samples (a slab has at most 3 unless the slab count is capped) are all in flight
// before the first add: one memory round trip per slab, the adds in order behind it.
__global__ __launch_bounds__(kBiasThreads) void k_bias_slabs_nhwc(const float *__restrict__ gy,
                                                                   float *__restrict__ part, int64_t n) {
  constexpr int C = 64, P = 49, Q = kBiasThreads / C, PQ = (P + Q - 1) / Q, UB = 3;
  __shared__ float red[kBiasThreads];
  const int tid = threadIdx.x, S = gridDim.x, c = tid / Q, qq = tid % Q;
  const int64_t b0 = (int64_t)blockIdx.x * n / S, b1 = (int64_t)(blockIdx.x + 1) * n / S;
  const int p0 = qq * PQ, np = (P - p0 < PQ ? P - p0 : PQ);
  float acc = 0.0f;
  for (int64_t b = b0; b < b1; b += UB) {
    float v[UB][PQ];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
      const float *src = gy + ((b + u < b1 ? b + u : b) * P + p0) * C + c;  // past the slab: a duplicate, unused
#pragma unroll
      for (int k = 0; k < PQ; ++k) v[u][k] = src[(k < np ? k : 0) * C];
    }
#pragma unroll
    for (int u = 0; u < UB; ++u)
#pragma unroll
      for (int k = 0; k < PQ; ++k)
        if (b + u < b1 && k < np) acc = radd(acc, v[u][k]);
  }
  red[tid] = acc;
  __syncthreads();
  if (tid < C) {
    float sum = red[tid * Q];
    for (int k = 1; k < Q; ++k) sum = radd(sum, red[tid * Q + k]);
    part[(int64_t)blockIdx.x * C + tid] = sum;
  }
}

// OHWI weights -> the B fragments of k_conv_x9: slot ((cb * NCH + c) * 3 + t) * 64 + lane holds
// term t of W[16 cb + (lane & 15)][32 c + 8 (lane >> 4) + j], j = 0..7 (k = (kh, kw, ci), ci fastest)
template <int KH, int KW, int S, int CIN, int HIN, int WIN, int NSAMP, int ROT, int KS>
__device__ __forceinline__ void pack_x9(const float *__restrict__ w, u32x4 *__restrict__ packed, int sl) {
  using G = X9Geom<KH, KW, S, CIN, HIN, WIN, NSAMP, ROT, KS>;
  if (sl >= G::PACKED_U4) return;
  const int lane = sl % 64, t = (sl / 64) % 3, c = (sl / 192) % G::NCH, cb = sl / (192 * G::NCH);
  const int co = cb * 16 + (lane & 15), k0 = c * 32 + 8 * (lane >> 4);
  const float4 *wp = reinterpret_cast<const float4 *>(w + (int64_t)co * G::K + k0);  // 32-byte aligned run
  const float4 w0 = wp[0], w1 = wp[1];  // both loads before the first split
  const float wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = bf16x3_term(wv[j], t);
  packed[sl] = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
}

template <int KH, int KW, int S, int CIN, int HIN, int WIN, int NSAMP, int ROT, int KS>
__global__ __launch_bounds__(256) void k_conv_pack_x9(const float *__restrict__ w, u32x4 *__restrict__ packed) {
  pack_x9<KH, KW, S, CIN, HIN, WIN, NSAMP, ROT, KS>(w, packed, blockIdx.x * 256 + threadIdx.x);
}

// The data gradient of a stride-1 KH x KW convolution as a forward one (rth_conv_dgrad, conv3):
//   gx[b, iy, ix, ci] = sum_{kh, kw, co} gy[b, iy - kh, ix - kw, co] W[co, kh, kw, ci]
// = the convolution of gy zero-padded by K - 1 with W' [ci][kh'][kw'][co] = W[co][K-1-kh'][K-1-kw'][ci]
// (the flipped, channel-transposed kernel), run by k_conv_x9 with PAD = K - 1 and no epilogue.
// This packs W' from the forward OHWI weights into the x9 B fragments (slot layout of pack_x9:
// output channel = ci, k' = (kh', kw', co), co fastest).
template <int KH, int KW, int CIN, int COUT, int HIN, int WIN, int NSAMP, int ROT, int KS>
__device__ __forceinline__ void pack_x9_dgrad(const float *__restrict__ w, u32x4 *__restrict__ packed, int sl) {
  using G = X9Geom<KH, KW, 1, COUT, HIN, WIN, NSAMP, ROT, KS>;  // the dgrad's "input" channels = the conv's COUT
  if (sl >= G::PACKED_U4) return;
  const int lane = sl % 64, t = (sl / 64) % 3, c = (sl / 192) % G::NCH, cb = sl / (192 * G::NCH);
  const int ci = cb * 16 + (lane & 15), k0 = c * 32 + 8 * (lane >> 4);
  const int tap = k0 / COUT, co0 = k0 % COUT, kh = KH - 1 - tap / KW, kw = KW - 1 - tap % KW;
  float wv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) wv[j] = w[((int64_t)(co0 + j) * KH * KW + kh * KW + kw) * CIN + ci];  // OHWI
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = bf16x3_term(wv[j], t);
  packed[sl] = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
}
template <int KH, int KW, int CIN, int COUT, int HIN, int WIN, int NSAMP, int ROT, int KS>
__global__ __launch_bounds__(256) void k_conv_pack_x9_dgrad(const float *__restrict__ w, u32x4 *__restrict__ packed) {
  pack_x9_dgrad<KH, KW, CIN, COUT, HIN, WIN, NSAMP, ROT, KS>(w, packed, blockIdx.x * 256 + threadIdx.x);
}

// conv2 (4x4, stride 2) has no single flipped kernel: its data gradient splits by the parity
// (py, px) of the input pixel, iy = 2 jy + py, ix = 2 jx + px.  Only taps kh = py + 2 a,
// kw = px + 2 c reach such a pixel, from output pixel (jy - a, jx - c), so each class is a
// stride-1 2x2 convolution of gy zero-padded by 1 with
//   W'_cls[ci][kh'][kw'][co] = W[co][py + 2 (1 - kh')][px + 2 (1 - kw')][ci]
// (kh' = 1 - a).  The 4 class kernels are packed back to back (class = 2 py + px), the slot
// layout of pack_x9 each (output channel = ci, k' = (kh', kw', co), co fastest).
template <int CIN, int COUT, int NSAMP, int ROT, int KS>
__device__ __forceinline__ void pack_x9_dgrad_cls(const float *__restrict__ w, u32x4 *__restrict__ packed, int slg) {
  using G = X9Geom<2, 2, 1, COUT, 11, 11, NSAMP, ROT, KS, CIN>;
  if (slg >= 4 * G::PACKED_U4) return;
  const int cls = slg / G::PACKED_U4, sl = slg - cls * G::PACKED_U4, py = cls >> 1, px = cls & 1;
  const int lane = sl % 64, t = (sl / 64) % 3, c = (sl / 192) % G::NCH, cb = sl / (192 * G::NCH);
  const int ci = cb * 16 + (lane & 15), k0 = c * 32 + 8 * (lane >> 4);
  const int tap = k0 / COUT, co0 = k0 % COUT, kh = py + 2 * (1 - tap / 2), kw = px + 2 * (1 - tap % 2);
  float wv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) wv[j] = w[((int64_t)(co0 + j) * 16 + kh * 4 + kw) * CIN + ci];  // OHWI, 4x4
  uint32_t e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = bf16x3_term(wv[j], t);
  packed[slg] = u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
}
template <int CIN, int COUT, int NSAMP, int ROT, int KS>
__global__ __launch_bounds__(256) void k_conv_pack_x9_dgrad_cls(const float *__restrict__ w,
                                                                u32x4 *__restrict__ packed) {
  pack_x9_dgrad_cls<CIN, COUT, NSAMP, ROT, KS>(w, packed, blockIdx.x * 256 + threadIdx.x);
}

// K parts per workgroup (waves = 4 channel blocks x KS): more parts, fewer weight registers per
// wave and more waves per CU
constexpr int kX9Conv3KS = 2, kX9Dgrad3KS = 2, kX9Dgrad2KS = 2;
#define X9_CONV3 3, 3, 1, 64, 9, 9, 4, 3, kX9Conv3KS

// the data gradients' packed kernels (X9Dgrad3 / X9Dgrad2: 1 sample per workgroup -- the
// packed layout does not depend on the samples per workgroup)
template <int NS>
using X9Dgrad3 = X9Geom<3, 3, 1, 64, 11, 11, NS, 3, kX9Dgrad3KS>;
template <int NS>
using X9Dgrad2 = X9Geom<2, 2, 1, 64, 11, 11, NS, 3, kX9Dgrad2KS, 32>;
__device__ __forceinline__ void pack_dgrad3(const float *w, u32x4 *packed, int sl) {
  pack_x9_dgrad<3, 3, 64, 64, 11, 11, 1, 3, kX9Dgrad3KS>(w, packed, sl);
}
__device__ __forceinline__ void pack_dgrad2(const float *w, u32x4 *packed, int sl) {
  pack_x9_dgrad_cls<32, 64, 1, 3, kX9Dgrad2KS>(w, packed, sl);
}

}  // namespace rth
