// The Nature-DQN convolution torso (reth/reth/algorithm/dqn/dqn_model.py:14-20: Conv2d(4,32,8,4)
// -> ReLU -> Conv2d(32,64,4,2) -> ReLU -> Conv2d(64,64,3,1) -> ReLU), forward and backward: the
// launch tables of the built geometries, the cost models that pick an instantiation, the
// several-layer weight pack and the C ABI.  The kernels:
//   conv_f32.hpp  k_conv_bias_relu, the fp32 MFMA forward (conv1 on f32 input, conv2)
//   conv1_u8.hpp  conv1 on uint8 frame stacks: forward, weight gradient, the backward's reduce
//   conv_x9.hpp   k_conv_x9, the exact-split bf16 MFMA: conv3's forward, conv3's and conv2's
//                 data gradients
#include <cstdlib>
#include <mutex>
#include <string>

#include "common.hpp"
#include "conv1_u8.hpp"
#include "conv_f32.hpp"
#include "conv_x9.hpp"
#include "optim.hpp"
#include "wgrad.hpp"

namespace rth {

// several layers in one launch (a network's torso, and the flipped data-gradient kernels of
// conv2 / conv3 for the backward of the same weights): block ranges per layer
constexpr int kPackMax = 6;
constexpr int kPackDgrad3 = 4, kPackDgrad2 = 5;  // PackJob::geom of the data-gradient packs
struct PackJob {
  int geom[kPackMax];  // index into the built geometries (find_conv order), or kPackDgrad*
  const float *w[kPackMax];
  f32x4 *packed[kPackMax];
  int first_block[kPackMax + 1];
  int n;
};

__global__ __launch_bounds__(256) void k_conv_pack_many(PackJob job) {
  int l = 0;
  while (l + 1 < job.n && (int)blockIdx.x >= job.first_block[l + 1]) ++l;
  const int sl = ((int)blockIdx.x - job.first_block[l]) * 256 + threadIdx.x;
  switch (job.geom[l]) {
    case 0: pack_conv1_bf16x3(job.w[l], reinterpret_cast<u32x4 *>(job.packed[l]), sl); break;
    case 1: pack_one<8, 8, 4, 4, 32, 84, 84>(job.w[l], job.packed[l], sl); break;
    case 2: pack_one<4, 4, 2, 32, 64, 20, 20>(job.w[l], job.packed[l], sl); break;
    case kPackDgrad3: pack_dgrad3(job.w[l], reinterpret_cast<u32x4 *>(job.packed[l]), sl); break;
    case kPackDgrad2: pack_dgrad2(job.w[l], reinterpret_cast<u32x4 *>(job.packed[l]), sl); break;
    default: pack_x9<X9_CONV3>(job.w[l], reinterpret_cast<u32x4 *>(job.packed[l]), sl); break;
  }
}

struct ConvLaunch {
  const void *fn, *pack;
  int waves;
  int lds_bytes;  // packed weight bytes
  int per_cu;  // resident workgroups per CU (occupancy query, cached)
  int u8;       // conv1 on uint8 stacks (k_conv1_u8_share, exact-split bf16 MFMA)
  int x9;       // k_conv_x9: samples per workgroup at most (0 = not an x9 kernel)
  const void *x9fn[5];  // k_conv_x9 by samples per workgroup (nullptr: not built)
  // the same kernel with its ragged last round split into channel parts (TS > 1), launched
  // instead of fn when a launch has at least tsfn_rounds whole rounds of tiles (nullptr: never)
  const void *tsfn = nullptr;
  int tsfn_rounds = 0;
};

template <int KH, int KW, int S, int CIN, int HIN, int WIN, int NSAMP, int ROT, int KS>
static ConvLaunch x9_launch() {
  using G = X9Geom<KH, KW, S, CIN, HIN, WIN, NSAMP, ROT, KS>;
  ConvLaunch l{reinterpret_cast<const void *>(&k_conv_x9<KH, KW, S, CIN, HIN, WIN, NSAMP, ROT, KS>),
               reinterpret_cast<const void *>(&k_conv_pack_x9<KH, KW, S, CIN, HIN, WIN, NSAMP, ROT, KS>), 4 * KS,
               G::PACKED_U4 * 16, 1, 0, NSAMP, {}};
  l.x9fn[1] = reinterpret_cast<const void *>(&k_conv_x9<KH, KW, S, CIN, HIN, WIN, 1, ROT, KS>);
  if (NSAMP >= 2) l.x9fn[2] = reinterpret_cast<const void *>(&k_conv_x9<KH, KW, S, CIN, HIN, WIN, (NSAMP >= 2 ? 2 : 1), ROT, KS>);
  if (NSAMP >= 3) l.x9fn[3] = reinterpret_cast<const void *>(&k_conv_x9<KH, KW, S, CIN, HIN, WIN, (NSAMP >= 3 ? 3 : 1), ROT, KS>);
  if (NSAMP >= 4) l.x9fn[4] = reinterpret_cast<const void *>(&k_conv_x9<KH, KW, S, CIN, HIN, WIN, (NSAMP >= 4 ? 4 : 1), ROT, KS>);
  return l;
}

template <int KH, int KW, int S, int CIN, int COUT, int HIN, int WIN, int WAVES, int MB, int TS = 1>
static ConvLaunch conv_launch() {
  static_assert(MB == 1, "conv_bias_relu counts 16-pixel wave tiles");
  using Gm = ConvGeom<KH, KW, S, CIN, COUT, HIN, WIN>;
  ConvLaunch l{reinterpret_cast<const void *>(&k_conv_bias_relu<KH, KW, S, CIN, COUT, HIN, WIN, WAVES, MB, TS>),
               reinterpret_cast<const void *>(&k_conv_pack<KH, KW, S, CIN, COUT, HIN, WIN>), WAVES,
               Gm::LDS_F4 * 16, 0, 0, 0, {}};
  int blocks = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, l.fn, WAVES * 64, 0) != hipSuccess || blocks < 1)
    blocks = 1;
  l.per_cu = blocks;
  return l;
}

// conv1 on the uint8 stacks: k_conv1_u8_share (r05: each lane converts half of its window and
// takes the other half from its neighbour by DPP)
static ConvLaunch conv1_u8_launch() {
  ConvLaunch l{reinterpret_cast<const void *>(&k_conv1_u8_share<false>),
               reinterpret_cast<const void *>(&k_conv1_pack_bf16x3), 4, kC1PackedBytes, 0, 1, 0, {}};
  int blocks = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, l.fn, 256, 0) != hipSuccess || blocks < 1) blocks = 1;
  l.per_cu = blocks;
  return l;
}

// persistent forward kernels: at most kWgPerCu workgroups per CU (each stages the weights
// once); the x9 kernels: one workgroup per CU, samples per workgroup = n / CUs rounded down to
// a built instantiation
constexpr int kWgPerCu = 2, kX9WgPerCu = 1;

// the supported geometries (the Nature-DQN torso on 4 x 84 x 84 stacks)
static bool find_conv(const rth_conv_shape &s, ConvLaunch *out, int *geom = nullptr) {
  auto is = [&](int mode, int cin, int hin, int win, int cout, int kh, int kw, int st) {
    return (s.input & ~RTH_CONV_OUT_NCHW) == mode && s.cin == cin && s.hin == hin && s.win == win && s.cout == cout && s.kh == kh &&
           s.kw == kw && s.stride == st;
  };
  if (is(RTH_CONV_U8_CHW, 4, 84, 84, 32, 8, 8, 4)) {
    static const ConvLaunch l = conv1_u8_launch();
    *out = l;
    if (geom) *geom = 0;
  } else if (is(RTH_CONV_F32_NHWC, 4, 84, 84, 32, 8, 8, 4)) {
    static const ConvLaunch l = conv_launch<8, 8, 4, 4, 32, 84, 84, 4, 1>();
    *out = l;
    if (geom) *geom = 1;
  } else if (is(RTH_CONV_F32_NHWC, 32, 20, 20, 64, 4, 4, 2)) {
    // the fp32-MFMA kernel at every batch size: standalone the x9 kernel won below ~400 samples
    // (16 vs 22 us at 256), but in the Ape-X loop its 77-154 KB of LDS per workgroup crowded the
    // concurrent stream's kernels out of the CUs, and the loop ran 0.5-1 % slower with it
    // (removed)
    // the tile schedule (r05 A/B, profiles/r05/ab_log.txt): 16-pixel x 64-channel wave tiles
    // round-robin, the ragged last round split into quarter-width units for launches of >= 4
    // whole rounds of tiles (the learner's 1,024 samples: 53.1 vs 57.9 us alone; whole tiles
    // below) -- the same outputs, bit for bit
    static const ConvLaunch l = [] {
      ConvLaunch l = conv_launch<4, 4, 2, 32, 64, 20, 20, 8, 1>();
      l.tsfn = conv_launch<4, 4, 2, 32, 64, 20, 20, 8, 1, 4>().fn;
      l.tsfn_rounds = 4;
      return l;
    }();
    *out = l;
    if (geom) *geom = 2;
  } else if (is(RTH_CONV_F32_NHWC, 64, 9, 9, 64, 3, 3, 1)) {
    static const ConvLaunch l = x9_launch<X9_CONV3>();  // x9 at every batch size
    *out = l;
    if (geom) *geom = 3;
  } else {
    return false;
  }
  return true;
}

static int cu_count() {
  static int cus = [] {
    int dev = 0, v = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || v < 1)
      v = 256;
    return v;
  }();
  return cus;
}

}  // namespace rth

using namespace rth;

// conv3's and conv2's data gradients on the exact-split bf16 MFMA (k_conv_x9 with PAD = K - 1
// and no epilogue; conv2 as its 4 stride-parity classes, one launch, blockIdx.y = class), the
// flipped kernels packed into a per-device workspace each launch.  No other geometry has a data
// gradient (the fp32-MFMA kernel that preceded these -- conv2: 43 vs 37.8 us alone, 0.574-0.575
// vs 0.571-0.573 ms/step, r04 -- is removed).
static bool is_dgrad3_x9(const rth_conv_shape *shape) {
  return shape->input == RTH_CONV_F32_NHWC && shape->cin == 64 && shape->hin == 9 && shape->win == 9 &&
         shape->cout == 64 && shape->kh == 3 && shape->kw == 3 && shape->stride == 1;
}
static bool is_dgrad2_x9(const rth_conv_shape *shape) {
  return shape->input == RTH_CONV_F32_NHWC && shape->cin == 32 && shape->hin == 20 &&
         shape->win == 20 && shape->cout == 64 && shape->kh == 4 && shape->kw == 4 && shape->stride == 2;
}

// the per-device packed-kernel workspace of one dgrad geometry (allocated on first use, which
// must not be inside a graph capture; the allocation is serialised across host threads).  It is
// shared by every caller of the NULL-workspace form on that device: that form is for one stream
// at a time (include/reth_hip.h, rth_conv_dgrad); concurrent learners pass their own workspace.
static int dgrad_workspace(u32x4 **ws, size_t bytes, hipStream_t st, u32x4 **out) {
  static std::mutex mu;
  int dev = 0;
  RTH_HIP(hipGetDevice(&dev));
  RTH_REQUIRE(dev >= 0 && dev < 64, "rth_conv_dgrad: device %d out of range", dev);
  std::lock_guard<std::mutex> lock(mu);
  if (!ws[dev]) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    RTH_REQUIRE(hipStreamIsCapturing(st, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone,
                "rth_conv_dgrad: the first data gradient of a geometry on a device must run outside graph capture");
    RTH_HIP(hipMalloc(&ws[dev], bytes));
  }
  *out = ws[dev];
  return RTH_OK;
}

// samples per workgroup (1 .. 3): the cost model of select_launch, `classes` workgroups per
// group, with each instantiation's resident workgroups per CU from the occupancy query (the
// LDS image: 1 - 3 per CU)
static int64_t dgrad_x9_nsamp(int64_t n, int classes, const void *const *fn, int threads, int cap) {
  int64_t ns = 0;
  double best = 0.0;
  for (int64_t k = 1; k <= 3; ++k) {
    if (!fn[k]) continue;  // not built
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn[k], threads, 0) != hipSuccess || per_cu < 1)
      per_cu = 1;
    const int64_t slots = (int64_t)cu_count() * (per_cu < cap ? per_cu : cap);
    const int64_t rounds = (classes * ((n + k - 1) / k) + slots - 1) / slots;
    const double cost = (double)rounds * ((double)k + 0.5);
    if (ns == 0 || cost < best) best = cost, ns = k;
  }
  return ns;
}

static int launch_dgrad_x9(const void *fn, const float *gy, int64_t n, int64_t ns, int classes, int threads,
                           const u32x4 *wpk, float *gx, hipStream_t st, const float *ymask = nullptr,
                           float *bpart = nullptr, const float *xmask = nullptr, float *xmasked = nullptr) {
  const int nsi = (int)ns;
  const int64_t grid = (n + ns - 1) / ns;
  const int64_t *n_dev = nullptr;
  const float *bias = nullptr;
  int out_nchw = 0;
  void *args[] = {(void *)&gy,    (void *)&n,     (void *)&n_dev,   (void *)&nsi,    (void *)&wpk,
                  (void *)&bias,  (void *)&gx,    (void *)&out_nchw, (void *)&ymask, (void *)&bpart,
                  (void *)&xmask, (void *)&xmasked};
  RTH_HIP(hipLaunchKernel(fn, dim3((unsigned)grid, (unsigned)classes), dim3(threads), args, 0, st));
  return RTH_OK;
}

// conv3's data gradient by mode -- kDgrad3Plain, kDgrad3Mask (+ the layer below's ReLU mask and
// bias slabs), kDgrad3Nchw (+ its own mask, read in NCHW where FC1 left the gradient) -- and
// samples per workgroup: each mode's cost model queries its own instantiations' occupancy
// (kDgrad3Nchw at 3 samples is not built: its phase B holds 64 staging registers across phase
// A's MFMA loop and spills)
enum { kDgrad3Plain = 0, kDgrad3Mask = 1, kDgrad3Nchw = 2 };
static const void *const *dgrad3_table(int mode) {
#define RTH_D3(NS, ...) \
  reinterpret_cast<const void *>(&k_conv_x9<3, 3, 1, 64, 11, 11, NS, 3, kX9Dgrad3KS, 2, ##__VA_ARGS__>)
  static const void *const fn[3][4] = {{nullptr, RTH_D3(1), RTH_D3(2), RTH_D3(3)},
                                       {nullptr, RTH_D3(1, 64, 0, 1), RTH_D3(2, 64, 0, 1), RTH_D3(3, 64, 0, 1)},
                                       {nullptr, RTH_D3(1, 64, 0, 1, 1), RTH_D3(2, 64, 0, 1, 1), nullptr}};
#undef RTH_D3
  return fn[mode];
}
// the samples per workgroup of conv3's data gradient at n samples (= its grid's divisor)
static int64_t dgrad3_nsamp(int64_t n, int mode) {
  return dgrad_x9_nsamp(n, 1, dgrad3_table(mode), X9Dgrad3<1>::NT, kX9WgPerCu);
}
// w == NULL: user_ws already holds the packed kernel (rth_conv_pack_many's data-gradient job)
static int conv_dgrad_x9_conv3(const float *gy, int64_t n, const float *w, float *gx, void *user_ws, hipStream_t st,
                               const float *ymask = nullptr, float *bpart = nullptr, const float *xmask = nullptr,
                               float *xmasked = nullptr) {
  static u32x4 *ws[64] = {};
  constexpr int PK = X9Dgrad3<1>::PACKED_U4;
  u32x4 *wpk = static_cast<u32x4 *>(user_ws);
  if (!wpk)
    if (const int rc = dgrad_workspace(ws, (size_t)PK * 16, st, &wpk)) return rc;
  RTH_REQUIRE(n * 49 * 64 * 4 < ((int64_t)1 << 31), "rth_conv_dgrad: gy of %lld samples exceeds 2 GiB", (long long)n);
  if (w) {
    hipLaunchKernelGGL((k_conv_pack_x9_dgrad<3, 3, 64, 64, 11, 11, 1, 3, kX9Dgrad3KS>), dim3((PK + 255) / 256),
                       dim3(256), 0, st, w, wpk);
    RTH_LAUNCHED();
  }
  const int mode = xmask ? kDgrad3Nchw : (ymask ? kDgrad3Mask : kDgrad3Plain);
  const int64_t ns = dgrad3_nsamp(n, mode);
  return launch_dgrad_x9(dgrad3_table(mode)[ns], gy, n, ns, 1, X9Dgrad3<1>::NT, wpk, gx, st, ymask, bpart, xmask,
                         xmasked);
}

// conv2: gy [n, 9, 9, 64] -> gx [n, 20, 20, 32]; each class reads gy padded to 11 x 11 and
// writes its 10 x 10 pixels
static int conv_dgrad_x9_conv2(const float *gy, int64_t n, const float *w, float *gx, void *user_ws, hipStream_t st) {
  // (w == NULL: user_ws holds the 4 packed class kernels already)
  static u32x4 *ws[64] = {};
  constexpr int PK = X9Dgrad2<1>::PACKED_U4;
  u32x4 *wpk = static_cast<u32x4 *>(user_ws);
  if (!wpk)
    if (const int rc = dgrad_workspace(ws, (size_t)4 * PK * 16, st, &wpk)) return rc;
  RTH_REQUIRE(n * 400 * 32 * 4 < ((int64_t)1 << 31), "rth_conv_dgrad: gx of %lld samples exceeds 2 GiB", (long long)n);
  if (w) {
    hipLaunchKernelGGL((k_conv_pack_x9_dgrad_cls<32, 64, 1, 3, kX9Dgrad2KS>), dim3((4 * PK + 255) / 256), dim3(256),
                       0, st, w, wpk);
    RTH_LAUNCHED();
  }
  const void *fn[4] = {
      nullptr, reinterpret_cast<const void *>(&k_conv_x9<2, 2, 1, 64, 11, 11, 1, 3, kX9Dgrad2KS, 1, 32, 1>),
      reinterpret_cast<const void *>(&k_conv_x9<2, 2, 1, 64, 11, 11, 2, 3, kX9Dgrad2KS, 1, 32, 1>),
      reinterpret_cast<const void *>(&k_conv_x9<2, 2, 1, 64, 11, 11, 3, 3, kX9Dgrad2KS, 1, 32, 1>)};
  // (4 waves per workgroup at COUT = 32: as many resident as the LDS image allows)
  const int64_t ns = dgrad_x9_nsamp(n, 4, fn, X9Dgrad2<1>::NT, 4);
  return launch_dgrad_x9(fn[ns], gy, n, ns, 4, X9Dgrad2<1>::NT, wpk, gx, st);
}

extern "C" {

int rth_conv_supported(const rth_conv_shape *shape) {
  ConvLaunch l;
  if (!shape || !find_conv(*shape, &l)) return 0;
  return (shape->input & RTH_CONV_OUT_NCHW) && l.u8 ? 0 : 1;  // NCHW output: not the conv1 u8 kernel
}

static int64_t select_launch(const ConvLaunch &l, int64_t n);

int rth_conv_impl(const rth_conv_shape *shape, int64_t n, int32_t *nsamp_out) {
  ConvLaunch l;
  if (nsamp_out) *nsamp_out = 0;
  if (!shape || n < 1 || !find_conv(*shape, &l)) return 0;
  if (nsamp_out) *nsamp_out = (int32_t)select_launch(l, n);
  return l.x9 ? RTH_CONV_IMPL_X9 : (l.u8 ? RTH_CONV_IMPL_BF16X3 : RTH_CONV_IMPL_F32);
}

int64_t rth_conv_packed_bytes(const rth_conv_shape *shape) {
  ConvLaunch l;
  return shape && find_conv(*shape, &l) ? (int64_t)l.lds_bytes : 0;
}

int rth_conv_pack(const rth_conv_shape *shape, const float *w, float *packed, void *stream) {
  RTH_REQUIRE(shape && w && packed, "rth_conv_pack: NULL argument");
  ConvLaunch l;
  RTH_REQUIRE(find_conv(*shape, &l), "rth_conv_pack: geometry not built");
  RTH_REQUIRE(((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(packed)) & 15) == 0,
              "rth_conv_pack: misaligned buffer");
  void *args[] = {(void *)&w, (void *)&packed};
  const int slots = l.lds_bytes / 16;
  RTH_HIP(hipLaunchKernel(l.pack, dim3((unsigned)((slots + 255) / 256)), dim3(256), args, 0, as_stream(stream)));
  return RTH_OK;
}

int rth_conv_pack_many(int32_t n, const rth_conv_shape *shapes, const float *const *w, float *const *packed,
                       void *stream) {
  RTH_REQUIRE(n >= 0 && n <= kPackMax && (n == 0 || (shapes && w && packed)), "rth_conv_pack_many: bad arguments");
  PackJob job{};
  job.n = n;
  int blocks = 0;
  for (int l = 0; l < n; ++l) {
    if (shapes[l].input & RTH_CONV_PACK_DGRAD) {  // the flipped data-gradient kernel of this forward shape
      rth_conv_shape fw = shapes[l];
      fw.input &= ~RTH_CONV_PACK_DGRAD;
      const bool d3 = is_dgrad3_x9(&fw), d2 = is_dgrad2_x9(&fw);
      RTH_REQUIRE(d3 || d2, "rth_conv_pack_many: job %d: no packed data-gradient kernel for this geometry", l);
      RTH_REQUIRE(w[l] && packed[l] && ((reinterpret_cast<uintptr_t>(w[l]) | reinterpret_cast<uintptr_t>(packed[l])) &
                                        15) == 0,
                  "rth_conv_pack_many: layer %d buffer NULL or misaligned", l);
      job.geom[l] = d3 ? kPackDgrad3 : kPackDgrad2;
      job.w[l] = w[l];
      job.packed[l] = reinterpret_cast<f32x4 *>(packed[l]);
      job.first_block[l] = blocks;
      blocks += (int)((rth_conv_dgrad_workspace(&fw) / 16 + 255) / 256);
      continue;
    }
    ConvLaunch cl;
    RTH_REQUIRE(find_conv(shapes[l], &cl, &job.geom[l]), "rth_conv_pack_many: layer %d geometry not built", l);
    RTH_REQUIRE(w[l] && packed[l] && ((reinterpret_cast<uintptr_t>(w[l]) | reinterpret_cast<uintptr_t>(packed[l])) &
                                      15) == 0,
                "rth_conv_pack_many: layer %d buffer NULL or misaligned", l);
    job.w[l] = w[l];
    job.packed[l] = reinterpret_cast<f32x4 *>(packed[l]);
    job.first_block[l] = blocks;
    blocks += (cl.lds_bytes / 16 + 255) / 256;
  }
  job.first_block[n] = blocks;
  if (n == 0) return RTH_OK;
  hipLaunchKernelGGL(k_conv_pack_many, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), job);
  RTH_LAUNCHED();
  return RTH_OK;
}

static bool is_conv1_u8(const rth_conv_shape *s) {
  return s && s->input == RTH_CONV_U8_CHW && s->cin == 4 && s->hin == 84 && s->win == 84 && s->cout == 32 &&
         s->kh == 8 && s->kw == 8 && s->stride == 4;
}

int64_t rth_conv_wgrad_workspace(const rth_conv_shape *shape) {
  return is_conv1_u8(shape) ? (int64_t)kWgBlocks * (32 * 256 + 32) * 4 : 0;
}

// (norm: clip_grad_norm_'s partials in the reduce launch, rth_conv1_relu_wgrad_norm)
struct NormJob {
  const rth_param_tensor *sq;
  int32_t n_sq;
  double lr, beta1, beta2;
  int64_t *step;
  void *adam_ws;
  int32_t *nparts_out;
};
static int conv1_relu_wgrad(const rth_conv_shape *shape, const void *x, const int64_t *rows, const int32_t *fids,
                            int64_t n, const float *g, const float *y, float *gw, float *gb, void *workspace,
                            const rth_bias_deferred *deferred, int32_t ndeferred, const rth_wgrad_deferred *wdeferred,
                            int32_t nwdeferred, void *stream, const NormJob *norm = nullptr);

int rth_conv_relu_wgrad_ex(const rth_conv_shape *shape, const void *x, const int64_t *rows, int64_t n, const float *g,
                           const float *y, float *gw, float *gb, void *workspace, const rth_bias_deferred *deferred,
                           int32_t ndeferred, const rth_wgrad_deferred *wdeferred, int32_t nwdeferred, void *stream) {
  return conv1_relu_wgrad(shape, x, rows, nullptr, n, g, y, gw, gb, workspace, deferred, ndeferred, wdeferred,
                          nwdeferred, stream);
}

int rth_conv1_frames_relu_wgrad_ex(const rth_conv_shape *shape, const uint8_t *store, const int32_t *ids, int64_t n,
                                   const float *g, const float *y, float *gw, float *gb, void *workspace,
                                   const rth_bias_deferred *deferred, int32_t ndeferred,
                                   const rth_wgrad_deferred *wdeferred, int32_t nwdeferred, void *stream) {
  RTH_REQUIRE(store && ids && (reinterpret_cast<uintptr_t>(ids) & 15) == 0,
              "rth_conv1_frames_relu_wgrad_ex: NULL / misaligned frame store or ids");
  return conv1_relu_wgrad(shape, store, nullptr, ids, n, g, y, gw, gb, workspace, deferred, ndeferred, wdeferred,
                          nwdeferred, stream);
}

int rth_conv1_relu_wgrad_norm(const rth_conv_shape *shape, const void *x, const int64_t *rows, const int32_t *fids,
                              int64_t n, const float *g, const float *y, float *gw, float *gb, void *workspace,
                              const rth_bias_deferred *deferred, int32_t ndeferred, const rth_wgrad_deferred *wdeferred,
                              int32_t nwdeferred, const rth_param_tensor *sq, int32_t n_sq, double lr, double beta1,
                              double beta2, int64_t *step_dev,
                              void *adam_workspace_dev, int32_t *nparts_out, void *stream) {
  RTH_REQUIRE(!(rows && fids) && sq && n_sq >= 1 && n_sq <= RTH_MAX_PARAM_TENSORS && step_dev && adam_workspace_dev &&
                  nparts_out && n > 0,
              "rth_conv1_relu_wgrad_norm: bad arguments (rows and fids, %d tensors, a batch of %lld)", n_sq,
              (long long)n);
  for (int i = 0; i < n_sq; ++i)
    RTH_REQUIRE(sq[i].grad && sq[i].n >= 1, "rth_conv1_relu_wgrad_norm: tensor %d incomplete", i);
  if (fids)
    RTH_REQUIRE((reinterpret_cast<uintptr_t>(fids) & 15) == 0, "rth_conv1_relu_wgrad_norm: misaligned frame ids");
  const NormJob nj{sq, n_sq, lr, beta1, beta2, step_dev, adam_workspace_dev, nparts_out};
  return conv1_relu_wgrad(shape, x, rows, fids, n, g, y, gw, gb, workspace, deferred, ndeferred, wdeferred, nwdeferred,
                          stream, &nj);
}

static int conv1_relu_wgrad(const rth_conv_shape *shape, const void *x, const int64_t *rows, const int32_t *fids,
                            int64_t n, const float *g, const float *y, float *gw, float *gb, void *workspace,
                            const rth_bias_deferred *deferred, int32_t ndeferred, const rth_wgrad_deferred *wdeferred,
                            int32_t nwdeferred, void *stream, const NormJob *norm) {
  RTH_REQUIRE(shape && x && g && y && gw && gb && workspace && n >= 0, "rth_conv_relu_wgrad: NULL argument");
  RTH_REQUIRE(nwdeferred >= 0 && nwdeferred <= kWgradJobsMax && (nwdeferred == 0 || wdeferred),
              "rth_conv_relu_wgrad_ex: %d deferred weight gradients (at most %d)", nwdeferred, kWgradJobsMax);
  WgradJobs wj{};
  wj.n = nwdeferred;
  int wblocks = 0;
  for (int j = 0; j < nwdeferred; ++j) {
    const rth_wgrad_deferred &d = wdeferred[j];
    RTH_REQUIRE(d.gw && (d.splits == 0 || d.partial) && d.splits >= 0 && d.splits <= kWgfRedMax && d.elems > 0 &&
                    d.nb >= 0 && d.K > 0,
                "rth_conv_relu_wgrad_ex: deferred weight gradient %d malformed", j);
    wj.j[j] = WgfJob{d.partial, d.gw, d.splits, d.elems, d.nb, d.K};
    wblocks += wgf_reduce_blocks(wj.j[j]);
  }
  RTH_REQUIRE(ndeferred >= 0 && ndeferred <= kBiasJobsMax && (ndeferred == 0 || deferred),
              "rth_conv_relu_wgrad_ex: %d deferred bias gradients (at most %d)", ndeferred, kBiasJobsMax);
  BiasJobs bj{};
  bj.n = ndeferred;
  for (int j = 0; j < ndeferred; ++j) {
    const rth_bias_deferred &d = deferred[j];
    RTH_REQUIRE(d.workspace && d.db && d.C >= 4 && d.C <= 256 && (d.C & (d.C - 1)) == 0 && d.rows >= 0 &&
                    d.slabs >= 0 && d.slabs <= kBiasSlabs,
                "rth_conv_relu_wgrad_ex: deferred bias gradient %d malformed", j);
    bj.part[j] = static_cast<const float *>(d.workspace);
    bj.db[j] = d.db;
    bj.C[j] = d.C;
    bj.slabs[j] = d.slabs > 0 ? d.slabs : (int)bias_grad_slabs(d.rows, d.C);
  }
  RTH_REQUIRE(is_conv1_u8(shape), "rth_conv_relu_wgrad: only the uint8 conv1 geometry (4x84x84 -> 32, k8 s4) is built");
  float *part = static_cast<float *>(workspace);
  if (n == 0) {
    RTH_HIP(hipMemsetAsync(gw, 0, 32 * 256 * 4, as_stream(stream)));
    RTH_HIP(hipMemsetAsync(gb, 0, 32 * 4, as_stream(stream)));
    for (int j = 0; j < ndeferred; ++j)  // an empty batch: every layer's slabs are empty too
      RTH_HIP(hipMemsetAsync(deferred[j].db, 0, deferred[j].C * 4, as_stream(stream)));
    for (int j = 0; j < nwdeferred; ++j)
      RTH_HIP(hipMemsetAsync(wdeferred[j].gw, 0, (size_t)wdeferred[j].elems * 4, as_stream(stream)));
    return RTH_OK;
  }
  hipLaunchKernelGGL(fids ? k_conv1_wgrad_bf16x3<2> : (rows ? k_conv1_wgrad_bf16x3<1> : k_conv1_wgrad_bf16x3<0>),
                     dim3(kWgBlocks), dim3(kWgWaves * 64), 0, as_stream(stream), static_cast<const uint8_t *>(x),
                     fids ? reinterpret_cast<const int64_t *>(fids) : rows, n, g, y, part);
  RTH_LAUNCHED();
  constexpr int RB = (32 * 256 + 32 + 63) / 64;
  if (!norm) {
    hipLaunchKernelGGL((k_wgrad_reduce<8, 8, 4, 32>), dim3(RB + ndeferred + wblocks), dim3(256), 0, as_stream(stream),
                       part, kWgBlocks, gw, gb, bj, wj);
    RTH_LAUNCHED();
    return RTH_OK;
  }
  OptArgs na{};
  const int64_t nsq = opt_segments(norm->sq, norm->n_sq, kOptChunk, &na);
  const int64_t nparts = nsq + RB + ndeferred + wblocks;
  RTH_REQUIRE(nparts <= kMaxPartials, "rth_conv1_relu_wgrad_norm: %lld norm partials (at most %d)",
              (long long)nparts, kMaxPartials);
  auto *npart = static_cast<double *>(norm->adam_ws);  // rth_clip_adam_workspace's layout (optim.hip)
  auto *bc = reinterpret_cast<BiasCorr *>(static_cast<uint8_t *>(norm->adam_ws) + (int64_t)kMaxPartials * 8 + 16);
  const SqStep st{norm->step, bc, norm->lr, norm->beta1, norm->beta2};
  hipLaunchKernelGGL((k_wgrad_reduce_norm<8, 8, 4, 32>), dim3((unsigned)nparts), dim3(256), 0, as_stream(stream), part,
                     kWgBlocks, gw, gb, bj, wj, na, (int)nsq, npart, st, (int)(ndeferred + wblocks));
  RTH_LAUNCHED();
  *norm->nparts_out = (int32_t)nparts;
  return RTH_OK;
}

int rth_conv_relu_wgrad(const rth_conv_shape *shape, const void *x, const int64_t *rows, int64_t n, const float *g,
                        const float *y, float *gw, float *gb, void *workspace, void *stream) {
  return rth_conv_relu_wgrad_ex(shape, x, rows, n, g, y, gw, gb, workspace, nullptr, 0, nullptr, 0, stream);
}

// the samples per workgroup of an x9 kernel at n samples (0: not an x9 kernel): the built
// instantiation with the least estimated time, rounds x per-round time, where one workgroup is
// resident per CU (the kernel's ~160-220 VGPRs) and a round of s-sample workgroups takes
// ~(s + 0.5) single-sample times (microbench: conv3 12.3 / 20.6 / 37.2 us for s = 1 / 2 / 4 on
// 256 CUs)
static int64_t select_launch(const ConvLaunch &l, int64_t n) {
  int64_t nsamp = 0;
  const int64_t slots = (int64_t)cu_count() * kX9WgPerCu;
  double best = 0.0;
  for (int64_t s = 1; s <= l.x9; ++s) {
    if (!l.x9fn[s]) continue;
    const int64_t rounds = ((n + s - 1) / s + slots - 1) / slots;
    const double cost = (double)rounds * ((double)s + 0.5);
    if (nsamp == 0 || cost < best) best = cost, nsamp = s;
  }
  return nsamp;
}

static int conv_bias_relu(const rth_conv_shape *shape, const void *x, const int64_t *rows, int64_t n,
                          const int64_t *n_dev, const float *w, const float *bias, float *y, void *stream,
                          const int32_t *fids = nullptr) {
  RTH_REQUIRE(shape && x && w && bias && y && n >= 0, "rth_conv_bias_relu: NULL argument");
  ConvLaunch l;
  RTH_REQUIRE(find_conv(*shape, &l),
              "rth_conv_bias_relu: geometry (input %d, %d x %d x %d -> %d, k %dx%d, stride %d) not built", shape->input,
              shape->cin, shape->hin, shape->win, shape->cout, shape->kh, shape->kw, shape->stride);
  const int input = shape->input & ~RTH_CONV_OUT_NCHW, out_nchw = (shape->input & RTH_CONV_OUT_NCHW) ? 1 : 0;
  RTH_REQUIRE(!rows || input == RTH_CONV_U8_CHW, "rth_conv_bias_relu: row index needs uint8 stacks");
  RTH_REQUIRE(!out_nchw || !l.u8, "rth_conv_bias_relu: NCHW output is not built for conv1 on uint8 stacks");
  RTH_REQUIRE(((reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(y)) & 15) == 0 &&
                  (input == RTH_CONV_U8_CHW ? (reinterpret_cast<uintptr_t>(x) & 3) == 0
                                                   : (reinterpret_cast<uintptr_t>(x) & 15) == 0),
              "rth_conv_bias_relu: misaligned buffer");
  if (n == 0) return RTH_OK;
  if (l.x9) {  // one workgroup per nsamp samples
    const int64_t nsamp = select_launch(l, n);
    RTH_REQUIRE(input == RTH_CONV_F32_NHWC, "rth_conv_bias_relu: the x9 kernels read f32 NHWC input");
    RTH_REQUIRE(n * (int64_t)shape->hin * shape->win * shape->cin * 4 < ((int64_t)1 << 31),
                "rth_conv_bias_relu: %lld input samples exceed the x9 kernels' 2 GiB buffer range", (long long)n);
    const int ns = (int)nsamp;
    const int64_t grid = (n + nsamp - 1) / nsamp;
    const float *xf = static_cast<const float *>(x);
    const float *no_mask = nullptr;
    float *no_part = nullptr;
    void *args[] = {(void *)&xf, (void *)&n, (void *)&n_dev, (void *)&ns, (void *)&w, (void *)&bias, (void *)&y,
                    (void *)&out_nchw, (void *)&no_mask, (void *)&no_part, (void *)&no_mask, (void *)&no_part};
    RTH_HIP(hipLaunchKernel(l.x9fn[nsamp], dim3((unsigned)grid), dim3(l.waves * 64), args, 0, as_stream(stream)));
    return RTH_OK;
  }
  const int hout = (shape->hin - shape->kh) / shape->stride + 1, wout = (shape->win - shape->kw) / shape->stride + 1;
  // (k_conv1_u8_share: 31 virtual pixels of 21 per output row per tile; k_conv_bias_relu: 16 pixels)
  RTH_REQUIRE(!l.u8 || n * hout * kC1VPix < ((int64_t)1 << 31),
              "rth_conv_bias_relu: %lld conv1 samples exceed the kernel's 32-bit pixel index", (long long)n);
  const int64_t tiles = l.u8 ? (n * hout * kC1VPix + kC1VPerTile - 1) / kC1VPerTile : (n * hout * wout + 15) / 16;
  int64_t grid = (tiles + l.waves - 1) / l.waves;
  // persistent: at most kWgPerCu workgroups per CU (each stages the weights once)
  const int64_t resident = (int64_t)cu_count() * (l.per_cu < kWgPerCu ? l.per_cu : kWgPerCu);
  if (grid > resident) grid = resident;
  RTH_REQUIRE(!fids || (l.u8 && !rows), "rth_conv1_frames_bias_relu: needs k_conv1_u8_share (not RTH_CONV1_NOSHARE)");
  if (l.u8) {
    void *args[] = {(void *)&x, (void *)&rows, (void *)&n, (void *)&n_dev, (void *)&w, (void *)&bias, (void *)&y,
                    (void *)&fids};
    const void *fn = fids ? reinterpret_cast<const void *>(&k_conv1_u8_share<true>) : l.fn;
    RTH_HIP(hipLaunchKernel(fn, dim3((unsigned)grid), dim3(l.waves * 64), args, 0, as_stream(stream)));
    return RTH_OK;
  }
  void *args[] = {(void *)&x, (void *)&rows, (void *)&n, (void *)&n_dev, (void *)&w, (void *)&bias, (void *)&y,
                  (void *)&out_nchw};
  // whole rounds of pixel tiles over one wave slot per SIMD (the kernel's own split rule)
  const bool ts = l.tsfn && l.waves % 4 == 0 && tiles / (grid * 4) >= l.tsfn_rounds;
  RTH_HIP(hipLaunchKernel(ts ? l.tsfn : l.fn, dim3((unsigned)grid), dim3(l.waves * 64), args, 0, as_stream(stream)));
  return RTH_OK;
}

int rth_conv_dgrad_supported(const rth_conv_shape *shape) {
  return shape && (is_dgrad3_x9(shape) || is_dgrad2_x9(shape)) ? 1 : 0;
}

int64_t rth_conv_dgrad_workspace(const rth_conv_shape *shape) {
  if (!shape) return 0;
  if (is_dgrad3_x9(shape)) return (int64_t)X9Dgrad3<1>::PACKED_U4 * 16;
  if (is_dgrad2_x9(shape)) return (int64_t)4 * X9Dgrad2<1>::PACKED_U4 * 16;
  return 0;
}

int rth_conv_dgrad(const rth_conv_shape *shape, const float *gy, int64_t n, const float *w, float *gx, void *stream) {
  return rth_conv_dgrad_ws(shape, gy, n, w, gx, nullptr, stream);
}

int rth_conv_dgrad_prepacked(const rth_conv_shape *shape, const float *gy, int64_t n, const void *packed, float *gx,
                             void *stream) {
  RTH_REQUIRE(shape && gy && packed && gx && n >= 0, "rth_conv_dgrad_prepacked: NULL argument");
  RTH_REQUIRE(((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(gx)) &
               15) == 0,
              "rth_conv_dgrad_prepacked: misaligned buffer");
  const bool d3 = is_dgrad3_x9(shape), d2 = is_dgrad2_x9(shape);
  RTH_REQUIRE(d3 || d2, "rth_conv_dgrad_prepacked: no packed data-gradient kernel for this geometry");
  if (n == 0) return RTH_OK;
  void *ws = const_cast<void *>(packed);
  return d3 ? conv_dgrad_x9_conv3(gy, n, nullptr, gx, ws, as_stream(stream))
            : conv_dgrad_x9_conv2(gy, n, nullptr, gx, ws, as_stream(stream));
}

int rth_conv_dgrad_relu_supported(const rth_conv_shape *shape) { return shape && is_dgrad3_x9(shape) ? 1 : 0; }

int rth_conv_dgrad_relu_prepacked(const rth_conv_shape *shape, const float *gy, int64_t n, const void *packed,
                                  const float *y, float *gx, void *bias_ws, int64_t *slabs_out, void *stream) {
  RTH_REQUIRE(shape && gy && packed && y && gx && bias_ws && slabs_out && n >= 0,
              "rth_conv_dgrad_relu_prepacked: NULL argument");
  RTH_REQUIRE(is_dgrad3_x9(shape), "rth_conv_dgrad_relu_prepacked: only conv3's geometry (64x9x9, k3 s1) is built");
  RTH_REQUIRE(((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(gx) |
                reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(bias_ws)) &
               15) == 0,
              "rth_conv_dgrad_relu_prepacked: misaligned buffer");
  *slabs_out = 0;
  if (n == 0) return RTH_OK;
  const int64_t slabs = (n + dgrad3_nsamp(n, kDgrad3Mask) - 1) / dgrad3_nsamp(n, kDgrad3Mask);
  RTH_REQUIRE(slabs <= kBiasSlabs, "rth_conv_dgrad_relu_prepacked: %lld samples need %lld bias slabs (at most %d)",
              (long long)n, (long long)slabs, kBiasSlabs);
  *slabs_out = slabs;
  return conv_dgrad_x9_conv3(gy, n, nullptr, gx, const_cast<void *>(packed), as_stream(stream), y,
                             static_cast<float *>(bias_ws));
}

int rth_conv_dgrad_relu_nchw_supported(const rth_conv_shape *shape) { return shape && is_dgrad3_x9(shape) ? 1 : 0; }

int rth_conv_dgrad_relu_nchw_prepacked(const rth_conv_shape *shape, const float *g, const float *y, int64_t n,
                                       const void *packed, const float *y_below, float *gy, float *gx, void *bias_ws,
                                       void *bias_ws_below, int64_t *slabs_out, void *stream) {
  RTH_REQUIRE(shape && g && y && packed && y_below && gy && gx && bias_ws && bias_ws_below && slabs_out && n >= 0,
              "rth_conv_dgrad_relu_nchw_prepacked: NULL argument");
  RTH_REQUIRE(is_dgrad3_x9(shape),
              "rth_conv_dgrad_relu_nchw_prepacked: only conv3's geometry (64x9x9, k3 s1) is built");
  RTH_REQUIRE(((reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(packed) |
                reinterpret_cast<uintptr_t>(y_below) | reinterpret_cast<uintptr_t>(gy) |
                reinterpret_cast<uintptr_t>(gx) | reinterpret_cast<uintptr_t>(bias_ws) |
                reinterpret_cast<uintptr_t>(bias_ws_below)) &
               15) == 0,
              "rth_conv_dgrad_relu_nchw_prepacked: misaligned buffer");
  *slabs_out = 0;
  if (n == 0) return RTH_OK;
  const int64_t ns = dgrad3_nsamp(n, kDgrad3Nchw), slabs = (n + ns - 1) / ns;
  RTH_REQUIRE(slabs <= kBiasSlabs,
              "rth_conv_dgrad_relu_nchw_prepacked: %lld samples need %lld bias slabs (at most %d)", (long long)n,
              (long long)slabs, kBiasSlabs);
  *slabs_out = slabs;
  if (const int rc = conv_dgrad_x9_conv3(g, n, nullptr, gx, const_cast<void *>(packed), as_stream(stream), y_below,
                                         static_cast<float *>(bias_ws_below), y, gy))
    return rc;
  // conv3's own slabs from gy in rth_relu_bias_grad_nchw's order (a deferred job with slabs = 0)
  hipLaunchKernelGGL(k_bias_slabs_nhwc, dim3((unsigned)bias_grad_slabs(n * 49, 64)), dim3(kBiasThreads), 0,
                     as_stream(stream), gy, static_cast<float *>(bias_ws), n);
  RTH_LAUNCHED();
  return RTH_OK;
}

int rth_conv_dgrad_ws(const rth_conv_shape *shape, const float *gy, int64_t n, const float *w, float *gx,
                      void *workspace, void *stream) {
  RTH_REQUIRE(shape && gy && w && gx && n >= 0, "rth_conv_dgrad: NULL argument");
  RTH_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15) == 0, "rth_conv_dgrad: misaligned workspace");
  if (is_dgrad3_x9(shape)) {
    RTH_REQUIRE(((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(gx)) &
                 15) == 0,
                "rth_conv_dgrad: misaligned buffer");
    if (n == 0) return RTH_OK;
    return conv_dgrad_x9_conv3(gy, n, w, gx, workspace, as_stream(stream));
  }
  if (is_dgrad2_x9(shape)) {
    RTH_REQUIRE(((reinterpret_cast<uintptr_t>(gy) | reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(gx)) &
                 15) == 0,
                "rth_conv_dgrad: misaligned buffer");
    if (n == 0) return RTH_OK;
    return conv_dgrad_x9_conv2(gy, n, w, gx, workspace, as_stream(stream));
  }
  RTH_REQUIRE(false, "rth_conv_dgrad: geometry (%d x %d x %d -> %d, k %dx%d, stride %d) not built", shape->cin,
              shape->hin, shape->win, shape->cout, shape->kh, shape->kw, shape->stride);
  return RTH_OK;
}

int rth_conv_bias_relu(const rth_conv_shape *shape, const void *x, const int64_t *rows, int64_t n, const float *w,
                       const float *bias, float *y, void *stream) {
  return conv_bias_relu(shape, x, rows, n, nullptr, w, bias, y, stream);
}

int rth_conv1_frames_bias_relu(const rth_conv_shape *shape, const uint8_t *store, const int32_t *ids, int64_t n,
                               const float *w, const float *bias, float *y, void *stream) {
  RTH_REQUIRE(store && ids && (reinterpret_cast<uintptr_t>(ids) & 15) == 0,
              "rth_conv1_frames_bias_relu: NULL / misaligned frame store or ids");
  RTH_REQUIRE(shape && is_conv1_u8(shape) && !(shape->input & RTH_CONV_OUT_NCHW),
              "rth_conv1_frames_bias_relu: only the uint8 conv1 geometry (4x84x84 -> 32, k8 s4) is built");
  return conv_bias_relu(shape, store, nullptr, n, nullptr, w, bias, y, stream, ids);
}

int rth_conv_bias_relu_upto(const rth_conv_shape *shape, const void *x, const int64_t *rows, int64_t n_max,
                            const int64_t *n_dev, const float *w, const float *bias, float *y, void *stream) {
  RTH_REQUIRE(n_dev, "rth_conv_bias_relu_upto: NULL count");
  return conv_bias_relu(shape, x, rows, n_max, n_dev, w, bias, y, stream);
}

}  // extern "C"
