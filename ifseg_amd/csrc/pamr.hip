// Pixel-adaptive mask refinement on gfx950 (PAMR: Araslanov & Roth, CVPR 2020; ifseg_amd/predict.py Segmenter(pamr_iters=)):
// a few iterations of a local, image-adaptive, convex averaging of the class values at image resolution, linear in the pixels.
// include/ifseg_hip.h states the rule and predict.py's pamr_reference is the specification.  Two kernels:
//
//   pamr_affinity_kernel   one 16 x 64 tile (tile.h) per workgroup: the image's tile plus a halo of R = max d, clamped to the
//                          image (replicate padding), staged in LDS as bytes; lane = x, a wave takes 4 rows, one pixel at a
//                          time.  Per channel the sums of x and x^2 over the 9 D taps in integers (M S2 - S1^2 < 2^31: no
//                          cancellation), the 8 D logits in registers (D is a template argument, the loops are unrolled), the
//                          accurate expf, IEEE divisions, the softmax denominator summed in tap order.  Writes w [8 D][H][W].
//   pamr_iterate_kernel    one launch per iteration, one (4 RPT) x 64 tile per workgroup: a thread keeps the 8 D weights of its
//                          RPT pixels in registers for the whole launch (they do not depend on the class) and the class loop
//                          sits inside the tile: one class plane's tile plus halo is staged in LDS as fp32, every pixel is
//                          8 D fused multiply-adds in tap order on LDS reads at lane-consecutive addresses (no bank
//                          conflict), and the running first maximum gives the labels and conf of the last iteration without
//                          an argmax pass.  The halo rows of a wave are loaded eight at a time before they are written to
//                          LDS (one at a time, the launch ran at the latency of a global load per row: 1.6 ms against 0.6 ms
//                          at 150 classes).  RPT = 4 (tile.h's 16 x 64 tile) up to D = 2, RPT = 2 (8 x 64) above: four rows
//                          read the halo 7 times over instead of 12, but 192 weights per thread at D = 6 leave two waves per
//                          SIMD, and two rows with four waves measured 13 % faster there (profiles/pamr_bench.txt).
// No atomics and no sums across threads: two runs give equal bits.
#include "tile.h"
#include "upsample.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using upsample::Best;

constexpr int PM_MAX_D = 8;              // dilations of a call at most
constexpr int PM_MAX_DILATION = 32;      // == hip.SEG_PAMR_MAX_DILATION: (16 + 64)(64 + 64) fp32 = 40 KiB of LDS
constexpr int PM_MAX_CLASSES = 512;
constexpr int PM_STAGE_CHUNK = 8;        // halo rows a wave loads before it writes them to LDS
constexpr int PM_STAGE_W = TILE_COLS + 2 * PM_MAX_DILATION;       // floats of a staged row, whatever R: row j of a thread is an immediate offset

struct Dilations {
  int d[PM_MAX_D];
};

// tap t = 0..7 of a dilation: (oy, ox) = (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0) (1,1)
__host__ __device__ constexpr int tap_oy(int t) { return (t + (t >= 4)) / 3 - 1; }
__host__ __device__ constexpr int tap_ox(int t) { return (t + (t >= 4)) % 3 - 1; }

template <int D>
__global__ __launch_bounds__(256) void pamr_affinity_kernel(const unsigned char* __restrict__ img, Dilations dil, int R, int H,
                                                            int W, float* __restrict__ w, int tiles_x, int tiles_y) {
  extern __shared__ __attribute__((aligned(16))) unsigned char halo[];      // [16 + 2 R][64 + 2 R][3]
  const Tile t = tile_decode(tiles_x, tiles_y, H, W);
  const int hw = TILE_COLS + 2 * R, hh = TILE_ROWS + 2 * R;

  // phase 0: a neighbour outside the image is the nearest pixel inside
  for (int hy = t.wave; hy < hh; hy += 4) {
    const int y = min(max(t.Y0 - R + hy, 0), H - 1);
    for (int hx = t.lane; hx < hw; hx += 64) {
      const int x = min(max(t.X0 - R + hx, 0), W - 1);
      const unsigned char* p = img + ((long long)y * W + x) * 3;
      unsigned char* q = halo + (hy * hw + hx) * 3;
      q[0] = p[0]; q[1] = p[1]; q[2] = p[2];
    }
  }
  __syncthreads();

  // phase 1: no barrier below
  constexpr int K = 8 * D, M = 9 * D;
  const long long plane = (long long)H * W;
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    const int ry = t.wave * 4 + j, y = t.Y0 + ry, x = t.X0 + t.lane;
    if (y >= t.yend || x >= t.xend) continue;
    const unsigned char* c0 = halo + ((ry + R) * hw + t.lane + R) * 3;
    const int xc[3] = {c0[0], c0[1], c0[2]};
    // S1, S2 over the 9 taps of every dilation, the centre once per dilation; M S2 - S1^2 <= 72^2 255^2 / 4 < 2^31
    int s1[3], s2[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) { s1[ch] = D * xc[ch]; s2[ch] = D * xc[ch] * xc[ch]; }
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int d = dil.d[i];
#pragma unroll
      for (int tp = 0; tp < 8; ++tp) {
        const unsigned char* q = c0 + (tap_oy(tp) * d * hw + tap_ox(tp) * d) * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) { const int v = q[ch]; s1[ch] += v; s2[ch] += v * v; }
      }
    }
    float den[3];
#pragma unroll
    for (int ch = 0; ch < 3; ++ch)
      den[ch] = 1e-8f + 0.1f * sqrtf((float)(M * s2[ch] - s1[ch] * s1[ch]) / (float)(M * (M - 1)));
    float a[K], m = -INFINITY;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      const int d = dil.d[i];
#pragma unroll
      for (int tp = 0; tp < 8; ++tp) {
        const unsigned char* q = c0 + (tap_oy(tp) * d * hw + tap_ox(tp) * d) * 3;
        const float s = (float)abs(xc[0] - (int)q[0]) / den[0] + (float)abs(xc[1] - (int)q[1]) / den[1] +
                        (float)abs(xc[2] - (int)q[2]) / den[2];
        a[i * 8 + tp] = -s / 3.f;
        m = fmaxf(m, a[i * 8 + tp]);
      }
    }
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { a[k] = expf(a[k] - m); sum += a[k]; }
    float* o = w + (long long)y * W + x;
#pragma unroll
    for (int k = 0; k < K; ++k) o[k * plane] = a[k] / sum;
  }
}

template <int D, int RPT>
__global__ __launch_bounds__(256, 2) void pamr_iterate_kernel(const float* __restrict__ w, const float* __restrict__ src,
                                                              float* __restrict__ dst, Dilations dil, int R, int n, int H, int W,
                                                              int tiles_x, void* __restrict__ labels, int label_bytes,
                                                              float* __restrict__ conf) {
  extern __shared__ __attribute__((aligned(16))) float stage[];             // [4 RPT + 2 R][PM_STAGE_W]: one class plane's tile + halo
  constexpr int K = 8 * D, TR = 4 * RPT;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int X0 = (blockIdx.x % tiles_x) * TILE_COLS, Y0 = (blockIdx.x / tiles_x) * TR;
  const int hw = TILE_COLS + 2 * R, hh = TR + 2 * R;
  const long long plane = (long long)H * W;
  const int x = X0 + lane;

  // the thread's weights, once per launch
  float wt[RPT][K];
  bool ok[RPT];
  long long pix[RPT];
#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    const int y = Y0 + wave * RPT + j;
    ok[j] = y < H && x < W;
    pix[j] = (long long)y * W + x;
    const long long pw = ok[j] ? pix[j] : 0;               // a pixel outside the image takes pixel 0's weights and stores nothing
#pragma unroll
    for (int k = 0; k < K; ++k) wt[j][k] = w[k * plane + pw];
  }
  // the two columns a lane stages of every halo row (hw <= 128), clamped to the image
  const int sx0 = min(max(X0 - R + lane, 0), W - 1), sx1 = min(max(X0 - R + lane + 64, 0), W - 1);

  Best best[RPT];
#pragma unroll
  for (int j = 0; j < RPT; ++j) { best[j].v = -INFINITY; best[j].c = 0; }

  for (int c = 0; c < n; ++c) {
    const float* s = src + c * plane;
    __syncthreads();                                       // the previous class's reads are done
    // PM_STAGE_CHUNK halo rows of a wave at a time: their loads (always inside the plane) are in flight together
    for (int h0 = wave; h0 < hh; h0 += 4 * PM_STAGE_CHUNK) {
      float v0[PM_STAGE_CHUNK], v1[PM_STAGE_CHUNK];
#pragma unroll
      for (int u = 0; u < PM_STAGE_CHUNK; ++u) {
        const float* row = s + (long long)min(max(Y0 - R + min(h0 + 4 * u, hh - 1), 0), H - 1) * W;
        v0[u] = row[sx0];
        v1[u] = row[sx1];
      }
#pragma unroll
      for (int u = 0; u < PM_STAGE_CHUNK; ++u) {
        const int hy = h0 + 4 * u;
        if (hy < hh) {
          stage[hy * PM_STAGE_W + lane] = v0[u];
          if (lane + 64 < hw) stage[hy * PM_STAGE_W + lane + 64] = v1[u];
        }
      }
    }
    __syncthreads();
    // the thread's first pixel in the staged plane; its row j lies j PM_STAGE_W floats further, an immediate offset of the read.
    // Opaque per class: hoisted out of the class loop, the 8 D tap addresses would take as many registers as the weights of a
    // row.  Four taps at a time: the sums are pinned behind them (the empty asm) and the scheduler does not cross
    // (sched_barrier); left alone, the compiler loads all 8 D RPT values first and the registers run out at D = 4
    int p = (wave * RPT + R) * PM_STAGE_W + lane + R;
    asm volatile("" : "+v"(p));
    float acc[RPT];
#pragma unroll
    for (int j = 0; j < RPT; ++j) acc[j] = 0.f;
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int tp = 0; tp < 8; ++tp) {
        const int q = p + (tap_oy(tp) * PM_STAGE_W + tap_ox(tp)) * dil.d[i];
#pragma unroll
        for (int j = 0; j < RPT; ++j) acc[j] = __builtin_fmaf(wt[j][i * 8 + tp], stage[q + j * PM_STAGE_W], acc[j]);
        if ((tp & 3) == 3) {
#pragma unroll
          for (int j = 0; j < RPT; ++j) asm volatile("" : "+v"(acc[j]));
          __builtin_amdgcn_sched_barrier(0);
        }
      }
    // a pixel outside the image has read clamped copies: finite, and not stored
#pragma unroll
    for (int j = 0; j < RPT; ++j) {
      if (ok[j]) dst[c * plane + pix[j]] = acc[j];
      if (acc[j] > best[j].v) { best[j].v = acc[j]; best[j].c = c; }
    }
  }

#pragma unroll
  for (int j = 0; j < RPT; ++j) {
    if (!ok[j]) continue;
    if (labels) {
      if (label_bytes == 1) reinterpret_cast<unsigned char*>(labels)[pix[j]] = (unsigned char)best[j].c;
      else reinterpret_cast<short*>(labels)[pix[j]] = (short)best[j].c;
    }
    if (conf) conf[pix[j]] = best[j].v;
  }
}

// the dilations of a call, checked -> R = the largest, or a negative error
int check_dilations(const int* dilations, int D, Dilations* dil) {
  if (!dilations || D < 1 || D > PM_MAX_D) return IFSEG_ERR_BAD_ARG;
  int R = 0;
  for (int i = 0; i < PM_MAX_D; ++i) {
    dil->d[i] = i < D ? dilations[i] : 0;
    if (i < D && (dilations[i] < 1 || dilations[i] > PM_MAX_DILATION)) return IFSEG_ERR_BAD_ARG;
    R = std::max(R, dil->d[i]);
  }
  return R;
}

}  // namespace

extern "C" int ifseg_pamr_limit(int which) {
  switch (which) {
    case 0: return PM_MAX_D;
    case 1: return PM_MAX_DILATION;
    case 2: return PM_MAX_CLASSES;
    default: return IFSEG_ERR_BAD_ARG;
  }
}

extern "C" int ifseg_pamr_affinity(const void* image, int H, int W, const int* dilations, int D, float* w, void* stream) {
  (void)hipGetLastError();
  if (!image || !w || ((size_t)w & 3)) return IFSEG_ERR_BAD_ARG;
  Dilations dil;
  const int R = check_dilations(dilations, D, &dil);
  if (R < 0) return R;
  if (H < 1 || W < 1 || (long long)H * W * 8 * D >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(H, W, 1, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const int lds = (TILE_ROWS + 2 * R) * (TILE_COLS + 2 * R) * 3;
  const unsigned char* img = (const unsigned char*)image;
#define PAMR_AFFINITY(DD)                                                                                                  \
  case DD:                                                                                                                 \
    hipLaunchKernelGGL(pamr_affinity_kernel<DD>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, img, dil, R, H, W, \
                       w, tiles_x, tiles_y);                                                                               \
    break;
  switch (D) {
    PAMR_AFFINITY(1) PAMR_AFFINITY(2) PAMR_AFFINITY(3) PAMR_AFFINITY(4)
    PAMR_AFFINITY(5) PAMR_AFFINITY(6) PAMR_AFFINITY(7) PAMR_AFFINITY(8)
  }
#undef PAMR_AFFINITY
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_pamr_iterate(const float* w, const float* src, float* dst, int n, int H, int W, const int* dilations, int D,
                                  void* labels, int label_bytes, float* conf, void* stream) {
  (void)hipGetLastError();
  if (!w || !src || !dst || ((size_t)w & 3) || ((size_t)src & 3) || ((size_t)dst & 3) || ((size_t)conf & 3)) return IFSEG_ERR_BAD_ARG;
  if (labels && (label_bytes != 1 && label_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if (labels && label_bytes == 2 && ((size_t)labels & 1)) return IFSEG_ERR_BAD_ARG;
  if (n < 1 || n > PM_MAX_CLASSES || (labels && label_bytes == 1 && n > 256)) return IFSEG_ERR_BAD_ARG;
  Dilations dil;
  const int R = check_dilations(dilations, D, &dil);
  if (R < 0) return R;
  if (H < 1 || W < 1 || (long long)H * W * n >= (1ll << 31) || (long long)H * W * 8 * D >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  const long long vbytes = (long long)H * W * n * 4, wbytes = (long long)H * W * 8 * D * 4;
  if (overlaps(dst, vbytes, src, vbytes) || overlaps(dst, vbytes, w, wbytes)) return IFSEG_ERR_BAD_ARG;
  // rows per thread, chosen by measurement (profiles/pamr_bench.txt): 4 (16 x 64 tiles, the smaller share of halo) while four
  // rows of weights leave four waves per SIMD (D <= 2), else 2 (8 x 64 tiles: half the registers, twice the waves).
  // IFSEG_PAMR_RPT=2 / 4 (a laboratory switch, common.h) forces one of them, 4 up to D = 6 (its registers run out above)
  static const char* lab_rpt = ifseg_lab_env("IFSEG_PAMR_RPT");
  int rpt = D <= 2 ? 4 : 2;
  if (lab_rpt && (lab_rpt[0] == '2' || lab_rpt[0] == '4')) rpt = (lab_rpt[0] == '4' && D <= 6) ? 4 : 2;
  const int tiles_x = (W + TILE_COLS - 1) / TILE_COLS, tiles_y = (H + 4 * rpt - 1) / (4 * rpt);
  const long long blocks = (long long)tiles_x * tiles_y;
  if (blocks >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  const int lds = (4 * rpt + 2 * R) * PM_STAGE_W * 4;
#define PAMR_LAUNCH(DD, RPT)                                                                                               \
  hipLaunchKernelGGL((pamr_iterate_kernel<DD, RPT>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, w, src, dst, dil, \
                     R, n, H, W, tiles_x, labels, label_bytes, conf)
#define PAMR_ITERATE(DD)                                                                                                   \
  case DD:                                                                                                                 \
    if (rpt == 4) PAMR_LAUNCH(DD, 4); else PAMR_LAUNCH(DD, 2);                                                             \
    break;
  switch (D) {
    PAMR_ITERATE(1) PAMR_ITERATE(2) PAMR_ITERATE(3) PAMR_ITERATE(4) PAMR_ITERATE(5) PAMR_ITERATE(6)
    case 7: PAMR_LAUNCH(7, 2); break;
    case 8: PAMR_LAUNCH(8, 2); break;
  }
#undef PAMR_LAUNCH
#undef PAMR_ITERATE
  IFSEG_CHECK_LAUNCH();
  return 0;
}
