// Per-class logit bias on gfx950 (ifseg_amd/predict.py Segmenter(class_bias=...), Segmenter.bias_sweep_raw; prior-shift
// correction, Saerens et al. 2002; logit adjustment, Menon et al., ICLR 2021; the calibration factor of the zero-shot
// segmentation tables): a vector b [n] is SUBTRACTED from the logits in front of the temperature, and K strengths of one bias
// direction are scored against one ground truth in ONE launch.  include/ifseg_hip.h states the rule and predict.py's
// bias_sweep_reference is the specification.  No [n, h, w] tensor is written: nothing but counters.
//
//   softmax_rows_bias_kernel  evalops.hip's softmax_rows_kernel with a = z_c - bias[c] in place of z_c (one fp32 subtraction of
//                             the widened bf16 logit): prob = softmax(a * inv_t), or a itself without do_softmax.  The
//                             operations behind the subtraction are the ones the compiler made of that kernel on gfx950 -- a
//                             rounded product for the maximum, ONE fused multiply-add a * inv_t - m for the exponent -- written
//                             out with contraction off, so that bias = 0 gives that kernel's bits in both modes.
//   seg_score_grids_kernel    seg_tsweep_kernel's walk (tsweep.hip): a workgroup of 256 threads owns 16 rows x 64 pixels
//                             (tile.h), lane = x, a wave takes 4 consecutive rows.  The ground truth of the thread's four
//                             pixels is read once; k is the outer loop.  Per k the footprint of grid k is staged in LDS at
//                             pt_stride(n) (a footprint that does not fit reads global memory in the same loop) and the class
//                             walk keeps the running first maximum of upsample.h's blend: the label is seg_predict's bit for
//                             bit.  No sum of squares, no fp64, no blend of the true class.
//                             The table: ONE workgroup-private uint32 [3][n] (+ the two tallies) in LDS, filled through
//                             count.h's bin_add, flushed to areas[k] and cleared behind every k.  A table [K][3][n] would be
//                             96 KiB at K = 16, n = 512, and it would save no atomic: the bins of different k go to different
//                             addresses, so the same non-zero bins leave either way, one 64-bit atomic each.  What the single
//                             table costs is one more barrier per k and 3 n LDS dwords read again; what it buys is one code
//                             path, 6 KiB at most, and 58 KiB left for the footprint at every K.  The two tallies leave with
//                             the last k's bins (count.h's bins_flush): once, not K times.
// Dynamic LDS of the second kernel: the staged footprint and the table: 64 KiB at most, nothing static.  Integers only, so every
// output is bit-reproducible.
#include <cfloat>
#include "count.h"
#include "tile.h"
#include "upsample.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using namespace count;
using namespace upsample;

constexpr int BS_MAX_K = 16;
constexpr int BS_MAX_CLASSES = 512;

// the table's dwords ([3][n], then scored / out of range), in whole 16-byte slots
__host__ __device__ inline int bs_table_dwords(int n) { return (3 * n + 2 + 3) & ~3; }
// what is left of 64 KiB for the staged footprint
inline int bs_stage_limit(int n) { return 65536 - bs_table_dwords(n) * 4; }

int g_bs_stage_limit = 65536;         // the caller's ceiling (ifseg_seg_score_grids_staging); the launch takes the smaller

// prob[r, 0..n) = softmax((logits[r, 0..n) - bias) * inv_t) in fp32 (do_softmax) or the fp32 difference; one thread per row
__global__ void softmax_rows_bias_kernel(const bf16_t* logits, long long row_bs, int rows_per_batch, int ld,
                                         const float* __restrict__ bias, float* prob, int rows, int n, float inv_t,
                                         int do_softmax) {
#pragma clang fp contract(off)
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  const bf16_t* lp = logits + (long long)(r / rows_per_batch) * row_bs + (long long)(r % rows_per_batch) * ld;
  float* pp = prob + (long long)r * n;
  if (!do_softmax) {
    for (int c = 0; c < n; ++c) pp[c] = bf2f(lp[c]) - bias[c];
    return;
  }
  float m = -INFINITY;
  for (int c = 0; c < n; ++c) m = fmaxf(m, (bf2f(lp[c]) - bias[c]) * inv_t);
  float s = 0.f;
  for (int c = 0; c < n; ++c) {
    const float e = __expf(__builtin_fmaf(bf2f(lp[c]) - bias[c], inv_t, -m));
    pp[c] = e;
    s += e;
  }
  const float inv = 1.f / s;
  for (int c = 0; c < n; ++c) pp[c] *= inv;
}

// classes [0, n) of the thread's four pixels on one grid: seg_tsweep_kernel's class_walk without the sum of squares -- the
// running first maximum alone.  VEC: 16-byte reads of 4 classes (the staged rows), else one class per read
template <bool VEC, typename Ptr>
__device__ __forceinline__ void label_walk(Ptr base, int n, int o0, int o1, const long long (&r0)[4], const long long (&r1)[4],
                                           const bool (&fresh)[4], const float (&w00)[4], const float (&w01)[4],
                                           const float (&w10)[4], const float (&w11)[4], Best (&best)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { best[j].v = -INFINITY; best[j].c = 0; }
  int c = 0;
  if (VEC) {
    for (; c + 4 <= n; c += 4) {
      f32x4 a, b, d, e;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j == 0 || fresh[j]) {
          a = *reinterpret_cast<const f32x4*>(base + r0[j] + o0 + c);
          b = *reinterpret_cast<const f32x4*>(base + r0[j] + o1 + c);
          d = *reinterpret_cast<const f32x4*>(base + r1[j] + o0 + c);
          e = *reinterpret_cast<const f32x4*>(base + r1[j] + o1 + c);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float v = blend(w00[j], w01[j], w10[j], w11[j], a[k], b[k], d[k], e[k]);
          if (v > best[j].v) { best[j].v = v; best[j].c = c + k; }
        }
      }
    }
  }
  for (; c < n; ++c) {
    float a, b, d, e;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j == 0 || fresh[j]) {
        a = base[r0[j] + o0 + c]; b = base[r0[j] + o1 + c]; d = base[r1[j] + o0 + c]; e = base[r1[j] + o1 + c];
      }
      const float v = blend(w00[j], w01[j], w10[j], w11[j], a, b, d, e);
      if (v > best[j].v) { best[j].v = v; best[j].c = c; }
    }
  }
}

// 168 VGPRs with the second launch bound (169 without it, one over the step to a third wave per SIMD); no spills either way
__global__ __launch_bounds__(256, 3) void seg_score_grids_kernel(const float* __restrict__ grids, int K, long long grid_stride,
                                                                 int hp, int wp, int n, int h, int w, int tiles_x, int tiles_y,
                                                                 const void* __restrict__ gt, int gt_bytes, int raw,
                                                                 unsigned long long* areas, unsigned long long* tally,
                                                                 int stage_floats) {
  extern __shared__ __attribute__((aligned(16))) float stage[];   // stage_floats of footprint, then the table
  uint32_t* tab = reinterpret_cast<uint32_t*>(stage + stage_floats);
  for (int i = threadIdx.x; i < 3 * n + 2; i += 256) tab[i] = 0;  // published by the barrier at the top of the k loop

  const auto [b, X0, Y0, xend, yend, lane, wave] = tile_decode(tiles_x, tiles_y, h, w);
  const FloatCoord cy{(float)hp / (float)h, hp}, cx{(float)wp / (float)w, wp};

  int ylo, yhi, xlo, xhi;
  footprint(cy, Y0, yend - 1, &ylo, &yhi);
  footprint(cx, X0, xend - 1, &xlo, &xhi);
  const int fh = yhi - ylo + 1, fw = xhi - xlo + 1, stride = pt_stride(n);
  const bool staged = (long long)fh * fw * stride <= (long long)stage_floats;       // workgroup-uniform, the same for every k

  // the thread's four pixels: coordinates, weights, and the ground truth, once
  const int x = min(X0 + lane, w - 1);
  int x0, x1;
  float lx;
  cx(x, &x0, &x1, &lx);
  int y0[4], y1[4], cls[4];
  float w00[4], w01[4], w10[4], w11[4];
  bool fresh[4], sc[4];
  int scored = 0, bad = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yr = Y0 + wave * 4 + j, y = min(yr, h - 1);
    float ly;
    cy(y, &y0[j], &y1[j], &ly);
    fresh[j] = j == 0 || y0[j] != y0[j - 1] || y1[j] != y1[j - 1];
    w00[j] = (1.f - ly) * (1.f - lx); w01[j] = (1.f - ly) * lx; w10[j] = ly * (1.f - lx); w11[j] = ly * lx;
    const bool ok = yr < h && X0 + lane < w;
    const long long pix = ((long long)b * h + y) * w + x;
    const int g = gt_bytes == 1 ? elem_at<1>(gt, pix) : elem_at<2>(gt, pix);
    const GtClass t = gt_class(n, raw, g, ok);
    cls[j] = t.sc ? t.cls : 0;          // an unscored pixel names bin 0 and adds nothing
    sc[j] = t.sc;
    scored += t.sc; bad += t.oor;
  }
  long long r0[4], r1[4];
  int o0, o1;
  if (staged) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { r0[j] = (y0[j] - ylo) * fw * stride; r1[j] = (y1[j] - ylo) * fw * stride; }
    o0 = (x0 - xlo) * stride; o1 = (x1 - xlo) * stride;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) { r0[j] = (long long)y0[j] * wp * n; r1[j] = (long long)y1[j] * wp * n; }
    o0 = x0 * n; o1 = x1 * n;
  }

  for (int k = 0; k < K; ++k) {
    const float* sb = grids + (long long)k * grid_stride + (long long)b * hp * wp * n;
    unsigned long long* out = areas + (long long)k * 3 * n;
    __syncthreads();                    // the table is zero; grid k - 1 has been read
    Best best[4];
    // the column offsets go through an empty asm per grid, as in seg_tsweep_kernel: the addresses built on them are then
    // worked out again for every k and not kept in registers across the loop
    int p0 = o0, p1 = o1;
    asm volatile("" : "+v"(p0), "+v"(p1));
    if (staged) {
      // the fw patches of one footprint row are contiguous in global memory: fw * n floats
      const int run = fw * n;
      for (int i = threadIdx.x; i < fh * run; i += 256) {
        const int ry = i / run, q = i - ry * run, rx = q / n, c = q - rx * n;
        stage[(ry * fw + rx) * stride + c] = sb[((long long)(ylo + ry) * wp + xlo) * n + q];
      }
      __syncthreads();
      label_walk<true>(stage, n, p0, p1, r0, r1, fresh, w00, w01, w10, w11, best);
    } else {
      label_walk<false>(sb, n, p0, p1, r0, r1, fresh, w00, w01, w10, w11, best);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bin_add(tab, 2 * n + cls[j], sc[j]);
      bin_add(tab, n + best[j].c, sc[j]);
      bin_add(tab, cls[j], sc[j] && best[j].c == cls[j]);
    }
    if (k == K - 1) {                   // the last grid's bins leave with the two tallies
      bins_flush(tab, 3 * n, scored, bad, out, tally);
      break;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * n; i += 256) {
      const uint32_t v = tab[i];
      if (v) {
        atomicAdd(out + i, (unsigned long long)v);
        tab[i] = 0;
      }
    }
  }
}

// whether [a, a + na) and [b, b + nb) share a byte
inline bool overlap(const void* a, long long na, const void* b, long long nb) {
  const char *pa = (const char*)a, *pb = (const char*)b;
  return pa < pb + nb && pb < pa + na;
}

}  // namespace

extern "C" int ifseg_softmax_rows_bias(const void* logits, long long batch_stride, int rows_per_batch, int ld, const float* bias,
                                       float* prob, int rows, int n, float inv_temperature, int do_softmax, void* stream) {
  (void)hipGetLastError();
  if (rows <= 0) return 0;
  if (!logits || !bias || !prob) return IFSEG_ERR_BAD_ARG;
  if (((size_t)logits & 1) || ((size_t)bias & 3) || ((size_t)prob & 3)) return IFSEG_ERR_BAD_ARG;
  if (n <= 0 || rows_per_batch <= 0) return IFSEG_ERR_BAD_ARG;
  if (overlap(bias, 4ll * n, prob, 4ll * rows * n)) return IFSEG_ERR_BAD_ARG;
  hipLaunchKernelGGL(softmax_rows_bias_kernel, dim3((rows + 127) / 128), dim3(128), 0, (hipStream_t)stream,
                     (const bf16_t*)logits, batch_stride, rows_per_batch, ld, bias, prob, rows, n, inv_temperature, do_softmax);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_score_grids_staging(int max_bytes) { return swap_limit(g_bs_stage_limit, 65536, max_bytes); }

extern "C" int ifseg_seg_score_grids(const float* grids, int K, int B, int hp, int wp, int n, int h, int w, const void* gt,
                                     int gt_bytes, int raw_labels, unsigned long long* areas, unsigned long long* tally,
                                     void* stream) {
  (void)hipGetLastError();
  if (!grids || !gt || !areas || !tally) return IFSEG_ERR_BAD_ARG;
  if (gt_bytes != 1 && gt_bytes != 2) return IFSEG_ERR_BAD_ARG;
  if (((size_t)grids & 3) || ((size_t)gt & (size_t)(gt_bytes - 1)) || ((size_t)areas & 7) || ((size_t)tally & 7))
    return IFSEG_ERR_BAD_ARG;
  if (K < 1 || K > BS_MAX_K || n < 1 || n > BS_MAX_CLASSES) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || hp < 1 || wp < 1 || h < 1 || w < 1) return IFSEG_ERR_BAD_SHAPE;
  if (2ll * hp * h >= (1ll << 31) || 2ll * wp * w >= (1ll << 31) || (long long)B * h * w >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  // offsets inside one image's grid are ints: hp wp n < 2^31
  if ((long long)hp * wp >= (1ll << 31) / BS_MAX_CLASSES) return IFSEG_ERR_BAD_SHAPE;
  // the counters are written while the inputs are read: they share no byte with them or with each other
  const long long abytes = 8ll * K * 3 * n, gbytes = (long long)B * h * w * gt_bytes;
  const long long sbytes = 4ll * K * B * ((long long)hp * wp) * n;         // K B < 2^35, hp wp n < 2^31: fits 63 bits with room
  if (overlap(areas, abytes, tally, 16) || overlap(areas, abytes, grids, sbytes) || overlap(areas, abytes, gt, gbytes) ||
      overlap(tally, 16, grids, sbytes) || overlap(tally, 16, gt, gbytes))
    return IFSEG_ERR_BAD_ARG;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(h, w, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const int fixed = bs_table_dwords(n) * 4;
  const int lds = stage_bytes(hp, wp, n, h, w, std::min(g_bs_stage_limit, bs_stage_limit(n)));
  hipLaunchKernelGGL(seg_score_grids_kernel, dim3((unsigned)blocks), dim3(256), lds + fixed, (hipStream_t)stream, grids, K,
                     (long long)B * hp * wp * n, hp, wp, n, h, w, tiles_x, tiles_y, gt, gt_bytes, raw_labels != 0, areas, tally,
                     lds / 4);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_score_grids_limit(int which) {
  switch (which) {
    case 0: return BS_MAX_K;
    case 1: return BS_MAX_CLASSES;
    case 2: return TILE_ROWS;
    case 3: return TILE_COLS;
    case 4: return bs_stage_limit(BS_MAX_CLASSES);
    default: return IFSEG_ERR_BAD_ARG;
  }
}
