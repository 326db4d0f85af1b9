// Temperature scaling on gfx950 (ifseg_amd/predict.py Segmenter.calibrate_raw; Guo et al., ICML 2017): K score grids of the same
// images -- one forward's logits softmaxed at K temperatures -- are scored against one ground truth in ONE launch: per
// temperature the reliability counts hist[k][bin(conf)][label == gt class] and the two proper scores a temperature is fitted
// on, NLL and Brier, summed over the scored pixels.  include/ifseg_hip.h states the rule and predict.py's
// temperature_sweep_reference is the specification.  No [n, h, w] tensor is written: nothing but counters and partials.
//
//   seg_tsweep_kernel       seg_predict_kernel's tile: a workgroup of 256 threads owns 16 rows x 64 pixels (tile.h), lane = x, a
//                           wave takes 4 consecutive rows.  The ground truth of the thread's four pixels is read once; k is the
//                           outer loop.  Per k the footprint of grid k is staged in LDS at pt_stride(n) as phase 0 of
//                           seg_predict_kernel stages it (a footprint that does not fit reads global memory in the same loop),
//                           and the class walk gives per pixel the running first maximum and sum_c p^2 in fp64; the true
//                           class's value is one more blend.  blend (blend4), pt_stride, Best and the host's stage_bytes are
//                           upsample.h's, shared with predict.hip: the value of a class is seg_predict's bit for bit.
//                           Integers: a workgroup-private uint32 table [K][256][2] (+ the two tallies) in LDS, filled through
//                           count.h's wave-aggregated bin_add; only the non-zero bins leave, one 64-bit atomic each
//                           (count.h's bins_flush, the exit of seg_predict's scoring epilogue).
//                           Floats: the pixel's terms are fp64; a wave adds its lanes' by a butterfly, the workgroup its four
//                           waves in wave order, and the tile's K x 2 sums go to partials[tile][k][2].  No floating-point
//                           atomics, so every output is bit-reproducible.
//   seg_tsweep_sum_kernel   one thread per (k, nll | brier) adds the tiles' partials in index order and ADDS the total to the
//                           caller's sums.
// Dynamic LDS of the first kernel: the staged footprint, the table (2 KiB per temperature, + 16 bytes), the waves' sums
// (64 bytes per temperature): 64 KiB at most, nothing static.
#include <cfloat>
#include "count.h"
#include "tile.h"
#include "upsample.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using namespace count;
using namespace upsample;

constexpr int TS_MAX_K = 16;
constexpr int TS_MAX_CLASSES = 512;
constexpr int TS_BINS = 256;

// the table's dwords ([K][256][2], then scored / out of range, in whole 16-byte slots) and the bytes of the waves' sums
__host__ __device__ inline int ts_table_dwords(int K) { return K * TS_BINS * 2 + 4; }
__host__ __device__ inline int ts_red_bytes(int K) { return K * 4 * 2 * 8; }
// what is left of 64 KiB for the staged footprint
inline int ts_stage_limit(int K) { return 65536 - ts_table_dwords(K) * 4 - ts_red_bytes(K); }

int g_ts_stage_limit = 65536;         // the caller's ceiling (ifseg_seg_temperature_sweep_staging); the launch takes the smaller

// classes [0, n) of the thread's four pixels on one grid: seg_predict's class_loop without the stores, with sum_c v^2 in fp64
// beside the running first maximum.  VEC: 16-byte reads of 4 classes (the staged rows), else one class per read; the offsets
// are class_loop's
template <bool VEC, typename Ptr>
__device__ __forceinline__ void class_walk(Ptr base, int n, int o0, int o1, const long long (&r0)[4], const long long (&r1)[4],
                                           const bool (&fresh)[4], const float (&w00)[4], const float (&w01)[4],
                                           const float (&w10)[4], const float (&w11)[4], Best (&best)[4], double (&sq)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) { best[j].v = -INFINITY; best[j].c = 0; sq[j] = 0.0; }
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
          sq[j] += (double)v * (double)v;
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
      sq[j] += (double)v * (double)v;
    }
  }
}

// the value of class cls[j] at the thread's four pixels: one more blend each, on the operands the walk read for that class.
// The four pixels go through blend4 as one vector (blend's operations, element by element), which the compiler packs pixel
// by pixel; written as four scalar blends it packed the two products of one pixel and added across the halves of the pair
template <typename Ptr>
__device__ __forceinline__ void class_value(Ptr base, int o0, int o1, const long long (&r0)[4], const long long (&r1)[4],
                                            const float (&w00)[4], const float (&w01)[4], const float (&w10)[4],
                                            const float (&w11)[4], const int (&cls)[4], const bool (&sc)[4], float (&pt)[4]) {
  f32x4 a, b, d, e;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int c = sc[j] ? cls[j] : 0;             // an unscored pixel reads class 0 and contributes nowhere
    a[j] = base[r0[j] + o0 + c]; b[j] = base[r0[j] + o1 + c]; d[j] = base[r1[j] + o0 + c]; e[j] = base[r1[j] + o1 + c];
  }
  const f32x4 v = blend4(f32x4{w00[0], w00[1], w00[2], w00[3]}, f32x4{w01[0], w01[1], w01[2], w01[3]},
                         f32x4{w10[0], w10[1], w10[2], w10[3]}, f32x4{w11[0], w11[1], w11[2], w11[3]}, a, b, d, e);
#pragma unroll
  for (int j = 0; j < 4; ++j) pt[j] = v[j];
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(256) void seg_tsweep_kernel(const float* __restrict__ grids, int K, long long grid_stride, int hp,
                                                         int wp, int n, int h, int w, int tiles_x, int tiles_y,
                                                         const void* __restrict__ gt, int gt_bytes, int raw,
                                                         unsigned long long* hist, unsigned long long* tally,
                                                         double* __restrict__ partials, int stage_floats) {
  extern __shared__ __attribute__((aligned(16))) float stage[];   // stage_floats of footprint, the table, the waves' sums
  uint32_t* tab = reinterpret_cast<uint32_t*>(stage + stage_floats);
  const int tdw = ts_table_dwords(K);
  double* red = reinterpret_cast<double*>(tab + tdw);             // [K][4 waves][2]
  for (int i = threadIdx.x; i < tdw; i += 256) tab[i] = 0;        // published by the barrier at the top of the k loop

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
    cls[j] = t.cls; sc[j] = t.sc;
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
    __syncthreads();                    // the table is zero (k = 0); grid k - 1 has been read
    Best best[4];
    double sq[4];
    float pt[4];
    // the column offsets go through an empty asm per grid: the addresses built on them are then worked out again for every k
    // and not kept in some hundred registers across the loop, which cost a wave per SIMD
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
      class_walk<true>(stage, n, p0, p1, r0, r1, fresh, w00, w01, w10, w11, best, sq);
      class_value(stage, p0, p1, r0, r1, w00, w01, w10, w11, cls, sc, pt);
    } else {
      class_walk<false>(sb, n, p0, p1, r0, r1, fresh, w00, w01, w10, w11, best, sq);
      class_value(sb, p0, p1, r0, r1, w00, w01, w10, w11, cls, sc, pt);
    }
    double nll = 0.0, brier = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bin_add(tab + k * (TS_BINS * 2), conf_bin(best[j].v) * 2 + (best[j].c == cls[j] ? 1 : 0), sc[j]);
      const double p = (double)pt[j];
      if (sc[j]) {
        nll += -log(fmax(p, (double)FLT_MIN));
        brier += sq[j] - 2.0 * p + 1.0;
      }
    }
    nll = wave_sum(nll);
    brier = wave_sum(brier);
    if (lane == 0) { red[(k * 4 + wave) * 2] = nll; red[(k * 4 + wave) * 2 + 1] = brier; }
  }

  bins_flush(tab, K * TS_BINS * 2, scored, bad, hist, tally);
  // the tile's sums: the four waves in wave order
  if ((int)threadIdx.x < 2 * K) {
    const int k = threadIdx.x >> 1, which = threadIdx.x & 1;
    double s = red[(k * 4) * 2 + which];
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) s += red[(k * 4 + wv) * 2 + which];
    partials[(long long)blockIdx.x * (2 * K) + threadIdx.x] = s;
  }
}

// sums[i] += the tiles' partials[t][i] in the order t = 0 .. tiles - 1, i = (k, nll | brier)
__global__ __launch_bounds__(64) void seg_tsweep_sum_kernel(const double* __restrict__ partials, long long tiles, int K2,
                                                            double* __restrict__ sums) {
  const int i = threadIdx.x;
  if (i >= K2) return;
  double s = 0.0;
  for (long long t = 0; t < tiles; ++t) s += partials[t * K2 + i];
  sums[i] += s;
}

}  // namespace

extern "C" int ifseg_seg_temperature_sweep_staging(int max_bytes) { return swap_limit(g_ts_stage_limit, 65536, max_bytes); }

extern "C" int ifseg_seg_temperature_sweep(const float* grids, int K, int B, int hp, int wp, int n, int h, int w, const void* gt,
                                           int gt_bytes, int raw_labels, unsigned long long* hist, unsigned long long* tally,
                                           double* sums, double* partials, void* stream) {
  (void)hipGetLastError();
  if (!grids || !gt || !hist || !tally || !sums || !partials) return IFSEG_ERR_BAD_ARG;
  if (gt_bytes != 1 && gt_bytes != 2) return IFSEG_ERR_BAD_ARG;
  if (((size_t)grids & 3) || ((size_t)gt & (size_t)(gt_bytes - 1)) || ((size_t)hist & 7) || ((size_t)tally & 7) ||
      ((size_t)sums & 7) || ((size_t)partials & 7))
    return IFSEG_ERR_BAD_ARG;
  if (K < 1 || K > TS_MAX_K || n < 1 || n > TS_MAX_CLASSES) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || hp < 1 || wp < 1 || h < 1 || w < 1) return IFSEG_ERR_BAD_SHAPE;
  if (2ll * hp * h >= (1ll << 31) || 2ll * wp * w >= (1ll << 31) || (long long)B * h * w >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  // offsets inside one image's grid are ints: hp wp n < 2^31
  if ((long long)hp * wp >= (1ll << 31) / TS_MAX_CLASSES) return IFSEG_ERR_BAD_SHAPE;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(h, w, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const int fixed = ts_table_dwords(K) * 4 + ts_red_bytes(K);
  const int lds = stage_bytes(hp, wp, n, h, w, std::min(g_ts_stage_limit, ts_stage_limit(K)));
  hipLaunchKernelGGL(seg_tsweep_kernel, dim3((unsigned)blocks), dim3(256), lds + fixed, (hipStream_t)stream, grids, K,
                     (long long)B * hp * wp * n, hp, wp, n, h, w, tiles_x, tiles_y, gt, gt_bytes, raw_labels != 0, hist, tally,
                     partials, lds / 4);
  IFSEG_CHECK_LAUNCH();
  hipLaunchKernelGGL(seg_tsweep_sum_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, blocks, 2 * K, sums);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_temperature_sweep_limit(int which) {
  switch (which) {
    case 0: return TS_MAX_K;
    case 1: return TS_MAX_CLASSES;
    case 2: return TILE_ROWS;
    case 3: return TILE_COLS;
    case 4: return ts_stage_limit(TS_MAX_K);
    default: return IFSEG_ERR_BAD_ARG;
  }
}
