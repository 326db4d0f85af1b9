// Distillation loss on the x16 bilinear upsample of the per-patch logits (gfx950): the per-pixel KL divergence from a teacher's
// softmax to the student's, at a temperature, without either [B, H*W, nseg] score tensor.
// criterions/seg_criterion.py states the rule (distill_loss_reference); include/ifseg_hip.h the entry points.
//
// With s_i, t_i the upsampled student / teacher logits of pixel i, p_i = softmax(s_i / T), q_i = softmax(t_i / T) and M the
// masked pixels (the loss kernel's valid pixels, or every pixel), N = |M| over the whole batch:
//   L_kd = T^2 (1 / N) sum_{i in M} sum_c q_ic (log q_ic - log p_ic)       d (w L_kd) / d s_ic = w (T / N) (p_ic - q_ic) on M
// The term needs nothing beyond the pixel's own two softmaxes: one tile pass.
//
//   seg_distill_tile_kernel   seg_tile.h's tile: one workgroup per low-res cell = one 16 x 16 pixel tile, the 3 x 3 cells of BOTH
//                          logits staged in LDS at an odd row stride (the student widened to fp32, the teacher as the bf16 it is and
//                          widened on read: exact, and 9 KB less at 512 classes), the four-tap value(c) for
//                          both, scaled by 1 / T after the interpolation.  One walk over the classes runs the two online softmaxes;
//                          A = sum_c exp(t_c - m_t) (t_c - s_c) is carried beside the teacher's denominator (rescaled when its
//                          maximum moves), so that KL_i = A / sum_t - lse_t + lse_s.  A second walk in chunks of 16 classes forms
//                          p_c - q_c on the pixels of M; seg_tile.h's separable adjoint (sD -> sE -> 9 x n) gives
//                          tile_partial [tiles][9][n], UNNORMALISED.  Per tile: [sum KL, |M and tile|].
//                          ifseg_reduce_parts(outer = 1, parts = tiles, n = 2) gives kd_stats [2] in a fixed order.
//   loss.hip's gather (ifseg_seg_loss_gather3) takes up to three sources, any of them null:
//                          dlogits = bf16(ce_sum * (1 / Z) + dice_sum + kd_sum * (w T / max(N, 1))), one rounding,
//                          loss_out = [total, ce, dice, kd], kd = w T^2 sum KL / N (0 when N = 0).
// Arithmetic, as in dice.hip: nothing rounds more than once where a whole tile sees the same logits (a single cell, every tap
// clamped): the accurate expf, the two denominators, A, the per-pixel difference and the tile's sum of 256 pixels in fp64, one
// rounding into the fp32 partial.
// No global atomics: two runs give equal bits.  All LDS is dynamic, every carve offset a multiple of 16 bytes.
#include <math.h>
#include "seg_tile.h"

namespace {

using namespace seg_tile;

__host__ __device__ constexpr int r4(int x) { return (x + 3) & ~3; }

// carve offsets of the dynamic region, in floats (each a multiple of 4)
struct Carve {
  int log, tea, d, ee, wy, wx, red, total;
};
__host__ __device__ inline Carve carve(int nseg) {
  Carve c;
  c.log = 0;
  c.tea = c.log + r4(9 * (nseg | 1));                   // the student's 3 x 3 cells, fp32
  c.d = c.tea + r4((9 * (nseg | 1) + 1) / 2);           // the teacher's, bf16
  c.ee = c.d + 256 * (CH + 1);
  c.wy = c.ee + TS * 3 * CH;
  c.wx = c.wy + TS * 3;
  c.red = c.wx + TS * 3;
  c.total = c.red + 2 * 256;                            // 256 fp64
  return c;
}

__global__ __launch_bounds__(256) void seg_distill_tile_kernel(const bf16_t* logits, int ldl, long long lbs, const bf16_t* teacher,
                                                               int ldt, long long tebs, const long long* target, long long tbs,
                                                               int hp, int wp, int W, int nseg, long long seg0, long long pad_id,
                                                               long long eos_id, float inv_t, int mask_all, float* tile_partial,
                                                               float* kd_part) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const Carve cv = carve(nseg);
  const int ls = nseg | 1;
  float* sS = dyn + cv.log;
  bf16_t* sT = reinterpret_cast<bf16_t*>(dyn + cv.tea);
  float (*sD)[CH + 1] = reinterpret_cast<float (*)[CH + 1]>(dyn + cv.d);
  float (*sE)[3][CH] = reinterpret_cast<float (*)[3][CH]>(dyn + cv.ee);        // [row][kx][cc]
  float (*sWY)[3] = reinterpret_cast<float (*)[3]>(dyn + cv.wy);
  float (*sWX)[3] = reinterpret_cast<float (*)[3]>(dyn + cv.wx);
  double* sRed = reinterpret_cast<double*>(dyn + cv.red);
  const int tid = threadIdx.x;
  const int ncell = hp * wp;
  const int b = blockIdx.x / ncell, cell = blockIdx.x % ncell;
  const int cy = cell / wp, cx = cell % wp;
  stage_cells(sS, ls, logits, ldl, lbs, b, cy, cx, hp, wp, nseg);
  stage_cells(sT, ls, teacher, ldt, tebs, b, cy, cx, hp, wp, nseg);
  stage_weights(sWY, sWX, cy, cx, hp, wp);
  __syncthreads();

  const int py = tid >> 4, px = tid & 15;
  const Taps value(ls, sWY, sWX, py, px);
  bool in_m = true;
  if (!mask_all) in_m = is_class(target[b * tbs + (long long)(cy * TS + py) * W + (cx * TS + px)], seg0, nseg, pad_id, eos_id);

  // both online softmaxes in one walk; the denominators and A = sum_c exp(t_c - mt) (t_c - s_c) in fp64
  float ms = -INFINITY, mt = -INFINITY;
  double sum_s = 0.0, sum_t = 0.0, acc = 0.0;
  for (int c = 0; c < nseg; ++c) {
    const float s = value(sS, c) * inv_t, t = value(sT, c) * inv_t;
    if (s > ms) { sum_s = sum_s * exp((double)(ms - s)) + 1.0; ms = s; }   // (rare: it scales the whole sum, so in fp64 as well)
    else sum_s += (double)expf(s - ms);
    const double diff = (double)t - (double)s;
    if (t > mt) {
      const double r = exp((double)(mt - t));
      sum_t = sum_t * r + 1.0;
      acc = acc * r + diff;
      mt = t;
    } else {
      const double x = (double)expf(t - mt);
      sum_t += x;
      acc += x * diff;
    }
  }
  // KL_i = sum_c q_c (t_c - s_c) - lse_t + lse_s; equal logits give equal sums and maxima, hence exactly 0
  const double kl = acc / sum_t - ((double)mt + log(sum_t)) + ((double)ms + log(sum_s));
  const float rs = (float)(1.0 / sum_s), rt = (float)(1.0 / sum_t);

  // the tile's sum KL and pixel count: a fixed tree over the 256 pixels in fp64, one rounding
  sRed[tid] = in_m ? kl : 0.0;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) sRed[tid] += sRed[tid + w];
    __syncthreads();
  }
  const double kl_sum = sRed[0];
  __syncthreads();
  sRed[tid] = in_m ? 1.0 : 0.0;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) sRed[tid] += sRed[tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    kd_part[2 * (long long)blockIdx.x] = (float)kl_sum;
    kd_part[2 * (long long)blockIdx.x + 1] = (float)sRed[0];
  }

  float* tp = tile_partial + (long long)blockIdx.x * 9 * nseg;
  for (int c0 = 0; c0 < nseg; c0 += CH) {
#pragma unroll
    for (int cc = 0; cc < CH; ++cc) {
      const int c = c0 + cc;
      float d = 0.f;
      if (in_m && c < nseg) {
        const float s = value(sS, c) * inv_t, t = value(sT, c) * inv_t;
        d = expf(s - ms) * rs - expf(t - mt) * rt;
      }
      sD[tid][cc] = d;
    }
    adjoint_chunk(sD, sE, sWY, sWX, tp, c0, nseg);
  }
}

}  // namespace

extern "C" int ifseg_seg_distill_tiles(const void* logits, int ldl, long long logits_bs, const void* teacher, int ldt,
                                       long long teacher_bs, const long long* target, long long target_bs, int B, int hp, int wp,
                                       int H, int W, int nseg, long long seg_id_offset, long long pad_id, long long eos_id,
                                       float temperature, int mask_all, float* tile_partial, float* kd_part, void* stream) {
  (void)hipGetLastError();
  if (!teacher || !tile_partial || !kd_part || ((size_t)teacher & 1) || ((size_t)tile_partial & 3) || ((size_t)kd_part & 3))
    return IFSEG_ERR_BAD_ARG;
  if (const int rc = check_tile_args(logits, ldl, logits_bs, target, target_bs, B, hp, wp, H, W, nseg, mask_all != 0)) return rc;
  if (ldt < nseg || !(temperature > 0.f) || !isfinite(temperature)) return IFSEG_ERR_BAD_SHAPE;
  if (teacher_bs < (long long)hp * wp * ldt) return IFSEG_ERR_BAD_ARG;
  const size_t dyn = (size_t)carve(nseg).total * 4;
  hipLaunchKernelGGL(seg_distill_tile_kernel, dim3(B * hp * wp), dim3(256), dyn, (hipStream_t)stream, (const bf16_t*)logits, ldl,
                     logits_bs, (const bf16_t*)teacher, ldt, teacher_bs, target, target_bs, hp, wp, W, nseg, seg_id_offset, pad_id,
                     eos_id, 1.f / temperature, mask_all ? 1 : 0, tile_partial, kd_part);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
