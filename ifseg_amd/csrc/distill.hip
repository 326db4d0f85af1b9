// Distillation loss on the x16 bilinear upsample of the per-patch logits (gfx950): the per-pixel KL divergence from a teacher's
// softmax to the student's, at a temperature, without either [B, H*W, nseg] score tensor.
// criterions/seg_criterion.py states the rule (distill_loss_reference); include/ifseg_hip.h the entry points.
//
// With s_i, t_i the upsampled student / teacher logits of pixel i, p_i = softmax(s_i / T), q_i = softmax(t_i / T) and M the
// masked pixels (the loss kernel's valid pixels, or every pixel), N = |M| over the whole batch:
//   L_kd = T^2 (1 / N) sum_{i in M} sum_c q_ic (log q_ic - log p_ic)       d (w L_kd) / d s_ic = w (T / N) (p_ic - q_ic) on M
// The term needs nothing beyond the pixel's own two softmaxes: one tile pass.
//
//   seg_distill_tile_kernel   loss.hip's tile: one workgroup per low-res cell = one 16 x 16 pixel tile, the 3 x 3 cells of BOTH
//                          logits staged in LDS at an odd row stride (the student widened to fp32, the teacher as the bf16 it is and
//                          widened on read: exact, and 9 KB less at 512 classes), the same four-tap value(c) in the same order for
//                          both, scaled by 1 / T after the interpolation.  One walk over the classes runs the two online softmaxes;
//                          A = sum_c exp(t_c - m_t) (t_c - s_c) is carried beside the teacher's denominator (rescaled when its
//                          maximum moves), so that KL_i = A / sum_t - lse_t + lse_s.  A second walk in chunks of 16 classes forms
//                          p_c - q_c on the pixels of M; loss.hip's separable adjoint (sD -> sE -> 9 x n) gives
//                          tile_partial [tiles][9][n], UNNORMALISED.  Per tile: [sum KL, |M and tile|].
//                          ifseg_reduce_parts(outer = 1, parts = tiles, n = 2) gives kd_stats [2] in a fixed order.
//   seg_loss_gather3_kernel   loss.hip's gather with up to three sources, any of them null:
//                          dlogits = bf16(ce_sum * (1 / Z) + dice_sum + kd_sum * (w T / max(N, 1))), one rounding,
//                          loss_out = [total, ce, dice, kd], kd = w T^2 sum KL / N (0 when N = 0).
// Arithmetic, as in dice.hip: nothing rounds more than once where a whole tile sees the same logits (a single cell, every tap
// clamped): the accurate expf, the two denominators, A, the per-pixel difference and the tile's sum of 256 pixels in fp64, one
// rounding into the fp32 partial.
// No global atomics: two runs give equal bits.  All LDS is dynamic, every carve offset a multiple of 16 bytes.
#include <math.h>
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace {

constexpr int TS = 16;       // pixels per cell side
constexpr int CH = 16;       // classes per chunk
constexpr int NS_MAX = 512;  // max classes

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

// the tap weights of the tile's 16 rows and 16 columns (source index of F.interpolate(mode='bilinear', align_corners=False):
// max((dst+0.5)/s-0.5, 0)) -- loss.hip's
__device__ __forceinline__ void stage_weights(float (*sWY)[3], float (*sWX)[3], int cy, int cx, int hp, int wp) {
  const int tid = threadIdx.x;
  if (tid < 2 * TS) {
    const bool isx = tid >= TS;
    const int t = tid & (TS - 1);
    const int c0 = isx ? cx : cy, lim = isx ? wp : hp;
    float src = ((c0 * TS + t) + 0.5f) * (1.f / TS) - 0.5f;
    src = fmaxf(src, 0.f);
    const int i0 = (int)src;
    const int i1 = min(i0 + 1, lim - 1);
    const float l1 = src - i0, l0 = 1.f - l1;
    const int s0 = i0 - (c0 - 1), s1 = i1 - (c0 - 1);
    float* wrow = isx ? sWX[t] : sWY[t];
#pragma unroll
    for (int k = 0; k < 3; ++k) wrow[k] = (k == s0 ? l0 : 0.f) + (k == s1 ? l1 : 0.f);
  }
}

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(bf16_t v) { return bf2f(v); }
__device__ __forceinline__ void narrow(float& d, bf16_t v) { d = bf2f(v); }
__device__ __forceinline__ void narrow(bf16_t& d, bf16_t v) { d = v; }

// the 3 x 3 cells around (cy, cx) of sample b -> sLog[9][ls] (zeros outside the grid); columns >= nseg and the eos row of the
// source are never read
template <typename S>
__device__ __forceinline__ void stage_cells(S* sLog, int ls, const bf16_t* logits, int ldl, long long lbs, int b, int cy, int cx,
                                            int hp, int wp, int nseg) {
  for (int i = threadIdx.x; i < 9 * nseg; i += 256) {
    const int k = i / nseg, c = i % nseg;
    const int ry = cy - 1 + k / 3, rx = cx - 1 + k % 3;
    bf16_t v = 0;
    if (ry >= 0 && ry < hp && rx >= 0 && rx < wp) v = logits[b * lbs + (long long)(ry * wp + rx) * ldl + c];
    narrow(sLog[k * ls + c], v);
  }
}

// the 2 x 2 non-zero taps among the 3 x 3 cells, accumulated in the order of loss.hip's value(c)
struct Taps {
  float wA, wB, wC, wD;
  int off, ls;
  __device__ __forceinline__ Taps(int ls_, const float (*sWY)[3], const float (*sWX)[3], int py, int px) {
    const float wy0 = sWY[py][0], wy1 = sWY[py][1], wy2 = sWY[py][2];
    const float wx0 = sWX[px][0], wx1 = sWX[px][1], wx2 = sWX[px][2];
    const int kyl = (wy0 != 0.f) ? 0 : 1, kxl = (wx0 != 0.f) ? 0 : 1;
    const float wya = kyl ? wy1 : wy0, wyb = kyl ? wy2 : wy1, wxa = kxl ? wx1 : wx0, wxb = kxl ? wx2 : wx1;
    wA = wya * wxa; wB = wya * wxb; wC = wyb * wxa; wD = wyb * wxb;
    ls = ls_;
    off = (kyl * 3 + kxl) * ls;
  }
  template <typename S>
  __device__ __forceinline__ float operator()(const S* sLog, int c) const {
    const S* lg = sLog + off;
    float v = 0.f;
    v += wA * widen(lg[c]);
    v += wB * widen(lg[ls + c]);
    v += wC * widen(lg[3 * ls + c]);
    v += wD * widen(lg[4 * ls + c]);
    return v;
  }
};

// the loss kernel's predicate: a class, not pad / eos / the ignore label
__device__ __forceinline__ bool is_class(long long tg, long long seg0, int nseg, long long pad_id, long long eos_id) {
  return !(tg == pad_id || tg == eos_id || tg == seg0 + nseg) && tg >= seg0 && tg < seg0 + nseg;
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
    __syncthreads();
    for (int i = tid; i < TS * 3 * CH; i += 256) {          // E[py][kx][cc] = sum_px WX[px][kx] D[py,px][cc]
      const int cc = i % CH, kx = (i / CH) % 3, yy = i / (3 * CH);
      float e = 0.f;
#pragma unroll
      for (int xx = 0; xx < TS; ++xx) e += sWX[xx][kx] * sD[yy * TS + xx][cc];
      sE[yy][kx][cc] = e;
    }
    __syncthreads();
    if (tid < 9 * CH) {                                      // G[ky][kx][cc] = sum_py WY[py][ky] E[py][kx][cc]
      const int cc = tid % CH, k = tid / CH, ky = k / 3, kx = k % 3;
      float gsum = 0.f;
#pragma unroll
      for (int yy = 0; yy < TS; ++yy) gsum += sWY[yy][ky] * sE[yy][kx][cc];
      if (c0 + cc < nseg) tp[k * nseg + c0 + cc] = gsum;
    }
    __syncthreads();
  }
}

// dlogits[b, cell, c] = bf16((1/Z) sum of the <=9 CE partials + sum of the <=9 Dice partials + (w T / max(N, 1)) sum of the <=9
// KD partials); loss_out = [total, ce, dice, kd]
__global__ void seg_loss_gather3_kernel(const float* ce_partial, const float* stats, const float* dice_partial,
                                        const float* dice_value, const float* kd_partial, const float* kd_stats, float kd_weight,
                                        float kd_t, bf16_t* dlogits, int ldl, long long dbs, int B, int hp, int wp, int nseg,
                                        float* loss_out) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int ncell = hp * wp;
  const long long total = (long long)B * (ncell + 1) * ldl;
  const float kd_n = kd_partial ? kd_stats[1] : 0.f;
  const float kd_rn = kd_n > 0.f ? 1.f / kd_n : 0.f;                         // N = 0: the term and its gradient are exactly 0
  if (gid == 0) {
    const float ce = ce_partial ? (stats[1] > 0.f ? stats[0] / stats[1] : 0.f) : 0.f;
    const float dv = dice_partial ? dice_value[0] : 0.f;
    const float kd = kd_n > 0.f ? (kd_weight * kd_t * kd_t) * (kd_stats[0] * kd_rn) : 0.f;
    loss_out[0] = (ce + dv) + kd;
    loss_out[1] = ce;
    loss_out[2] = dv;
    loss_out[3] = kd;
  }
  if (gid >= total) return;
  const int c = (int)(gid % ldl);
  const long long r = gid / ldl;
  const int cell = (int)(r % (ncell + 1)), b = (int)(r / (ncell + 1));
  float g = 0.f;
  if (cell < ncell && c < nseg) {
    const int cy = cell / wp, cx = cell % wp;
    float gd = 0.f, gk = 0.f;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int ty = cy - (ky - 1);
      if (ty < 0 || ty >= hp) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int tx = cx - (kx - 1);
        if (tx < 0 || tx >= wp) continue;
        const long long at = (((long long)b * ncell + ty * wp + tx) * 9 + ky * 3 + kx) * nseg + c;
        if (ce_partial) g += ce_partial[at];
        if (dice_partial) gd += dice_partial[at];
        if (kd_partial) gk += kd_partial[at];
      }
    }
    if (ce_partial) g *= stats[1] > 0.f ? 1.f / stats[1] : 0.f;
    g += gd;
    g += gk * ((kd_weight * kd_t) * kd_rn);
  }
  dlogits[b * dbs + (long long)cell * ldl + c] = f2bf(g);
}

}  // namespace

extern "C" int ifseg_seg_distill_tiles(const void* logits, int ldl, long long logits_bs, const void* teacher, int ldt,
                                       long long teacher_bs, const long long* target, long long target_bs, int B, int hp, int wp,
                                       int H, int W, int nseg, long long seg_id_offset, long long pad_id, long long eos_id,
                                       float temperature, int mask_all, float* tile_partial, float* kd_part, void* stream) {
  (void)hipGetLastError();
  if (!logits || !teacher || !tile_partial || !kd_part || (!target && !mask_all) || ((size_t)logits & 1) || ((size_t)teacher & 1) ||
      ((size_t)target & 7) || ((size_t)tile_partial & 3) || ((size_t)kd_part & 3))
    return IFSEG_ERR_BAD_ARG;
  if (B < 1 || hp < 1 || wp < 1 || H != hp * TS || W != wp * TS || nseg > NS_MAX || nseg < 1 || ldl < nseg || ldt < nseg ||
      (long long)B * hp * wp >= (1ll << 31) || !(temperature > 0.f) || !isfinite(temperature))
    return IFSEG_ERR_BAD_SHAPE;
  if ((target && target_bs < (long long)H * W) || logits_bs < (long long)hp * wp * ldl || teacher_bs < (long long)hp * wp * ldt)
    return IFSEG_ERR_BAD_ARG;
  const size_t dyn = (size_t)carve(nseg).total * 4;
  hipLaunchKernelGGL(seg_distill_tile_kernel, dim3(B * hp * wp), dim3(256), dyn, (hipStream_t)stream, (const bf16_t*)logits, ldl,
                     logits_bs, (const bf16_t*)teacher, ldt, teacher_bs, target, target_bs, hp, wp, W, nseg, seg_id_offset, pad_id,
                     eos_id, 1.f / temperature, mask_all ? 1 : 0, tile_partial, kd_part);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_loss_gather3(const float* ce_partial, const float* stats, const float* dice_partial,
                                      const float* dice_value, const float* kd_partial, const float* kd_stats, float kd_weight,
                                      float kd_temperature, void* dlogits, int ldl, long long dlogits_bs, int B, int hp, int wp,
                                      int nseg, float* loss_out, void* stream) {
  (void)hipGetLastError();
  if (!dlogits || !loss_out || (!ce_partial && !dice_partial && !kd_partial) || (ce_partial && !stats) ||
      (dice_partial && !dice_value) || (kd_partial && !kd_stats) || ((size_t)ce_partial & 3) || ((size_t)stats & 3) ||
      ((size_t)dice_partial & 3) || ((size_t)dice_value & 3) || ((size_t)kd_partial & 3) || ((size_t)kd_stats & 3) ||
      ((size_t)dlogits & 1) || ((size_t)loss_out & 3))
    return IFSEG_ERR_BAD_ARG;
  if (B < 1 || hp < 1 || wp < 1 || nseg > NS_MAX || nseg < 1 || ldl < nseg || (long long)B * hp * wp >= (1ll << 31))
    return IFSEG_ERR_BAD_SHAPE;
  if (kd_partial && (!(kd_temperature > 0.f) || !isfinite(kd_temperature))) return IFSEG_ERR_BAD_SHAPE;
  if (kd_partial && (!(kd_weight > 0.f) || !isfinite(kd_weight))) return IFSEG_ERR_BAD_ARG;
  if (dlogits_bs < (long long)(hp * wp + 1) * ldl) return IFSEG_ERR_BAD_ARG;
  const long long total = (long long)B * (hp * wp + 1) * ldl;
  hipLaunchKernelGGL(seg_loss_gather3_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ce_partial,
                     stats, dice_partial, dice_value, kd_partial, kd_stats, kd_weight, kd_temperature, (bf16_t*)dlogits, ldl,
                     dlogits_bs, B, hp, wp, nseg, loss_out);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
