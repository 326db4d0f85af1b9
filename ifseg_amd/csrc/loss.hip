// Fused criterion kernel for the segmentation loss (gfx950, HBM-bound):
//   bilinear upsample (align_corners=False) of per-patch logits [B, hp*wp, nseg] to pixel
//   resolution, masked mean cross entropy, its gradient w.r.t. the per-patch logits, argmax
//   and the per-class intersect / pred / label area histograms -- without ever materialising
//   the [B, H*W, nseg] fp32 score tensor (1.26 GB at B=8, 150 classes).
// Reference: criterions/seg_criterion.py:237-244 (upsample_logits), :269-347 (compute_loss),
//            :349-362 (compute_metric).  Scale factor H/hp == W/wp == 16 (every shipped config).
//
// One workgroup per low-res cell = one 16x16 pixel tile.  The tile reads the 3x3 cells its
// pixels interpolate from, each thread owns one pixel (online softmax over the classes), and
// the adjoint of the interpolation is applied separably (over x, then over y) in LDS, giving
// a [3][3][nseg] partial per tile; a second kernel gathers the <=9 partials of every cell.  seg_tile.h holds the tile's shared
// pieces (staging, tap weights, value(c), the label predicate, the adjoint); the gather here serves the whole family: the CE
// partials alone, or with dice.hip's and distill.hip's.
// No global atomics: deterministic.
//
// WT (ifseg_seg_loss_tiles_weighted): the same tile with a per-pixel weight q (uint8 plane, or 1) and a per-class weight cw
// (fp32 [nseg] staged in LDS behind the histograms, or ones):
//   l_i = (1 - eps) cw[y] (lse - v_y) + (eps / n) (lse sum_c cw[c] - sum_c cw[c] v_c)       F.cross_entropy(weight=cw)
//   d_c = q (p_c A - [c = y] (1 - eps) cw[y] - (eps / n) cw[c]),   A = (1 - eps) cw[y] + (eps / n) sum_c cw[c]
// sp[0] = sum q l, sp[1] = the tile's share of the normaliser (sum q cw[y], or qmax per valid pixel), so the reduction and the
// gather kernel below serve both.  q enters by one multiplication each: a plane times two gives the same bits.
#include <math.h>
#include "prof.h"
#include "seg_tile.h"

namespace {

using namespace seg_tile;

template <bool WT>
__global__ __launch_bounds__(256) void seg_loss_tile_kernel(const bf16_t* logits, int ldl, long long lbs,
                                                            const long long* target, long long tbs, int hp, int wp,
                                                            int W, int nseg, long long seg0, long long pad_id,
                                                            long long eos_id, float* tile_partial, float* stats_part,
                                                            int* bad_label, float eps, const unsigned char* pixel_weight,
                                                            long long pwbs, const float* class_weight, int norm_pixels) {
  extern __shared__ float dyn[];
  const int ls = nseg | 1;
  float* sLog = dyn;                                      // [9][ls]: 9 x (nseg | 1) floats + 3 x nseg ints (+ nseg floats, WT)
  int* sHist = reinterpret_cast<int*>(dyn + 9 * ls);      // [3][nseg]
  [[maybe_unused]] float* sCw = dyn + 9 * ls + 3 * nseg;  // [nseg] (WT)
  [[maybe_unused]] __shared__ float sCwSum[4];
  __shared__ float sWY[TS][3], sWX[TS][3];
  __shared__ float sD[256][CH + 1];
  __shared__ float sE[TS][3][CH];
  __shared__ float sRed[8];
  const int tid = threadIdx.x;
  const int ncell = hp * wp;
  const int b = blockIdx.x / ncell, cell = blockIdx.x % ncell;
  const int cy = cell / wp, cx = cell % wp;
  const int nstat = 2 + 3 * nseg;

  stage_cells(sLog, ls, logits, ldl, lbs, b, cy, cx, hp, wp, nseg);
  for (int i = tid; i < 3 * nseg; i += 256) sHist[i] = 0;
  if constexpr (WT) {
    float part = 0.f;                                       // nseg <= 512: at most two classes per thread
    for (int i = tid; i < nseg; i += 256) {
      const float w = class_weight ? class_weight[i] : 1.f;
      sCw[i] = w;
      part += w;
    }
    part = warp_sum(part);
    if ((tid & 63) == 0) sCwSum[tid >> 6] = part;
  }
  stage_weights(sWY, sWX, cy, cx, hp, wp);
  __syncthreads();

  const int py = tid >> 4, px = tid & 15;
  const Taps value(ls, sWY, sWX, py, px);
  const long long tg = target[b * tbs + (long long)(cy * TS + py) * W + (cx * TS + px)];
  // labels outside [seg0, seg0 + nseg) that are not pad / eos / ignore would index the LDS histograms out of bounds:
  // they are dropped here and (rare) reported to the criterion's deferred range check -- F.cross_entropy raises on them
  const bool valid = is_class(tg, seg0, nseg, pad_id, eos_id);
  const int label = valid ? (int)(tg - seg0) : 0;
  if (bad_label && !valid && !(tg == pad_id || tg == eos_id || tg == seg0 + nseg)) bad_label[0] = 1;
  float m = -INFINITY, sum = 0.f, vl = 0.f, vall = 0.f;
  int pred = 0;
#pragma unroll 2
  for (int c = 0; c < nseg; ++c) {
    const float v = value(sLog, c);
    if (v > m) { sum = sum * __expf(m - v) + 1.f; m = v; pred = c; }
    else sum += __expf(v - m);
    if (c == label) vl = v;
    if constexpr (WT) vall += sCw[c] * v;                   // sum_c cw[c] v_c
    else vall += v;
  }
  const float lse = m + __logf(sum);
  // F.cross_entropy(label_smoothing = eps): (1 - eps) * nll(label) + eps * mean_c nll(c)   (seg_criterion.py:269-287 with
  // --label-smoothing; eps == 0 keeps the plain expression, bit for bit)
  float lpix = valid ? (lse - vl) : 0.f, cnt = valid ? 1.f : 0.f;
  if (eps != 0.f && valid) lpix = (1.f - eps) * (lse - vl) + eps * (lse - vall / nseg);
  float hot = 1.f - eps;
  const float unif = eps / nseg;
  [[maybe_unused]] float q = 0.f, soft = 1.f;
  if constexpr (WT) {
    const float scw = (sCwSum[0] + sCwSum[1]) + (sCwSum[2] + sCwSum[3]);
    const float cwy = valid ? sCw[label] : 0.f;
    if (valid) q = pixel_weight ? (float)pixel_weight[b * pwbs + (long long)(cy * TS + py) * W + (cx * TS + px)] : 1.f;
    hot *= cwy;
    soft = hot + unif * scw;
    // every term of the pixel's loss before q, then q once
    lpix = q * (hot * (lse - vl) + unif * (scw * lse - vall));
    cnt = !valid ? 0.f : norm_pixels ? (pixel_weight ? 255.f : 1.f) : q * cwy;
  }
  if (valid) {
    atomicAdd(&sHist[nseg + pred], 1);
    atomicAdd(&sHist[2 * nseg + label], 1);
    if (pred == label) atomicAdd(&sHist[label], 1);
  }
  lpix = warp_sum(lpix); cnt = warp_sum(cnt);
  if ((tid & 63) == 0) { sRed[tid >> 6] = lpix; sRed[4 + (tid >> 6)] = cnt; }

  // ---- gradient: d value[c] = softmax - onehot (masked); adjoint of the interpolation
  float* tp = tile_partial + (long long)blockIdx.x * 9 * nseg;
  for (int c0 = 0; c0 < nseg; c0 += CH) {
#pragma unroll
    for (int cc = 0; cc < CH; ++cc) {
      const int c = c0 + cc;
      float d = 0.f;
      if constexpr (WT) {
        if (valid && c < nseg) d = q * (__expf(value(sLog, c) - lse) * soft - (c == label ? hot : 0.f) - unif * sCw[c]);
      } else {
        if (valid && c < nseg) d = __expf(value(sLog, c) - lse) - (c == label ? hot : 0.f) - unif;
      }
      sD[tid][cc] = d;
    }
    adjoint_chunk(sD, sE, sWY, sWX, tp, c0, nseg);
  }
  float* sp = stats_part + (long long)blockIdx.x * nstat;
  if (tid == 0) { sp[0] = sRed[0] + sRed[1] + sRed[2] + sRed[3]; sp[1] = sRed[4] + sRed[5] + sRed[6] + sRed[7]; }
  for (int i = tid; i < 3 * nseg; i += 256) sp[2 + i] = (float)sHist[i];
}

// The one gather of the family, behind three entry points: dlogits[b, cell, c] = bf16((1 / Z) sum of the <= 9 CE partials whose
// 3 x 3 stencil contains `cell` + sum of the <= 9 Dice partials + (w T / max(N, 1)) sum of the <= 9 KD partials), one rounding;
// loss_out[0 .. nout) = total, ce, dice, kd with kd = w T^2 sum KL / N (0 when N = 0).  Any source may be null: its term enters
// neither g nor the total (it is not added as a zero, so one source alone keeps the sign of a zero), its loss_out word is 0.
__global__ void seg_loss_gather_kernel(const float* ce_partial, const float* stats, const float* dice_partial,
                                       const float* dice_value, const float* kd_partial, const float* kd_stats, float kd_weight,
                                       float kd_t, bf16_t* dlogits, int ldl, long long dbs, int B, int hp, int wp, int nseg,
                                       float* loss_out, int nout) {
  const long long gid = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const int ncell = hp * wp;
  const long long total = (long long)B * (ncell + 1) * ldl;
  const float kd_n = kd_partial ? kd_stats[1] : 0.f;
  const float kd_rn = kd_n > 0.f ? 1.f / kd_n : 0.f;                         // N = 0: the term and its gradient are exactly 0
  if (gid == 0) {
    const float ce = ce_partial ? (stats[1] > 0.f ? stats[0] / stats[1] : 0.f) : 0.f;
    const float dv = dice_partial ? dice_value[0] : 0.f;
    const float kd = kd_n > 0.f ? (kd_weight * kd_t * kd_t) * (kd_stats[0] * kd_rn) : 0.f;
    float sum = ce;
    if (dice_partial) sum += dv;
    if (kd_partial) sum += kd;
    loss_out[0] = sum;
    if (nout > 1) { loss_out[1] = ce; loss_out[2] = dv; }
    if (nout > 3) loss_out[3] = kd;
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
    if (dice_partial) g += gd;
    if (kd_partial) g += gk * ((kd_weight * kd_t) * kd_rn);
  }
  dlogits[b * dbs + (long long)cell * ldl + c] = f2bf(g);
}

int launch_gather(const float* ce_partial, const float* stats, const float* dice_partial, const float* dice_value,
                  const float* kd_partial, const float* kd_stats, float kd_weight, float kd_t, void* dlogits, int ldl,
                  long long dlogits_bs, int B, int hp, int wp, int nseg, float* loss_out, int nout, void* stream) {
  const long long total = (long long)B * (hp * wp + 1) * ldl;
  hipLaunchKernelGGL(seg_loss_gather_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ce_partial,
                     stats, dice_partial, dice_value, kd_partial, kd_stats, kd_weight, kd_t, (bf16_t*)dlogits, ldl, dlogits_bs, B,
                     hp, wp, nseg, loss_out, nout);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int ifseg_seg_loss_tiles(const void* logits, int ldl, long long logits_bs, const long long* target,
                                    long long target_bs, int B, int hp, int wp, int H, int W, int nseg,
                                    long long seg_id_offset, long long pad_id, long long eos_id,
                                    float* tile_partial, float* stats_part, int* bad_label, float label_smoothing,
                                    void* stream) {
  (void)hipGetLastError();
  // (the pointer and stride refusals are the other tile entries': every caller of this one passes them)
  if (const int rc = check_tile_args(logits, ldl, logits_bs, target, target_bs, B, hp, wp, H, W, nseg)) return rc;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return IFSEG_ERR_BAD_ARG;
  const size_t dyn = (size_t)(9 * (nseg | 1) + 3 * nseg) * 4;
  hipLaunchKernelGGL(seg_loss_tile_kernel<false>, dim3(B * hp * wp), dim3(256), dyn, (hipStream_t)stream,
                     (const bf16_t*)logits, ldl, logits_bs, target, target_bs, hp, wp, W, nseg, seg_id_offset, pad_id,
                     eos_id, tile_partial, stats_part, bad_label, label_smoothing, nullptr, 0ll, nullptr, 0);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_loss_tiles_weighted(const void* logits, int ldl, long long logits_bs, const long long* target,
                                             long long target_bs, int B, int hp, int wp, int H, int W, int nseg,
                                             long long seg_id_offset, long long pad_id, long long eos_id,
                                             const unsigned char* pixel_weight, long long pw_bs, const float* class_weight,
                                             int norm_pixels, float* tile_partial, float* stats_part, int* bad_label,
                                             float label_smoothing, void* stream) {
  (void)hipGetLastError();
  if (const int rc = check_tile_args(logits, ldl, logits_bs, target, target_bs, B, hp, wp, H, W, nseg)) return rc;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return IFSEG_ERR_BAD_ARG;
  if ((pixel_weight && pw_bs < (long long)H * W) || ((size_t)class_weight & 3)) return IFSEG_ERR_BAD_ARG;
  const size_t dyn = (size_t)(9 * (nseg | 1) + 3 * nseg + nseg) * 4;
  hipLaunchKernelGGL(seg_loss_tile_kernel<true>, dim3(B * hp * wp), dim3(256), dyn, (hipStream_t)stream,
                     (const bf16_t*)logits, ldl, logits_bs, target, target_bs, hp, wp, W, nseg, seg_id_offset, pad_id,
                     eos_id, tile_partial, stats_part, bad_label, label_smoothing, pixel_weight, pw_bs, class_weight,
                     norm_pixels ? 1 : 0);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

// ---- the three doors of seg_loss_gather_kernel: CE alone (loss_out [1]), CE or none + Dice ([3]), any of the three ([4]) ----
extern "C" int ifseg_seg_loss_gather(const float* tile_partial, const float* stats, void* dlogits, int ldl,
                                     long long dlogits_bs, int B, int hp, int wp, int nseg, float* loss_out,
                                     void* stream) {
  (void)hipGetLastError();
  return launch_gather(tile_partial, stats, nullptr, nullptr, nullptr, nullptr, 0.f, 0.f, dlogits, ldl, dlogits_bs, B, hp, wp, nseg,
                       loss_out, 1, stream);
}

extern "C" int ifseg_seg_loss_gather_sum(const float* ce_partial, const float* stats, const float* dice_partial,
                                         const float* dice_value, void* dlogits, int ldl, long long dlogits_bs, int B, int hp,
                                         int wp, int nseg, float* loss_out, void* stream) {
  (void)hipGetLastError();
  if (!dice_partial || !dice_value || !dlogits || !loss_out || (ce_partial && !stats) || ((size_t)ce_partial & 3) ||
      ((size_t)stats & 3) || ((size_t)dice_partial & 3) || ((size_t)dice_value & 3) || ((size_t)dlogits & 1) ||
      ((size_t)loss_out & 3))
    return IFSEG_ERR_BAD_ARG;
  if (B < 1 || hp < 1 || wp < 1 || nseg > NS_MAX || nseg < 1 || ldl < nseg || (long long)B * hp * wp >= (1ll << 31))
    return IFSEG_ERR_BAD_SHAPE;
  if (dlogits_bs < (long long)(hp * wp + 1) * ldl) return IFSEG_ERR_BAD_ARG;
  return launch_gather(ce_partial, stats, dice_partial, dice_value, nullptr, nullptr, 0.f, 0.f, dlogits, ldl, dlogits_bs, B, hp, wp,
                       nseg, loss_out, 3, stream);
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
  return launch_gather(ce_partial, stats, dice_partial, dice_value, kd_partial, kd_stats, kd_weight, kd_temperature, dlogits, ldl,
                       dlogits_bs, B, hp, wp, nseg, loss_out, 4, stream);
}
