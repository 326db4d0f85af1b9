// Per-sample soft Dice loss on the x16 bilinear upsample of the per-patch logits (gfx950): the second term of mmseg's decode-head
// recipe (DiceLoss(smooth, exponent=2) beside CrossEntropyLoss), without the [B, H*W, nseg] score tensor.
// criterions/seg_criterion.py states the rule (dice_sums_reference, dice_loss_reference); include/ifseg_hip.h the entry points.
//
// With p_ic = softmax_c(v_i) over the valid pixels i of sample b (seg_tile.h's predicate):
//   I_bc = sum_i p_ic [y_i = c]   P_bc = sum_i p_ic^2   Y_bc = sum_i [y_i = c]      N = 2 I + s,  Q = P + Y + s
//   dice_weight L_dice = sum_b sum_c k_c (1 - N_bc / Q_bc),   k_c = dice_weight w_c / (B n)
// The gradient at a pixel needs the three sums of its whole sample: two passes with a device-side reduction between them.
//
//   seg_dice_sums_kernel   pass A.  seg_tile.h's tile: one workgroup per low-res cell = one 16 x 16 pixel tile, the 3 x 3 cells staged
//                          in LDS at an odd row stride, the four-tap value(c), one online-softmax walk; a
//                          second walk in chunks of 16 classes puts p into sD[256][17] and reduces it over the tile in two fixed
//                          steps (16 pixels of a row, then 16 rows; in fp64, rounded once) -> [tiles][3 n] fp32 partials.
//                          ifseg_reduce_parts(outer = B, parts = hp wp, n = 3 n) gives sums [B][3][n].
//   seg_dice_tile_kernel   pass B.  Stages a_bc = -2 k_c / Q_bc and e_bc = k_c N_bc / Q_bc^2 of its sample behind the logits, repeats
//                          the online softmax with T = sum_k exp(v_k - m)^2 e_bk carried beside the denominator (rescaled by
//                          exp(m - v)^2 when the maximum moves), so that S_i = a_{b,y} p_y + 2 T / sum^2, and forms
//                            d loss / d v_ic = p_ic (a_bc [y_i = c] + 2 p_ic e_bc - S_i)
//                          on the valid pixels; seg_tile.h's separable adjoint (sD -> sE -> 9 x n) gives tile_partial [tiles][9][n] in
//                          final scale.  Workgroup 0 also sums k_c (1 - N / Q) over (b, c) in a fixed order into dice_out[0].
//   loss.hip's gather (ifseg_seg_loss_gather_sum) adds the partials to the CE's: dlogits = bf16(ce_sum * (1 / Z) + dice_sum), one
//                          rounding, loss_out = [total, ce, dice]; a null CE source is Dice alone.
// No global atomics: two runs give equal bits.  All LDS is dynamic, every carve offset a multiple of 16 bytes.
#include <math.h>
#include "seg_tile.h"

namespace {

using namespace seg_tile;

__host__ __device__ constexpr int r4(int x) { return (x + 3) & ~3; }

// carve offsets of the dynamic region, in floats (each a multiple of 4)
struct Carve {
  int log, a, e, d, ee, wy, wx, red, lab, total;
};
__host__ __device__ inline Carve carve(int nseg, bool pass_b) {
  Carve c;
  c.log = 0;
  c.a = c.log + r4(9 * (nseg | 1));
  c.e = c.a + (pass_b ? r4(nseg) : 0);
  c.d = c.e + (pass_b ? r4(nseg) : 0);
  c.ee = c.d + 256 * (CH + 1);
  c.wy = c.ee + (pass_b ? 1 : 2) * 3 * TS * CH;         // pass A keeps its [3][16][16] row sums in fp64
  c.wx = c.wy + TS * 3;
  c.red = c.wx + TS * 3;
  c.lab = c.red + 256;
  c.total = c.lab + 256;
  return c;
}

// ---- pass A: the tile's I_c, P_c, Y_c ----
__global__ __launch_bounds__(256) void seg_dice_sums_kernel(const bf16_t* logits, int ldl, long long lbs, const long long* target,
                                                            long long tbs, int hp, int wp, int W, int nseg, long long seg0,
                                                            long long pad_id, long long eos_id, float* sums_part) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const Carve cv = carve(nseg, false);
  const int ls = nseg | 1;
  float* sLog = dyn + cv.log;
  float (*sD)[CH + 1] = reinterpret_cast<float (*)[CH + 1]>(dyn + cv.d);
  double (*sE)[TS][CH] = reinterpret_cast<double (*)[TS][CH]>(dyn + cv.ee);    // [3][row][cc]
  float (*sWY)[3] = reinterpret_cast<float (*)[3]>(dyn + cv.wy);
  float (*sWX)[3] = reinterpret_cast<float (*)[3]>(dyn + cv.wx);
  int* sLab = reinterpret_cast<int*>(dyn + cv.lab);
  const int tid = threadIdx.x;
  const int ncell = hp * wp;
  const int b = blockIdx.x / ncell, cell = blockIdx.x % ncell;
  const int cy = cell / wp, cx = cell % wp;
  stage_cells(sLog, ls, logits, ldl, lbs, b, cy, cx, hp, wp, nseg);
  stage_weights(sWY, sWX, cy, cx, hp, wp);
  __syncthreads();

  const int py = tid >> 4, px = tid & 15;
  const Taps value(ls, sWY, sWX, py, px);
  const long long tg = target[b * tbs + (long long)(cy * TS + py) * W + (cx * TS + px)];
  const bool valid = is_class(tg, seg0, nseg, pad_id, eos_id);
  sLab[tid] = valid ? (int)(tg - seg0) : -1;
  // The sums are held to 4 e N_b of the fp64 specification, e the specification's own fp32 error on one probability.  Where every
  // pixel of a tile sees the same logits (a single cell, every tap clamped) a rounding repeats in all 256 pixels instead of
  // averaging out, so nothing here rounds more than once: ohem.hip's softmax (the accurate expf, the denominator in fp64), p
  // rounded to fp32 once, the tile's sums in fp64, one rounding into the fp32 partial.
  float m = -INFINITY;
  double sum = 0.0;
  for (int c = 0; c < nseg; ++c) {
    const float v = value(sLog, c);
    if (v > m) { sum = sum * exp((double)(m - v)) + 1.0; m = v; }   // (rare: it scales the whole sum, so in fp64 as well)
    else sum += (double)expf(v - m);
  }
  const double rsum = 1.0 / sum;

  float* out = sums_part + (long long)blockIdx.x * 3 * nseg;
  const int rc = tid & (CH - 1), rr = tid >> 4;                 // reducer: class rc of the chunk, pixel row rr
  for (int c0 = 0; c0 < nseg; c0 += CH) {
#pragma unroll
    for (int cc = 0; cc < CH; ++cc) {
      const int c = c0 + cc;
      sD[tid][cc] = (valid && c < nseg) ? (float)((double)expf(value(sLog, c) - m) * rsum) : 0.f;
    }
    __syncthreads();
    {
      double si = 0.0, sp = 0.0, sy = 0.0;
#pragma unroll
      for (int xx = 0; xx < TS; ++xx) {
        const double p = (double)sD[rr * TS + xx][rc];
        const bool hit = sLab[rr * TS + xx] == c0 + rc;
        si += hit ? p : 0.0;
        sp += p * p;
        sy += hit ? 1.0 : 0.0;
      }
      sE[0][rr][rc] = si;
      sE[1][rr][rc] = sp;
      sE[2][rr][rc] = sy;
    }
    __syncthreads();
    if (tid < 3 * CH) {
      const int cc = tid % CH, q = tid / CH;
      double s = 0.0;
#pragma unroll
      for (int yy = 0; yy < TS; ++yy) s += sE[q][yy][cc];
      if (c0 + cc < nseg) out[q * nseg + c0 + cc] = (float)s;
    }
  }
}

// ---- pass B: the gradient tile and (workgroup 0) the value ----
__global__ __launch_bounds__(256) void seg_dice_tile_kernel(const bf16_t* logits, int ldl, long long lbs, const long long* target,
                                                            long long tbs, int B, int hp, int wp, int W, int nseg, long long seg0,
                                                            long long pad_id, long long eos_id, const float* sums,
                                                            const float* class_weight, float dice_weight, float smooth,
                                                            float* tile_partial, float* dice_out) {
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  const Carve cv = carve(nseg, true);
  const int ls = nseg | 1;
  float* sLog = dyn + cv.log;
  float* sA = dyn + cv.a;                                       // [nseg] a_bc
  float* sEc = dyn + cv.e;                                      // [nseg] e_bc
  float (*sD)[CH + 1] = reinterpret_cast<float (*)[CH + 1]>(dyn + cv.d);
  float (*sE)[3][CH] = reinterpret_cast<float (*)[3][CH]>(dyn + cv.ee);        // [row][kx][cc]
  float (*sWY)[3] = reinterpret_cast<float (*)[3]>(dyn + cv.wy);
  float (*sWX)[3] = reinterpret_cast<float (*)[3]>(dyn + cv.wx);
  float* sRed = dyn + cv.red;
  const int tid = threadIdx.x;
  const int ncell = hp * wp;
  const int b = blockIdx.x / ncell, cell = blockIdx.x % ncell;
  const int cy = cell / wp, cx = cell % wp;
  const float kscale = dice_weight / ((float)B * (float)nseg);  // k_c = kscale w_c

  stage_cells(sLog, ls, logits, ldl, lbs, b, cy, cx, hp, wp, nseg);
  stage_weights(sWY, sWX, cy, cx, hp, wp);
  for (int c = tid; c < nseg; c += 256) {
    const float* sb = sums + (long long)b * 3 * nseg;
    const float N = 2.f * sb[c] + smooth, Q = sb[nseg + c] + sb[2 * nseg + c] + smooth;
    const float k = kscale * (class_weight ? class_weight[c] : 1.f);
    sA[c] = -2.f * k / Q;
    sEc[c] = k * N / (Q * Q);
  }
  if (blockIdx.x == 0) {
    // dice_weight L_dice = sum_{b,c} k_c (1 - N_bc / Q_bc): a thread takes every 256th term, then a fixed tree
    float part = 0.f;
    for (int i = tid; i < B * nseg; i += 256) {
      const int bb = i / nseg, c = i % nseg;
      const float* sb = sums + (long long)bb * 3 * nseg;
      const float N = 2.f * sb[c] + smooth, Q = sb[nseg + c] + sb[2 * nseg + c] + smooth;
      part += kscale * (class_weight ? class_weight[c] : 1.f) * (1.f - N / Q);
    }
    sRed[tid] = part;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (tid < w) sRed[tid] += sRed[tid + w];
      __syncthreads();
    }
    if (tid == 0) dice_out[0] = sRed[0];
  }
  __syncthreads();

  const int py = tid >> 4, px = tid & 15;
  const Taps value(ls, sWY, sWX, py, px);
  const long long tg = target[b * tbs + (long long)(cy * TS + py) * W + (cx * TS + px)];
  const bool valid = is_class(tg, seg0, nseg, pad_id, eos_id);
  const int label = valid ? (int)(tg - seg0) : 0;
  float m = -INFINITY, sum = 0.f, tt = 0.f, vl = 0.f;            // tt = sum_k exp(v_k - m)^2 e_k
  for (int c = 0; c < nseg; ++c) {
    const float v = value(sLog, c);
    const float ec = sEc[c];
    if (v > m) {
      const float r = __expf(m - v);
      sum = sum * r + 1.f;
      tt = tt * (r * r) + ec;
      m = v;
    } else {
      const float x = __expf(v - m);
      sum += x;
      tt += x * x * ec;
    }
    if (c == label) vl = v;
  }
  const float lse = m + __logf(sum);
  const float rs = 1.f / sum;
  // S_i = sum_k p_k g_k = a_y p_y + 2 sum_k p_k^2 e_k
  const float S = sA[label] * __expf(vl - lse) + 2.f * tt * (rs * rs);

  float* tp = tile_partial + (long long)blockIdx.x * 9 * nseg;
  for (int c0 = 0; c0 < nseg; c0 += CH) {
#pragma unroll
    for (int cc = 0; cc < CH; ++cc) {
      const int c = c0 + cc;
      float d = 0.f;
      if (valid && c < nseg) {
        const float p = __expf(value(sLog, c) - lse);
        d = p * ((c == label ? sA[c] : 0.f) + 2.f * p * sEc[c] - S);
      }
      sD[tid][cc] = d;
    }
    adjoint_chunk(sD, sE, sWY, sWX, tp, c0, nseg);
  }
}

}  // namespace

extern "C" int ifseg_seg_dice_sums(const void* logits, int ldl, long long logits_bs, const long long* target, long long target_bs,
                                   int B, int hp, int wp, int H, int W, int nseg, long long seg_id_offset, long long pad_id,
                                   long long eos_id, float* sums_part, void* stream) {
  (void)hipGetLastError();
  if (const int rc = check_tile_args(logits, ldl, logits_bs, target, target_bs, B, hp, wp, H, W, nseg)) return rc;
  if (!sums_part || ((size_t)sums_part & 3)) return IFSEG_ERR_BAD_ARG;
  const size_t dyn = (size_t)carve(nseg, false).total * 4;
  hipLaunchKernelGGL(seg_dice_sums_kernel, dim3(B * hp * wp), dim3(256), dyn, (hipStream_t)stream, (const bf16_t*)logits, ldl,
                     logits_bs, target, target_bs, hp, wp, W, nseg, seg_id_offset, pad_id, eos_id, sums_part);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_dice_tiles(const void* logits, int ldl, long long logits_bs, const long long* target, long long target_bs,
                                    int B, int hp, int wp, int H, int W, int nseg, long long seg_id_offset, long long pad_id,
                                    long long eos_id, const float* sums, const float* class_weight, float dice_weight, float smooth,
                                    float* tile_partial, float* dice_out, void* stream) {
  (void)hipGetLastError();
  if (const int rc = check_tile_args(logits, ldl, logits_bs, target, target_bs, B, hp, wp, H, W, nseg)) return rc;
  if (!sums || !tile_partial || !dice_out || ((size_t)sums & 3) || ((size_t)tile_partial & 3) || ((size_t)dice_out & 3) ||
      ((size_t)class_weight & 3))
    return IFSEG_ERR_BAD_ARG;
  if (!(smooth > 0.f) || !isfinite(smooth) || !(dice_weight > 0.f) || !isfinite(dice_weight)) return IFSEG_ERR_BAD_ARG;
  const size_t dyn = (size_t)carve(nseg, true).total * 4;
  hipLaunchKernelGGL(seg_dice_tile_kernel, dim3(B * hp * wp), dim3(256), dyn, (hipStream_t)stream, (const bf16_t*)logits, ldl,
                     logits_bs, target, target_bs, B, hp, wp, W, nseg, seg_id_offset, pad_id, eos_id, sums, class_weight,
                     dice_weight, smooth, tile_partial, dice_out);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
