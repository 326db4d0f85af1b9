// The 16 x 16 pixel tile of the segmentation-loss kernels (loss.hip, ohem.hip, dice.hip, distill.hip), once.
//
// One workgroup of 256 threads per low-res cell = one 16 x 16 pixel tile of the x16 bilinear upsample (align_corners=False) of
// the per-patch logits.  The tile stages the 3 x 3 cells its pixels interpolate from at an odd row stride, thread tid owns
// pixel (tid >> 4, tid & 15) and reads its value(c) through `Taps`, and a kernel with a gradient fills sD[256][CH + 1] per chunk
// of CH classes and hands it to `adjoint_chunk`, which applies the adjoint of the interpolation separably (over x, then over y)
// into the tile's [9][nseg] partial.  The arithmetic order of everything here is a contract: the tests pin the same four taps in
// the same order across the kernels, the OHEM plane feeds an order statistic, and a captured step equals eager bit for bit.
// What differs per kernel -- the softmax walk and its fp32 / fp64 choices, the LDS carve, the fill of sD -- stays in its file.
#pragma once
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace seg_tile {

constexpr int TS = 16;       // pixels per cell side
constexpr int CH = 16;       // classes per gradient chunk
constexpr int NS_MAX = 512;  // max classes (LDS: 9 x (nseg | 1) floats and what the kernel adds, sized per launch)

__device__ __forceinline__ float widen(float v) { return v; }
__device__ __forceinline__ float widen(bf16_t v) { return bf2f(v); }
__device__ __forceinline__ void narrow(float& d, bf16_t v) { d = bf2f(v); }
__device__ __forceinline__ void narrow(bf16_t& d, bf16_t v) { d = v; }

// the 3 x 3 cells around (cy, cx) of sample b -> sLog[9][ls] (zeros outside the grid), widened to fp32 or kept as the bf16 they
// are (widened on read: exact).  ls = nseg | 1: odd, so the four taps of a pixel (rows k apart) fall into different banks.
// Columns >= nseg and the eos row of the source are never read.
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

// the tap weights of the tile's 16 rows and 16 columns over the 3 cells of each axis
__device__ __forceinline__ void stage_weights(float (*sWY)[3], float (*sWX)[3], int cy, int cx, int hp, int wp) {
  const int tid = threadIdx.x;
  if (tid < 2 * TS) {
    // source index of F.interpolate(mode='bilinear', align_corners=False): max((dst+0.5)/s-0.5, 0)
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

// A pixel's bilinear value has at most 2 x 2 non-zero taps among the 3 x 3 cells around its own: rows {0,1} or {1,2},
// columns likewise.  Only those four are read and accumulated, in the same (increasing k) order as the nine-term sum this
// replaces -- whose other five terms were exact zeros: the result is bit-identical, at 4 instead of 9 LDS reads per class
// (the loop over the classes runs twice per pixel; at 150 - 171 classes the loss kernel was 0.6 - 1.0 ms of a step).
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
  // value(c) of the cells staged at sLog, fp32 or bf16
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

// the valid-label predicate: a class, not pad / eos / the ignore label
__device__ __forceinline__ bool is_class(long long tg, long long seg0, int nseg, long long pad_id, long long eos_id) {
  return !(tg == pad_id || tg == eos_id || tg == seg0 + nseg) && tg >= seg0 && tg < seg0 + nseg;
}

// The adjoint of the interpolation for the chunk of classes c0 .. c0 + CH - 1, whose per-pixel derivatives every thread has just
// written to sD[tid][0 .. CH): over x (xx ascending) into sE, then over y (yy ascending) into tp[9][nseg], with the barriers
// before, between and after.  Every thread of the workgroup calls it.
__device__ __forceinline__ void adjoint_chunk(const float (*sD)[CH + 1], float (*sE)[3][CH], const float (*sWY)[3],
                                              const float (*sWX)[3], float* tp, int c0, int nseg) {
  const int tid = threadIdx.x;
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

// the refusals every tile launch shares (host); target_optional: a launch that does not read the target may pass none
inline int check_tile_args(const void* logits, int ldl, long long logits_bs, const long long* target, long long target_bs, int B,
                           int hp, int wp, int H, int W, int nseg, bool target_optional = false) {
  if (!logits || (!target && !target_optional) || ((size_t)logits & 1) || ((size_t)target & 7)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || hp < 1 || wp < 1 || H != hp * TS || W != wp * TS || nseg > NS_MAX || nseg < 1 || ldl < nseg ||
      (long long)B * hp * wp >= (1ll << 31))
    return IFSEG_ERR_BAD_SHAPE;
  if ((target && target_bs < (long long)H * W) || logits_bs < (long long)hp * wp * ldl) return IFSEG_ERR_BAD_ARG;
  return 0;
}

}  // namespace seg_tile
