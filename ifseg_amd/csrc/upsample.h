// The value rule of the score-grid upsampling kernels (predict.hip: the four seg_predict* kernels; tsweep.hip:
// seg_tsweep_kernel), each part written once: the LDS stride of a staged patch, a pixel's running first maximum and the flat
// four-weight value of one class (and of four at once); and the host's size of the staged patches under a tile (stage_bytes:
// seg_predict_kernel, seg_tsweep_kernel).  Both files promise the same bits for the same grid, so neither keeps a copy.
#pragma once
#include "tile.h"

namespace upsample {

// LDS stride of one patch row of n classes, in floats: a multiple of 4 whose quarter is odd
__host__ __device__ inline int pt_stride(int n) {
  const int q = (n + 3) >> 2;
  return ((q & 1) ? q : q + 1) << 2;
}

struct Best {
  float v;
  int c;
};

// one class of one pixel: the flat four-weight rule, first maximum wins.  Four rounded products, added in order: contraction
// is off here, because which of the products the compiler fuses into an fma depends on the code around the call, and the
// kernels that call it have to give the same bits for the same view
__device__ __forceinline__ float blend(float w00, float w01, float w10, float w11, float a, float b, float c, float d) {
#pragma clang fp contract(off)
  return w00 * a + w01 * b + w10 * c + w11 * d;
}

// blend for four values at once (four consecutive classes of a pixel, or one class of four pixels with a weight vector each),
// element by element the same operations in the same order.  Written on the vectors, so that the compiler packs two elements
// into one instruction and not the two products of one element, whose sum would then be an addition across the halves of a
// register pair (tools/check_isa.py)
template <typename W>
__device__ __forceinline__ f32x4 blend4(W w00, W w01, W w10, W w11, f32x4 a, f32x4 b, f32x4 c, f32x4 d) {
#pragma clang fp contract(off)
  return w00 * a + w01 * b + w10 * c + w11 * d;
}

// ---- host ----
// the dynamic LDS, in bytes, of the staged patches of an [hp, wp, n] grid under any tile of an [h, w] output: the bound of
// the footprint, at most `limit`, in whole 16-byte slots
inline int stage_bytes(int hp, int wp, int n, int h, int w, int limit) {
  const long long need = tile::footprint_bound(hp, hp, h, tile::TILE_ROWS, 3) * tile::footprint_bound(wp, wp, w, tile::TILE_COLS, 3) *
                         pt_stride(n) * 4;
  return (int)std::min<long long>(need, std::max(limit, 0)) & ~15;
}

}  // namespace upsample
