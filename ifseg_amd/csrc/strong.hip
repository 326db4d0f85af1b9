// The strong augmentation of a mixed batch on the device (ifseg_amd/augment.py, "the strong augmentation", is the
// specification, bit for bit): DACS' strong_transform behind the mix -- colour jitter, then Gaussian blur -- on images
// [B, 3, P, P] (fp32 or bf16) in train_load's layout.  Labels and weight planes are not touched.
//
//   ifseg_strong_draw    records int32 [B, 16] <- splitmix64(seed + (ordinal << 32) + slot), slots 192..199     one launch
//                        One thread per sample.  The 64 x 5 table of 12-bit blur weights is a constant copy of
//                        augment.BLUR_WEIGHTS; ifseg_strong_blur_table hands the host's copy out without touching a device.
//   ifseg_strong_apply   one launch per batch, tile.h's 16 x 64 tile, 256 threads.  A workgroup stages the table and derives
//                        the 3 x 255 midpoints between its levels; loads the (16 + 8) x (64 + 8) halo of its tile, reflected
//                        on the indices; recovers the grey level of every halo pixel (a binary search over the midpoints:
//                        the number of midpoints at or below the value, 0 for a NaN); runs photo.h's chain in registers and
//                        keeps the result as bytes in LDS; writes the horizontal pass of 24 rows as 32-bit sums to LDS; then
//                        the vertical pass, the rounding, the table and coalesced plane stores (bf16: pairs).
//                        LDS: 3 KiB table + 3 KiB midpoints + 5 KiB levels + 18 KiB sums.
//                        A record that is not valid poisons its sample with NaN; nothing is indexed through a record.
// No scratch buffer, no memset, static launch shapes, nothing read back.
// The counter stream, the ordinal check and the overlap test: common.h; words 0..8 of a record, drawn, read back and validated:
// photo.h; the NaN tile: tile.h.
#include "tile.h"
#include "photo.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using namespace photo;

constexpr int SG_MAX_P = 4096;
constexpr int SG_R = 4;                                      // blur radius
constexpr int SG_HW = TILE_COLS + 2 * SG_R, SG_HH = TILE_ROWS + 2 * SG_R;
constexpr int SG_SLOT = 192;
enum { S_PHOTO = 0, S_SIGMA = 9, S_W0, S_ZERO = 15 };         // S_PHOTO: photo.h's nine words

// w0..w4 for sigma = 0.15 + s / 64, s = 0..63: w_i = floor(4096 g_i / Z + 0.5), w_0 = 4096 - 2 sum w_i (augment.BLUR_WEIGHTS)
#define SG_BLUR_TABLE                                                                                   \
  4096, 0, 0, 0, 0, 4096, 0, 0, 0, 0, 4096, 0, 0, 0, 0, 4096, 0, 0, 0, 0,                               \
  4096, 0, 0, 0, 0, 4096, 0, 0, 0, 0, 4094, 1, 0, 0, 0, 4092, 2, 0, 0, 0,                               \
  4086, 5, 0, 0, 0, 4074, 11, 0, 0, 0, 4056, 20, 0, 0, 0, 4032, 32, 0, 0, 0,                            \
  3996, 50, 0, 0, 0, 3952, 72, 0, 0, 0, 3898, 99, 0, 0, 0, 3836, 130, 0, 0, 0,                          \
  3766, 165, 0, 0, 0, 3688, 204, 0, 0, 0, 3606, 245, 0, 0, 0, 3520, 288, 0, 0, 0,                       \
  3434, 331, 0, 0, 0, 3344, 375, 1, 0, 0, 3256, 419, 1, 0, 0, 3172, 461, 1, 0, 0,                       \
  3086, 503, 2, 0, 0, 3004, 543, 3, 0, 0, 2924, 581, 5, 0, 0, 2850, 617, 6, 0, 0,                       \
  2776, 652, 8, 0, 0, 2706, 684, 11, 0, 0, 2638, 715, 14, 0, 0, 2574, 743, 18, 0, 0,                    \
  2514, 769, 22, 0, 0, 2454, 794, 27, 0, 0, 2398, 817, 32, 0, 0, 2346, 837, 38, 0, 0,                   \
  2294, 856, 45, 0, 0, 2244, 874, 52, 0, 0, 2196, 890, 59, 1, 0, 2152, 904, 67, 1, 0,                   \
  2110, 917, 75, 1, 0, 2066, 929, 84, 2, 0, 2028, 939, 93, 2, 0, 1988, 948, 103, 3, 0,                  \
  1950, 957, 113, 3, 0, 1914, 964, 123, 4, 0, 1880, 970, 133, 5, 0, 1848, 975, 143, 6, 0,               \
  1816, 979, 154, 7, 0, 1786, 983, 164, 8, 0, 1754, 986, 175, 10, 0, 1728, 988, 185, 11, 0,             \
  1698, 990, 196, 13, 0, 1670, 991, 207, 15, 0, 1646, 991, 217, 17, 0, 1618, 991, 227, 20, 1,           \
  1592, 991, 238, 22, 1, 1568, 990, 248, 25, 1, 1548, 988, 258, 27, 1, 1526, 987, 267, 30, 1,           \
  1502, 985, 277, 33, 2, 1482, 982, 286, 37, 2, 1462, 980, 295, 40, 2, 1440, 977, 304, 44, 3

const int g_blur_table[320] = {SG_BLUR_TABLE};
__constant__ int c_blur_table[320] = {SG_BLUR_TABLE};

// ------------------------------------------------------------------------------------------------------------- draw
__global__ __launch_bounds__(64) void strong_draw_kernel(int B, unsigned long long seed, unsigned long long first, int jitter_p8,
                                                         int blur_p8, int* __restrict__ records) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const unsigned long long base = stream_base(seed, first, b);
  const int gate = (int)(draw32(base, SG_SLOT) >> 24) < jitter_p8 ? 1 : 0;
  const bool blur = (int)(draw32(base, SG_SLOT + 6) >> 24) < blur_p8;
  const int s = (int)(draw32(base, SG_SLOT + 7) >> 26);
  int* rec = records + (long long)b * 16;
  photo_draw(rec + S_PHOTO, base, SG_SLOT + 1, gate);
  rec[S_SIGMA] = blur ? s : -1;
#pragma unroll
  for (int i = 0; i < 5; ++i) rec[S_W0 + i] = blur ? c_blur_table[5 * s + i] : (i == 0 ? 4096 : 0);
  rec[S_ZERO] = 0;
}

// ------------------------------------------------------------------------------------------------------------- apply
__device__ __forceinline__ float sg_load(const float* p, long long e) { return p[e]; }
__device__ __forceinline__ float sg_load(const bf16_t* p, long long e) { return bf2f(p[e]); }

// r(i) on an axis of P samples, P >= 16 > radius: the border reflected without repeating the edge.  (The clamp changes no
// index the blur needs; it keeps the address inside the plane whatever the caller asks for.)
__device__ __forceinline__ int sg_reflect(int i, int P) {
  i = i < 0 ? -i : (i >= P ? 2 * (P - 1) - i : i);
  return min(max(i, 0), P - 1);
}

// the number of midpoints m[1..255] at or below x; m does not decrease, so the set is a prefix and eight probes find its
// length.  A NaN compares false everywhere: 0
__device__ __forceinline__ int sg_level(float x, const float* m) {
  int q = 0;
#pragma unroll
  for (int step = 128; step > 0; step >>= 1)
    if (x >= m[q + step]) q += step;
  return q;
}

template <typename T>
__global__ __launch_bounds__(256) void strong_apply_kernel(const int* __restrict__ records, const T* __restrict__ images, int P,
                                                           int tiles_x, int tiles_y, const float* __restrict__ lut_g, int rev,
                                                           T* __restrict__ out) {
  __shared__ float lut[3 * 256];
  __shared__ float mid[3 * 256];                              // mid[c][k], k = 1..255: halfway between lut[c][k-1] and lut[c][k]
  __shared__ unsigned char lev[3][SG_HH][SG_HW];              // the jittered grey levels of the halo, per plane
  __shared__ uint32_t hsum[3][SG_HH][TILE_COLS];              // the horizontal pass

  const Tile t = tile_decode(tiles_x, tiles_y, P, P);
  const auto [b, X0, Y0, xend, yend, lane, wave] = t;
  const int tid = threadIdx.x;
  const int* rec = records + (long long)b * 16;
  const long long plane = (long long)P * P, img0 = (long long)b * 3 * plane;
  const int x = min(X0 + lane, P - 1);

  int w[5];
  long long wsum = 0;
  bool bad = false;                                                                // workgroup-uniform
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    w[i] = rec[S_W0 + i];
    bad |= w[i] < 0;
    wsum += (i ? 2ll : 1ll) * w[i];
  }
  bad |= wsum != 4096;
  bad |= !photo_valid(rec + S_PHOTO);
  if (bad) {
    store_nan_tile(out, img0, plane, P, t, x);
    return;
  }
  const Photo ph = photo_read(rec + S_PHOTO);

  for (int i = tid; i < 768; i += 256) lut[i] = lut_g[i];
  __syncthreads();
  // the sum of two floats is exact in double and so is its half: one rounding, to fp32, as the specification's
  for (int i = tid; i < 768; i += 256)
    mid[i] = (i & 255) ? (float)(((double)lut[i - 1] + (double)lut[i]) * 0.5) : 0.f;
  __syncthreads();

  // the halo: rows Y0 - 4 .. Y0 + 19, columns X0 - 4 .. xend + 3; plane c holds colour 2 - c under rev
  const int hw = xend - X0 + 2 * SG_R;
  for (int i = tid; i < SG_HH * hw; i += 256) {
    const int hy = i / hw, hx = i - hy * hw;
    const long long e = img0 + (long long)sg_reflect(Y0 - SG_R + hy, P) * P + sg_reflect(X0 - SG_R + hx, P);
    int q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = sg_level(sg_load(images, e + c * plane), mid + c * 256);
    if (rev) { const int t = q[0]; q[0] = q[2]; q[2] = t; }
    photometric(ph, &q[0], &q[1], &q[2]);
    if (rev) { const int t = q[0]; q[0] = q[2]; q[2] = t; }
#pragma unroll
    for (int c = 0; c < 3; ++c) lev[c][hy][hx] = (unsigned char)q[c];
  }
  __syncthreads();

  // horizontal: hsum[c][hy][lane] = sum_d w|d| lev[c][hy][lane + 4 + d], at most 255 * 4096
  if (X0 + lane < P) {
    for (int hy = wave; hy < SG_HH; hy += 4) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const unsigned char* r = &lev[c][hy][lane];
        uint32_t s = (uint32_t)w[0] * r[SG_R];
#pragma unroll
        for (int d = 1; d <= SG_R; ++d) s += (uint32_t)w[d] * ((uint32_t)r[SG_R - d] + (uint32_t)r[SG_R + d]);
        hsum[c][hy][lane] = s;
      }
    }
  }
  __syncthreads();

  // vertical, the rounding and the table: at most 255 * 2^24 + 2^23, inside 32 bits
  const bool live = X0 + lane < P;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ry = wave * 4 + j, yr = Y0 + ry;
    const bool ok = yr < P && live;
    const long long erow = img0 + (long long)min(yr, P - 1) * P;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t v = 0;
      if (live) {
        v = (uint32_t)w[0] * hsum[c][ry + SG_R][lane];
#pragma unroll
        for (int d = 1; d <= SG_R; ++d) v += (uint32_t)w[d] * (hsum[c][ry + SG_R - d][lane] + hsum[c][ry + SG_R + d][lane]);
      }
      const int q = (int)((v + (1u << 23)) >> 24);
      store_plane(out, erow + c * plane + x, ok, lut[c * 256 + q], lane, x, xend);
    }
  }
}

}  // namespace

extern "C" int ifseg_strong_blur_table(int* out) {
  if (!out) return IFSEG_ERR_BAD_ARG;
  for (int i = 0; i < 320; ++i) out[i] = g_blur_table[i];
  return 0;
}

extern "C" int ifseg_strong_draw(int B, unsigned long long seed, long long first_ordinal, int jitter_p8, int blur_p8,
                                 int* records, void* stream) {
  (void)hipGetLastError();
  if (!records || ((size_t)records & 3)) return IFSEG_ERR_BAD_ARG;
  if (jitter_p8 < 0 || jitter_p8 > 256 || blur_p8 < 0 || blur_p8 > 256) return IFSEG_ERR_BAD_ARG;
  if (B < 1) return IFSEG_ERR_BAD_SHAPE;
  if (!ordinals_ok(first_ordinal, B)) return IFSEG_ERR_BAD_ARG;
  hipLaunchKernelGGL(strong_draw_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, (hipStream_t)stream, B, seed,
                     (unsigned long long)first_ordinal, jitter_p8, blur_p8, records);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_strong_apply(const int* records, const void* images, int B, int P, int elem_bytes, const float* lut,
                                  int reverse_channels, void* out, void* stream) {
  (void)hipGetLastError();
  if (!records || !images || !lut || !out || (elem_bytes != 4 && elem_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if (((size_t)records & 3) || ((size_t)lut & 3) || (((size_t)images | (size_t)out) & 15)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || P < 16 || P % 16 || P > SG_MAX_P) return IFSEG_ERR_BAD_SHAPE;
  const long long n = (long long)B * 3 * P * P;
  if (n >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  // the blur reads neighbours: no in-place form
  if (overlaps(out, n * elem_bytes, images, n * elem_bytes) || overlaps(out, n * elem_bytes, records, (long long)B * 64) ||
      overlaps(out, n * elem_bytes, lut, 3 * 256 * 4))
    return IFSEG_ERR_BAD_ARG;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(P, P, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  if (elem_bytes == 4)
    hipLaunchKernelGGL(strong_apply_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, records,
                       (const float*)images, P, tiles_x, tiles_y, lut, reverse_channels, (float*)out);
  else
    hipLaunchKernelGGL(strong_apply_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, records,
                       (const bf16_t*)images, P, tiles_x, tiles_y, lut, reverse_channels, (bf16_t*)out);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
