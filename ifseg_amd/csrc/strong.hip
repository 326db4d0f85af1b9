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
enum { S_BRIGHT, S_CONTRAST, S_SAT, S_HUE, S_MODE, S_BETA, S_ALPHA_C, S_ALPHA_S, S_DELTA, S_SIGMA, S_W0, S_ZERO = 15 };

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

__device__ __forceinline__ unsigned sg_draw32(unsigned long long base, unsigned slot) { return (unsigned)(splitmix64(base + slot) >> 32); }

// ------------------------------------------------------------------------------------------------------------- draw
__global__ __launch_bounds__(64) void strong_draw_kernel(int B, unsigned long long seed, unsigned long long first, int jitter_p8,
                                                         int blur_p8, int* __restrict__ records) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const unsigned long long base = seed + ((first + (unsigned)b) << 32);
  const int gate = (int)(sg_draw32(base, SG_SLOT) >> 24) < jitter_p8 ? 1 : 0;
  const unsigned bits = sg_draw32(base, SG_SLOT + 1);
  const bool blur = (int)(sg_draw32(base, SG_SLOT + 6) >> 24) < blur_p8;
  const int s = (int)(sg_draw32(base, SG_SLOT + 7) >> 26);
  int* rec = records + (long long)b * 16;
  rec[S_BRIGHT] = gate & (bits >> 1);
  rec[S_MODE] = (bits >> 2) & 1;
  rec[S_CONTRAST] = gate & (bits >> 3);
  rec[S_SAT] = gate & (bits >> 4);
  rec[S_HUE] = gate & (bits >> 5);
  // exact in fp32: integers below 2^24 times a power of two
  rec[S_BETA] = __float_as_int((float)((int)(sg_draw32(base, SG_SLOT + 2) >> 9) - (1 << 22)) * (1.f / 131072.f));
  rec[S_ALPHA_C] = __float_as_int((float)((1 << 22) + (int)(sg_draw32(base, SG_SLOT + 3) >> 9)) * (1.f / 8388608.f));
  rec[S_ALPHA_S] = __float_as_int((float)((1 << 22) + (int)(sg_draw32(base, SG_SLOT + 4) >> 9)) * (1.f / 8388608.f));
  rec[S_DELTA] = (int)__umulhi(sg_draw32(base, SG_SLOT + 5), 36u) - 18;
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

  const auto [b, X0, Y0, xend, yend, lane, wave] = tile_decode(tiles_x, tiles_y, P, P);
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
#pragma unroll
  for (int i = S_BRIGHT; i <= S_MODE; ++i) bad |= (unsigned)rec[i] > 1u;
#pragma unroll
  for (int i = S_BETA; i <= S_ALPHA_S; ++i) bad |= (rec[i] & 0x7f800000) == 0x7f800000;
  if (bad) {
    const float nanv = __int_as_float(0x7fc00000);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int yr = Y0 + wave * 4 + j;
      const bool ok = yr < P && X0 + lane < P;
      const long long erow = img0 + (long long)min(yr, P - 1) * P;
#pragma unroll
      for (int c = 0; c < 3; ++c) store_plane(out, erow + c * plane + x, ok, nanv, lane, x, xend);
    }
    return;
  }
  Photo ph;
  ph.bright = rec[S_BRIGHT]; ph.contrast = rec[S_CONTRAST]; ph.sat = rec[S_SAT]; ph.hue = rec[S_HUE]; ph.mode = rec[S_MODE];
  ph.delta = (rec[S_DELTA] % 180 + 180) % 180;
  ph.beta = __int_as_float(rec[S_BETA]); ph.alpha_c = __int_as_float(rec[S_ALPHA_C]); ph.alpha_s = __int_as_float(rec[S_ALPHA_S]);

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

// [a, a + na) and [b, b + nb) share a byte
bool sg_overlaps(const void* a, long long na, const void* b, long long nb) {
  const size_t x = (size_t)a, y = (size_t)b;
  return x < y + (size_t)nb && y < x + (size_t)na;
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
  if (first_ordinal < 0 || first_ordinal + (long long)B > (1ll << 32)) return IFSEG_ERR_BAD_ARG;
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
  if (sg_overlaps(out, n * elem_bytes, images, n * elem_bytes) || sg_overlaps(out, n * elem_bytes, records, (long long)B * 64) ||
      sg_overlaps(out, n * elem_bytes, lut, 3 * 256 * 4))
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
