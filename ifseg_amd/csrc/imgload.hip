// The reference's evaluation transform on the device (ifseg_amd/predict.py Segmenter.segment_raw): raw uint8 images
// [B, H0, W0, 3] (HWC) -> normalised patch_images [B, 3, oh, ow] (NCHW, fp32 or bf16).  Per output element, in this order:
//   bilinear resize (align_corners=False, no antialiasing) with the source coordinate in INTEGERS,
//       num = max((2 d + 1) in - out, 0),  i0 = min(num / (2 out), in - 1),  i1 = min(i0 + 1, in - 1),
//       l = float(num - i0 2 out) / float(2 out)   (0 when i0 == i1)
//   the flat four-weight rule of predict.hip in fp32,  q = clamp(floor(v + 0.5), 0, 255)  (the reference's resize returns
//   uint8), the normalised value LUT[c_out][q] from a host-built [3, 256] table, channel c_out reading source channel
//   2 - c_out when the caller asks for reversed channels (the reference's two reversals, segmentation_dataset.py:218 and :256,
//   cancel: its network sees RGB, so the callers leave the switch off by default).
//
// A workgroup of 256 threads owns a tile of 16 rows x 64 pixels.
//   phase 0  the table goes to LDS; the source footprint of the tile (rows ylo..yhi, the bytes of pixels xlo..xhi) is staged
//            behind it with ALIGNED dword loads: a source row is 3 W0 bytes and starts at any byte alignment, so every staged
//            row begins at the dword that holds its first byte and keeps its own shift (0..3).  A tile whose footprint does not
//            fit the staging buffer (strong downscaling) skips the copy and reads global memory in the same loop.
//   phase 1  lane = x, wave = 4 consecutive rows: the two source rows and the vertical weight are wave-uniform.  Twelve byte
//            taps per pixel (4 corners x 3 channels); three coalesced stores per row, one per channel plane (256 contiguous
//            bytes per wave in fp32).  bf16: the lane on an even flat index also takes its right neighbour's value and stores
//            one dword; the odd element in front of a row's first pair and the even one behind its last leave as halves.
// All LDS lives in the dynamic region (table first, 3072 bytes, then the staged rows).  No atomics, no scratch buffer, static
// launch shape, nothing read back.
#include <algorithm>
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace {

constexpr int IL_ROWS = 16, IL_COLS = 64;
constexpr int IL_LUT_BYTES = 3 * 256 * 4;
constexpr int IL_STAGE_LIMIT = 65536 - IL_LUT_BYTES;              // 64 KiB of LDS per workgroup in all

int g_stage_limit = IL_STAGE_LIMIT;

// (2 d + 1) in - out and 2 out stay below 2^31: the entry point refuses 2 in out >= 2^31
__device__ __forceinline__ void src_coord(int d, int in, int out, int* i0, int* i1, float* l) {
  const int num = max((2 * d + 1) * in - out, 0), den = 2 * out;
  *i0 = min((int)((unsigned)num / (unsigned)den), in - 1);
  *i1 = min(*i0 + 1, in - 1);
  *l = *i0 == *i1 ? 0.f : (float)(num - *i0 * den) / (float)den;          // IEEE division: the fraction is rounded once
}

// LDS bytes of one staged row of fw pixels: up to 3 bytes of shift in front, whole dwords
__host__ __device__ inline int il_rstride(int fw) { return (fw * 3 + 3 + 3) & ~3; }

__device__ __forceinline__ void store_plane(float* out, long long e, bool ok, float v, int, int, int) {
  if (ok) out[e] = v;
}
// bf16: e = flat element index of the lane's pixel; pairs on even e
__device__ __forceinline__ void store_plane(bf16_t* out, long long e, bool ok, float v, int lane, int x, int xend) {
  const uint32_t h = f2bf(v);
  const uint32_t right = (uint32_t)__shfl_down((int)h, 1);                // every lane takes part
  if (!ok) return;
  if ((e & 1) == 0) {
    if (lane < IL_COLS - 1 && x + 1 < xend) *reinterpret_cast<uint32_t*>(out + e) = h | (right << 16);
    else out[e] = (bf16_t)h;
  } else if (lane == 0) {
    out[e] = (bf16_t)h;                                                   // (any other odd element left with lane - 1)
  }
}

// the thread's four pixels (rows j = 0..3 of its wave, one x), three channels each.  r0[j] / r1[j]: wave-uniform byte offset of
// the upper / lower source row from `base` (its shift included), o0 / o1: per-lane byte offset of the left / right pixel
template <typename T, typename Ptr>
__device__ __forceinline__ void pixel_loop(Ptr base, const long long (&r0)[4], const long long (&r1)[4], int o0, int o1,
                                           const float (&ly)[4], float lx, const float* lut, bool rev, T* out,
                                           const long long (&erow)[4], long long plane, const bool (&ok)[4], int lane, int x,
                                           int xend) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float w00 = (1.f - ly[j]) * (1.f - lx), w01 = (1.f - ly[j]) * lx, w10 = ly[j] * (1.f - lx), w11 = ly[j] * lx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int cs = rev ? 2 - c : c;
      const float a = (float)base[r0[j] + o0 + cs], b = (float)base[r0[j] + o1 + cs];
      const float d = (float)base[r1[j] + o0 + cs], e = (float)base[r1[j] + o1 + cs];
      const float v = w00 * a + w01 * b + w10 * d + w11 * e;
      const int q = (int)fminf(fmaxf(floorf(v + 0.5f), 0.f), 255.f);
      store_plane(out, erow[j] + c * plane + x, ok[j], lut[c * 256 + q], lane, x, xend);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void image_load_kernel(const unsigned char* __restrict__ src, int H0, int W0, int oh, int ow,
                                                         int tiles_x, int tiles_y, const float* __restrict__ lut_g, int rev,
                                                         T* __restrict__ out, int stage_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* lut = reinterpret_cast<float*>(smem);
  unsigned char* stage = smem + IL_LUT_BYTES;

  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const int X0 = tx * IL_COLS, Y0 = ty * IL_ROWS;
  const int xend = min(X0 + IL_COLS, ow), yend = min(Y0 + IL_ROWS, oh);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned char* sb = src + (long long)b * H0 * W0 * 3;

  for (int i = threadIdx.x; i < 768; i += 256) lut[i] = lut_g[i];

  // the tile's footprint: source coordinates are monotone in the destination, so the first and the last pixel bound it
  int ylo, yhi, xlo, xhi, t0;
  float tf;
  src_coord(Y0, H0, oh, &ylo, &t0, &tf);
  src_coord(yend - 1, H0, oh, &t0, &yhi, &tf);
  src_coord(X0, W0, ow, &xlo, &t0, &tf);
  src_coord(xend - 1, W0, ow, &t0, &xhi, &tf);
  const int fh = yhi - ylo + 1, fw = xhi - xlo + 1, rstride = il_rstride(fw);
  const bool staged = (long long)fh * rstride <= (long long)stage_bytes;            // workgroup-uniform
  // footprint row ry starts at row0 + ry 3 W0: its shift is that address modulo 4
  const unsigned char* row0 = sb + ((long long)ylo * W0 + xlo) * 3;
  if (staged) {
    const int dpr = rstride >> 2;
    uint32_t* st32 = reinterpret_cast<uint32_t*>(stage);
    for (int i = threadIdx.x; i < fh * dpr; i += 256) {
      const int ry = i / dpr, k = i - ry * dpr;
      const unsigned char* a = row0 + (long long)ry * W0 * 3;
      const int sh = (int)((size_t)a & 3);
      // the dwords that hold at least one byte of the row's fw pixels: up to 3 bytes in front of the first pixel and behind the
      // last one are read with them, also in front of / behind the caller's buffer (an aligned dword never crosses a page)
      if (4 * k < sh + fw * 3) st32[i] = *reinterpret_cast<const uint32_t*>(a - sh + 4 * k);
    }
  }
  __syncthreads();

  // phase 1
  const int x = min(X0 + lane, ow - 1);
  int x0, x1;
  float lx;
  src_coord(x, W0, ow, &x0, &x1, &lx);
  int y0[4], y1[4];
  float ly[4];
  bool ok[4];
  long long erow[4], r0[4], r1[4];
  const long long plane = (long long)oh * ow;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yr = Y0 + wave * 4 + j, y = min(yr, oh - 1);
    src_coord(y, H0, oh, &y0[j], &y1[j], &ly[j]);
    ok[j] = yr < oh && X0 + lane < ow;
    erow[j] = (long long)b * 3 * plane + (long long)y * ow;
  }
  if (staged) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r0[j] = (y0[j] - ylo) * rstride + (int)((size_t)(row0 + (long long)(y0[j] - ylo) * W0 * 3) & 3);
      r1[j] = (y1[j] - ylo) * rstride + (int)((size_t)(row0 + (long long)(y1[j] - ylo) * W0 * 3) & 3);
    }
    pixel_loop<T>(stage, r0, r1, (x0 - xlo) * 3, (x1 - xlo) * 3, ly, lx, lut, rev != 0, out, erow, plane, ok, lane, x, xend);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) { r0[j] = (long long)y0[j] * W0 * 3; r1[j] = (long long)y1[j] * W0 * 3; }
    pixel_loop<T>(sb, r0, r1, x0 * 3, x1 * 3, ly, lx, lut, rev != 0, out, erow, plane, ok, lane, x, xend);
  }
}

}  // namespace

extern "C" int ifseg_image_load_staging(int max_bytes) {
  const int prev = g_stage_limit;
  g_stage_limit = max_bytes < 0 ? IL_STAGE_LIMIT : (max_bytes < IL_STAGE_LIMIT ? max_bytes : IL_STAGE_LIMIT);
  return prev;
}

extern "C" int ifseg_image_load(const void* images, int B, int H0, int W0, int oh, int ow, const float* lut,
                                int reverse_channels, void* out, int out_bytes, void* stream) {
  (void)hipGetLastError();
  if (!images || !lut || !out || (out_bytes != 4 && out_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if (((size_t)out & 15) || ((size_t)lut & 3)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || H0 < 1 || W0 < 1 || oh < 1 || ow < 1) return IFSEG_ERR_BAD_SHAPE;
  const long long lim = 1ll << 31;
  if ((long long)B * H0 * W0 * 3 >= lim || (long long)B * 3 * oh * ow >= lim) return IFSEG_ERR_BAD_SHAPE;
  // the integer source coordinate: (2 d + 1) in - out < 2 in out
  if (2ll * H0 * oh >= lim || 2ll * W0 * ow >= lim) return IFSEG_ERR_BAD_SHAPE;
  const int tiles_x = (ow + IL_COLS - 1) / IL_COLS, tiles_y = (oh + IL_ROWS - 1) / IL_ROWS;
  const long long blocks = (long long)tiles_x * tiles_y * B;
  if (blocks >= lim) return IFSEG_ERR_BAD_SHAPE;
  // an upper bound of any tile's footprint: R destination samples span at most floor((R - 1) in/out) + 1 source samples, + 1 for
  // the lower / right neighbour, + 1 for the rounding of the coordinate
  const long long fh = std::min<long long>(H0, (long long)IL_ROWS * H0 / oh + 3), fw = std::min<long long>(W0, (long long)IL_COLS * W0 / ow + 3);
  const long long need = fh * ((fw * 3 + 6) & ~3ll);
  // a bound beyond the limit: (nearly) every tile reads global memory, and a buffer nobody uses would only cost occupancy
  const int stage = need > g_stage_limit ? 0 : (int)((need + 15) & ~15ll);
  const int lds = IL_LUT_BYTES + stage;
  const unsigned char* src = (const unsigned char*)images;
  if (out_bytes == 4)
    hipLaunchKernelGGL(image_load_kernel<float>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, src, H0, W0, oh, ow,
                       tiles_x, tiles_y, lut, reverse_channels, (float*)out, stage);
  else
    hipLaunchKernelGGL(image_load_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, src, H0, W0, oh, ow,
                       tiles_x, tiles_y, lut, reverse_channels, (bf16_t*)out, stage);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
