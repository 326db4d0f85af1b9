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
// A workgroup of 256 threads owns a tile of 16 rows x 64 pixels.  The tile, the coordinate rule, the staging, the pixel loop and
// the stores are tile.h's, shared with trainload.hip; this file wires them together.
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
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;

int g_stage_limit = U8_STAGE_LIMIT;

template <typename T>
__global__ __launch_bounds__(256) void image_load_kernel(const unsigned char* __restrict__ src, int H0, int W0, int oh, int ow,
                                                         int tiles_x, int tiles_y, const float* __restrict__ lut_g, int rev,
                                                         T* __restrict__ out, int stage_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* lut = reinterpret_cast<float*>(smem);

  const auto [b, X0, Y0, xend, yend, lane, wave] = tile_decode(tiles_x, tiles_y, oh, ow);
  const IntCoord cy{H0, oh}, cx{W0, ow};

  for (int i = threadIdx.x; i < 768; i += 256) lut[i] = lut_g[i];
  const U8Source s = u8_stage(src + (long long)b * H0 * W0 * 3, W0, cy, Y0, yend - 1, cx, X0, xend - 1, smem + U8_LUT_BYTES,
                              stage_bytes);
  __syncthreads();

  // phase 1
  const int x = min(X0 + lane, ow - 1);
  int x0, x1;
  float lx;
  cx(x, &x0, &x1, &lx);
  int y0[4], y1[4];
  float ly[4];
  bool ok[4];
  long long erow[4];
  const long long plane = (long long)oh * ow;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yr = Y0 + wave * 4 + j, y = min(yr, oh - 1);
    cy(y, &y0[j], &y1[j], &ly[j]);
    ok[j] = yr < oh && X0 + lane < ow;
    erow[j] = (long long)b * 3 * plane + (long long)y * ow;
  }
  u8_pixels(s, y0, y1, x0, x1, ly, lx, lut, rev != 0, [](int*, int*, int*) {}, out, erow, plane, ok, lane, x, xend);
}

}  // namespace

extern "C" int ifseg_image_load_staging(int max_bytes) { return swap_limit(g_stage_limit, U8_STAGE_LIMIT, max_bytes); }

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
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(oh, ow, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const long long need = footprint_bound(H0, H0, oh, TILE_ROWS, 3) * u8_rstride(footprint_bound(W0, W0, ow, TILE_COLS, 3));
  // a bound beyond the limit: (nearly) every tile reads global memory, and a buffer nobody uses would only cost occupancy
  const int stage = need > g_stage_limit ? 0 : (int)((need + 15) & ~15ll);
  const int lds = U8_LUT_BYTES + stage;
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
