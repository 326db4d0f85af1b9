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
// ifseg_image_load_windows (sliding-window inference) is the same tile body on another destination: the windows of the
// [oh, ow] plane as a batch [B Nw, 3, ch, cw], each pixel by the plane's coordinate rule at the window's offset.
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;

int g_stage_limit = U8_STAGE_LIMIT;

// one tile of a [dh, dw] destination plane whose first element is out[ebase]: cy / cx map its rows / columns to the source.
// MIRROR: cx runs DOWN the source columns, so the tile's last column bounds its footprint from below
template <typename T, bool MIRROR = false, typename Coord>
__device__ __forceinline__ void load_tile(const unsigned char* sb, int W0, const Coord& cy, const Coord& cx, const Tile& t, int dh,
                                          int dw, long long ebase, const float* __restrict__ lut_g, int rev, T* __restrict__ out,
                                          int stage_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* lut = reinterpret_cast<float*>(smem);
  const auto [b, X0, Y0, xend, yend, lane, wave] = t;

  for (int i = threadIdx.x; i < 768; i += 256) lut[i] = lut_g[i];
  const U8Source s = u8_stage(sb, W0, cy, Y0, yend - 1, cx, MIRROR ? xend - 1 : X0, MIRROR ? X0 : xend - 1,
                              smem + U8_LUT_BYTES, stage_bytes);
  __syncthreads();

  // phase 1
  const int x = min(X0 + lane, dw - 1);
  int x0, x1;
  float lx;
  cx(x, &x0, &x1, &lx);
  int y0[4], y1[4];
  float ly[4];
  bool ok[4];
  long long erow[4];
  const long long plane = (long long)dh * dw;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yr = Y0 + wave * 4 + j, y = min(yr, dh - 1);
    cy(y, &y0[j], &y1[j], &ly[j]);
    ok[j] = yr < dh && X0 + lane < dw;
    erow[j] = ebase + (long long)y * dw;
  }
  u8_pixels(s, y0, y1, x0, x1, ly, lx, lut, rev != 0, [](int*, int*, int*) {}, out, erow, plane, ok, lane, x, xend);
}

template <typename T>
__global__ __launch_bounds__(256) void image_load_kernel(const unsigned char* __restrict__ src, int H0, int W0, int oh, int ow,
                                                         int tiles_x, int tiles_y, const float* __restrict__ lut_g, int rev,
                                                         T* __restrict__ out, int stage_bytes) {
  const Tile t = tile_decode(tiles_x, tiles_y, oh, ow);
  load_tile(src + (long long)t.b * H0 * W0 * 3, W0, IntCoord{H0, oh}, IntCoord{W0, ow}, t, oh, ow, (long long)t.b * 3 * oh * ow,
            lut_g, rev, out, stage_bytes);
}

// ---- the windows of sliding-window inference, written directly ----
// Element (b Nw + k, c, y, x) of the output is element (b, c, ys[k] + y, xs[k] + x) of image_load's [B, 3, oh, ow]: the
// integer rule of the whole plane at the window's offset, so the bits are image_load's and no [B, 3, oh, ow] image is written
struct WinCoord {
  IntCoord c;
  int off;
  __device__ __forceinline__ void operator()(int d, int* i0, int* i1, float* l) const { c(d + off, i0, i1, l); }
};
// the windows of the MIRRORED plane: column d of a window at offset off is column ow - 1 - off - d of the plane (dir = -1);
// the rows are WinCoord's (dir = 1): one type for both axes, as u8_stage takes them
struct MirrorCoord {
  IntCoord c;
  int off, dir;
  __device__ __forceinline__ void operator()(int d, int* i0, int* i1, float* l) const { c(off + dir * d, i0, i1, l); }
};

template <typename T, bool MIRROR>
__global__ __launch_bounds__(256) void image_load_windows_kernel(const unsigned char* __restrict__ src, int H0, int W0, SlideAxis ay,
                                                                 SlideAxis ax, int tiles_x, int tiles_y,
                                                                 const float* __restrict__ lut_g, int rev, T* __restrict__ out,
                                                                 int stage_bytes) {
  const Tile t = tile_decode(tiles_x, tiles_y, ay.e, ax.e);       // t.b: the window's index in the batch, b Nw + iy gx + ix
  const int nw = ay.g * ax.g, b = t.b / nw, k = t.b - b * nw, iy = k / ax.g, ix = k - iy * ax.g;
  if constexpr (MIRROR)
    load_tile<T, true>(src + (long long)b * H0 * W0 * 3, W0, MirrorCoord{{H0, ay.o}, ay.start(iy), 1},
                       MirrorCoord{{W0, ax.o}, ax.o - 1 - ax.start(ix), -1}, t, ay.e, ax.e, (long long)t.b * 3 * ay.e * ax.e, lut_g, rev,
                       out, stage_bytes);
  else
    load_tile(src + (long long)b * H0 * W0 * 3, W0, WinCoord{{H0, ay.o}, ay.start(iy)}, WinCoord{{W0, ax.o}, ax.start(ix)}, t, ay.e,
              ax.e, (long long)t.b * 3 * ay.e * ax.e, lut_g, rev, out, stage_bytes);
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

namespace {

// ifseg_image_load_windows and ifseg_image_load_windows_mirrored
template <bool MIRROR>
int launch_load_windows(const void* images, int B, int H0, int W0, int oh, int ow, int crop_h, int crop_w, int stride_h,
                        int stride_w, const float* lut, int reverse_channels, void* out, int out_bytes, void* stream) {
  (void)hipGetLastError();
  if (!images || !lut || !out || (out_bytes != 4 && out_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if (((size_t)out & 15) || ((size_t)lut & 3)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || H0 < 1 || W0 < 1) return IFSEG_ERR_BAD_SHAPE;
  SlideAxis ay, ax;
  if (!slide_axis(oh, crop_h, stride_h, &ay) || !slide_axis(ow, crop_w, stride_w, &ax)) return IFSEG_ERR_BAD_SHAPE;
  if ((long long)ay.g * ax.g > IFSEG_SLIDE_MAX_WINDOWS) return IFSEG_ERR_BAD_SHAPE;
  const long long lim = 1ll << 31, nb = (long long)B * ay.g * ax.g;
  if ((long long)B * H0 * W0 * 3 >= lim || nb * 3 * ay.e * ax.e >= lim) return IFSEG_ERR_BAD_SHAPE;
  if (2ll * H0 * oh >= lim || 2ll * W0 * ow >= lim) return IFSEG_ERR_BAD_SHAPE;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(ay.e, ax.e, (int)nb, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  // a window's tile is 16 x 64 neighbouring pixels of the [oh, ow] plane: ifseg_image_load's bound and staging decision
  const long long need = footprint_bound(H0, H0, oh, TILE_ROWS, 3) * u8_rstride(footprint_bound(W0, W0, ow, TILE_COLS, 3));
  const int stage = need > g_stage_limit ? 0 : (int)((need + 15) & ~15ll);
  const int lds = U8_LUT_BYTES + stage;
  const unsigned char* src = (const unsigned char*)images;
  if (out_bytes == 4)
    hipLaunchKernelGGL(HIP_KERNEL_NAME(image_load_windows_kernel<float, MIRROR>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, src, H0, W0,
                       ay, ax, tiles_x, tiles_y, lut, reverse_channels, (float*)out, stage);
  else
    hipLaunchKernelGGL(HIP_KERNEL_NAME(image_load_windows_kernel<bf16_t, MIRROR>), dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, src, H0, W0,
                       ay, ax, tiles_x, tiles_y, lut, reverse_channels, (bf16_t*)out, stage);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int ifseg_image_load_windows(const void* images, int B, int H0, int W0, int oh, int ow, int crop_h, int crop_w,
                                        int stride_h, int stride_w, const float* lut, int reverse_channels, void* out,
                                        int out_bytes, void* stream) {
  return launch_load_windows<false>(images, B, H0, W0, oh, ow, crop_h, crop_w, stride_h, stride_w, lut, reverse_channels, out,
                                    out_bytes, stream);
}

extern "C" int ifseg_image_load_windows_mirrored(const void* images, int B, int H0, int W0, int oh, int ow, int crop_h, int crop_w,
                                                 int stride_h, int stride_w, const float* lut, int reverse_channels, void* out,
                                                 int out_bytes, void* stream) {
  return launch_load_windows<true>(images, B, H0, W0, oh, ow, crop_h, crop_w, stride_h, stride_w, lut, reverse_channels, out,
                                   out_bytes, stream);
}
