// The demo's last step on gfx950 (ifseg_amd/predict.py Segmenter.render_raw; cell 4 of the reference's
// visualize_segmentation_web.ipynb: `cmap[labels]` and `image * (1 - opacity) + cmap[labels] * opacity`): a label map and the
// photograph it was predicted on -> the colour overlay with class contours, uint8 HWC in, uint8 HWC out, one launch.
// `predict.render_reference` is the specification, in integers, and include/ifseg_hip.h states the rule.
//
// A workgroup owns a 16 x 64 tile (tile.h).  Source and destination rows are 3 W bytes and start at any byte alignment, so a
// tile row of 192 bytes neither starts nor ends on a dword and neighbouring workgroups share dwords:
//   phase 0  the tile's image bytes go to LDS with tile.h's aligned dword loads (u8_stage under the identity coordinate), the
//            tile's labels plus a halo of r (tile.h's halo_stage), and the palette as one dword per class;
//   phase 1  lane = x, a wave takes 4 rows: contour test on the staged labels (tile.h's halo_differs), blend, three bytes into
//            the staged output row, which keeps the shift (address modulo 4) of its destination row;
//   phase 2  the staged rows leave as aligned dwords where a dword lies entirely inside the tile's bytes of the row -- such a
//            dword has this workgroup as its only writer -- and as single bytes in front of the first and behind the last one.
// Nothing outside the output's bytes is written, and no dword is written by two workgroups or lanes with partial contents.
// About 7 B per pixel (11 with conf) and no arithmetic to speak of: bandwidth- and launch-bound.
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;

constexpr int MAX_N = 512;
constexpr int ROW_BYTES = 196;                                    // u8_rstride(TILE_COLS): 192 bytes, up to 3 of shift, whole dwords

// source sample = destination sample: the footprint of a tile is the tile
struct SameCoord {
  __device__ __forceinline__ void operator()(int d, int* i0, int* i1, float* l) const { *i0 = d; *i1 = d; *l = 0.f; }
};

// q = clamp(floor(conf * 255 + 0.5), 0, 255) with a rounded product and a rounded sum, NaN -> 0; the pixel's alpha
__device__ __forceinline__ int faded(int alpha, float conf) {
  const float q = fminf(fmaxf(floorf(__fadd_rn(__fmul_rn(conf, 255.f), 0.5f)), 0.f), 255.f);      // fmaxf(NaN, 0) = 0
  return (alpha * (int)q + 127) / 255;
}

template <typename L>
__global__ __launch_bounds__(256) void seg_render_kernel(const L* labels, const unsigned char* image, const unsigned char* palette,
                                                         int n, const float* conf, int H, int W, int alpha, int r, uint32_t edge_rgb,
                                                         unsigned char* out, int tiles_x, int tiles_y) {
  __shared__ uint32_t pal[MAX_N];                                 // r | g << 8 | b << 16
  __shared__ short halo[HALO_H * HALO_W];
  __shared__ __attribute__((aligned(4))) unsigned char src[TILE_ROWS * ROW_BYTES];
  __shared__ __attribute__((aligned(4))) unsigned char dst[TILE_ROWS * ROW_BYTES];
  const Tile t = tile_decode(tiles_x, tiles_y, H, W);
  const long long pix0 = (long long)t.b * H * W;                  // B H W < 2^31; times 3 it is not
  const int rows = t.yend - t.Y0, cols = t.xend - t.X0;

  // phase 0
  for (int c = threadIdx.x; c < n; c += 256)
    pal[c] = (uint32_t)palette[3 * c] | (uint32_t)palette[3 * c + 1] << 8 | (uint32_t)palette[3 * c + 2] << 16;
  halo_stage(labels, pix0, t, H, W, r, halo);
  const SameCoord same;
  const U8Source s = u8_stage(image + pix0 * 3, W, same, t.Y0, t.yend - 1, same, t.X0, t.xend - 1, src, (int)sizeof(src));
  __syncthreads();

  // phase 1
  unsigned char* const out0 = out + (pix0 + (long long)t.Y0 * W + t.X0) * 3;      // the tile's first byte
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ry = t.wave * 4 + j;
    if (ry >= rows || t.lane >= cols) continue;
    const int l = halo_label(halo, ry, t.lane, r);
    const bool edge = halo_differs(halo, ry, t.lane, r, l);
    const unsigned char* p = s.stage + ry * s.rstride + (int)((size_t)(s.row0 + (long long)ry * W * 3) & 3) + t.lane * 3;
    uint32_t v = (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
    if (edge) {
      v = edge_rgb;
    } else if ((unsigned)l < (unsigned)n) {                       // a label outside the palette keeps the image's pixel
      const int a = conf ? faded(alpha, conf[pix0 + (long long)(t.Y0 + ry) * W + t.X0 + t.lane]) : alpha;
      const uint32_t c = pal[l];
      v = (((v & 255) * (256 - a) + (c & 255) * a) >> 8) | ((((v >> 8) & 255) * (256 - a) + ((c >> 8) & 255) * a) >> 8) << 8 |
          (((v >> 16) * (256 - a) + (c >> 16) * a) >> 8) << 16;
    }
    unsigned char* d = dst + ry * ROW_BYTES + (int)((size_t)(out0 + (long long)ry * W * 3) & 3) + t.lane * 3;
    d[0] = (unsigned char)v, d[1] = (unsigned char)(v >> 8), d[2] = (unsigned char)(v >> 16);
  }
  __syncthreads();

  // phase 2: row ry holds its cols * 3 bytes at dst[ry ROW_BYTES + sh ..), sh = its destination address modulo 4
  constexpr int DPR = ROW_BYTES / 4;
  const int nbytes = cols * 3;
  for (int i = threadIdx.x; i < rows * DPR; i += 256) {
    const int ry = i / DPR, k = i - ry * DPR;
    unsigned char* a = out0 + (long long)ry * W * 3;
    const int sh = (int)((size_t)a & 3), lo = 4 * k, end = sh + nbytes;
    if (lo >= end) continue;
    const unsigned char* from = dst + ry * ROW_BYTES + lo;
    if (lo >= sh && lo + 4 <= end) {
      *reinterpret_cast<uint32_t*>(a - sh + lo) = *reinterpret_cast<const uint32_t*>(from);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)                                 // at most three of the four are this row's
        if (lo + e >= sh && lo + e < end) a[lo + e - sh] = from[e];
    }
  }
}

}  // namespace

extern "C" int ifseg_seg_render(const void* labels, int label_bytes, const void* image, const void* palette, int n,
                                const float* conf, int B, int H, int W, int alpha, int boundary, int boundary_rgb, void* out,
                                void* stream) {
  (void)hipGetLastError();
  if (!labels || !image || !palette || !out || (label_bytes != 1 && label_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if ((label_bytes == 2 && ((size_t)labels & 1)) || ((size_t)conf & 3)) return IFSEG_ERR_BAD_ARG;
  if (n < 1 || n > MAX_N || boundary < 0 || boundary > HALO_MAX_R || alpha < 0 || alpha > 256) return IFSEG_ERR_BAD_ARG;
  if (boundary_rgb < 0 || boundary_rgb > 0xffffff) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(H, W, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  if (label_bytes == 1)
    hipLaunchKernelGGL(seg_render_kernel<unsigned char>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)labels, (const unsigned char*)image, (const unsigned char*)palette, n, conf, H, W, alpha,
                       boundary, (uint32_t)boundary_rgb, (unsigned char*)out, tiles_x, tiles_y);
  else
    hipLaunchKernelGGL(seg_render_kernel<short>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const short*)labels,
                       (const unsigned char*)image, (const unsigned char*)palette, n, conf, H, W, alpha, boundary,
                       (uint32_t)boundary_rgb, (unsigned char*)out, tiles_x, tiles_y);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
