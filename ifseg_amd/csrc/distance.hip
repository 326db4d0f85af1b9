// The exact squared Euclidean distance of every pixel of a label map to the nearest pixel of another value, and the trimap
// counters built on it (ifseg_amd/predict.py: distance_reference and trimap_areas_reference are the specifications).
//
// D2(p) = min over the pixels q of p's image with L(q) != L(p) of |p - q|^2 -- with `border`, also over every position
// outside the image -- is separable: with v(x, y) the vertical distance from (x, y) to the nearest pixel of column x that holds
// another value (a property of the pixel's own value, so one plane serves every value at once),
//   D2(x, y) = min over dx of  dx^2                       where (x + dx, y) holds another value (or, with border, lies outside),
//                              dx^2 + v(x + dx, y)^2      where it holds the same value,
// and nothing behind the first other value on a side can win (its dx^2 alone is larger).  Two launches over tile.h's 16 x 64
// tiles (lane = x, a wave takes 4 consecutive rows), integers throughout, no atomics, nothing allocated, nothing read back:
//   seg_distance_cols_kernel  the tile's column segments plus R rows above and below go to LDS as shorts, (16 + 2 R) rows of
//            64, coordinates clamped to the image (a clamped row repeats a value of the same run: it adds no edge, and the
//            first other value a walk meets is always inside the image).  Every wave walks the R + 4 halo rows that end at
//            its own 4 rows downwards, with the length of the run of equal values that ends at the row, and the R + 4 rows
//            below them upwards: 2 (R + 4) LDS reads per thread for its 4 pixels, all four waves alike.  v = min(up, down),
//            clamped to 1 .. R, 255 for "farther than R or none", leaves as a uint8 plane.
//   seg_distance_rows_kernel  the tile's rows of labels (shorts) and of v (bytes) plus R columns left and right go to LDS, each
//            wave its own 4 rows.  A pixel starts at best = v^2 and looks at x - k and x + k for k = 1, 2, ... while
//            k <= R, k^2 < best and a side is open; another value (or the image's edge with border) gives k^2 and closes the
//            side, the same value gives k^2 + v^2.  The work of a pixel is bounded by its own distance, not by the width.
//            best <= R^2 leaves as a uint16, anything else as 65535.
// Lanes read consecutive shorts / bytes of one LDS row: no bank conflict in either kernel.
// Dynamic LDS: (16 + 2 R) 128 bytes for the columns (R = 128: 34 816), 16 (64 + 2 R) 3 for the rows (R = 128: 15 360).
//
// seg_trimap_kernel: count.h's walk over labels, ground truth and the ground truth's distance plane (its third stream, read
// as shorts) into a workgroup-private direct table of K 3 n uint32 (K rings of seg_areas' three rows; 48 KiB at K = 8,
// n = 512): ring k holds r_{k-1}^2 < d2 <= r_k^2.  Only non-zero bins leave, one 64-bit integer atomic each.
// Registers (tools/regs.py, gfx950, -O3): see the README's entry.
#include <climits>
#include "count.h"
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using namespace count;

constexpr int SEG_DISTANCE_MAX = 128;         // 128^2 = 16384 fits the uint16 beside SEG_DISTANCE_FAR
constexpr int SEG_DISTANCE_FAR = 65535;       // farther than R, or no other value at all
constexpr int SEG_TRIMAP_MAX_RADII = 8;
constexpr int SD_MAX_CLASSES = 512;           // the scoring kernels' limit (predict.hip: PT_MAX_CLASSES)
constexpr int SD_NONE = 255;                  // v: farther than R or none; 255^2 > 128^2

inline int sd_cols_lds(int R) { return (TILE_ROWS + 2 * R) * TILE_COLS * 2; }
__host__ __device__ inline int sd_rows_stride(int R) { return TILE_COLS + 2 * R; }
inline int sd_rows_lds(int R) { return TILE_ROWS * sd_rows_stride(R) * 3; }

template <int EB>
__global__ __launch_bounds__(256) void seg_distance_cols_kernel(const void* __restrict__ map, int h, int w, int tiles_x,
                                                                int tiles_y, int R, int border, unsigned char* __restrict__ v) {
  extern __shared__ __attribute__((aligned(16))) short sd_cols[];            // sd_cols_lds(R)
  const Tile t = tile_decode(tiles_x, tiles_y, h, w);
  const long long pix0 = (long long)t.b * h * w;
  const int HH = TILE_ROWS + 2 * R;
  const int xs = min(t.X0 + t.lane, w - 1);
  // halo[hy][lane] = the value at (Y0 - R + hy, X0 + lane), clamped.  A wave takes every fourth row, four of them at a time
  // with their loads in flight together; only the LDS stores look at the halo's bounds
  for (int hy0 = t.wave; hy0 < HH; hy0 += 16) {
    short val[4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
      val[r] = (short)elem_at<EB>(map, pix0 + (long long)min(max(t.Y0 - R + hy0 + 4 * r, 0), h - 1) * w + xs);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (hy0 + 4 * r < HH) sd_cols[(hy0 + 4 * r) * TILE_COLS + t.lane] = val[r];
  }
  __syncthreads();

  // the wave's window: halo rows 4 wave .. 4 wave + 2 R + 3; its pixel j sits at window row R + j
  const short* c = sd_cols + (t.wave * 4) * TILE_COLS + t.lane;
  int up[4], down[4];
  int prev = c[0], run = 1;                     // the equal values that end at window row k
  for (int k = 1; k < R; ++k) {
    const int val = c[k * TILE_COLS];
    run = val == prev ? run + 1 : 1;
    prev = val;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int val = c[(R + j) * TILE_COLS];
    run = val == prev ? run + 1 : 1;
    prev = val;
    up[j] = run;                                // the other value lies `run` rows up, inside the window iff run <= R
  }
  prev = c[(2 * R + 3) * TILE_COLS], run = 1;   // the equal values that begin at window row k
  for (int k = 2 * R + 2; k > R + 3; --k) {
    const int val = c[k * TILE_COLS];
    run = val == prev ? run + 1 : 1;
    prev = val;
  }
#pragma unroll
  for (int j = 3; j >= 0; --j) {
    const int val = c[(R + j) * TILE_COLS];
    run = val == prev ? run + 1 : 1;
    prev = val;
    down[j] = run;
  }
  const int x = t.X0 + t.lane;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = t.Y0 + t.wave * 4 + j;
    int u = up[j] <= R ? up[j] : SD_NONE, d = down[j] <= R ? down[j] : SD_NONE;
    if (border) {
      if (y + 1 <= R) u = min(u, y + 1);
      if (h - y <= R) d = min(d, h - y);
    }
    if (y < t.yend && x < t.xend) v[pix0 + (long long)y * w + x] = (unsigned char)min(u, d);
  }
}

template <int EB>
__global__ __launch_bounds__(256) void seg_distance_rows_kernel(const void* __restrict__ map, const unsigned char* __restrict__ v,
                                                                int h, int w, int tiles_x, int tiles_y, int R, int border,
                                                                unsigned short* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) short sd_rows[];            // sd_rows_lds(R)
  static_assert(TILE_COLS + 2 * SEG_DISTANCE_MAX <= 5 * 64, "five chunks of 64 columns per halo row");
  const Tile t = tile_decode(tiles_x, tiles_y, h, w);
  const long long pix0 = (long long)t.b * h * w;
  const int hs = sd_rows_stride(R);
  short* lab = sd_rows;
  unsigned char* vv = reinterpret_cast<unsigned char*>(sd_rows + TILE_ROWS * hs);
  // a wave stages its own four rows, columns X0 - R .. X0 + 63 + R clamped: a position outside the image is found by
  // arithmetic below, never by its staged value.  A chunk wholly outside the halo row is left out, uniformly
  int xs[5];
#pragma unroll
  for (int q = 0; q < 5; ++q) xs[q] = min(max(t.X0 - R + t.lane + 64 * q, 0), w - 1);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = t.wave * 4 + j;
    const long long at = pix0 + (long long)min(t.Y0 + row, h - 1) * w;
    short lv[5];
    unsigned char sv[5];
#pragma unroll
    for (int q = 0; q < 5; ++q) {
      lv[q] = 64 * q < hs ? (short)elem_at<EB>(map, at + xs[q]) : (short)0;
      sv[q] = 64 * q < hs ? v[at + xs[q]] : (unsigned char)0;
    }
#pragma unroll
    for (int q = 0; q < 5; ++q)
      if (t.lane + 64 * q < hs) {
        lab[row * hs + t.lane + 64 * q] = lv[q];
        vv[row * hs + t.lane + 64 * q] = sv[q];
      }
  }
  __syncthreads();

  const int x = t.X0 + t.lane, R2 = R * R;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int row = t.wave * 4 + j, y = t.Y0 + row;
    const bool live = y < t.yend && x < t.xend;
    const short* lr = lab + row * hs + R + t.lane;
    const unsigned char* vr = vv + row * hs + R + t.lane;
    const int own = lr[0], v0 = vr[0];
    int best = live ? v0 * v0 : 0;
    bool left = true, right = true;
    for (int k = 1; k <= R && k * k < best && (left || right); ++k) {
      const int kk = k * k;
      const bool lin = x - k >= 0, rin = x + k < w;
      const int ll = lr[-k], ls = vr[-k], rl = lr[k], rs = vr[k];
      const int lc = !lin ? (border ? kk : INT_MAX) : ll != own ? kk : kk + ls * ls;
      const int rc = !rin ? (border ? kk : INT_MAX) : rl != own ? kk : kk + rs * rs;
      if (left) best = min(best, lc);
      if (right) best = min(best, rc);
      left = left && lin && ll == own;
      right = right && rin && rl == own;
    }
    if (live) out[pix0 + (long long)y * w + x] = (unsigned short)(best <= R2 ? best : SEG_DISTANCE_FAR);
  }
}

// the squares of the K radii, ascending; INT_MAX behind them
struct Rings {
  int r2[SEG_TRIMAP_MAX_RADII];
};

__host__ __device__ inline int st_dwords(int n, int K) { return (K * 3 * n + 3) & ~3; }

template <int LB, int GB>
__global__ __launch_bounds__(256) void seg_trimap_kernel(const unsigned char* __restrict__ lab, const unsigned char* __restrict__ gt,
                                                         const unsigned char* __restrict__ dist, int head, int groups, int tail,
                                                         int n, int raw, int K, Rings rings, unsigned long long* trimap) {
  extern __shared__ __attribute__((aligned(16))) uint32_t st_tab[];          // st_dwords(n, K)
  table_zero(st_tab, false, K * 3 * n);
  walk_pixels<LB, MapStream<GB>, MapStream<2>>(lab, gt, head, groups, tail, [&](int pred, int g, int d, bool live) {
    const int d2 = d & 0xffff;                  // the stream sign-extends its shorts
    int k = 0;                                  // the radii below the pixel's distance: its ring, K beyond the last one
#pragma unroll
    for (int i = 0; i < SEG_TRIMAP_MAX_RADII; ++i) k += d2 > rings.r2[i] ? 1 : 0;
    const GtClass c = gt_class(n, raw, g, live && k < K);
    const bool pin = c.sc && (unsigned)pred < (unsigned)n;
    const int base = min(k, K - 1) * 3 * n;
    bin_add(st_tab, base + 2 * n + c.cls, c.sc);
    bin_add(st_tab, base + n + pred, pin);
    bin_add(st_tab, base + c.cls, pin && pred == c.cls);
  }, dist);
  table_flush(st_tab, false, K * 3 * n, trimap);
}

// B h w pixels in [1, 2^31)
inline bool sd_shape(int B, int h, int w) {
  return B >= 1 && h >= 1 && w >= 1 && (long long)h * w < (1ll << 31) && (long long)h * w * B < (1ll << 31);
}

}  // namespace

extern "C" int ifseg_seg_distance(const void* labels, int label_bytes, int B, int h, int w, int max_distance, int border,
                                  void* work, void* out, void* stream) {
  (void)hipGetLastError();
  if (!labels || (label_bytes != 1 && label_bytes != 2) || ((size_t)labels & (size_t)(label_bytes - 1))) return IFSEG_ERR_BAD_ARG;
  if (!work || !out || ((size_t)out & 1)) return IFSEG_ERR_BAD_ARG;
  if (max_distance < 1 || max_distance > SEG_DISTANCE_MAX) return IFSEG_ERR_BAD_ARG;
  if (!sd_shape(B, h, w)) return IFSEG_ERR_BAD_SHAPE;
  const long long npix = (long long)B * h * w;
  if (overlaps(labels, npix * label_bytes, work, npix) || overlaps(labels, npix * label_bytes, out, npix * 2) ||
      overlaps(work, npix, out, npix * 2))
    return IFSEG_ERR_BAD_ARG;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(h, w, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const int R = max_distance, edge = border != 0;
  const hipStream_t s = (hipStream_t)stream;
  unsigned char* v = (unsigned char*)work;
  unsigned short* d2 = (unsigned short*)out;
#define IFSEG_DISTANCE(EB)                                                                                                  \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_distance_cols_kernel<EB>), dim3((unsigned)blocks), dim3(256), (size_t)sd_cols_lds(R), s,  \
                     labels, h, w, tiles_x, tiles_y, R, edge, v);                                                            \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_distance_rows_kernel<EB>), dim3((unsigned)blocks), dim3(256), (size_t)sd_rows_lds(R), s,  \
                     labels, (const unsigned char*)v, h, w, tiles_x, tiles_y, R, edge, d2)
  if (label_bytes == 1) { IFSEG_DISTANCE(1); }
  else { IFSEG_DISTANCE(2); }
#undef IFSEG_DISTANCE
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_trimap_areas(const void* labels, int label_bytes, const void* gt, int gt_bytes, const void* dist, int B,
                                      int h, int w, int n, const int* radii, int K, int raw_labels, void* trimap, void* stream) {
  if (!dist || ((size_t)dist & 1) || !radii || K < 1 || K > SEG_TRIMAP_MAX_RADII) return IFSEG_ERR_BAD_ARG;
  Rings rings;
  for (int i = 0; i < SEG_TRIMAP_MAX_RADII; ++i) {
    if (i < K && (radii[i] < 1 || radii[i] > SEG_DISTANCE_MAX || (i && radii[i] <= radii[i - 1]))) return IFSEG_ERR_BAD_ARG;
    rings.r2[i] = i < K ? radii[i] * radii[i] : INT_MAX;
  }
  if (!labels || !gt || !trimap || (label_bytes != 1 && label_bytes != 2) || (gt_bytes != 1 && gt_bytes != 2) || n < 1 ||
      n > SD_MAX_CLASSES)
    return IFSEG_ERR_BAD_ARG;
  if (!sd_shape(B, h, w)) return IFSEG_ERR_BAD_SHAPE;
  const long long npix = (long long)B * h * w, tbytes = 8ll * K * 3 * n;
  if (overlaps(trimap, tbytes, labels, npix * label_bytes) || overlaps(trimap, tbytes, gt, npix * gt_bytes) ||
      overlaps(trimap, tbytes, dist, npix * 2))
    return IFSEG_ERR_BAD_ARG;
  unsigned long long* counts = (unsigned long long*)trimap;
  return walk_launch<true, false>({labels, label_bytes, gt, gt_bytes, nullptr}, counts, counts, n, SD_MAX_CLASSES, npix,
                                  [&](auto LB, auto GB, const WalkSplit& ws) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_trimap_kernel<LB(), GB()>), dim3(ws.blocks), dim3(256),
                       (size_t)st_dwords(n, K) * sizeof(uint32_t), (hipStream_t)stream, (const unsigned char*)labels,
                       (const unsigned char*)gt, (const unsigned char*)dist, ws.head, ws.groups, ws.tail, n, raw_labels != 0, K,
                       rings, counts);
  });
}

extern "C" int ifseg_seg_distance_limit(int which) {
  switch (which) {
    case 0: return SEG_DISTANCE_MAX;
    case 1: return SEG_DISTANCE_FAR;
    case 2: return SEG_TRIMAP_MAX_RADII;
    case 3: return SD_MAX_CLASSES;
    default: return IFSEG_ERR_BAD_ARG;
  }
}
