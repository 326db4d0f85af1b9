// Boundary IoU (Cheng et al., CVPR 2021) of a label map against ground truth: the counters of ifseg_seg_areas restricted to the
// pixels within d of a contour (ifseg_amd/predict.py: boundary_areas_reference is the specification).
//
// A pixel is in the band of a map iff its (2 d + 1)^2 window leaves the image or holds another value than its own.  The first
// is arithmetic (y < d, y >= h - d, x < d, x >= w - d); the second is a uniformity test of the window, and separable: the
// window holds one value iff each of its 2 d + 1 row segments holds one value and the segments' centres are equal.
//
// A workgroup of 256 threads owns a tile of 16 rows x 64 pixels of a [B, h, w] map (tile.h's decode and grid) and handles the
// ground truth, then the labels, in the same LDS:
//   phase 0  the tile's values plus d pixels around it go to LDS as shorts, (16 + 2 d) rows of 64 + 2 d, coordinates clamped
//            to the image: a clamped neighbour repeats a value of the same window and adds no edge, and a pixel whose window
//            was clamped is in the band by the arithmetic test anyway.  A row's stride is an ODD number of dwords.
//   phase 1  thread = halo row, walking it left to right with the length of the run of equal values that ends at the position:
//            O(1) per entry instead of the 2 d + 1 reads of a brute-force test.  flag[tile column][halo row] = the run covers
//            the 2 d + 1 values of the segment.  The lanes of a wave read one column of consecutive rows: odd dword stride,
//            32 banks, no conflict; they write consecutive bytes.
//   phase 2  lane = x, a wave takes 4 consecutive rows and walks the 2 d + 4 halo rows under them top to bottom with the length
//            of the run of flagged rows of equal centres: the window of row ry holds one value iff the run that ends at halo
//            row ry + 2 d covers 2 d + 1 rows.  No sentinel value: an int16 label may be any short.  The lanes read
//            consecutive shorts of one halo row, and flag bytes a column stride apart (an odd number of dwords again).
// So a thread makes 2 (64 + 2 d) + 4 (2 d + 4) LDS reads per launch at the most, 500 at d = 17 and 1000 at d = 64, where the
// brute-force form makes (16 + 2 d) (2 d + 1) / 4 + 4 (2 d + 1) per map: 1150 at d = 17, 10300 at d = 64.  Phase 1 keeps only
// 16 + 2 d of the 256 threads busy; it is a tenth of the launch's LDS traffic and was left so.
// Measured (tools/boundary_bench.py, 1024 x 2048, d = 46): staging four rows per step with their loads in flight together took
// the launch from 171 to 136 us; reading phases 1 and 2 eight values ahead of their run counters made it slower (150 us) and
// is not done.
//
// Counting: a workgroup-private direct table of 3 n uint32 (count.h: bin_add, table_zero, table_flush), so only the non-zero
// bins leave, one 64-bit integer atomic each: integer sums, bit-reproducible.  Nothing is allocated, nothing read back.
//
// Dynamic LDS = table + halo + flags, sized by d (n = 150; the table is (3 n + 3 & ~3) * 4 bytes):
//   d =  1    1 808 +  2 376 + 1 280 =   5 464        d = 46    1 808 + 34 128 + 6 912 = 42 848
//   d = 17    1 808 +  9 800 + 3 328 =  14 936        d = 64    1 808 + 55 872 + 9 472 = 67 152  (n = 512: 71 488)
// Above 64 KiB the launcher raises the kernel's dynamic-LDS attribute (once per instantiation); gfx950 has 160 KiB.
// Registers (tools/regs.py, gfx950, -O3): each of the four instantiations seg_boundary_kernel<1|2, 1|2> takes 34 VGPRs, no VGPR
// or SGPR spills, no scratch, occupancy 8 waves per SIMD by registers (LDS bounds it to 160 KiB / the bytes above).
#include "count.h"
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using namespace count;

constexpr int SEG_BOUNDARY_MAX_D = 64;        // 2 % of a 3200-pixel diagonal
constexpr int SB_MAX_CLASSES = 512;           // the scoring kernels' limit (predict.hip: PT_MAX_CLASSES)
// shorts per halo row: at least 64 + 2 d, an odd number of dwords
__host__ __device__ inline int sb_halo_stride(int d) { return ((TILE_COLS / 2 + d) | 1) * 2; }
// bytes per flag column: at least 16 + 2 d, an odd number of dwords
__host__ __device__ inline int sb_flag_stride(int d) { return (((TILE_ROWS + 2 * d + 3) >> 2) | 1) * 4; }
// the table's dwords, in whole 16-byte slots
__host__ __device__ inline int sb_table_dwords(int n) { return (3 * n + 3) & ~3; }
inline int sb_lds_bytes(int n, int d) {
  return sb_table_dwords(n) * 4 + (TILE_ROWS + 2 * d) * sb_halo_stride(d) * 2 + TILE_COLS * sb_flag_stride(d);
}

// phase 0: halo[hy][hx] = the value at (Y0 - d + hy, X0 - d + hx) of the image that starts at pix0, coordinates clamped to
// the image.  A wave takes every fourth row, four of them at a time: a clamped coordinate is a valid one, so the twelve loads
// of a step (4 rows x 3 chunks of 64 columns cover 64 + 2 d <= 192; a chunk wholly outside the row is left out, uniformly) are
// not predicated per lane and are in flight together; only the LDS stores look at the halo's bounds.  The caller's barrier publishes it
template <int EB>
__device__ __forceinline__ void sb_stage(const void* map, long long pix0, const Tile& t, int h, int w, int d, int hs, short* halo) {
  const int HH = TILE_ROWS + 2 * d, HW = TILE_COLS + 2 * d;
  static_assert(TILE_COLS + 2 * SEG_BOUNDARY_MAX_D <= 3 * 64, "three chunks of 64 columns per halo row");
  int xs[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) xs[c] = min(max(t.X0 - d + t.lane + 64 * c, 0), w - 1);
  for (int hy0 = t.wave; hy0 < HH; hy0 += 16) {
    short v[4][3];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long long row = pix0 + (long long)min(max(t.Y0 - d + hy0 + 4 * r, 0), h - 1) * w;
#pragma unroll
      for (int c = 0; c < 3; ++c) v[r][c] = 64 * c < HW ? (short)elem_at<EB>(map, row + xs[c]) : (short)0;    // uniform
    }
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (hy0 + 4 * r < HH && t.lane + 64 * c < HW) halo[(hy0 + 4 * r) * hs + t.lane + 64 * c] = v[r][c];
  }
}

// phase 1: flag[tx][hy] = the 2 d + 1 values halo[hy][tx .. tx + 2 d] are equal.  The caller's barrier publishes it
__device__ __forceinline__ void sb_rows(const short* halo, int hs, int d, unsigned char* flag, int fs) {
  const int HH = TILE_ROWS + 2 * d, HW = TILE_COLS + 2 * d, hy = threadIdx.x;
  if (hy >= HH) return;
  const short* r = halo + hy * hs;
  int prev = r[0], run = 1;                     // the equal values that end at hx
  for (int hx = 1; hx < HW; ++hx) {
    const int v = r[hx];
    run = v == prev ? run + 1 : 1;
    prev = v;
    if (hx >= 2 * d) flag[(hx - 2 * d) * fs + hy] = run > 2 * d;
  }
}

// phase 2 -> bit j: the window of the pixel at row wave * 4 + j, column lane of the tile holds one value; own[j]: that pixel's
__device__ __forceinline__ unsigned sb_cols(const short* halo, int hs, const unsigned char* flag, int fs, int d, const Tile& t,
                                            int (&own)[4]) {
  const short* c = halo + (t.wave * 4) * hs + d + t.lane;           // the centres of the lane's row segments
  const unsigned char* f = flag + t.lane * fs + t.wave * 4;
  int prev = 0, run = 0;                        // the flagged rows of equal centres that end at row k
  unsigned uniform = 0;
  for (int k = 0; k < 2 * d + 4; ++k) {
    const int v = c[k * hs];
    run = f[k] ? (run && v == prev ? run + 1 : 1) : 0;
    prev = v;
    if (k >= 2 * d && run > 2 * d) uniform |= 1u << (k - 2 * d);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) own[j] = c[(j + d) * hs];
  return uniform;
}

template <int LB, int GB>
__global__ __launch_bounds__(256) void seg_boundary_kernel(const void* __restrict__ lab, const void* __restrict__ gt, int h, int w,
                                                           int tiles_x, int tiles_y, int n, int d, int raw,
                                                           unsigned long long* bareas, unsigned char* __restrict__ band) {
  extern __shared__ __attribute__((aligned(16))) uint32_t sb_lds[];          // sb_lds_bytes(n, d)
  const Tile t = tile_decode(tiles_x, tiles_y, h, w);
  const int hs = sb_halo_stride(d), fs = sb_flag_stride(d);
  uint32_t* tab = sb_lds;
  short* halo = reinterpret_cast<short*>(sb_lds + sb_table_dwords(n));
  unsigned char* flag = reinterpret_cast<unsigned char*>(halo + (TILE_ROWS + 2 * d) * hs);
  const long long pix0 = (long long)t.b * h * w;
  table_zero(tab, false, 3 * n);

  int gv[4], pv[4];
  sb_stage<GB>(gt, pix0, t, h, w, d, hs, halo);
  __syncthreads();
  sb_rows(halo, hs, d, flag, fs);
  __syncthreads();
  const unsigned gu = sb_cols(halo, hs, flag, fs, d, t, gv);
  __syncthreads();
  sb_stage<LB>(lab, pix0, t, h, w, d, hs, halo);
  __syncthreads();
  sb_rows(halo, hs, d, flag, fs);
  __syncthreads();
  const unsigned pu = sb_cols(halo, hs, flag, fs, d, t, pv);

  const int x = t.X0 + t.lane;
  const bool xin = x >= d && x < w - d;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = t.Y0 + t.wave * 4 + j;
    const bool live = y < t.yend && x < t.xend, inside = xin && y >= d && y < h - d;
    const bool gb = !(inside && ((gu >> j) & 1u)), pb = !(inside && ((pu >> j) & 1u));
    if (band && live) band[pix0 + (long long)y * w + x] = (unsigned char)((gb ? 1 : 0) | (pb ? 2 : 0));
    const GtClass c = gt_class(n, raw, gv[j], live);
    const bool pin = c.sc && (unsigned)pv[j] < (unsigned)n;
    bin_add(tab, 2 * n + c.cls, c.sc && gb);
    bin_add(tab, n + pv[j], pin && pb);
    bin_add(tab, c.cls, pin && pv[j] == c.cls && gb && pb);
  }
  table_flush(tab, false, 3 * n, bareas);
}

// the launch of one instantiation; above 64 KiB of LDS the kernel's attribute is raised first, once, to the most a launch asks
template <int LB, int GB>
void sb_launch(long long blocks, int lds, hipStream_t stream, const void* labels, const void* gt, int h, int w, int tiles_x,
               int tiles_y, int n, int d, int raw, unsigned long long* bareas, unsigned char* band) {
  static bool raised = false;
  if (lds > 65536 && !raised) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&seg_boundary_kernel<LB, GB>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              sb_lds_bytes(SB_MAX_CLASSES, SEG_BOUNDARY_MAX_D));
    raised = true;
  }
  hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_boundary_kernel<LB, GB>), dim3((unsigned)blocks), dim3(256), (size_t)lds, stream, labels,
                     gt, h, w, tiles_x, tiles_y, n, d, raw, bareas, band);
}

}  // namespace

extern "C" int ifseg_seg_boundary_areas(const void* labels, int label_bytes, const void* gt, int gt_bytes, int B, int h, int w,
                                        int n, int d, int raw_labels, void* bareas, void* band, void* stream) {
  (void)hipGetLastError();
  if (!labels || (label_bytes != 1 && label_bytes != 2) || ((size_t)labels & (size_t)(label_bytes - 1))) return IFSEG_ERR_BAD_ARG;
  if (!gt || (gt_bytes != 1 && gt_bytes != 2) || ((size_t)gt & (size_t)(gt_bytes - 1))) return IFSEG_ERR_BAD_ARG;
  if (!bareas || ((size_t)bareas & 7)) return IFSEG_ERR_BAD_ARG;
  if (n < 1 || n > SB_MAX_CLASSES || d < 1 || d > SEG_BOUNDARY_MAX_D) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || h < 1 || w < 1 || (long long)h * w >= (1ll << 31) || (long long)h * w * B >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(h, w, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const int lds = sb_lds_bytes(n, d), raw = raw_labels != 0;
#define IFSEG_BOUNDARY(LB, GB)                                                                                              \
  sb_launch<LB, GB>(blocks, lds, (hipStream_t)stream, labels, gt, h, w, tiles_x, tiles_y, n, d, raw,                         \
                    (unsigned long long*)bareas, (unsigned char*)band)
  if (label_bytes == 1 && gt_bytes == 1) IFSEG_BOUNDARY(1, 1);
  else if (label_bytes == 1) IFSEG_BOUNDARY(1, 2);
  else if (gt_bytes == 1) IFSEG_BOUNDARY(2, 1);
  else IFSEG_BOUNDARY(2, 2);
#undef IFSEG_BOUNDARY
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_boundary_limit(int which) {
  switch (which) {
    case 0: return SEG_BOUNDARY_MAX_D;
    case 1: return SB_MAX_CLASSES;
    default: return IFSEG_ERR_BAD_ARG;
  }
}
