// Connected regions of a label map on gfx950 (ifseg_amd/predict.py: regions_reference / region_drop_reference are the
// specifications; include/ifseg_hip.h states the rule): which pixels belong together, each region named by the smallest flat
// index y W + x of its pixels inside its image, with its pixel count -- and, on top, the filter that drops the regions below
// min_region pixels from a pseudo-label map (Segmenter.pseudo_label_raw(min_region=)).
//
// A block-based union-find on tile.h's 16 x 64 tile, four kernels, no workgroup ever waits for another:
//   regions_tile_kernel     one workgroup per tile (tile_decode: lane = x, a wave takes 4 rows).  The labels go to LDS as shorts; a
//                           row's runs of equal values come from one ballot (a pixel's parent starts as its run's first pixel),
//                           the vertical edges -- and the two upper diagonals at connectivity 8 -- are united in LDS, the
//                           parents flattened.  root[p] = the local root as a flat image index: raster order inside a tile is
//                           monotone in the flat index, so the local minimum is the global minimum within the tile.
//                           count[p] = the pixels of the local region at its root's pixel, 0 elsewhere (count.h's bin_add).
//   regions_seam_kernel     a thread per pixel of a tile's first row and first column unites it with its equal-valued
//                           neighbours across the seam (the diagonal ones and the corner's at connectivity 8): find both roots,
//                           atomicMin the larger root's parent with the smaller, continue from what the atomic returned; roots
//                           that agree issue no atomic.  EVERY access to the root plane here is an agent-scope atomic (the XCDs'
//                           L2s are not coherent with each other and a CU's L1 is never refreshed by another CU's stores: a
//                           plain re-read of a parent can be stale, and a union-find that reads stale parents drops merges).
//                           The tile pass's plain stores reach it through the kernel boundary.
//   regions_flatten_kernel  reads the merged plane, which nobody writes any more, and writes the end of every pixel's chain to
//                           ANOTHER plane; a tile-local root that is not its region's root adds its count to the root's with
//                           one 32-bit integer atomic: one per tile-local region, not per pixel.
//   regions_gather_kernel   size[p] = count[root[p]]; with a min_region, the drop rule in the same launch: the filtered uint8
//                           map, the zeroed weights, and dropped[class] through a workgroup-private table (bin_add), flushed
//                           with 64-bit integer atomics as the other counters are.
// Edges that other edges imply are not united: a vertical edge at x whose left neighbours (x - 1 in both rows) carry the value
// too follows from the edge at x - 1 and the two rows' runs; a diagonal follows where the vertical or the horizontal
// neighbour on its side carries the value.  Horizontal edges across a seam are never skipped (skipping both kinds around a
// corner where four tiles meet would leave nothing to follow from).  tests/test_regions_cpu.py runs a transcription of this
// edge set, with the seam edges in shuffled orders, against the specification.
//
// Every chase and every union ends because root[q] <= q holds from the first store on: each step strictly lowers an index.
// As a guard, every loop also carries a budget of steps (a chase: the image's pixel count + 1; a union: twice that, both of its
// indices only fall); past it the thread sets the flag word and leaves, it never spins.  The results are canonical (minimum
// index, exact counts), so two runs give equal bits although the atomics run in any order.  Nothing synchronises with the
// host, nothing is allocated here.
// Registers (tools/regs.py regions.hip, gfx950, -O3): the tile and seam kernels 20 VGPRs each (both label types), the flatten 14,
// the gather 18 and 27 with the drop; no VGPR or SGPR spills, no scratch, occupancy 8 waves per SIMD by registers.  Static LDS:
// 10 KiB in the tile kernel (2 KiB of labels, 4 KiB of parents, 4 KiB of counts), 1 KiB in the gather with the drop.
#include "count.h"
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using count::bin_add;

constexpr int TILE_PIX = TILE_ROWS * TILE_COLS;
constexpr int RG_MAX_CLASSES = 255;             // the classes of the drop's counter: values of a uint8 map
constexpr int RG_GATHER_MAX_BLOCKS = 2048;

#define RG_RLX_WG __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP
#define RG_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// ---- the tile pass: union-find over a tile's 1024 pixels in LDS ----
__device__ __forceinline__ int lds_find(int* par, int a, int* flag) {
  for (int it = 0; it <= TILE_PIX; ++it) {
    const int p = __hip_atomic_load(&par[a], RG_RLX_WG);
    if (p == a) return a;
    a = p;
  }
  atomicOr(flag, 1);
  return a;
}

__device__ __forceinline__ void lds_union(int* par, int a, int b, int* flag) {
  a = lds_find(par, a, flag);
  b = lds_find(par, b, flag);
  for (int it = 0; a != b; ++it) {
    if (it > TILE_PIX) { atomicOr(flag, 1); return; }
    if (a < b) { const int t = a; a = b; b = t; }               // a > b: a's parent takes b
    const int old = __hip_atomic_fetch_min(&par[a], b, RG_RLX_WG);
    if (old == a) return;                                       // a was a root and is linked now
    a = lds_find(par, old, flag);                               // a had a parent: what it pointed to joins b instead
    b = lds_find(par, b, flag);
  }
}

template <typename L>
__global__ __launch_bounds__(256) void regions_tile_kernel(const L* __restrict__ labels, int H, int W, int conn8, int tiles_x,
                                                           int tiles_y, int* root, int* count, int* flag) {
  __shared__ short lab[TILE_PIX];
  __shared__ int par[TILE_PIX];
  __shared__ uint32_t cnt[TILE_PIX];
  const Tile t = tile_decode(tiles_x, tiles_y, H, W);
  const long long pix0 = (long long)t.b * H * W;                  // B H W < 2^31
  const int rows = t.yend - t.Y0, cols = t.xend - t.X0, lane = t.lane;

  // phase 0: the labels, and every pixel's parent = the first pixel of its row's run of equal values
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ry = t.wave * 4 + j, li = ry * TILE_COLS + lane;
    const bool ok = ry < rows && lane < cols;
    const int l = ok ? (int)(short)labels[pix0 + (long long)(t.Y0 + ry) * W + t.X0 + lane] : 0;
    const int left = __shfl_up(l, 1);                             // every lane takes part
    const unsigned long long brk = __ballot(!ok || lane == 0 || left != l);      // lane 0 is always set
    const int start = 63 - __clzll((long long)(brk & (~0ull >> (63 - lane))));
    lab[li] = (short)l;
    par[li] = ok ? ry * TILE_COLS + start : li;
    cnt[li] = 0u;
  }
  __syncthreads();

  // phase 1: the edges to the row above that nothing else implies
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ry = t.wave * 4 + j, li = ry * TILE_COLS + lane;
    if (ry < 1 || ry >= rows || lane >= cols) continue;
    const int l = lab[li], up = lab[li - TILE_COLS];
    const bool hasl = lane > 0, hasr = lane + 1 < cols;
    const int lf = hasl ? lab[li - 1] : 0, ul = hasl ? lab[li - TILE_COLS - 1] : 0;
    if (up == l) {
      if (!(hasl && lf == l && ul == l)) lds_union(par, li, li - TILE_COLS, flag);
    } else if (conn8) {
      if (hasl && ul == l && lf != l) lds_union(par, li, li - TILE_COLS - 1, flag);
      if (hasr && lab[li - TILE_COLS + 1] == l && lab[li + 1] != l) lds_union(par, li, li - TILE_COLS + 1, flag);
    }
  }
  __syncthreads();

  // phase 2: the local roots (the parents only fall, and no one writes them any more), counted per region
  int r[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ry = t.wave * 4 + j, li = ry * TILE_COLS + lane;
    const bool ok = ry < rows && lane < cols;
    r[j] = ok ? lds_find(par, li, flag) : li;
    bin_add(cnt, r[j], ok);                                       // whole waves
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ry = t.wave * 4 + j, li = ry * TILE_COLS + lane;
    if (ry >= rows || lane >= cols) continue;
    const long long p = pix0 + (long long)(t.Y0 + ry) * W + t.X0 + lane;
    root[p] = (t.Y0 + (r[j] >> 6)) * W + t.X0 + (r[j] & 63);
    count[p] = r[j] == li ? (int)cnt[li] : 0;
  }
}

// ---- the seam pass: every access to the root plane is an agent-scope atomic ----
// the root of a's chain in the image that starts at `img`; steps: what is left of the caller's budget
__device__ __forceinline__ int seam_find(int* img, int a, unsigned& steps, int* flag) {
  for (;;) {
    const int p = __hip_atomic_load(&img[a], RG_RLX_AGENT);
    if (p == a) return a;
    if (steps == 0u) { atomicOr(flag, 1); return a; }
    --steps;
    a = p;
  }
}

__device__ __forceinline__ void seam_union(int* img, int a, int b, unsigned budget, int* flag) {
  unsigned steps = budget;
  a = seam_find(img, a, steps, flag);
  b = seam_find(img, b, steps, flag);
  while (a != b) {
    if (steps == 0u) { atomicOr(flag, 1); return; }
    --steps;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(&img[a], b, RG_RLX_AGENT);
    if (old == a) return;
    a = seam_find(img, old, steps, flag);
    b = seam_find(img, b, steps, flag);
  }
}

// 128 threads per tile: 0..63 the first row's pixels, 64..79 the first column's
template <typename L>
__global__ __launch_bounds__(128) void regions_seam_kernel(const L* __restrict__ labels, int H, int W, int conn8, int tiles_x,
                                                           int tiles_y, int* root, unsigned budget, int* flag) {
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const int X0 = tx * TILE_COLS, Y0 = ty * TILE_ROWS;
  const long long pix0 = (long long)b * H * W;
  const L* lb = labels + pix0;
  int* img = root + pix0;
  const int k = threadIdx.x;
  auto at = [&](int y, int x) { return (int)(short)lb[(long long)y * W + x]; };
  if (k < TILE_COLS) {
    const int x = X0 + k, y = Y0;
    if (y < 1 || x >= W) return;
    const int l = at(y, x), up = at(y - 1, x);
    const bool hasl = x > 0, hasr = x + 1 < W;
    const int lf = hasl ? at(y, x - 1) : 0, ul = hasl ? at(y - 1, x - 1) : 0;
    const int p = y * W + x;
    if (up == l) {
      if (!(hasl && lf == l && ul == l)) seam_union(img, p, p - W, budget, flag);
    } else if (conn8) {
      if (hasl && ul == l && lf != l) seam_union(img, p, p - W - 1, budget, flag);
      if (hasr && at(y - 1, x + 1) == l && at(y, x + 1) != l) seam_union(img, p, p - W + 1, budget, flag);
    }
  } else if (k < TILE_COLS + TILE_ROWS) {
    const int x = X0, y = Y0 + (k - TILE_COLS);
    if (x < 1 || y >= H) return;
    const int l = at(y, x), lf = at(y, x - 1);
    const int p = y * W + x;
    if (lf == l) {
      seam_union(img, p, p - 1, budget, flag);
    } else if (conn8) {
      // the upper-left neighbour of the tile's first pixel went with the first row; the lower-left one of its last row goes
      // with the first row of the tile below
      if (y > Y0 && at(y - 1, x - 1) == l && at(y - 1, x) != l) seam_union(img, p, p - W - 1, budget, flag);
      if (y + 1 < min(Y0 + TILE_ROWS, H) && at(y + 1, x - 1) == l && at(y + 1, x) != l) seam_union(img, p, p + W - 1, budget, flag);
    }
  }
}

// ---- the flatten pass: merged -> root_out, the tile-local counts summed at the regions' roots ----
__global__ __launch_bounds__(256) void regions_flatten_kernel(const int* merged, int HW, long long npix, int* root_out, int* count,
                                                              int* flag) {
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p >= npix) return;
  const long long pix0 = p / HW * HW;
  const int* img = merged + pix0;
  const int self = (int)(p - pix0);
  int a = self;
  for (int it = 0;; ++it) {
    const int q = img[a];
    if (q == a) break;
    if (it >= HW) { atomicOr(flag, 1); break; }
    a = q;
  }
  root_out[p] = a;
  if (a != self) {
    const int c = count[p];       // a tile-local root that is not its region's: nobody adds to this word
    if (c > 0) atomicAdd(&count[pix0 + a], c);
  }
}

// ---- the gather pass, with the drop ----
// DROP: labels are uint8; out / weight / dropped as ifseg_seg_region_drop states them
template <bool DROP>
__global__ __launch_bounds__(256) void regions_gather_kernel(const int* __restrict__ root, const int* __restrict__ count, int HW,
                                                             long long npix, int* __restrict__ size,
                                                             const unsigned char* __restrict__ labels, int min_region, int fill,
                                                             int n, int raw, unsigned char* __restrict__ out,
                                                             unsigned char* weight, unsigned long long* dropped) {
  __shared__ uint32_t dtab[DROP ? RG_MAX_CLASSES + 1 : 1];
  if (DROP) {
    for (int c = threadIdx.x; c < n; c += 256) dtab[c] = 0u;
    __syncthreads();
  }
  // whole waves walk: the bound is the wave's first pixel
  for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); base < npix; base += (long long)gridDim.x * 256) {
    const long long p = base + (threadIdx.x & 63);
    const bool ok = p < npix;
    int cls = 0;
    bool cnt = false;
    if (ok) {
      const int s = count[p / HW * HW + root[p]];
      size[p] = s;
      if (DROP) {
        const int v = labels[p];
        const bool drop = v != fill && s < min_region;
        out[p] = drop ? (unsigned char)fill : (unsigned char)v;
        if (drop && weight) weight[p] = 0;
        cls = v - raw;
        cnt = drop && (unsigned)cls < (unsigned)n;
      }
    }
    if (DROP) bin_add(dtab, cnt ? cls : 0, cnt);
  }
  if (DROP) {
    __syncthreads();
    for (int c = threadIdx.x; c < n; c += 256) {
      const uint32_t v = dtab[c];
      if (v) atomicAdd(&dropped[c], (unsigned long long)v);
    }
  }
}

struct DropArgs {
  int min_region, fill, n, raw;
  unsigned char* out;
  unsigned char* weight;
  unsigned long long* dropped;
};

int regions_launch(const void* labels, int label_bytes, int B, int H, int W, int connectivity, int* work, int* count, int* root,
                   int* size, int* flag, const DropArgs* drop, void* stream) {
  (void)hipGetLastError();
  if (!labels || !work || !count || !root || !size || !flag || (label_bytes != 1 && label_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if ((label_bytes == 2 && ((size_t)labels & 1)) || (((size_t)work | (size_t)count | (size_t)root | (size_t)size | (size_t)flag) & 3))
    return IFSEG_ERR_BAD_ARG;
  if (connectivity != 4 && connectivity != 8) return IFSEG_ERR_BAD_ARG;
  if (drop) {
    if (label_bytes != 1 || !drop->out || !drop->dropped || ((size_t)drop->dropped & 7)) return IFSEG_ERR_BAD_ARG;
    if (drop->min_region < 1 || drop->fill < 0 || drop->fill > 255 || drop->n < 1 || drop->n > RG_MAX_CLASSES) return IFSEG_ERR_BAD_ARG;
  }
  if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  const long long npix = (long long)B * H * W;
  const int* planes[4] = {work, count, root, size};
  for (int i = 0; i < 4; ++i) {
    for (int j = i + 1; j < 4; ++j)
      if (overlaps(planes[i], npix * 4, planes[j], npix * 4)) return IFSEG_ERR_BAD_ARG;
    if (overlaps(planes[i], npix * 4, labels, npix * label_bytes) || overlaps(planes[i], npix * 4, flag, 4)) return IFSEG_ERR_BAD_ARG;
    if (drop && (overlaps(planes[i], npix * 4, drop->out, npix) || overlaps(planes[i], npix * 4, drop->weight, npix) ||
                 overlaps(planes[i], npix * 4, drop->dropped, 8ll * drop->n)))
      return IFSEG_ERR_BAD_ARG;
  }
  if (drop && (overlaps(drop->out, npix, labels, npix) || overlaps(drop->out, npix, drop->weight, npix) ||
               overlaps(drop->weight, npix, labels, npix)))
    return IFSEG_ERR_BAD_ARG;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(H, W, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const hipStream_t s = (hipStream_t)stream;
  const int conn8 = connectivity == 8 ? 1 : 0, HW = H * W;
  const unsigned budget = 2u * (unsigned)HW + 1u;                 // H W < 2^31: below 2^32
  if (label_bytes == 1) {
    hipLaunchKernelGGL(regions_tile_kernel<unsigned char>, dim3((unsigned)blocks), dim3(256), 0, s, (const unsigned char*)labels,
                       H, W, conn8, tiles_x, tiles_y, work, count, flag);
    if (blocks > B)
      hipLaunchKernelGGL(regions_seam_kernel<unsigned char>, dim3((unsigned)blocks), dim3(128), 0, s,
                         (const unsigned char*)labels, H, W, conn8, tiles_x, tiles_y, work, budget, flag);
  } else {
    hipLaunchKernelGGL(regions_tile_kernel<short>, dim3((unsigned)blocks), dim3(256), 0, s, (const short*)labels, H, W, conn8,
                       tiles_x, tiles_y, work, count, flag);
    if (blocks > B)
      hipLaunchKernelGGL(regions_seam_kernel<short>, dim3((unsigned)blocks), dim3(128), 0, s, (const short*)labels, H, W, conn8,
                         tiles_x, tiles_y, work, budget, flag);
  }
  const long long fblocks = (npix + 255) / 256;                   // < 2^23
  hipLaunchKernelGGL(regions_flatten_kernel, dim3((unsigned)fblocks), dim3(256), 0, s, work, HW, npix, root, count, flag);
  const unsigned gblocks = (unsigned)std::min<long long>(fblocks, RG_GATHER_MAX_BLOCKS);
  if (drop)
    hipLaunchKernelGGL(regions_gather_kernel<true>, dim3(gblocks), dim3(256), 0, s, root, count, HW, npix, size,
                       (const unsigned char*)labels, drop->min_region, drop->fill, drop->n, drop->raw, drop->out, drop->weight,
                       drop->dropped);
  else
    hipLaunchKernelGGL(regions_gather_kernel<false>, dim3(gblocks), dim3(256), 0, s, root, count, HW, npix, size, nullptr, 0, 0, 0,
                       0, nullptr, nullptr, nullptr);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int ifseg_seg_regions(const void* labels, int label_bytes, int B, int H, int W, int connectivity, int* work, int* count,
                                 int* root, int* size, int* flag, void* stream) {
  return regions_launch(labels, label_bytes, B, H, W, connectivity, work, count, root, size, flag, nullptr, stream);
}

extern "C" int ifseg_seg_region_drop(const void* labels, int B, int H, int W, int connectivity, int min_region, int fill, int n,
                                     int raw_labels, int* work, int* count, int* root, int* size, void* out, void* weight,
                                     unsigned long long* dropped, int* flag, void* stream) {
  const DropArgs d = {min_region, fill, n, raw_labels ? 1 : 0, (unsigned char*)out, (unsigned char*)weight, dropped};
  return regions_launch(labels, 1, B, H, W, connectivity, work, count, root, size, flag, &d, stream);
}

extern "C" int ifseg_seg_regions_limit(int which) {
  switch (which) {
    case 0: return TILE_ROWS;
    case 1: return TILE_COLS;
    case 2: return RG_MAX_CLASSES;
    default: return IFSEG_ERR_BAD_ARG;
  }
}
