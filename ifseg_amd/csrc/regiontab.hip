// The region table of a label map on gfx950 (ifseg_amd/predict.py: region_table_reference is the specification;
// include/ifseg_hip.h states the rule): one row per connected region -- value, root, area, bounding box, the coordinate sums of
// the centroid and the summed confidence -- numbered in ascending order of the regions' roots, and the plane that names every
// pixel's row (Segmenter.regions_raw).  Regions, roots and sizes come from regions.hip through its C entry, which this file
// calls and does not change.
//
// A call: ifseg_seg_regions' launches (root, size), then four of this file's on the same stream:
//   regtab_count_kernel  1-D workgroups of RT_BLOCK = 1024 consecutive flat pixels of ONE image (256 threads, four steps of a
//                        wave's 64).  A pixel is flagged iff it is its region's root (root[p] == p) and the region is listed
//                        (size >= min_region, value not `ignore`); the workgroup's count = 16 ballots' popcounts summed through
//                        LDS -> blk[b][block].
//   regtab_scan_kernel   one workgroup per image turns its block counts into exclusive offsets in place, 256 at a time in block
//                        order with a carried total, and writes count[b].  No look-back: no workgroup ever waits for another.
//   regtab_rows_kernel   the blocks of the count launch again: rank = the block's offset + the popcounts of the 64-pixel groups
//                        in front + the ballot's bits below the lane -- the number of listed roots with a smaller flat index,
//                        which IS the canonical number.  A listed root with rank s < R writes its row (value, root, size,
//                        INT_MAX, INT_MAX, -1, -1, 0) and zeroes its three sums; every root writes s or -1 at its own pixel of
//                        the slot plane.
//   regtab_stats_kernel  one workgroup per tile of tile.h's 16 x 64 (tile_decode: lane = x, a wave takes 4 rows).  A pixel reads
//                        root[p] and the slot at that root, writes slot[p].  Pixels with a slot are reduced per row run first:
//                        the run of equal roots from one ballot (as regions_tile_kernel finds its runs); length, x-extent and
//                        sum of x in closed form, the sum of q by a segmented shuffle sum.  The run's leader adds into a
//                        workgroup-private LDS table keyed by slot: RT_SLOTS entries claimed by LDS compare-and-swap over
//                        RT_PROBES probes (count.h's hashed regime), each holding the tile-relative box (LDS min / max) and
//                        the pixel count, sum of x - X0, of y - Y0 and of q as uint32 -- 1024 pixels of at most 63, 15 and
//                        65535 each, so none wraps.  A run that finds no entry goes to its row directly.  After a barrier
//                        every claimed entry leaves as four 32-bit integer min / max atomics and three 64-bit integer adds
//                        (two without conf) on its row, agent scope, results unread: one set per tile-local region, not per
//                        pixel.  A tile of 1024 distinct regions (a checkerboard at connectivity 4) fills the table and sends
//                        the rest directly: the result never depends on the table's size.
// Plain loads: root and size were written by ifseg_seg_regions' launches, blk by the count / scan launches, the slot words at
// the roots by the rows launch -- each an EARLIER launch on the same stream.  Inside the stats launch a slot word is read only at
// a root (written before the launch; the root's own thread stores the same value again) and written only at the thread's own
// pixel, so no thread reads what another thread of the launch writes.  The rows and sums are touched by atomics only.
//
// Canonical: the numbering is a count of smaller roots, minima, maxima and integer sums do not depend on the order of their
// operands -- two calls give equal bits.  Nothing synchronises with the host, nothing is allocated here.  Every index read or
// written lies inside its buffer: a root is below H W, a slot is used only where 0 <= slot < R, a block index below the
// image's blocks, and rows behind min(count[b], R) are never touched.
// Registers (tools/regs.py regiontab.hip, gfx950, -O3): the count kernel 17 VGPRs (both label types), the scan 22, the rows
// kernel 44 (uint8) / 54 (int16), the stats kernel 32; no VGPR or SGPR spills, no scratch, occupancy 8 waves per SIMD by
// registers.  Static LDS: 18 KiB in the stats kernel (RT_SLOTS = 512 entries of 9 dwords; no dynamic LDS anywhere, so well inside
// the 64 KiB the other kernels budget), 64 bytes in the count and rows kernels, 16 in the scan.
#include <climits>
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;

constexpr int RT_BLOCK = 1024;                  // flat pixels of a block of the count / rows launches
constexpr int RT_GROUPS = RT_BLOCK / 64;        // a wave's 64 pixels at a time
constexpr int RT_MAX_REGIONS = 1 << 20;         // the largest R
constexpr int RT_SLOT_BITS = 9;
constexpr int RT_SLOTS = 1 << RT_SLOT_BITS;     // entries of the stats kernel's table
constexpr int RT_PROBES = 8;
constexpr uint32_t RT_EMPTY = 0xffffffffu;      // no key: keys are below RT_MAX_REGIONS
constexpr int RT_FIELDS = 9;                    // key, x0, y0, x1, y1, pixels, sum x, sum y, sum q

// the confidence in 16-bit fixed point: clamp(floor(conf * 65536), 0, 65535), the product exact, NaN -> 0 by fmaxf(NaN, 0) = 0
__device__ __forceinline__ uint32_t conf_q16(float conf) {
  return (uint32_t)fminf(fmaxf(floorf(__fmul_rn(conf, 65536.f)), 0.f), 65535.f);
}

// whether pixel i (inside the image that starts at lb / rt / sz) is the root of a listed region
template <typename L>
__device__ __forceinline__ bool listed_root(const L* lb, const int* rt, const int* sz, int i, int min_region, int ign) {
  return rt[i] == i && sz[i] >= min_region && (int)(short)lb[i] != ign;
}

// the 16 ballots of a block: group g = step * 4 + wave holds pixels [64 g, 64 g + 64) of the block.  -> this thread's four
// flags as bits; cnt[g] = the group's popcount, published by the barrier at the end
template <typename L>
__device__ __forceinline__ void block_ballots(const L* lb, const int* rt, const int* sz, int first, int HW, int min_region,
                                              int ign, int* cnt, unsigned long long (&ballot)[4]) {
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned i = (unsigned)first + (unsigned)((k * 4 + wave) * 64 + lane);      // H W < 2^31: no wrap in 32 bits
    const bool f = i < (unsigned)HW && listed_root(lb, rt, sz, (int)i, min_region, ign);
    ballot[k] = __ballot(f);
    if (lane == 0) cnt[k * 4 + wave] = __popcll(ballot[k]);
  }
  __syncthreads();
}

template <typename L>
__global__ __launch_bounds__(256) void regtab_count_kernel(const L* __restrict__ labels, const int* __restrict__ root,
                                                           const int* __restrict__ size, int HW, int nblk, int min_region,
                                                           int ign, int* __restrict__ blk) {
  __shared__ int cnt[RT_GROUPS];
  const int b = blockIdx.x / nblk, k = blockIdx.x - b * nblk;
  const long long pix0 = (long long)b * HW;
  unsigned long long ballot[4];
  block_ballots(labels + pix0, root + pix0, size + pix0, k * RT_BLOCK, HW, min_region, ign, cnt, ballot);
  if (threadIdx.x == 0) {
    int s = 0;
#pragma unroll
    for (int g = 0; g < RT_GROUPS; ++g) s += cnt[g];
    blk[blockIdx.x] = s;
  }
}

// blk[b][0 .. nblk) -> its exclusive prefix sums, nreg[b] = the total
__global__ __launch_bounds__(256) void regtab_scan_kernel(int* blk, int nblk, int* __restrict__ nreg) {
  __shared__ int wsum[4];
  int* mine = blk + (long long)blockIdx.x * nblk;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < nblk; base += 256) {
    const int i = base + threadIdx.x;
    const int v = i < nblk ? mine[i] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o);                            // every lane takes part
      if (lane >= o) inc += t;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wsum[w] : 0;
      total += wsum[w];
    }
    if (i < nblk) mine[i] = carry + before + inc - v;
    carry += total;
    __syncthreads();                                              // wsum is written again
  }
  if (threadIdx.x == 0) nreg[blockIdx.x] = carry;
}

template <typename L>
__global__ __launch_bounds__(256) void regtab_rows_kernel(const L* __restrict__ labels, const int* __restrict__ root,
                                                          const int* __restrict__ size, int HW, int nblk, int min_region,
                                                          int ign, const int* __restrict__ blk, int R, int* __restrict__ rows,
                                                          unsigned long long* __restrict__ sums, int* __restrict__ slot) {
  __shared__ int cnt[RT_GROUPS];
  const int b = blockIdx.x / nblk, k = blockIdx.x - b * nblk;
  const long long pix0 = (long long)b * HW;
  const L* lb = labels + pix0;
  const int* rt = root + pix0;
  const int* sz = size + pix0;
  unsigned long long ballot[4];
  block_ballots(lb, rt, sz, k * RT_BLOCK, HW, min_region, ign, cnt, ballot);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int off = blk[blockIdx.x];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int g = j * 4 + wave;
    const unsigned ui = (unsigned)(k * RT_BLOCK) + (unsigned)(g * 64 + lane);
    if (ui >= (unsigned)HW) continue;                             // no shuffle below
    const int i = (int)ui;
    if (rt[i] != i) continue;
    int s = -1;
    if ((ballot[j] >> lane) & 1ull) {
      s = off + __popcll(ballot[j] & ((1ull << lane) - 1ull));
      for (int q = 0; q < g; ++q) s += cnt[q];
      if (s < R) {
        const long long row = (long long)b * R + s;
        int* r = rows + row * 8;
        r[0] = (int)(short)lb[i];
        r[1] = i;
        r[2] = sz[i];
        r[3] = INT_MAX;
        r[4] = INT_MAX;
        r[5] = -1;
        r[6] = -1;
        r[7] = 0;
        sums[row * 3] = 0ull;
        sums[row * 3 + 1] = 0ull;
        sums[row * 3 + 2] = 0ull;
      } else {
        s = -1;
      }
    }
    slot[pix0 + i] = s;
  }
}

// a run's (or an entry's) statistics onto its row: x0 .. y1 and the sums in image coordinates
__device__ __forceinline__ void row_add(int* row, unsigned long long* sum, int x0, int y0, int x1, int y1, unsigned long long sx,
                                        unsigned long long sy, unsigned long long sq, bool has_conf) {
  (void)__hip_atomic_fetch_min(&row[3], x0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_min(&row[4], y0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_max(&row[5], x1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_max(&row[6], y1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_add(&sum[0], sx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  (void)__hip_atomic_fetch_add(&sum[1], sy, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (has_conf) (void)__hip_atomic_fetch_add(&sum[2], sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void regtab_stats_kernel(const int* __restrict__ root, const float* __restrict__ conf, int H,
                                                           int W, int tiles_x, int tiles_y, int R, int* rows,
                                                           unsigned long long* sums, int* slot) {
  __shared__ uint32_t tab[RT_FIELDS * RT_SLOTS];
  const Tile t = tile_decode(tiles_x, tiles_y, H, W);
  const long long pix0 = (long long)t.b * H * W;                  // B H W < 2^31
  const int rows_t = t.yend - t.Y0, cols = t.xend - t.X0, lane = t.lane;
  const bool has_conf = conf != nullptr;
  int* myrows = rows + (long long)t.b * R * 8;
  unsigned long long* mysums = sums + (long long)t.b * R * 3;
  // keys empty, the lower corners at the largest value, everything else 0
  for (int i = threadIdx.x; i < RT_FIELDS * RT_SLOTS; i += 256)
    tab[i] = i < RT_SLOTS ? RT_EMPTY : i < 3 * RT_SLOTS ? 0x7fffffffu : 0u;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ry = t.wave * 4 + j;                                // wave-uniform
    const bool ok = ry < rows_t && lane < cols;
    const long long p = pix0 + (long long)(t.Y0 + ry) * W + t.X0 + lane;
    int r = -1 - lane, s = -1;                                    // outside the tile: a root no neighbour shares
    if (ok) {
      r = root[p];
      if ((unsigned)r < (unsigned)(H * W)) s = slot[pix0 + r];    // always, unless ifseg_seg_regions raised its flag
      if ((unsigned)s >= (unsigned)R) s = -1;
      slot[p] = s;
    }
    const bool on = s >= 0;
    if (!__ballot(on)) continue;                                  // whole waves leave: the shuffles below see every lane
    const int left = __shfl_up(r, 1);
    const unsigned long long brk = __ballot(lane == 0 || left != r);      // lane 0 is always set
    const int start = 63 - __clzll((long long)(brk & (~0ull >> (63 - lane))));
    const unsigned long long above = lane == 63 ? 0ull : brk & (~0ull << (lane + 1));
    const int end = above ? __ffsll((long long)above) - 2 : 63;   // the run's last lane
    uint32_t q = 0u;
    if (has_conf) {
      q = on ? conf_q16(conf[p]) : 0u;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {                          // q = the sum over lane .. min(lane + 2 o - 1, end)
        const uint32_t up = (uint32_t)__shfl_down((int)q, o);
        if (lane + o <= end) q += up;
      }
    }
    if (!on || lane != start) continue;                           // the run's leader goes on
    const uint32_t len = (uint32_t)(end - start + 1);
    const uint32_t sx = (uint32_t)(start + end) * len / 2u;       // (start + end) len is even
    const uint32_t sy = (uint32_t)ry * len;
    uint32_t e = ((uint32_t)s * 2654435761u) >> (32 - RT_SLOT_BITS);
    bool placed = false;
    for (int probe = 0; probe < RT_PROBES; ++probe, e = (e + 1) & (RT_SLOTS - 1)) {
      const uint32_t was = atomicCAS(&tab[e], RT_EMPTY, (uint32_t)s);
      if (was == RT_EMPTY || was == (uint32_t)s) {
        placed = true;
        break;
      }
    }
    if (placed) {
      atomicMin(&tab[1 * RT_SLOTS + e], (uint32_t)start);
      atomicMin(&tab[2 * RT_SLOTS + e], (uint32_t)ry);
      atomicMax(&tab[3 * RT_SLOTS + e], (uint32_t)end);
      atomicMax(&tab[4 * RT_SLOTS + e], (uint32_t)ry);
      atomicAdd(&tab[5 * RT_SLOTS + e], len);
      atomicAdd(&tab[6 * RT_SLOTS + e], sx);
      atomicAdd(&tab[7 * RT_SLOTS + e], sy);
      if (has_conf) atomicAdd(&tab[8 * RT_SLOTS + e], q);
    } else {
      row_add(myrows + (long long)s * 8, mysums + (long long)s * 3, t.X0 + start, t.Y0 + ry, t.X0 + end, t.Y0 + ry,
              (unsigned long long)sx + (unsigned long long)len * t.X0, (unsigned long long)sy + (unsigned long long)len * t.Y0,
              (unsigned long long)q, has_conf);
    }
  }
  __syncthreads();
  for (int e = threadIdx.x; e < RT_SLOTS; e += 256) {
    const uint32_t key = tab[e];
    if (key == RT_EMPTY) continue;
    const unsigned long long n = tab[5 * RT_SLOTS + e];
    row_add(myrows + (long long)key * 8, mysums + (long long)key * 3, t.X0 + (int)tab[1 * RT_SLOTS + e],
            t.Y0 + (int)tab[2 * RT_SLOTS + e], t.X0 + (int)tab[3 * RT_SLOTS + e], t.Y0 + (int)tab[4 * RT_SLOTS + e],
            (unsigned long long)tab[6 * RT_SLOTS + e] + n * t.X0, (unsigned long long)tab[7 * RT_SLOTS + e] + n * t.Y0,
            (unsigned long long)tab[8 * RT_SLOTS + e], has_conf);
  }
}

template <typename L>
void table_launches(const L* labels, const float* conf, int B, int H, int W, int min_region, int ign, int R, const int* root,
                    const int* size, int* blk, int* rows, unsigned long long* sums, int* nreg, int* slot, int nblk, int tiles_x,
                    int tiles_y, long long tiles, hipStream_t s) {
  const int HW = H * W;
  const unsigned blocks = (unsigned)((long long)B * nblk);
  hipLaunchKernelGGL(regtab_count_kernel<L>, dim3(blocks), dim3(256), 0, s, labels, root, size, HW, nblk, min_region, ign, blk);
  hipLaunchKernelGGL(regtab_scan_kernel, dim3((unsigned)B), dim3(256), 0, s, blk, nblk, nreg);
  hipLaunchKernelGGL(regtab_rows_kernel<L>, dim3(blocks), dim3(256), 0, s, labels, root, size, HW, nblk, min_region, ign, blk, R,
                     rows, sums, slot);
  hipLaunchKernelGGL(regtab_stats_kernel, dim3((unsigned)tiles), dim3(256), 0, s, root, conf, H, W, tiles_x, tiles_y, R, rows,
                     sums, slot);
}

}  // namespace

extern "C" int ifseg_seg_region_table(const void* labels, int label_bytes, const float* conf, int B, int H, int W,
                                      int connectivity, int min_region, int ignore, int has_ignore, int R, int* work, int* count,
                                      int* root, int* size, int* blk, int* rows, long long* sums, int* nreg, int* slot, int* flag,
                                      void* stream) {
  (void)hipGetLastError();
  if (!labels || !work || !count || !root || !size || !blk || !rows || !sums || !nreg || !slot || !flag) return IFSEG_ERR_BAD_ARG;
  if (label_bytes != 1 && label_bytes != 2) return IFSEG_ERR_BAD_ARG;
  if (label_bytes == 2 && ((size_t)labels & 1)) return IFSEG_ERR_BAD_ARG;
  if ((((size_t)conf | (size_t)work | (size_t)count | (size_t)root | (size_t)size | (size_t)blk | (size_t)rows | (size_t)nreg |
        (size_t)slot | (size_t)flag) & 3) || ((size_t)sums & 7))
    return IFSEG_ERR_BAD_ARG;
  if (connectivity != 4 && connectivity != 8) return IFSEG_ERR_BAD_ARG;
  if (min_region < 1 || R < 1 || R > RT_MAX_REGIONS) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  const long long npix = (long long)B * H * W;
  const int nblk = (int)(((long long)H * W + RT_BLOCK - 1) / RT_BLOCK);
  if ((long long)B * nblk >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  const struct { const void* p; long long bytes; } bufs[12] = {
      {labels, npix * label_bytes}, {conf, npix * 4}, {work, npix * 4}, {count, npix * 4}, {root, npix * 4}, {size, npix * 4},
      {blk, 4ll * B * nblk}, {rows, 32ll * B * R}, {sums, 24ll * B * R}, {nreg, 4ll * B}, {slot, npix * 4}, {flag, 4}};
  for (int i = 0; i < 12; ++i)
    for (int j = i + 1; j < 12; ++j)
      if (overlaps(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes)) return IFSEG_ERR_BAD_ARG;
  int tiles_x, tiles_y;
  long long tiles;
  if (!tile_grid(H, W, B, &tiles_x, &tiles_y, &tiles)) return IFSEG_ERR_BAD_SHAPE;
  const int rc = ifseg_seg_regions(labels, label_bytes, B, H, W, connectivity, work, count, root, size, flag, stream);
  if (rc) return rc;
  const int ign = has_ignore ? ignore : (int)0x7fffffff;          // a label is a byte or a short: no label takes this
  const hipStream_t s = (hipStream_t)stream;
  if (label_bytes == 1)
    table_launches((const unsigned char*)labels, conf, B, H, W, min_region, ign, R, root, size, blk, rows,
                   (unsigned long long*)sums, nreg, slot, nblk, tiles_x, tiles_y, tiles, s);
  else
    table_launches((const short*)labels, conf, B, H, W, min_region, ign, R, root, size, blk, rows, (unsigned long long*)sums,
                   nreg, slot, nblk, tiles_x, tiles_y, tiles, s);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_region_table_limit(int which) {
  switch (which) {
    case 0: return TILE_ROWS;
    case 1: return TILE_COLS;
    case 2: return RT_BLOCK;
    case 3: return RT_MAX_REGIONS;
    default: return IFSEG_ERR_BAD_ARG;
  }
}
