// The sieve of a label map on gfx950 (ifseg_amd/predict.py: sieve_reference is the specification; include/ifseg_hip.h states
// the rule): a connected region of fewer than min_region pixels takes the value of its largest 4-adjacent neighbour region --
// the island of "sofa" inside "wall" becomes "wall", the hole closes (Segmenter(sieve=)).  Regions and their sizes come from
// regions.hip through its C entry, which this file calls and does not change.
//
// A pass: ifseg_seg_regions' launches (root, size of the pass's input map), then three of this file's on the same stream:
//   sieve_clear_kernel   best[p] = 0, one uint64 word per pixel (only the words at the regions' roots are ever used)
//   sieve_vote_kernel    one workgroup per tile of tile.h's 16 x 64 (tile_decode: lane = x, a wave takes 4 rows).  A region's key
//                        is (uint64)size << 32 | (0xFFFFFFFF - root): size first, the smaller root wins a tie, unique within an
//                        image.  A pixel of a small region (size < min_region, value not `ignore`) takes the largest key over
//                        its up to four neighbours inside the image whose root differs, whose value is not `ignore` and whose
//                        key exceeds its own, and puts it into best[its region's root] with ONE agent-scope 64-bit integer
//                        atomic maximum whose result nobody reads (global_atomic_umax_x2, no compare-and-swap loop).  Votes
//                        that cannot matter are not cast: a wave without a small pixel leaves after its loads, a pixel without
//                        a candidate casts none, and a lane whose left neighbour in the wave votes for the same region with
//                        the same candidate leaves the vote to it (the interior of a run along a straight edge).
//                        root / size were written by earlier launches, so plain loads are right; the 1-pixel halo of (root,
//                        size) is read through the cache, not staged in LDS: only small pixels read neighbours at all, a wave
//                        of which on a real map has a handful, so a staged 18 x 66 x 8 B halo would be loaded by every tile for
//                        the few that use it.  (The LDS form was not built and so not measured against this one.)
//   sieve_apply_kernel   a later launch, so plain loads of best are right: a pixel of a small region whose best != 0 becomes
//                        in[pix0 + (0xFFFFFFFF - low32(best))], the value at the winning neighbour's root; every other pixel is
//                        copied.  In the LAST pass, against the ORIGINAL input: conf is zeroed where the value changed, and
//                        moved[2][n] goes through a workgroup-private LDS table (count.h's bin_add), flushed with 64-bit
//                        integer atomics as the other counters are.
// Passes ping-pong between the caller's tmp and out so that the last one lands in out; one pass needs no tmp.
//
// Canonical: every decision of a pass reads the pass's input map, its roots and sizes (canonical themselves) and best, which
// holds the maximum of the votes cast -- a maximum does not depend on the order of its operands, and the votes left out are
// duplicates of votes cast.  Integers throughout: two runs give equal bits.  Nothing synchronises with the host, nothing is
// allocated here.  Every index read or written lies inside the pixel's own image: neighbours are tested against 0, W, H, a
// root is below H W, and best holds only keys made from roots.
// Registers (tools/regs.py sieve.hip, gfx950, -O3): the clear kernel 6 VGPRs, the vote kernel 21 (both label types), the apply
// kernel 24 and in the last pass 29 (uint8) / 27 (int16); no VGPR or SGPR spills, no scratch, occupancy 8 waves per SIMD by
// registers.  Static LDS: 4 KiB in the last pass's apply kernel (moved[2][512]), none elsewhere.
#include "count.h"
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using count::bin_add;

constexpr int SV_MAX_PASSES = 8;
constexpr int SV_MAX_CLASSES = 512;
constexpr int SV_MAX_BLOCKS = 2048;             // of the clear and the apply launches: grid-stride beyond

#define SV_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

__device__ __forceinline__ unsigned long long sieve_key(int size, int root) {
  return ((unsigned long long)(unsigned)size << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)root);
}

__global__ __launch_bounds__(256) void sieve_clear_kernel(unsigned long long* __restrict__ best, long long npix) {
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < npix; p += (long long)gridDim.x * 256) best[p] = 0ull;
}

// ign: the ignored value, or a value no label takes
template <typename L>
__global__ __launch_bounds__(256) void sieve_vote_kernel(const L* __restrict__ labels, const int* __restrict__ root,
                                                         const int* __restrict__ size, int H, int W, int tiles_x, int tiles_y,
                                                         int min_region, int ign, unsigned long long* best) {
  const Tile t = tile_decode(tiles_x, tiles_y, H, W);
  const long long pix0 = (long long)t.b * H * W;                  // B H W < 2^31
  const L* lb = labels + pix0;
  const int* rt = root + pix0;
  const int* sz = size + pix0;
  const int x = t.X0 + t.lane;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = t.Y0 + t.wave * 4 + j;                          // wave-uniform
    const bool ok = y < t.yend && x < t.xend;
    const int p = y * W + x;
    int r = -1, s = 0;
    bool small = false;
    if (ok) {
      r = rt[p];
      s = sz[p];
      small = s < min_region && (int)(short)lb[p] != ign;
    }
    if (!__ballot(small)) continue;                               // whole waves leave: the shuffles below see every lane
    unsigned long long cand = 0ull;
    if (small) {
      const unsigned long long own = sieve_key(s, r);
      auto look = [&](int q) {
        const int rq = rt[q];
        if (rq == r) return;
        const unsigned long long k = sieve_key(sz[q], rq);
        if (k > own && k > cand && (int)(short)lb[q] != ign) cand = k;
      };
      if (y > 0) look(p - W);
      if (x > 0) look(p - 1);
      if (x + 1 < W) look(p + 1);
      if (y + 1 < H) look(p + W);
    }
    const int left_r = __shfl_up(r, 1);
    const unsigned left_hi = __shfl_up((unsigned)(cand >> 32), 1), left_lo = __shfl_up((unsigned)cand, 1);
    const bool dup = t.lane > 0 && left_r == r && (((unsigned long long)left_hi << 32) | left_lo) == cand;
    if (cand != 0ull && !dup) (void)__hip_atomic_fetch_max(&best[pix0 + r], cand, SV_RLX_AGENT);
  }
}

// in: the pass's input map; orig / conf / moved: read and written in the LAST pass only
template <typename L, bool LAST>
__global__ __launch_bounds__(256) void sieve_apply_kernel(const L* __restrict__ in, const int* __restrict__ root,
                                                          const int* __restrict__ size,
                                                          const unsigned long long* __restrict__ best, int HW, long long npix,
                                                          int min_region, int ign, L* __restrict__ out,
                                                          const L* __restrict__ orig, float* conf, int n, int raw,
                                                          unsigned long long* moved) {
  __shared__ uint32_t mtab[LAST ? 2 * SV_MAX_CLASSES : 1];
  if (LAST) {
    for (int c = threadIdx.x; c < 2 * n; c += 256) mtab[c] = 0u;
    __syncthreads();
  }
  // whole waves walk: the bound is the wave's first pixel
  for (long long base = (long long)blockIdx.x * 256 + (threadIdx.x & ~63); base < npix; base += (long long)gridDim.x * 256) {
    const long long p = base + (threadIdx.x & 63);
    const bool ok = p < npix;
    int was = 0, now = 0;
    bool changed = false;
    if (ok) {
      const int v = (int)(short)in[p];
      int nv = v;
      if (size[p] < min_region && v != ign) {
        const long long pix0 = p / HW * HW;
        const unsigned long long b = best[pix0 + root[p]];
        if (b != 0ull) nv = (int)(short)in[pix0 + (long long)(0xFFFFFFFFu - (unsigned)b)];
      }
      out[p] = (L)nv;
      if (LAST) {
        const int o = (int)(short)orig[p];
        changed = nv != o;
        if (changed && conf) conf[p] = 0.f;
        was = o - raw;
        now = nv - raw;
      }
    }
    if (LAST) {
      const bool cw = changed && (unsigned)was < (unsigned)n, cn = changed && (unsigned)now < (unsigned)n;
      bin_add(mtab, cw ? was : 0, cw);
      bin_add(mtab, cn ? n + now : 0, cn);
    }
  }
  if (LAST) {
    __syncthreads();
    for (int c = threadIdx.x; c < 2 * n; c += 256) {
      const uint32_t v = mtab[c];
      if (v) atomicAdd(&moved[c], (unsigned long long)v);
    }
  }
}

// uint8 labels read through (short) as regions.hip reads them: 0 .. 255 stay 0 .. 255
template <typename L>
int sieve_passes(const L* labels, int B, int H, int W, int connectivity, int min_region, int passes, int ign, int n, int raw,
                 int* work, int* count, int* root, int* size, unsigned long long* best, L* tmp, L* out, float* conf,
                 unsigned long long* moved, int* flag, int tiles_x, int tiles_y, long long blocks, hipStream_t s) {
  const long long npix = (long long)B * H * W;
  const int HW = H * W;
  const unsigned fblocks = (unsigned)std::min<long long>((npix + 255) / 256, SV_MAX_BLOCKS);
  const L* in = labels;
  for (int k = 0; k < passes; ++k) {
    L* dst = ((passes - 1 - k) & 1) ? tmp : out;                  // the last pass lands in out
    const int rc = ifseg_seg_regions(in, (int)sizeof(L), B, H, W, connectivity, work, count, root, size, flag, (void*)s);
    if (rc) return rc;
    hipLaunchKernelGGL(sieve_clear_kernel, dim3(fblocks), dim3(256), 0, s, best, npix);
    hipLaunchKernelGGL(sieve_vote_kernel<L>, dim3((unsigned)blocks), dim3(256), 0, s, in, root, size, H, W, tiles_x, tiles_y,
                       min_region, ign, best);
    if (k == passes - 1)
      hipLaunchKernelGGL((sieve_apply_kernel<L, true>), dim3(fblocks), dim3(256), 0, s, in, root, size, best, HW, npix, min_region,
                         ign, dst, labels, conf, n, raw, moved);
    else
      hipLaunchKernelGGL((sieve_apply_kernel<L, false>), dim3(fblocks), dim3(256), 0, s, in, root, size, best, HW, npix,
                         min_region, ign, dst, (const L*)nullptr, (float*)nullptr, 0, 0, (unsigned long long*)nullptr);
    in = dst;
  }
  IFSEG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int ifseg_seg_sieve(const void* labels, int label_bytes, int B, int H, int W, int connectivity, int min_region,
                               int passes, int ignore, int has_ignore, int n, int raw_labels, int* work, int* count, int* root,
                               int* size, unsigned long long* best, void* tmp, void* out, float* conf, unsigned long long* moved,
                               int* flag, void* stream) {
  (void)hipGetLastError();
  if (!labels || !work || !count || !root || !size || !best || !out || !moved || !flag) return IFSEG_ERR_BAD_ARG;
  if (label_bytes != 1 && label_bytes != 2) return IFSEG_ERR_BAD_ARG;
  if (passes < 1 || passes > SV_MAX_PASSES || (passes > 1 && !tmp)) return IFSEG_ERR_BAD_ARG;
  if (label_bytes == 2 && (((size_t)labels | (size_t)out | (size_t)tmp) & 1)) return IFSEG_ERR_BAD_ARG;
  if ((((size_t)work | (size_t)count | (size_t)root | (size_t)size | (size_t)flag | (size_t)conf) & 3) ||
      (((size_t)best | (size_t)moved) & 7))
    return IFSEG_ERR_BAD_ARG;
  if (connectivity != 4 && connectivity != 8) return IFSEG_ERR_BAD_ARG;
  if (min_region < 1 || n < 1 || n > SV_MAX_CLASSES) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  const long long npix = (long long)B * H * W;
  if (passes == 1) tmp = nullptr;                                  // not used: it may lie anywhere
  const struct { const void* p; long long bytes; } bufs[12] = {
      {labels, npix * label_bytes}, {work, npix * 4}, {count, npix * 4}, {root, npix * 4}, {size, npix * 4}, {best, npix * 8},
      {tmp, npix * label_bytes}, {out, npix * label_bytes}, {conf, npix * 4}, {moved, 16ll * n}, {flag, 4}, {nullptr, 0}};
  for (int i = 0; i < 11; ++i)
    for (int j = i + 1; j < 11; ++j)
      if (overlaps(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes)) return IFSEG_ERR_BAD_ARG;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(H, W, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const int ign = has_ignore ? ignore : (int)0x7fffffff;          // a label is a byte or a short: no label takes this
  const int raw = raw_labels ? 1 : 0;
  const hipStream_t s = (hipStream_t)stream;
  if (label_bytes == 1)
    return sieve_passes<unsigned char>((const unsigned char*)labels, B, H, W, connectivity, min_region, passes, ign, n, raw, work,
                                       count, root, size, best, (unsigned char*)tmp, (unsigned char*)out, conf, moved, flag,
                                       tiles_x, tiles_y, blocks, s);
  return sieve_passes<short>((const short*)labels, B, H, W, connectivity, min_region, passes, ign, n, raw, work, count, root, size,
                             best, (short*)tmp, (short*)out, conf, moved, flag, tiles_x, tiles_y, blocks, s);
}

extern "C" int ifseg_seg_sieve_limit(int which) {
  switch (which) {
    case 0: return TILE_ROWS;
    case 1: return TILE_COLS;
    case 2: return SV_MAX_PASSES;
    case 3: return SV_MAX_CLASSES;
    default: return IFSEG_ERR_BAD_ARG;
  }
}
