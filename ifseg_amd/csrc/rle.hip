// Run-length label maps on gfx950 (ifseg_amd/predict.py: rle_encode_reference / rle_decode_reference are the specifications;
// include/ifseg_hip.h states the rule): a label map [H, W] as the table of its runs (start, value) in COCO's run order --
// column-major, flat position i = x H + y -- and back (Segmenter.export_raw, RunLengthMap).  Position i starts a run iff
// i == 0 or f[i] != f[i - 1]; a run goes on across a column boundary and never from one image of a batch into the next.
//
// The decomposition is the dual of regiontab.hip's count / scan / rank: flat order is COLUMN order here, memory order is row
// order, so a lane keeps one column (lane = x: a wave loads one coalesced row of 64 labels) and walks DOWN it.
//   rle_count_kernel   a workgroup of 256 takes RL_COLS = 64 columns x a chunk of RL_CHUNK = 32 rows; wave w takes the chunk's
//                      rows [8 w, 8 w + 8), each lane loads its column's label of those eight rows (eight independent loads) and
//                      the label of the position in front of the first one: the row above, or for y = 0 the last row of the
//                      column to the left, or nothing for x = 0 (position 0 always starts a run).  The four waves' per-column
//                      counts meet in LDS and one count leaves per segment (x, chunk) at index x nchunk + chunk -- which IS
//                      flat order: ascending x, then ascending y.
//   rle_scan_kernel    one workgroup per image turns its W nchunk segment counts into exclusive offsets in place, 256 at a time
//                      with a carried total, and writes count[b] (regtab_scan_kernel's rule, written again here so that
//                      regiontab.hip's code stays what it was).  No look-back: no workgroup ever waits for another.
//   rle_write_kernel   the count walk again (the labels stay in registers across the one barrier).  A run's number = its
//                      segment's offset + the counts of the waves above it in the same column (from LDS) + the runs the thread
//                      has met so far; with number s < R it stores (start, value) as ONE 8-byte store.  Entries from
//                      min(count, R) on are never written.
//   rle_decode_kernel  the same thread-to-pixel map.  A thread binary-searches start[0 .. m), m = min(count[b], R), for its
//                      first position, then walks down and moves on while the next run starts at or below its position; it
//                      stores with lane = x, so a wave stores one coalesced row.  Every index into the table is in [0, m)
//                      whatever the table holds (the search keeps lo < hi <= m, the walk tests s + 1 < m before it reads): a
//                      malformed table gives wrong pixels and never an out-of-range access, and the walk ends after at most m
//                      steps.  With m <= 0 the image is `fill`.  One thread per image ORs the image's flag bits into the flag
//                      word, and only where a bit is set (the one atomic of this file; the encoder has none).
// Plain loads: the segment counts are written by the count launch, the offsets by the scan, runs and count by earlier launches
// or by the host -- each BEFORE the launch that reads them, on the same stream.  Everything is an integer and every output
// word has one writer: two calls give equal bits.  Nothing synchronises with the host, nothing is allocated here.
//
// The chunk height.  A chunk of RL_CHUNK rows costs the scan W ceil(H / RL_CHUNK) / 256 serial iterations in ONE workgroup
// and gives the walk launches ceil(W / 64) ceil(H / RL_CHUNK) workgroups.  At 512 x 683 (the evaluation size of a COCO-Stuff
// image) 32 rows are 176 workgroups -- most of the 256 compute units, where 64 rows would be 88 -- for 43 scan iterations
// (10928 segments, 43 KB), and a thread's 8 labels stay in registers between the count and the write with all eight loads in
// flight at once.  16 rows would double the scan (86 iterations, two barriers each) for 352 workgroups of half the work
// each; 128 rows would quarter it and leave 44 workgroups with 32 rows per thread.  (Measured at 32 only.)  At 4096 x 4096 the scan is 2048
// iterations, which a larger chunk would shorten: the choice is made for the sizes a Segmenter produces.
// Registers (tools/regs.py rle.hip, gfx950, -O3): the count kernel 20 VGPRs, the scan 22, the write kernel 32, the decoder 13
// (the same for both label types); no VGPR or SGPR spills, no scratch, occupancy 8 waves per SIMD by registers.
// Static LDS: 1 KiB in the count and write kernels, 16 bytes in the scan, none in the decoder.
#include <climits>
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace {

constexpr int RL_CHUNK = 32;                    // rows of a chunk
constexpr int RL_COLS = 64;                     // columns of a workgroup: a wave's lanes
constexpr int RL_ROWS = RL_CHUNK / 4;           // a wave's rows of the chunk, a thread's labels
constexpr int RL_MAX_RUNS = 1 << 24;            // the largest R

struct Segment {
  int b, chunk, x, y0, lane, wave;              // image, chunk, the thread's column and first row; wave is wave-uniform
};

// blockIdx.x -> (image, column group, chunk), the chunk fastest
__device__ __forceinline__ Segment segment_decode(int ncg, int nchunk) {
  const int chunk = blockIdx.x % nchunk, cg = (blockIdx.x / nchunk) % ncg, b = blockIdx.x / (nchunk * ncg);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  return {b, chunk, cg * RL_COLS + lane, chunk * RL_CHUNK + wave * RL_ROWS, lane, wave};
}

// the thread's RL_ROWS labels of column x from row y0 on (lb: the image's first label) -> bit j set iff position x H + y0 + j
// starts a run; v[j] its value.  A thread outside the image returns 0.  H W < 2^31: every index fits an int
template <typename L>
__device__ __forceinline__ unsigned column_walk(const L* lb, int H, int W, int x, int y0, int (&v)[RL_ROWS]) {
#pragma unroll
  for (int j = 0; j < RL_ROWS; ++j) v[j] = 0;
  if (x >= W || y0 >= H) return 0u;
  int prev = 0;
  bool none = false;                            // position 0: nothing in front
  if (y0 > 0) prev = (int)lb[(y0 - 1) * W + x];
  else if (x > 0) prev = (int)lb[(H - 1) * W + x - 1];
  else none = true;
#pragma unroll
  for (int j = 0; j < RL_ROWS; ++j)
    if (y0 + j < H) v[j] = (int)lb[(y0 + j) * W + x];
  unsigned bits = 0u;
#pragma unroll
  for (int j = 0; j < RL_ROWS; ++j) {
    if (y0 + j < H) {
      if ((j == 0 && none) || v[j] != prev) bits |= 1u << j;
      prev = v[j];
    }
  }
  return bits;
}

template <typename L>
__global__ __launch_bounds__(256) void rle_count_kernel(const L* __restrict__ labels, int H, int W, int ncg, int nchunk,
                                                        int* __restrict__ seg) {
  __shared__ int cnt[4][RL_COLS];
  const Segment t = segment_decode(ncg, nchunk);
  int v[RL_ROWS];
  const unsigned bits = column_walk(labels + (long long)t.b * H * W, H, W, t.x, t.y0, v);
  cnt[t.wave][t.lane] = __popc(bits);
  __syncthreads();
  if (t.wave == 0 && t.x < W)
    seg[(long long)t.b * W * nchunk + (long long)t.x * nchunk + t.chunk] =
        cnt[0][t.lane] + cnt[1][t.lane] + cnt[2][t.lane] + cnt[3][t.lane];
}

// seg[b][0 .. nseg) -> its exclusive prefix sums, count[b] = the total
__global__ __launch_bounds__(256) void rle_scan_kernel(int* seg, int nseg, int* __restrict__ count) {
  __shared__ int wsum[4];
  int* mine = seg + (long long)blockIdx.x * nseg;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int carry = 0;
  for (int base = 0; base < nseg; base += 256) {
    const int i = base + threadIdx.x;
    const int v = i < nseg ? mine[i] : 0;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o);                           // every lane takes part
      if (lane >= o) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      before += w < wave ? wsum[w] : 0;
      total += wsum[w];
    }
    if (i < nseg) mine[i] = carry + before + inc - v;
    carry += total;
    __syncthreads();                                              // wsum is written again
  }
  if (threadIdx.x == 0) count[blockIdx.x] = carry;
}

template <typename L>
__global__ __launch_bounds__(256) void rle_write_kernel(const L* __restrict__ labels, int H, int W, int ncg, int nchunk,
                                                        const int* __restrict__ seg, int R, int2* __restrict__ runs) {
  __shared__ int cnt[4][RL_COLS];
  const Segment t = segment_decode(ncg, nchunk);
  int v[RL_ROWS];
  const unsigned bits = column_walk(labels + (long long)t.b * H * W, H, W, t.x, t.y0, v);
  cnt[t.wave][t.lane] = __popc(bits);
  __syncthreads();
  if (!bits) return;                                              // (so x < W and y0 < H)
  int s = seg[(long long)t.b * W * nchunk + (long long)t.x * nchunk + t.chunk];
  for (int w = 0; w < t.wave; ++w) s += cnt[w][t.lane];
  int2* mine = runs + (long long)t.b * R;
  const int first = t.x * H + t.y0;
#pragma unroll
  for (int j = 0; j < RL_ROWS; ++j) {
    if (bits & (1u << j)) {
      if (s < R) mine[s] = make_int2(first + j, v[j]);
      ++s;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void rle_decode_kernel(const int2* __restrict__ runs, const int* __restrict__ count, int H,
                                                         int W, int ncg, int nchunk, int R, int fill, T* __restrict__ out,
                                                         int* flag) {
  const Segment t = segment_decode(ncg, nchunk);
  const int c = count[t.b];
  const int m = c < R ? c : R;
  const int2* tab = runs + (long long)t.b * R;
  if (blockIdx.x % (nchunk * ncg) == 0 && threadIdx.x == 0) {
    const int bits = (c > R ? 1 : 0) | ((m <= 0 || tab[0].x != 0) ? 2 : 0);
    if (bits) (void)__hip_atomic_fetch_or(flag, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (t.x >= W || t.y0 >= H) return;
  T* o = out + (long long)t.b * H * W;
  if (m <= 0) {
#pragma unroll
    for (int j = 0; j < RL_ROWS; ++j)
      if (t.y0 + j < H) o[(t.y0 + j) * W + t.x] = (T)fill;
    return;
  }
  const int first = t.x * H + t.y0;
  int lo = 0, hi = m;                                             // 0 <= lo < hi <= m: the answer is in [lo, hi)
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (tab[mid].x <= first) lo = mid;
    else hi = mid;
  }
  int s = lo, val = tab[lo].y;
  int2 nxt = s + 1 < m ? tab[s + 1] : make_int2(INT_MAX, 0);      // a position is at most 2^31 - 2
#pragma unroll
  for (int j = 0; j < RL_ROWS; ++j) {
    if (t.y0 + j >= H) break;
    while (nxt.x <= first + j) {                                  // s only grows and stays below m
      val = nxt.y;
      ++s;
      nxt = s + 1 < m ? tab[s + 1] : make_int2(INT_MAX, 0);
    }
    o[(t.y0 + j) * W + t.x] = (T)val;
  }
}

// the grid of the walk launches; false where it does not fit 31 bits
inline bool rle_grid(int B, int H, int W, int* ncg, int* nchunk, long long* blocks) {
  *ncg = (W + RL_COLS - 1) / RL_COLS;
  *nchunk = (H + RL_CHUNK - 1) / RL_CHUNK;
  *blocks = (long long)B * *ncg * *nchunk;
  return *blocks < (1ll << 31) && (long long)B * W * *nchunk < (1ll << 31);
}

template <typename L>
void encode_launches(const L* labels, int B, int H, int W, int R, int* seg, int* runs, int* count, int ncg, int nchunk,
                     long long blocks, hipStream_t s) {
  hipLaunchKernelGGL(rle_count_kernel<L>, dim3((unsigned)blocks), dim3(256), 0, s, labels, H, W, ncg, nchunk, seg);
  hipLaunchKernelGGL(rle_scan_kernel, dim3((unsigned)B), dim3(256), 0, s, seg, W * nchunk, count);
  hipLaunchKernelGGL(rle_write_kernel<L>, dim3((unsigned)blocks), dim3(256), 0, s, labels, H, W, ncg, nchunk, (const int*)seg, R,
                     reinterpret_cast<int2*>(runs));
}

}  // namespace

extern "C" int ifseg_seg_rle_encode(const void* labels, int label_bytes, int B, int H, int W, int R, int* seg, int* runs,
                                    int* count, void* stream) {
  (void)hipGetLastError();
  if (!labels || !seg || !runs || !count) return IFSEG_ERR_BAD_ARG;
  if (label_bytes != 1 && label_bytes != 2) return IFSEG_ERR_BAD_ARG;
  if (label_bytes == 2 && ((size_t)labels & 1)) return IFSEG_ERR_BAD_ARG;
  if ((((size_t)seg | (size_t)count) & 3) || ((size_t)runs & 7)) return IFSEG_ERR_BAD_ARG;
  if (R < 1 || R > RL_MAX_RUNS) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  int ncg, nchunk;
  long long blocks;
  if (!rle_grid(B, H, W, &ncg, &nchunk, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const struct { const void* p; long long bytes; } bufs[4] = {
      {labels, (long long)B * H * W * label_bytes}, {seg, 4ll * B * W * nchunk}, {runs, 8ll * B * R}, {count, 4ll * B}};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (overlaps(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes)) return IFSEG_ERR_BAD_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (label_bytes == 1) encode_launches((const unsigned char*)labels, B, H, W, R, seg, runs, count, ncg, nchunk, blocks, s);
  else encode_launches((const short*)labels, B, H, W, R, seg, runs, count, ncg, nchunk, blocks, s);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_rle_decode(const int* runs, const int* count, int B, int H, int W, int R, int label_bytes, int fill,
                                    void* out, int* flag, void* stream) {
  (void)hipGetLastError();
  if (!runs || !count || !out || !flag) return IFSEG_ERR_BAD_ARG;
  if (label_bytes != 1 && label_bytes != 2) return IFSEG_ERR_BAD_ARG;
  if (label_bytes == 2 && ((size_t)out & 1)) return IFSEG_ERR_BAD_ARG;
  if ((((size_t)count | (size_t)flag) & 3) || ((size_t)runs & 7)) return IFSEG_ERR_BAD_ARG;
  if (R < 1 || R > RL_MAX_RUNS) return IFSEG_ERR_BAD_ARG;
  if (label_bytes == 1 ? (fill < 0 || fill > 255) : (fill < -32768 || fill > 32767)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  int ncg, nchunk;
  long long blocks;
  if (!rle_grid(B, H, W, &ncg, &nchunk, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const struct { const void* p; long long bytes; } bufs[4] = {
      {runs, 8ll * B * R}, {count, 4ll * B}, {out, (long long)B * H * W * label_bytes}, {flag, 4}};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j)
      if (overlaps(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes)) return IFSEG_ERR_BAD_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const int2* tab = reinterpret_cast<const int2*>(runs);
  if (label_bytes == 1)
    hipLaunchKernelGGL(rle_decode_kernel<unsigned char>, dim3((unsigned)blocks), dim3(256), 0, s, tab, count, H, W, ncg, nchunk, R,
                       fill, (unsigned char*)out, flag);
  else
    hipLaunchKernelGGL(rle_decode_kernel<short>, dim3((unsigned)blocks), dim3(256), 0, s, tab, count, H, W, ncg, nchunk, R, fill,
                       (short*)out, flag);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_rle_limit(int which) {
  switch (which) {
    case 0: return RL_CHUNK;
    case 1: return RL_COLS;
    case 2: return RL_MAX_RUNS;
    default: return IFSEG_ERR_BAD_ARG;
  }
}
