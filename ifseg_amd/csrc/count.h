// Counting over a finished label map (predict.hip: seg_areas_kernel, seg_confusion_kernel and the scoring epilogues;
// pseudo.hip: seg_conf_hist_kernel, seg_pseudo_kernel; calib.hip: seg_calibration_kernel), each part written once:
//   bin_add       the wave pre-aggregated add into an LDS count
//   walk_pixels   the grid-stride walk over a flat label map and a second stream of the same pixels -- an integer map
//                 (ground truth: MapStream) or fp32 values (confidences: FloatStream) -- or of both
//   table_*       the workgroup-private table of keyed counts, direct or hashed: table_zero, table_add, table_flush
//   tally_flush, bins_flush   the two ways a thread's pair of tallies leaves: by wave, or through a table of plain bins
//   walk_launch   the host's side of the walk: what every counter on it refuses, walk_split, the (label, gt) element sizes
// Integers throughout, so every counter built from these is bit-reproducible.
#pragma once
#include <algorithm>
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace count {

// tab[idx] += 1 for every lane with `on`; whole (converged) waves call it.  A label map is piecewise constant, so most lanes
// of a wave name the same bin, and an LDS atomic takes the lanes of one address one after the other: the lanes that share the
// first active lane's bin leave as one add of their count, the others one each.  (table_add below is this in front of
// table_count; written through it, the two adds here merge into one and the scoring epilogues compile to other code.)
__device__ __forceinline__ void bin_add(uint32_t* tab, int idx, bool on) {
  const unsigned long long m = __ballot(on);
  if (!m) return;
  const int lead = __ffsll((long long)m) - 1;
  const int first = __builtin_amdgcn_readlane(idx, lead);
  const unsigned long long same = __ballot(on && idx == first);
  if ((int)(threadIdx.x & 63) == lead) atomicAdd(&tab[first], (uint32_t)__popcll(same));
  else if (on && idx != first) atomicAdd(&tab[idx], 1u);
}

// the ground-truth rule of include/ifseg_hip.h, its one statement (predict.hip's scoring, boundary.hip): the class of the
// value g, whether the pixel (where `live`) is scored, and whether it is not ignored but of a class outside [0, n)
struct GtClass {
  int cls;
  bool sc, oor;
};
__device__ __forceinline__ GtClass gt_class(int n, int raw, int g, bool live) {
  const bool ign = raw ? (g == 0 || g == 255) : (g == n || g == 255);
  const int cls = raw ? g - 1 : g;
  const bool inr = (unsigned)cls < (unsigned)n;
  return {cls, live && !ign && inr, live && !ign && !inr};
}

// the confidence bin of the histogram, the filter and the calibration counters (pseudo.hip, calib.hip), its one statement:
// bin(conf) = clamp(floor(conf * 256), 0, 255): the product is exact (a power of two), NaN -> 0 by fmaxf(NaN, 0) = 0
__device__ __forceinline__ int conf_bin(float conf) {
  return (int)fminf(fmaxf(floorf(__fmul_rn(conf, 256.f)), 0.f), 255.f);
}

// ---- the walk ----
// A lane takes 16 consecutive pixels per step: their labels come as aligned 16-byte loads.  The body starts at the first
// 16-byte boundary of `lab`; the second stream's elements of the same pixels sit wherever they sit (MapStream, FloatStream).
// The pixels in front of the body and behind its last whole group of 16 (fewer than 16 each) are read one by one.  Grid-stride
// over at most MAX_BLOCKS workgroups, so the flush does not grow with the image.
constexpr int MAX_BLOCKS = 512;

template <int EB>
__device__ __forceinline__ int elem_at(const void* p, long long i) {
  return EB == 1 ? (int)((const unsigned char*)p)[i] : (int)((const short*)p)[i];
}

// o[i] = dword i of the byte string w shifted down by 4 SD + sb bytes
template <int SD, int N>
__device__ __forceinline__ void shifted(const uint32_t (&w)[N + 4], int sb, uint32_t (&o)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i) o[i] = __builtin_amdgcn_alignbyte(w[i + SD + 1], w[i + SD], (uint32_t)sb);
}

// v[0..16) = the 16 elements of EB bytes that start s bytes (0 <= s < 16, wave-uniform) behind the 16-byte boundary p: EB
// aligned chunks, and one more only where s != 0 -- that one holds bytes of the elements, so it lies inside their buffer's pages
template <int EB>
__device__ __forceinline__ void load16(const unsigned char* p, int s, int (&v)[16]) {
  constexpr int N = 4 * EB;
  uint32_t w[N + 4], o[N];
#pragma unroll
  for (int c = 0; c <= EB; ++c) {
    uint4 q = make_uint4(0, 0, 0, 0);
    if (c < EB || s) q = *reinterpret_cast<const uint4*>(p + 16 * c);
    w[4 * c] = q.x; w[4 * c + 1] = q.y; w[4 * c + 2] = q.z; w[4 * c + 3] = q.w;
  }
  switch (s >> 2) {
    case 0: shifted<0, N>(w, s & 3, o); break;
    case 1: shifted<1, N>(w, s & 3, o); break;
    case 2: shifted<2, N>(w, s & 3, o); break;
    default: shifted<3, N>(w, s & 3, o); break;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i)
    v[i] = EB == 1 ? (int)((o[i >> 2] >> (8 * (i & 3))) & 255u) : (int)(short)(o[i >> 1] >> (16 * (i & 1)));
}

// The second stream of a walk, made from its first element and the head's length: at(p, i) reads element i (head and tail),
// group(g, v) the 16 elements of the body's group g.
// An integer map of EB bytes per element: its group sits s bytes behind a 16-byte boundary of its own, s the same for every
// lane, and is read as the aligned chunks around it, shifted into place
template <int EB>
struct MapStream {
  using T = int;
  using P = const unsigned char*;
  P gb;                           // the 16-byte boundary at or in front of the body's first element
  int s;                          // that element's distance from it, wave-uniform
  __device__ __forceinline__ MapStream(P p, int head) {
    gb = p + (long long)head * EB;
    s = __builtin_amdgcn_readfirstlane((int)((size_t)gb & 15));
    gb -= s;
  }
  static __device__ __forceinline__ int at(P p, long long i) { return elem_at<EB>(p, i); }
  __device__ __forceinline__ void group(long long g, int (&v)[16]) const { load16<EB>(gb + g * (16 * EB), s, v); }
};

// four floats at a 4-byte boundary
struct __attribute__((packed, aligned(4))) Float4A4 {
  float v[4];
};

// fp32 values: a group's 16 sit at a 4-byte boundary, four loads of 16 bytes
struct FloatStream {
  using T = float;
  using P = const float*;
  P gb;                           // the body's first element
  __device__ __forceinline__ FloatStream(P p, int head) : gb(p + head) {}
  static __device__ __forceinline__ float at(P p, long long i) { return p[i]; }
  __device__ __forceinline__ void group(long long g, float (&v)[16]) const {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const Float4A4 f = *reinterpret_cast<const Float4A4*>(gb + g * 16 + 4 * q);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * q + e] = f.v[e];
    }
  }
};

// no further stream
struct NoStream {
  using T = int;
  using P = const void*;
  __device__ __forceinline__ NoStream(P, int) {}
};

// the walk of a label map (LB bytes per label) and one or two further streams, its one statement: f(label, second, live), or
// f(label, second, third, live) where there is a Third, for every pixel, called by whole (converged) waves.  Head and tail go
// to lanes 0..15 and 16..31 of the grid's first wave, one pixel each; the body's groups of 16 to the lanes, grid-stride
template <int LB, typename Second, typename Third = NoStream, typename F>
__device__ __forceinline__ void walk_pixels(const unsigned char* lab, typename Second::P sec, int head, int groups, int tail, F f,
                                            typename Third::P thi = nullptr) {
  using T = typename Second::T;
  using U = typename Third::T;
  constexpr bool three = !std::is_same<Third, NoStream>::value;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (blockIdx.x == 0 && wave == 0) {
    long long i = -1;
    if (lane < head) i = lane;
    else if (lane >= 16 && lane - 16 < tail) i = (long long)head + (long long)groups * 16 + (lane - 16);
    const bool live = i >= 0;
    if constexpr (three) f(live ? elem_at<LB>(lab, i) : 0, live ? Second::at(sec, i) : T(0), live ? Third::at(thi, i) : U(0), live);
    else f(live ? elem_at<LB>(lab, i) : 0, live ? Second::at(sec, i) : T(0), live);
  }
  const unsigned char* lb = lab + (long long)head * LB;           // on a 16-byte boundary
  const Second second(sec, head);
  [[maybe_unused]] const Third third(thi, head);
  for (long long base = (long long)blockIdx.x * 256 + wave * 64; base < groups; base += (long long)gridDim.x * 256) {
    const long long g = base + lane;
    const bool live = g < groups;
    int pv[16] = {};
    T sv[16] = {};
    [[maybe_unused]] U tv[three ? 16 : 1] = {};
    if (live) {
      load16<LB>(lb + g * (16 * LB), 0, pv);
      second.group(g, sv);
      if constexpr (three) third.group(g, tv);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if constexpr (three) f(pv[i], sv[i], tv[i], live);
      else f(pv[i], sv[i], live);
    }
  }
}

// the host's side of the walk: the pixels in front of the labels' first 16-byte boundary, whole groups of 16, the rest, and
// the workgroups of the launch
struct WalkSplit {
  int head, groups, tail, blocks;
};
inline WalkSplit walk_split(const void* labels, int label_bytes, long long npix) {
  WalkSplit w;
  w.head = (int)std::min<long long>(npix, (long long)((0 - (size_t)labels) & 15) / label_bytes);
  w.groups = (int)((npix - w.head) / 16);
  w.tail = (int)(npix - w.head - 16ll * w.groups);
  w.blocks = std::min(std::max((w.groups + 255) / 256, 1), MAX_BLOCKS);
  return w;
}

// The launch of a counter on the walk (ifseg_seg_areas, _confusion, _conf_hist, _calibration), its one statement.  GT / CONF:
// the counter reads a ground truth / confidences beside the labels.  Refused, as IFSEG_ERR_BAD_ARG: a missing map or counter
// array, an element size other than 1 | 2, a misaligned pointer, n outside [1, max_n]; then, as IFSEG_ERR_BAD_SHAPE, npix
// outside [1, 2^31).  launch(LB, GB, w) starts the kernel of the label / ground-truth element sizes LB() / GB() (a
// std::integral_constant each; GB() = 1 without GT) on the split w
struct WalkMaps {
  const void* labels;
  int label_bytes;
  const void* gt;
  int gt_bytes;
  const float* conf;
};

template <bool GT, bool CONF, typename Launch>
int walk_launch(const WalkMaps& m, const unsigned long long* counts, const unsigned long long* tally, int n, int max_n,
                long long npix, Launch launch) {
  (void)hipGetLastError();
  const int gb = GT ? m.gt_bytes : 1;
  if (!m.labels || (GT && !m.gt) || (CONF && !m.conf) || !counts || !tally) return IFSEG_ERR_BAD_ARG;
  if ((m.label_bytes != 1 && m.label_bytes != 2) || (gb != 1 && gb != 2)) return IFSEG_ERR_BAD_ARG;
  if (((size_t)m.labels & (size_t)(m.label_bytes - 1)) || (GT && ((size_t)m.gt & (size_t)(gb - 1))) ||
      (CONF && ((size_t)m.conf & 3)) || ((size_t)counts & 7) || ((size_t)tally & 7))
    return IFSEG_ERR_BAD_ARG;
  if (n < 1 || n > max_n) return IFSEG_ERR_BAD_ARG;
  if (npix < 1 || npix >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  const WalkSplit w = walk_split(m.labels, m.label_bytes, npix);
  using B1 = std::integral_constant<int, 1>;
  using B2 = std::integral_constant<int, 2>;
  if (m.label_bytes == 1 && gb == 1) launch(B1{}, B1{}, w);
  else if (m.label_bytes == 1) launch(B1{}, B2{}, w);
  else if (gb == 1) launch(B2{}, B1{}, w);
  else launch(B2{}, B2{}, w);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

// ---- the table ----
// The keyed counts of one workgroup, behind bin_add's wave pre-aggregation (table_add); one of two, chosen by the host:
//   direct   uint32 [dwords] in LDS, the key its index
//   hashed   SLOTS keys (EMPTY = free) and SLOTS counts.  A key takes the first slot of its PROBES-long probe sequence that is
//            free (claimed by an LDS compare-and-swap) or already its own; a key that finds none adds to the global table
//            directly, so the result never depends on the table's size
// A workgroup sees fewer than 2^31 pixels in all (npix < 2^31), so no uint32 count wraps.  After a barrier every non-zero
// bin / claimed slot leaves as one 64-bit atomic; a workgroup never walks the global table.
constexpr int SLOT_BITS = 12;
constexpr int SLOTS = 1 << SLOT_BITS;           // slots of the hashed regime (4096): 32 KiB of keys and counts
constexpr int PROBES = 16;
constexpr uint32_t EMPTY = 0xffffffffu;         // no key: keys are below 512 * 513

// keys empty, counts 0, and the barrier that publishes them
__device__ __forceinline__ void table_zero(uint32_t* tab, bool hashed, int dwords) {
  const int keys = hashed ? SLOTS : 0;
  for (int i = threadIdx.x; i < dwords; i += 256) tab[i] = i < keys ? EMPTY : 0u;
  __syncthreads();
}

// cnt pixels of `key` into the workgroup's table, or past a crowded hashed table into the global one itself
__device__ __forceinline__ void table_count(uint32_t* tab, bool hashed, uint32_t key, uint32_t cnt, unsigned long long* global) {
  if (!hashed) {
    atomicAdd(&tab[key], cnt);
    return;
  }
  uint32_t s = (key * 2654435761u) >> (32 - SLOT_BITS);           // Fibonacci hashing to a slot
  for (int probe = 0; probe < PROBES; ++probe, s = (s + 1) & (SLOTS - 1)) {
    const uint32_t was = atomicCAS(&tab[s], EMPTY, key);
    if (was == EMPTY || was == key) {
      atomicAdd(&tab[SLOTS + s], cnt);
      return;
    }
  }
  atomicAdd(&global[key], (unsigned long long)cnt);
}

// bin_add for a key: the lanes that share the first active lane's key leave as one table_count of their number, the others
// one each; whole (converged) waves call it
__device__ __forceinline__ void table_add(uint32_t* tab, bool hashed, int key, bool on, unsigned long long* global) {
  const unsigned long long m = __ballot(on);
  if (!m) return;
  const int lead = __ffsll((long long)m) - 1;
  const int first = __builtin_amdgcn_readlane(key, lead);
  const unsigned long long same = __ballot(on && key == first);
  if ((int)(threadIdx.x & 63) == lead) table_count(tab, hashed, (uint32_t)first, (uint32_t)__popcll(same), global);
  else if (on && key != first) table_count(tab, hashed, (uint32_t)key, 1u, global);
}

// a barrier, and every non-zero bin / claimed slot leaves
__device__ __forceinline__ void table_flush(uint32_t* tab, bool hashed, int dwords, unsigned long long* global) {
  __syncthreads();
  if (hashed) {
    for (int i = threadIdx.x; i < SLOTS; i += 256) {
      const uint32_t key = tab[i];
      if (key != EMPTY) atomicAdd(&global[key], (unsigned long long)tab[SLOTS + i]);
    }
  } else {
    for (int i = threadIdx.x; i < dwords; i += 256) {
      const uint32_t v = tab[i];
      if (v) atomicAdd(&global[i], (unsigned long long)v);
    }
  }
}

// ---- the tallies ----
// A thread's pair of tallies, kept in registers over the walk or the tile.  Summed over the wave, they leave as two 64-bit
// atomics where the table is keyed or fills the LDS budget (tally_flush) ...
__device__ __forceinline__ void wave_tallies(int& a, int& b) {
#pragma unroll
  for (int o = 32; o; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
}
__device__ __forceinline__ void tally_flush(int a, int b, unsigned long long* tally) {
  wave_tallies(a, b);
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&tally[0], (unsigned long long)a);
    if (b) atomicAdd(&tally[1], (unsigned long long)b);
  }
}

// ... or join a direct table of `bins` plain bins as two more (tab holds bins + 2 dwords); then a barrier, and the non-zero
// bins leave to counts[bins] / tally[2]: one 64-bit atomic per workgroup and bin
__device__ __forceinline__ void bins_flush(uint32_t* tab, int bins, int a, int b, unsigned long long* counts,
                                           unsigned long long* tally) {
  wave_tallies(a, b);
  if ((threadIdx.x & 63) == 0) {
    if (a) atomicAdd(&tab[bins], (uint32_t)a);
    if (b) atomicAdd(&tab[bins + 1], (uint32_t)b);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < bins + 2; i += 256) {
    const uint32_t v = tab[i];
    if (v) atomicAdd(i < bins ? counts + i : tally + (i - bins), (unsigned long long)v);
  }
}

}  // namespace count
