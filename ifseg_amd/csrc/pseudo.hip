// Confidence-filtered pseudo-labels on gfx950 (ifseg_amd/predict.py Segmenter.pseudo_label_raw): what lies between a predicted
// label map with its confidences and the raw label map ifseg_train_load takes, for self-training on unlabeled photographs.
// Two kernels, integers throughout; include/ifseg_hip.h states the rules and predict.py's confidence_histogram_reference /
// pseudo_label_reference are the specifications.
//
//   seg_conf_hist_kernel   hist[label][bin(conf)] over a label map of any length: the input walk of seg_areas_kernel /
//                          seg_confusion_kernel (predict.hip; a private copy, so that file compiles to what it did) -- 256 lanes
//                          x 16 pixels per step, grid-stride over at most HC_MAX_BLOCKS workgroups -- into a workgroup-private
//                          LDS table, direct up to n = 64, hashed above (seg_confusion_kernel's scheme)
//   seg_pseudo_kernel      one 16 x 64 tile (tile.h) per workgroup: labels plus a halo of r staged as in render.hip phase 0,
//                          the thresholds staged, lane = x reads its own conf and stores its own byte
// Both are bandwidth- and launch-bound: 5 B (hist) and 6 B (filter) per pixel, no arithmetic to speak of.
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;

// bin(conf) = clamp(floor(conf * 256), 0, 255): the product is exact (a power of two), NaN -> 0 by fmaxf(NaN, 0) = 0
__device__ __forceinline__ int conf_bin(float conf) {
  return (int)fminf(fmaxf(floorf(__fmul_rn(conf, 256.f)), 0.f), 255.f);
}

// tab[idx] += 1 for every lane with `on`; whole (converged) waves call it.  The lanes that share the first active lane's index
// leave as one add of their count, the others one each (predict.hip's bin_add)
__device__ __forceinline__ void bin_add(uint32_t* tab, int idx, bool on) {
  const unsigned long long m = __ballot(on);
  if (!m) return;
  const int lead = __ffsll((long long)m) - 1;
  const int first = __builtin_amdgcn_readlane(idx, lead);
  const unsigned long long same = __ballot(on && idx == first);
  if ((int)(threadIdx.x & 63) == lead) atomicAdd(&tab[first], (uint32_t)__popcll(same));
  else if (on && idx != first) atomicAdd(&tab[idx], 1u);
}

// ---- the histogram ----
// key = label * 256 + bin, below 512 * 256.  The table of a workgroup is one of two, chosen by the host:
//   direct   n <= HC_DIRECT_CLASSES: uint32 [n][256] in LDS (64 KiB at n = 64), the key its index
//   hashed   HC_SLOTS keys (HC_EMPTY = free) and HC_SLOTS counts.  A key takes the first slot of its HC_PROBES-long probe
//            sequence that is free (claimed by an LDS compare-and-swap) or already its own; a key that finds none adds to
//            the global histogram directly, so the result never depends on the table's size
// A workgroup sees fewer than 2^31 pixels, so no uint32 count wraps.  After a barrier every non-zero bin / claimed slot leaves
// as one 64-bit atomic.  The two tallies stay in registers and leave per wave (the direct table at n = 64 fills the LDS budget).
constexpr int HC_MAX_CLASSES = 512;
constexpr int HC_DIRECT_CLASSES = 64;
constexpr int HC_SLOT_BITS = 12;
constexpr int HC_SLOTS = 1 << HC_SLOT_BITS;
constexpr int HC_PROBES = 16;
constexpr int HC_MAX_BLOCKS = 512;
constexpr uint32_t HC_EMPTY = 0xffffffffu;

inline bool hc_hashed(int n) { return n > HC_DIRECT_CLASSES; }
inline int hc_dwords(int n) { return hc_hashed(n) ? 2 * HC_SLOTS : n * 256; }

__device__ __forceinline__ void pair_count(uint32_t* tab, bool hashed, uint32_t key, uint32_t cnt, unsigned long long* hist) {
  if (!hashed) {
    atomicAdd(&tab[key], cnt);
    return;
  }
  uint32_t s = (key * 2654435761u) >> (32 - HC_SLOT_BITS);        // Fibonacci hashing to a slot
  for (int probe = 0; probe < HC_PROBES; ++probe, s = (s + 1) & (HC_SLOTS - 1)) {
    const uint32_t was = atomicCAS(&tab[s], HC_EMPTY, key);
    if (was == HC_EMPTY || was == key) {
      atomicAdd(&tab[HC_SLOTS + s], cnt);
      return;
    }
  }
  atomicAdd(&hist[key], (unsigned long long)cnt);
}

// bin_add for a pair; whole (converged) waves call it
__device__ __forceinline__ void pair_add(uint32_t* tab, bool hashed, int key, bool on, unsigned long long* hist) {
  const unsigned long long m = __ballot(on);
  if (!m) return;
  const int lead = __ffsll((long long)m) - 1;
  const int first = __builtin_amdgcn_readlane(key, lead);
  const unsigned long long same = __ballot(on && key == first);
  if ((int)(threadIdx.x & 63) == lead) pair_count(tab, hashed, (uint32_t)first, (uint32_t)__popcll(same), hist);
  else if (on && key != first) pair_count(tab, hashed, (uint32_t)key, 1u, hist);
}

template <int LB>
__device__ __forceinline__ int label_at(const unsigned char* p, long long i) {
  return LB == 1 ? (int)p[i] : (int)((const short*)p)[i];
}

// 16 labels from the 16-byte boundary p: LB aligned chunks
template <int LB>
__device__ __forceinline__ void labels16(const unsigned char* p, int (&v)[16]) {
  uint32_t w[4 * LB];
#pragma unroll
  for (int c = 0; c < LB; ++c) {
    const uint4 q = *reinterpret_cast<const uint4*>(p + 16 * c);
    w[4 * c] = q.x; w[4 * c + 1] = q.y; w[4 * c + 2] = q.z; w[4 * c + 3] = q.w;
  }
#pragma unroll
  for (int i = 0; i < 16; ++i)
    v[i] = LB == 1 ? (int)((w[i >> 2] >> (8 * (i & 3))) & 255u) : (int)(short)(w[i >> 1] >> (16 * (i & 1)));
}

// four floats at a 4-byte boundary
struct __attribute__((packed, aligned(4))) Float4A4 {
  float v[4];
};

// The walk: the pixels in front of the labels' first 16-byte boundary (head) and behind the last whole group of 16 (tail),
// fewer than 16 each, go to lanes 0..15 and 16..31 of the grid's first wave, one pixel each; the groups of 16 to the lanes,
// grid-stride.  A group's 16 confidences sit at a 4-byte boundary: four loads of 16 bytes.
template <int LB>
__global__ __launch_bounds__(256) void seg_conf_hist_kernel(const unsigned char* __restrict__ lab, const float* __restrict__ conf,
                                                            int head, int groups, int tail, int n, int hashed_,
                                                            unsigned long long* hist, unsigned long long* tally) {
  extern __shared__ __attribute__((aligned(16))) uint32_t htab[];  // hc_dwords(n)
  const bool hashed = hashed_ != 0;                                // uniform over the grid
  const int keys = hashed ? HC_SLOTS : 0, dwords = hashed ? 2 * HC_SLOTS : n * 256;
  for (int i = threadIdx.x; i < dwords; i += 256) htab[i] = i < keys ? HC_EMPTY : 0u;
  __syncthreads();

  int inside = 0, outside = 0;
  auto pixel = [&](int l, float c, bool live) {
    const bool in = live && (unsigned)l < (unsigned)n;
    inside += in;
    outside += live && !in;
    pair_add(htab, hashed, in ? l * 256 + conf_bin(c) : 0, in, hist);
  };
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (blockIdx.x == 0 && wave == 0) {
    long long i = -1;
    if (lane < head) i = lane;
    else if (lane >= 16 && lane - 16 < tail) i = (long long)head + (long long)groups * 16 + (lane - 16);
    const bool live = i >= 0;
    pixel(live ? label_at<LB>(lab, i) : 0, live ? conf[i] : 0.f, live);
  }
  const unsigned char* lb = lab + (long long)head * LB;           // on a 16-byte boundary
  const float* cb = conf + head;
  for (long long base = (long long)blockIdx.x * 256 + wave * 64; base < groups; base += (long long)gridDim.x * 256) {
    const long long g = base + lane;
    const bool live = g < groups;
    int lv[16] = {};
    float cv[16] = {};
    if (live) {
      labels16<LB>(lb + g * (16 * LB), lv);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const Float4A4 f = *reinterpret_cast<const Float4A4*>(cb + g * 16 + 4 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) cv[4 * q + e] = f.v[e];
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) pixel(lv[i], cv[i], live);
  }

#pragma unroll
  for (int o = 32; o; o >>= 1) { inside += __shfl_xor(inside, o); outside += __shfl_xor(outside, o); }
  if (lane == 0) {
    if (inside) atomicAdd(&tally[0], (unsigned long long)inside);
    if (outside) atomicAdd(&tally[1], (unsigned long long)outside);
  }
  __syncthreads();
  if (hashed) {
    for (int i = threadIdx.x; i < HC_SLOTS; i += 256) {
      const uint32_t key = htab[i];
      if (key != HC_EMPTY) atomicAdd(&hist[key], (unsigned long long)htab[HC_SLOTS + i]);
    }
  } else {
    for (int i = threadIdx.x; i < dwords; i += 256) {
      const uint32_t v = htab[i];
      if (v) atomicAdd(&hist[i], (unsigned long long)v);
    }
  }
}

// ---- the filter ----
constexpr int MAX_R = 4, PL_MAX_CLASSES = 255;
constexpr int HALO_W = TILE_COLS + 2 * MAX_R, HALO_H = TILE_ROWS + 2 * MAX_R;

template <typename L>
__global__ __launch_bounds__(256) void seg_pseudo_kernel(const L* __restrict__ labels, const float* __restrict__ conf,
                                                         const int* __restrict__ thresholds, int n, int H, int W, int r, int raw,
                                                         unsigned char* __restrict__ out, unsigned long long* kept, int tiles_x,
                                                         int tiles_y) {
  __shared__ short halo[HALO_H * HALO_W];
  __shared__ int thr[PL_MAX_CLASSES];
  __shared__ uint32_t ktab[2 * PL_MAX_CLASSES];                   // [0, n) kept, [n, 2 n) predicted
  const Tile t = tile_decode(tiles_x, tiles_y, H, W);
  const long long pix0 = (long long)t.b * H * W;                  // B H W < 2^31
  const int rows = t.yend - t.Y0, cols = t.xend - t.X0;

  // phase 0
  for (int c = threadIdx.x; c < n; c += 256) thr[c] = thresholds[c];
  for (int c = threadIdx.x; c < 2 * n; c += 256) ktab[c] = 0u;
  const int hw = TILE_COLS + 2 * r;
  for (int i = threadIdx.x; i < (TILE_ROWS + 2 * r) * hw; i += 256) {
    const int hy = i / hw, hx = i - hy * hw;
    // a neighbour outside the image reads the nearest pixel inside, which lies in the same window: it adds no edge
    const int y = min(max(t.Y0 - r + hy, 0), H - 1), x = min(max(t.X0 - r + hx, 0), W - 1);
    halo[hy * HALO_W + hx] = (short)labels[pix0 + (long long)y * W + x];
  }
  __syncthreads();

  // phase 1: lane = x, a wave takes 4 rows; the two bin_adds are reached by whole waves
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ry = t.wave * 4 + j;
    const bool ok = ry < rows && t.lane < cols;
    int l = 0;
    bool in = false, keep = false;
    if (ok) {
      l = halo[(ry + r) * HALO_W + t.lane + r];
      in = (unsigned)l < (unsigned)n;
      const long long p = pix0 + (long long)(t.Y0 + ry) * W + t.X0 + t.lane;
      if (in) {
        bool edge = false;
        for (int dy = 0; dy <= 2 * r; ++dy)
          for (int dx = 0; dx <= 2 * r; ++dx) edge |= halo[(ry + dy) * HALO_W + t.lane + dx] != l;
        keep = !edge && conf_bin(conf[p]) >= thr[l];
      }
      out[p] = keep ? (unsigned char)(l + raw) : (unsigned char)255;
    }
    bin_add(ktab, n + l, in);
    bin_add(ktab, l, keep);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * n; i += 256) {
    const uint32_t v = ktab[i];
    if (v) atomicAdd(&kept[i], (unsigned long long)v);
  }
}

}  // namespace

extern "C" int ifseg_seg_conf_hist(const void* labels, int label_bytes, const float* conf, long long npix, int n,
                                   unsigned long long* hist, unsigned long long* tally, void* stream) {
  (void)hipGetLastError();
  if (!labels || !conf || !hist || !tally || (label_bytes != 1 && label_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if ((label_bytes == 2 && ((size_t)labels & 1)) || ((size_t)conf & 3) || ((size_t)hist & 7) || ((size_t)tally & 7))
    return IFSEG_ERR_BAD_ARG;
  if (n < 1 || n > HC_MAX_CLASSES) return IFSEG_ERR_BAD_ARG;
  if (npix < 1 || npix >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  // the pixels in front of the labels' first 16-byte boundary, whole groups of 16, the rest
  const int head = (int)std::min<long long>(npix, (long long)((0 - (size_t)labels) & 15) / label_bytes);
  const int groups = (int)((npix - head) / 16);
  const int tail = (int)(npix - head - 16ll * groups);
  const int blocks = std::min(std::max((groups + 255) / 256, 1), HC_MAX_BLOCKS);
  const int hashed = hc_hashed(n) ? 1 : 0, lds = hc_dwords(n) * 4;
  const unsigned char* l = (const unsigned char*)labels;
  if (label_bytes == 1)
    hipLaunchKernelGGL(seg_conf_hist_kernel<1>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, l, conf, head, groups, tail, n,
                       hashed, hist, tally);
  else
    hipLaunchKernelGGL(seg_conf_hist_kernel<2>, dim3(blocks), dim3(256), lds, (hipStream_t)stream, l, conf, head, groups, tail, n,
                       hashed, hist, tally);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_pseudo(const void* labels, int label_bytes, const float* conf, const int* thresholds, int n, int B, int H,
                                int W, int boundary, int raw_labels, void* out, unsigned long long* kept, void* stream) {
  (void)hipGetLastError();
  if (!labels || !conf || !thresholds || !out || !kept || (label_bytes != 1 && label_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if ((label_bytes == 2 && ((size_t)labels & 1)) || ((size_t)conf & 3) || ((size_t)thresholds & 3) || ((size_t)kept & 7))
    return IFSEG_ERR_BAD_ARG;
  if (n < 1 || n > (raw_labels ? PL_MAX_CLASSES - 1 : PL_MAX_CLASSES) || boundary < 0 || boundary > MAX_R) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(H, W, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const int raw = raw_labels ? 1 : 0;
  if (label_bytes == 1)
    hipLaunchKernelGGL(seg_pseudo_kernel<unsigned char>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)labels, conf, thresholds, n, H, W, boundary, raw, (unsigned char*)out, kept, tiles_x,
                       tiles_y);
  else
    hipLaunchKernelGGL(seg_pseudo_kernel<short>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const short*)labels,
                       conf, thresholds, n, H, W, boundary, raw, (unsigned char*)out, kept, tiles_x, tiles_y);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
