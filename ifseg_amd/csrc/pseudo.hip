// Confidence-filtered pseudo-labels on gfx950 (ifseg_amd/predict.py Segmenter.pseudo_label_raw): what lies between a predicted
// label map with its confidences and the raw label map ifseg_train_load takes, for self-training on unlabeled photographs.
// Two kernels, integers throughout; include/ifseg_hip.h states the rules and predict.py's confidence_histogram_reference /
// pseudo_label_reference are the specifications.
//
//   seg_conf_hist_kernel   hist[label][bin(conf)] over a label map of any length: count.h's walk with the confidences as its
//                          second stream -- 256 lanes x 16 pixels per step, grid-stride -- into count.h's workgroup-private
//                          table, direct up to n = 64, hashed above; the two tallies leave by wave (tally_flush), and the
//                          host's side is count.h's walk_launch
//   seg_pseudo_kernel      one 16 x 64 tile (tile.h) per workgroup: labels plus a halo of r (tile.h's halo_stage /
//                          halo_differs), the thresholds staged, lane = x reads its own conf and stores its own byte
// Both are bandwidth- and launch-bound: 5 B (hist) and 6 B (filter) per pixel, no arithmetic to speak of.
#include "count.h"
#include "tile.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using namespace count;

// ---- the histogram ----
// key = label * 256 + bin (count.h's conf_bin), below 512 * 256, into count.h's table: direct (uint32 [n][256] in LDS, 64 KiB at n = 64) up to
// HC_DIRECT_CLASSES, hashed above.  The two tallies stay in registers and leave per wave (the direct table at n = 64 fills
// the LDS budget).
constexpr int HC_MAX_CLASSES = 512;
constexpr int HC_DIRECT_CLASSES = 64;

__host__ __device__ inline bool hc_hashed(int n) { return n > HC_DIRECT_CLASSES; }
__host__ __device__ inline int hc_dwords(int n) { return hc_hashed(n) ? 2 * SLOTS : n * 256; }

template <int LB>
__global__ __launch_bounds__(256) void seg_conf_hist_kernel(const unsigned char* __restrict__ lab, const float* __restrict__ conf,
                                                            int head, int groups, int tail, int n,
                                                            unsigned long long* hist, unsigned long long* tally) {
  extern __shared__ __attribute__((aligned(16))) uint32_t htab[];  // hc_dwords(n)
  const bool hashed = hc_hashed(n);                                // uniform over the grid
  const int dwords = hc_dwords(n);
  table_zero(htab, hashed, dwords);

  int inside = 0, outside = 0;
  walk_pixels<LB, FloatStream>(lab, conf, head, groups, tail, [&](int l, float c, bool live) {
    const bool in = live && (unsigned)l < (unsigned)n;
    inside += in;
    outside += live && !in;
    table_add(htab, hashed, in ? l * 256 + conf_bin(c) : 0, in, hist);
  });

  tally_flush(inside, outside, tally);
  table_flush(htab, hashed, dwords, hist);
}

// ---- the filter ----
constexpr int PL_MAX_CLASSES = 255;

template <typename L>
__global__ __launch_bounds__(256) void seg_pseudo_kernel(const L* __restrict__ labels, const float* __restrict__ conf,
                                                         const int* __restrict__ thresholds, int n, int H, int W, int r, int raw,
                                                         unsigned char* __restrict__ out, unsigned long long* kept, int tiles_x,
                                                         int tiles_y, unsigned char* __restrict__ weight) {
  __shared__ short halo[HALO_H * HALO_W];
  __shared__ int thr[PL_MAX_CLASSES];
  __shared__ uint32_t ktab[2 * PL_MAX_CLASSES];                   // [0, n) kept, [n, 2 n) predicted
  const Tile t = tile_decode(tiles_x, tiles_y, H, W);
  const long long pix0 = (long long)t.b * H * W;                  // B H W < 2^31
  const int rows = t.yend - t.Y0, cols = t.xend - t.X0;

  // phase 0
  for (int c = threadIdx.x; c < n; c += 256) thr[c] = thresholds[c];
  for (int c = threadIdx.x; c < 2 * n; c += 256) ktab[c] = 0u;
  halo_stage(labels, pix0, t, H, W, r, halo);
  __syncthreads();

  // phase 1: lane = x, a wave takes 4 rows; the two bin_adds are reached by whole waves
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int ry = t.wave * 4 + j;
    const bool ok = ry < rows && t.lane < cols;
    int l = 0;
    bool in = false, keep = false;
    if (ok) {
      l = halo_label(halo, ry, t.lane, r);
      in = (unsigned)l < (unsigned)n;
      const long long p = pix0 + (long long)(t.Y0 + ry) * W + t.X0 + t.lane;
      int bin = 0;
      if (in) {
        bin = conf_bin(conf[p]);
        keep = !halo_differs(halo, ry, t.lane, r, l) && bin >= thr[l];
      }
      out[p] = keep ? (unsigned char)(l + raw) : (unsigned char)255;
      // the loss weight of the pixel (ifseg_seg_loss_tiles_weighted): its confidence bin, at least 1 where it is kept
      if (weight) weight[p] = keep ? (unsigned char)max(bin, 1) : (unsigned char)0;
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
  return walk_launch<false, true>({labels, label_bytes, nullptr, 0, conf}, hist, tally, n, HC_MAX_CLASSES, npix,
                                  [&](auto LB, auto, const WalkSplit& w) {
    hipLaunchKernelGGL(seg_conf_hist_kernel<LB()>, dim3(w.blocks), dim3(256), hc_dwords(n) * 4, (hipStream_t)stream,
                       (const unsigned char*)labels, conf, w.head, w.groups, w.tail, n, hist, tally);
  });
}

namespace {
int seg_pseudo_launch(const void* labels, int label_bytes, const float* conf, const int* thresholds, int n, int B, int H, int W,
                      int boundary, int raw_labels, void* out, unsigned long long* kept, unsigned char* weight, void* stream) {
  (void)hipGetLastError();
  if (!labels || !conf || !thresholds || !out || !kept || (label_bytes != 1 && label_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if ((label_bytes == 2 && ((size_t)labels & 1)) || ((size_t)conf & 3) || ((size_t)thresholds & 3) || ((size_t)kept & 7))
    return IFSEG_ERR_BAD_ARG;
  if (n < 1 || n > (raw_labels ? PL_MAX_CLASSES - 1 : PL_MAX_CLASSES) || boundary < 0 || boundary > HALO_MAX_R) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || H < 1 || W < 1 || (long long)B * H * W >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(H, W, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  const int raw = raw_labels ? 1 : 0;
  if (label_bytes == 1)
    hipLaunchKernelGGL(seg_pseudo_kernel<unsigned char>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)labels, conf, thresholds, n, H, W, boundary, raw, (unsigned char*)out, kept, tiles_x,
                       tiles_y, weight);
  else
    hipLaunchKernelGGL(seg_pseudo_kernel<short>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const short*)labels,
                       conf, thresholds, n, H, W, boundary, raw, (unsigned char*)out, kept, tiles_x, tiles_y, weight);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int ifseg_seg_pseudo(const void* labels, int label_bytes, const float* conf, const int* thresholds, int n, int B, int H,
                                int W, int boundary, int raw_labels, void* out, unsigned long long* kept, void* stream) {
  return seg_pseudo_launch(labels, label_bytes, conf, thresholds, n, B, H, W, boundary, raw_labels, out, kept, nullptr, stream);
}

extern "C" int ifseg_seg_pseudo_weighted(const void* labels, int label_bytes, const float* conf, const int* thresholds, int n,
                                         int B, int H, int W, int boundary, int raw_labels, void* out, void* weight,
                                         unsigned long long* kept, void* stream) {
  if (!weight || weight == out) return IFSEG_ERR_BAD_ARG;
  return seg_pseudo_launch(labels, label_bytes, conf, thresholds, n, B, H, W, boundary, raw_labels, out, kept,
                           (unsigned char*)weight, stream);
}
