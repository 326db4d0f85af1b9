// Confidence calibration on gfx950 (ifseg_amd/predict.py Segmenter.evaluate_raw(calibration=True)): "when the model says 0.9, is
// it right 90 % of the time?" -- the counts behind the reliability diagram and ECE (Guo et al., ICML 2017), per predicted class.
// One kernel, integers throughout; include/ifseg_hip.h states the rule and predict.py's calibration_reference is the
// specification.
//
//   seg_calibration_kernel   calibration[label][bin(conf)][label == gt class] over the scored pixels of a label map of any
//                            length: seg_conf_hist_kernel's walk with the ground truth as a third stream (count.h's
//                            walk_pixels3) -- 256 lanes x 16 pixels per step, grid-stride -- into count.h's workgroup-private
//                            table, direct up to n = 32, hashed above
// Bandwidth- and launch-bound: 6 B per pixel (8 with int16 maps), no arithmetic to speak of.  The direct table at n = 32 is
// the whole 64 KiB LDS budget of the project, so two workgroups share a CU's 160 KiB there; the walk has no barrier between
// table_zero and table_flush, and its LDS atomics are one per wave and step on a piecewise-constant map (table_add).
#include "count.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace count;

// key = (label * 256 + bin) * 2 + hit, below 512 * 512 (so EMPTY stays free), into count.h's table: direct (uint32 [n][256][2]
// in LDS, 64 KiB at n = 32) up to CB_DIRECT_CLASSES, hashed above.  The two tallies stay in registers and leave per wave.
constexpr int CB_MAX_CLASSES = 512;
constexpr int CB_DIRECT_CLASSES = 32;
constexpr int CB_STEP_PIXELS = 256 * 16;  // the pixels a workgroup takes per step of the walk

__host__ __device__ inline bool cb_hashed(int n) { return n > CB_DIRECT_CLASSES; }
__host__ __device__ inline int cb_dwords(int n) { return cb_hashed(n) ? 2 * SLOTS : n * 512; }

template <int LB, int GB>
__global__ __launch_bounds__(256) void seg_calibration_kernel(const unsigned char* __restrict__ lab, const float* __restrict__ conf,
                                                              const unsigned char* __restrict__ gt, int head, int groups, int tail,
                                                              int n, int raw, unsigned long long* calibration,
                                                              unsigned long long* tally) {
  extern __shared__ __attribute__((aligned(16))) uint32_t btab[];  // cb_dwords(n)
  const bool hashed = cb_hashed(n);                                // uniform over the grid
  const int dwords = cb_dwords(n);
  table_zero(btab, hashed, dwords);

  int inside = 0, outside = 0;
  walk_pixels3<LB, FloatStream, MapStream<GB>>(lab, conf, gt, head, groups, tail, [&](int l, float c, int g, bool live) {
    const GtClass t = gt_class(n, raw, g, live);
    const bool in = t.sc && (unsigned)l < (unsigned)n;
    inside += in;
    outside += t.sc && !in;
    table_add(btab, hashed, in ? (l * 256 + conf_bin(c)) * 2 + (l == t.cls ? 1 : 0) : 0, in, calibration);
  });

#pragma unroll
  for (int o = 32; o; o >>= 1) { inside += __shfl_xor(inside, o); outside += __shfl_xor(outside, o); }
  if ((threadIdx.x & 63) == 0) {
    if (inside) atomicAdd(&tally[0], (unsigned long long)inside);
    if (outside) atomicAdd(&tally[1], (unsigned long long)outside);
  }
  table_flush(btab, hashed, dwords, calibration);
}

}  // namespace

extern "C" int ifseg_seg_calibration(const void* labels, int label_bytes, const float* conf, const void* gt, int gt_bytes,
                                     long long npix, int n, int raw_labels, unsigned long long* calibration,
                                     unsigned long long* tally, void* stream) {
  (void)hipGetLastError();
  if (!labels || !conf || !gt || !calibration || !tally) return IFSEG_ERR_BAD_ARG;
  if ((label_bytes != 1 && label_bytes != 2) || (gt_bytes != 1 && gt_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if (((size_t)labels & (size_t)(label_bytes - 1)) || ((size_t)gt & (size_t)(gt_bytes - 1)) || ((size_t)conf & 3) ||
      ((size_t)calibration & 7) || ((size_t)tally & 7))
    return IFSEG_ERR_BAD_ARG;
  if (n < 1 || n > CB_MAX_CLASSES) return IFSEG_ERR_BAD_ARG;
  if (npix < 1 || npix >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  const WalkSplit w = walk_split(labels, label_bytes, npix);
  const size_t lds = (size_t)cb_dwords(n) * sizeof(uint32_t);
  const unsigned char* l = (const unsigned char*)labels;
  const unsigned char* g = (const unsigned char*)gt;
  const int raw = raw_labels != 0;
#define IFSEG_CALIBRATION(LB, GB)                                                                                            \
  hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_calibration_kernel<LB, GB>), dim3(w.blocks), dim3(256), lds, (hipStream_t)stream, l, \
                     conf, g, w.head, w.groups, w.tail, n, raw, calibration, tally)
  if (label_bytes == 1 && gt_bytes == 1) IFSEG_CALIBRATION(1, 1);
  else if (label_bytes == 1) IFSEG_CALIBRATION(1, 2);
  else if (gt_bytes == 1) IFSEG_CALIBRATION(2, 1);
  else IFSEG_CALIBRATION(2, 2);
#undef IFSEG_CALIBRATION
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_seg_calibration_limit(int which) {
  switch (which) {
    case 0: return CB_DIRECT_CLASSES;
    case 1: return SLOTS;
    case 2: return CB_STEP_PIXELS;
    case 3: return MAX_BLOCKS;
    default: return IFSEG_ERR_BAD_ARG;
  }
}
