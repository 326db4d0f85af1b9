// Confidence calibration on gfx950 (ifseg_amd/predict.py Segmenter.evaluate_raw(calibration=True)): "when the model says 0.9, is
// it right 90 % of the time?" -- the counts behind the reliability diagram and ECE (Guo et al., ICML 2017), per predicted class.
// One kernel, integers throughout; include/ifseg_hip.h states the rule and predict.py's calibration_reference is the
// specification.
//
//   seg_calibration_kernel   calibration[label][bin(conf)][label == gt class] over the scored pixels of a label map of any
//                            length: seg_conf_hist_kernel's walk with the ground truth as a third stream (count.h's
//                            walk_pixels) -- 256 lanes x 16 pixels per step, grid-stride -- into count.h's workgroup-private
//                            table, direct up to n = 32, hashed above; the two tallies leave by wave (tally_flush),
//                            and the host's side is count.h's walk_launch
// Bandwidth- and launch-bound: 6 B per pixel (8 with int16 maps), no arithmetic to speak of.  The direct table at n = 32 is
// the whole 64 KiB LDS budget of the project, so two workgroups share a CU's 160 KiB there; the walk has no barrier between
// table_zero and table_flush, and its LDS atomics are one per wave and step on a piecewise-constant map (table_add).
#include "count.h"

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
  walk_pixels<LB, FloatStream, MapStream<GB>>(lab, conf, head, groups, tail, [&](int l, float c, int g, bool live) {
    const GtClass t = gt_class(n, raw, g, live);
    const bool in = t.sc && (unsigned)l < (unsigned)n;
    inside += in;
    outside += t.sc && !in;
    table_add(btab, hashed, in ? (l * 256 + conf_bin(c)) * 2 + (l == t.cls ? 1 : 0) : 0, in, calibration);
  }, gt);

  tally_flush(inside, outside, tally);
  table_flush(btab, hashed, dwords, calibration);
}

}  // namespace

extern "C" int ifseg_seg_calibration(const void* labels, int label_bytes, const float* conf, const void* gt, int gt_bytes,
                                     long long npix, int n, int raw_labels, unsigned long long* calibration,
                                     unsigned long long* tally, void* stream) {
  return walk_launch<true, true>({labels, label_bytes, gt, gt_bytes, conf}, calibration, tally, n, CB_MAX_CLASSES, npix,
                                 [&](auto LB, auto GB, const WalkSplit& w) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_calibration_kernel<LB(), GB()>), dim3(w.blocks), dim3(256),
                       (size_t)cb_dwords(n) * sizeof(uint32_t), (hipStream_t)stream, (const unsigned char*)labels, conf,
                       (const unsigned char*)gt, w.head, w.groups, w.tail, n, raw_labels != 0, calibration, tally);
  });
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
