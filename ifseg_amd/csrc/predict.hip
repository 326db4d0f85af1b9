// Label maps at image resolution (the inference path of ifseg_amd/predict.py): bilinear resize of the per-patch class
// scores [B, hp*wp, n] to [B, h, w] (align_corners=False, any ratio -- the value rule of seg_eval_kernel in evalops.hip),
// argmax over the classes (first maximum), optionally the winning value and every interpolated value, in one pass: the
// [n, h, w] tensor is only written when the caller asks for it.
//
// A workgroup of 256 threads owns a tile of 16 rows x 64 pixels (the tile decode, the coordinate rule and the footprint on top of
// it are tile.h's).
//   phase 0  the patch rows the tile touches (3 x 6 patches at x16) are copied to LDS once, each padded to a stride of an ODD
//            number of 16-byte slots: the 16 slots of a bank row then hold 16 consecutive patches, so lanes of one ds_read_b128
//            that sit in different patches hit different banks for every n (n % 64 == 0 included) and lanes in the same patch
//            read one address (a broadcast).  A tile whose footprint does not fit the staging buffer (strong downscaling, many
//            classes) skips the copy and reads global memory in the same loop.
//   phase 1  lane = x, wave = 4 consecutive rows: y, and with it the two patch rows and the vertical weight, is wave-uniform.
//            The four patch vectors of a class chunk are reloaded only when the row pair changes (at x16: once per chunk for
//            the wave's four rows, three times out of four).  probs leaves here, 256 contiguous bytes per wave and class.
//   phase 2  labels and conf go through a 16 x 64 LDS tile and leave as one dword / dwordx2 / dwordx4 per lane: a lane takes the
//            four pixels of a 4-ALIGNED element quad of the flat [B, h, w] index, so the wide stores are aligned whatever w is;
//            the up to three pixels in front of the first whole quad and behind the last one leave as single elements.
// No atomics, no scratch buffer, static launch shape, nothing read back.
// Three more kernels on the same tile follow it: K views of differing grids (seg_predict_views_kernel), the sliding windows of
// one plane (seg_predict_windows_kernel), and K views of sliding windows (seg_predict_slide_views_kernel).  They walk the
// classes in chunks.  What the kernels share is written once: phase 2 is finish_tile (the views kernel, whose scoring
// instantiation measured slower through it, keeps those lines in place), a view's value add_view; the two sliding kernels
// share the window bookkeeping of a plane under a tile (plane_tile) and a pixel's merged value (slide_pixel).  Two loops
// stay written out in each chunked kernel because as functions they measured slower: the running maximum between the chunks
// (both view kernels) and the staging of a grid (the windows kernel at few classes).  The launchers share their refusals
// and the tile grid (launch_grid), the two sliding ones the check of their windows (make_slide).
//
// Scoring (ifseg_seg_score / ifseg_seg_score_views / ifseg_seg_areas): the same kernels with an epilogue behind a template flag
// that counts the tile's pixels against ground truth -- per class #(pred = gt = c), #(pred = c), #(gt = c) and the two tallies --
// in a workgroup-private uint32 table in LDS (LDS atomics), and a stand-alone kernel that does the same for label maps that come
// from elsewhere.  Only the non-zero bins leave a workgroup, one 64-bit integer atomic each: integer sums, so the counters
// are bit-reproducible.  The instantiations without the flag have none of this.
// The confusion matrix (ifseg_seg_confusion) is a second stand-alone kernel on a label map, seg_confusion_kernel: its table does
// not fit the epilogues' LDS budget.  The wave pre-aggregated add (bin_add), the walk over a flat label map (walk_pixels), the
// direct / hashed workgroup table (table_*), the exit of the epilogues' table with its two tallies (bins_flush) and the host's
// launch path of the two stand-alone kernels (walk_launch) are count.h's, shared with pseudo.hip, calib.hip and tsweep.hip.
#include "count.h"
#include "tile.h"
#include "upsample.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using namespace count;
using namespace upsample;

constexpr int PT_MAX_CLASSES = 512;
constexpr int PT_TILE_LDS = TILE_ROWS * TILE_COLS * 8;            // the label + conf tile of phase 2
constexpr int PT_STAGE_LIMIT = 65536 - PT_TILE_LDS;               // 64 KiB of LDS per workgroup in all

int g_stage_limit = PT_STAGE_LIMIT;

// (pt_stride, Best, blend and blend4 -- the stride of a staged patch, the running first maximum and the flat four-weight value
// of one class, and of four at once -- are upsample.h's, shared with tsweep.hip)

// classes [0, n) of the thread's four pixels (rows j = 0..3 of its wave, one x).  VEC: 16-byte reads of 4 classes (the staged
// rows: stride and base are multiples of 4 floats), else one class per read.  o0 / o1: per-lane offset of the left / right
// patch column, r0[j] / r1[j]: wave-uniform offset of the upper / lower patch row, fresh[j]: row j has another pair than j-1;
// probs: the image's [n, h, w] block (or null), pofs[j]: the pixel's offset in a class plane, cstride = h * w.
template <bool VEC, typename Ptr>
__device__ __forceinline__ void class_loop(Ptr base, int n, int o0, int o1, const long long (&r0)[4], const long long (&r1)[4],
                                           const bool (&fresh)[4], const float (&ly)[4], float lx, Best (&best)[4],
                                           float* probs, const int (&pofs)[4], long long cstride, const bool (&ok)[4]) {
  float w00[4], w01[4], w10[4], w11[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    w00[j] = (1.f - ly[j]) * (1.f - lx); w01[j] = (1.f - ly[j]) * lx; w10[j] = ly[j] * (1.f - lx); w11[j] = ly[j] * lx;
    best[j].v = -INFINITY; best[j].c = 0;
  }
  int c = 0;
  if (VEC) {
    for (; c + 4 <= n; c += 4) {
      f32x4 a, b, d, e;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j == 0 || fresh[j]) {
          a = *reinterpret_cast<const f32x4*>(base + r0[j] + o0 + c);
          b = *reinterpret_cast<const f32x4*>(base + r0[j] + o1 + c);
          d = *reinterpret_cast<const f32x4*>(base + r1[j] + o0 + c);
          e = *reinterpret_cast<const f32x4*>(base + r1[j] + o1 + c);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float v = blend(w00[j], w01[j], w10[j], w11[j], a[k], b[k], d[k], e[k]);
          if (v > best[j].v) { best[j].v = v; best[j].c = c + k; }
          if (probs && ok[j]) probs[(long long)(c + k) * cstride + pofs[j]] = v;
        }
      }
    }
  }
  for (; c < n; ++c) {
    float a, b, d, e;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j == 0 || fresh[j]) {
        a = base[r0[j] + o0 + c]; b = base[r0[j] + o1 + c]; d = base[r1[j] + o0 + c]; e = base[r1[j] + o1 + c];
      }
      const float v = blend(w00[j], w01[j], w10[j], w11[j], a, b, d, e);
      if (v > best[j].v) { best[j].v = v; best[j].c = c; }
      if (probs && ok[j]) probs[(long long)c * cstride + pofs[j]] = v;
    }
  }
}

// phase 2 of both kernels: the 16 x 64 label / conf tile of image b at (X0, Y0) leaves LDS in wide, aligned stores.
// OPT: labels may be null (the scoring launches)
template <bool OPT>
__device__ __forceinline__ void store_tile(const int (&t_lab)[TILE_ROWS][TILE_COLS], const float (&t_conf)[TILE_ROWS][TILE_COLS],
                                           int b, int X0, int Y0, int xend, int h, int w, void* __restrict__ labels,
                                           int label_bytes, float* __restrict__ conf) {
  // 16 lanes per row; lane k takes the aligned quad at X0 - a + 4k, lanes k < a also one pixel of the last a
  const int r = threadIdx.x >> 4, k = threadIdx.x & 15, y = Y0 + r;
  if (y >= h) return;
  const long long row = ((long long)b * h + y) * w;
  const int a = (int)((row + X0) & 3);
  unsigned char* l8 = (unsigned char*)labels;
  short* l16 = (short*)labels;
  auto put = [&](int xx) {
    const int v = t_lab[r][xx - X0];
    if (!OPT || labels) {
      if (label_bytes == 1) l8[row + xx] = (unsigned char)v; else l16[row + xx] = (short)v;
    }
    if (conf) conf[row + xx] = t_conf[r][xx - X0];
  };
  const int xs = X0 - a + 4 * k;
  if (xs >= X0 && xs + 4 <= xend) {
    const int* tl = &t_lab[r][xs - X0];
    if (OPT && !labels)
      ;
    else if (label_bytes == 1)
      *reinterpret_cast<uint32_t*>(l8 + row + xs) = (uint32_t)tl[0] | ((uint32_t)tl[1] << 8) | ((uint32_t)tl[2] << 16) | ((uint32_t)tl[3] << 24);
    else
      *reinterpret_cast<uint2*>(l16 + row + xs) = make_uint2((uint32_t)tl[0] | ((uint32_t)tl[1] << 16), (uint32_t)tl[2] | ((uint32_t)tl[3] << 16));
    if (conf) {
      const float* tc = &t_conf[r][xs - X0];
      *reinterpret_cast<float4*>(conf + row + xs) = make_float4(tc[0], tc[1], tc[2], tc[3]);
    }
  } else {
    for (int e = 0; e < 4; ++e)
      if (xs + e >= X0 && xs + e < xend) put(xs + e);
  }
  if (k < a && X0 + TILE_COLS - a + k < xend) put(X0 + TILE_COLS - a + k);
}


// ---- scoring against ground truth ----
// The table of one workgroup: uint32 [3][n] (intersect, predicted, label) + [2] (scored, out of range), in the dynamic LDS
// (behind seg_predict_kernel's staging buffer, in front of seg_predict_views_kernel's coordinates), zeroed at entry.
struct NoScore {
  static constexpr bool on = false;
};
struct Score {
  static constexpr bool on = true;
  const void* gt;                 // [B, h, w] uint8 or int16
  int gt_bytes, raw;
  unsigned long long* areas;      // [3, n]
  unsigned long long* tally;      // [2]
};

// the table's dwords, in whole 16-byte slots
__host__ __device__ inline int score_dwords(int n) { return (3 * n + 2 + 3) & ~3; }

__device__ __forceinline__ void score_zero(uint32_t* tab, int n) {
  for (int i = threadIdx.x; i < 3 * n + 2; i += 256) tab[i] = 0;
}

// one pixel (where `live`) into the table: the ground-truth rule, then the three bins.  scored / bad: the thread's own
// tallies, which leave through the table (count.h's bins_flush)
__device__ __forceinline__ void score_pixel(uint32_t* tab, int n, int raw, int pred, int g, bool live, int& scored, int& bad) {
  const GtClass t = gt_class(n, raw, g, live);
  const int cls = t.cls;
  const bool sc = t.sc, pin = sc && (unsigned)pred < (unsigned)n;
  scored += sc;
  bad += t.oor;
  bin_add(tab, 2 * n + cls, sc);
  bin_add(tab, n + pred, pin);
  bin_add(tab, cls, pin && pred == cls);
}

// the epilogue of both predict kernels: lane = x, the wave's four rows; pred[j] is the label of row wave * 4 + j
__device__ __forceinline__ void score_tile(const Score& sc, uint32_t* tab, int n, long long image, const int (&pofs)[4],
                                           const bool (&ok)[4], const int (&pred)[4]) {
  int scored = 0, bad = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    int g = 0;
    if (ok[j]) g = sc.gt_bytes == 1 ? elem_at<1>(sc.gt, image + pofs[j]) : elem_at<2>(sc.gt, image + pofs[j]);
    score_pixel(tab, n, sc.raw, pred[j], g, ok[j], scored, bad);
  }
  bins_flush(tab, 3 * n, scored, bad, sc.areas, sc.tally);
}

// phase 2 of the four predict kernels, behind the barrier that publishes the label / conf tile: store_tile writes the tile
// out, and the scoring instantiations (whose labels and conf are optional) count it against ground truth into the table `tab`.
// pofs, ok, pred: score_tile's, the lane's column in its wave's four rows
template <typename S>
__device__ __forceinline__ void finish_tile(const S& sc, uint32_t* tab, int n, const int (&t_lab)[TILE_ROWS][TILE_COLS],
                                            const float (&t_conf)[TILE_ROWS][TILE_COLS], int b, int X0, int Y0, int xend, int h,
                                            int w, void* __restrict__ labels, int label_bytes, float* __restrict__ conf,
                                            const int (&pofs)[4], const bool (&ok)[4], const int (&pred)[4]) {
  if constexpr (S::on) {
    if (labels || conf) store_tile<true>(t_lab, t_conf, b, X0, Y0, xend, h, w, labels, label_bytes, conf);
    score_tile(sc, tab, n, (long long)b * h * w, pofs, ok, pred);
  } else {
    store_tile<false>(t_lab, t_conf, b, X0, Y0, xend, h, w, labels, label_bytes, conf);
  }
}

// the same for a kernel that kept nothing of its pixels in registers (the three chunked ones): the offsets and the validity
// are worked out again and the labels gathered from the tile
template <typename S>
__device__ __forceinline__ void finish_tile(const S& sc, uint32_t* tab, int n, const int (&t_lab)[TILE_ROWS][TILE_COLS],
                                            const float (&t_conf)[TILE_ROWS][TILE_COLS], int b, int X0, int Y0, int xend, int h,
                                            int w, void* __restrict__ labels, int label_bytes, float* __restrict__ conf, int lane,
                                            int wave) {
  int pofs[4], pred[4];
  bool ok[4];
  if constexpr (S::on) {
    const int x = min(X0 + lane, w - 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = wave * 4 + j;
      pofs[j] = min(Y0 + row, h - 1) * w + x;
      ok[j] = Y0 + row < h && X0 + lane < w;
      pred[j] = t_lab[row][lane];
    }
  }
  finish_tile(sc, tab, n, t_lab, t_conf, b, X0, Y0, xend, h, w, labels, label_bytes, conf, pofs, ok, pred);
}

template <typename S>
__global__ __launch_bounds__(256) void seg_predict_kernel(const float* __restrict__ scores, int hp, int wp, int n, int h, int w,
                                                          int tiles_x, int tiles_y, void* __restrict__ labels, int label_bytes,
                                                          float* __restrict__ conf, float* __restrict__ probs,
                                                          int stage_floats, S sc) {
  extern __shared__ __attribute__((aligned(16))) float stage[];   // stage_floats of footprint (scoring: then the table)
  __shared__ int t_lab[TILE_ROWS][TILE_COLS];
  __shared__ float t_conf[TILE_ROWS][TILE_COLS];
  uint32_t* tab = reinterpret_cast<uint32_t*>(stage + stage_floats);
  if constexpr (S::on) score_zero(tab, n);                        // published by the barrier in front of phase 2

  const auto [b, X0, Y0, xend, yend, lane, wave] = tile_decode(tiles_x, tiles_y, h, w);
  const FloatCoord cy{(float)hp / (float)h, hp}, cx{(float)wp / (float)w, wp};
  const float* sb = scores + (long long)b * hp * wp * n;

  int ylo, yhi, xlo, xhi;
  footprint(cy, Y0, yend - 1, &ylo, &yhi);
  footprint(cx, X0, xend - 1, &xlo, &xhi);
  const int fh = yhi - ylo + 1, fw = xhi - xlo + 1, stride = pt_stride(n);
  const bool staged = (long long)fh * fw * stride <= (long long)stage_floats;       // workgroup-uniform
  if (staged) {
    // the fw patches of one footprint row are contiguous in global memory: fw * n floats
    const int run = fw * n;
    for (int i = threadIdx.x; i < fh * run; i += 256) {
      const int ry = i / run, k = i - ry * run, rx = k / n, c = k - rx * n;
      stage[(ry * fw + rx) * stride + c] = sb[((long long)(ylo + ry) * wp + xlo) * n + k];
    }
    __syncthreads();
  }

  // phase 1
  const int x = min(X0 + lane, w - 1);
  int x0, x1;
  float lx;
  cx(x, &x0, &x1, &lx);
  int y0[4], y1[4];
  float ly[4];
  bool fresh[4], ok[4];
  int pofs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yr = Y0 + wave * 4 + j, y = min(yr, h - 1);
    cy(y, &y0[j], &y1[j], &ly[j]);
    fresh[j] = j == 0 || y0[j] != y0[j - 1] || y1[j] != y1[j - 1];
    ok[j] = yr < h && X0 + lane < w;
    pofs[j] = y * w + x;
  }
  Best best[4];
  float* pb = probs ? probs + (long long)b * n * h * w : nullptr;
  long long r0[4], r1[4];
  if (staged) {
#pragma unroll
    for (int j = 0; j < 4; ++j) { r0[j] = (y0[j] - ylo) * fw * stride; r1[j] = (y1[j] - ylo) * fw * stride; }
    class_loop<true>(stage, n, (x0 - xlo) * stride, (x1 - xlo) * stride, r0, r1, fresh, ly, lx, best, pb, pofs,
                     (long long)h * w, ok);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) { r0[j] = (long long)y0[j] * wp * n; r1[j] = (long long)y1[j] * wp * n; }
    class_loop<false>(sb, n, x0 * n, x1 * n, r0, r1, fresh, ly, lx, best, pb, pofs, (long long)h * w, ok);
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) { t_lab[wave * 4 + j][lane] = best[j].c; t_conf[wave * 4 + j][lane] = best[j].v; }
  __syncthreads();

  const int pred[4] = {best[0].c, best[1].c, best[2].c, best[3].c};
  finish_tile(sc, tab, n, t_lab, t_conf, b, X0, Y0, xend, h, w, labels, label_bytes, conf, pofs, ok, pred);
}

// ---- K views of different grids into one label map (multi-scale + flip test-time augmentation) ----
// The tile and the lane mapping are those of seg_predict_kernel, phase 2 is finish_tile's lines.  The classes are walked in
// chunks of PV_CHUNK: per chunk the footprints of all views are staged side by side in LDS (PV_CHUNK floats per patch at the odd-slot
// stride), then a wave takes its four rows one after the other, and per row the view loop runs innermost and adds each view's
// flat four-weight value into the row's PV_CHUNK registers, in view order.  The running maximum of a pixel lives in the label /
// conf tile between the chunks.  A flipped view is staged in its mirrored (logical) column order, so the inner
// loop is the same for both.  Views are given LDS in order while the buffer lasts; a view that no longer fits reads global
// memory in the same loop.
// The source coordinates of a view under the tile do not depend on the class: they are worked out once, as offsets into
// the view's staged footprint (or its grid in global memory), and kept in LDS, PV_COORDS dwords per view.
constexpr int PV_MAX_VIEWS = 16, PV_CHUNK = 16, PV_STRIDE = 20;   // PV_STRIDE == pt_stride(PV_CHUNK)
constexpr int PV_COORDS = 3 * TILE_COLS + 3 * TILE_ROWS;          // per view: o0, o1, lx per column; r0, r1, ly per row
constexpr int PV_META_LDS = 1024;                                 // >= sizeof(ViewMeta) * PV_MAX_VIEWS
constexpr int PV_STAGE_LIMIT = 65536 - PT_TILE_LDS - PV_META_LDS; // coordinates + staged footprints

int g_views_stage_limit = PV_STAGE_LIMIT;

struct ViewTable {
  ifseg_predict_view v[PV_MAX_VIEWS];
};

// one view under one tile; off: its first float in the staging buffer, < 0 when it reads global memory
struct ViewMeta {
  const float* base;      // the image's grid
  int hp, wp, flip, ylo, xlo, fw, cells, off;
};
static_assert(sizeof(ViewMeta) * PV_MAX_VIEWS <= PV_META_LDS, "PV_META_LDS");

// four consecutive classes of one patch: a 16-byte LDS read, or (global memory) single reads of the classes below cn
template <bool VEC>
__device__ __forceinline__ f32x4 quad(const float* p, int c, int cn) {
  if (VEC) return *reinterpret_cast<const f32x4*>(p + c);
  f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c + k < cn) v[k] = p[c + k];
  return v;
}

// acc[c] += the view's value of class c at one pixel, whose four patches start at p00 .. p11
template <bool VEC>
__device__ __forceinline__ void add_view(const float* p00, const float* p01, const float* p10, const float* p11, int cn, float ly,
                                         float lx, f32x4 (&acc)[PV_CHUNK / 4]) {
  // the empty asm keeps 1 - ly and 1 - lx in registers of their own: computed as a pair, their product is a packed multiply
  // that reads across the halves of the pair (tools/check_isa.py again)
  float my = 1.f - ly, mx = 1.f - lx;
  asm("" : "+v"(my), "+v"(mx));
  const float w00 = my * mx, w01 = my * lx, w10 = ly * mx, w11 = ly * lx;
#pragma unroll
  for (int c = 0; c < PV_CHUNK; c += 4) {
    if (VEC || c < cn) {
      const f32x4 a = quad<VEC>(p00, c, cn), b = quad<VEC>(p01, c, cn), d = quad<VEC>(p10, c, cn), e = quad<VEC>(p11, c, cn);
      acc[c >> 2] += blend4(w00, w01, w10, w11, a, b, d, e);
    }
  }
}

template <typename S>
__global__ __launch_bounds__(256) void seg_predict_views_kernel(ViewTable views, int K, float inv_k, int n, int h, int w,
                                                                int tiles_x, int tiles_y, void* __restrict__ labels,
                                                                int label_bytes, float* __restrict__ conf,
                                                                float* __restrict__ probs, int stage_floats, S sc) {
  // (scoring: the table,) K * PV_COORDS coordinates, then stage_floats of footprints
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ int t_lab[TILE_ROWS][TILE_COLS];
  __shared__ float t_conf[TILE_ROWS][TILE_COLS];
  __shared__ ViewMeta vm[PV_MAX_VIEWS];
  int* coords = reinterpret_cast<int*>(dyn);
  if constexpr (S::on) {
    score_zero(reinterpret_cast<uint32_t*>(dyn), n);              // published by the barriers below
    coords += score_dwords(n);
  }
  float* stage = reinterpret_cast<float*>(coords) + K * PV_COORDS;

  const auto [b, X0, Y0, xend, yend, lane, wave] = tile_decode(tiles_x, tiles_y, h, w);

  // every view's footprint under this tile, in the view's logical (un-mirrored) columns: thread k takes view k (picked by a
  // chain of selects: the table is a kernel argument, and indexing it by a variable would move it to private memory)
  if (threadIdx.x < K) {
    ifseg_predict_view v = views.v[0];
#pragma unroll
    for (int i = 1; i < PV_MAX_VIEWS; ++i)
      if (threadIdx.x == i) v = views.v[i];
    int ylo, yhi, xlo, xhi;
    footprint(FloatCoord{(float)v.hp / (float)h, v.hp}, Y0, yend - 1, &ylo, &yhi);
    footprint(FloatCoord{(float)v.wp / (float)w, v.wp}, X0, xend - 1, &xlo, &xhi);
    ViewMeta& m = vm[threadIdx.x];
    m.base = v.scores + (long long)b * v.hp * v.wp * n;
    m.hp = v.hp; m.wp = v.wp; m.flip = v.flip;
    m.ylo = ylo; m.xlo = xlo; m.fw = xhi - xlo + 1; m.cells = (yhi - ylo + 1) * m.fw;
  }
  __syncthreads();
  // its place in the staging buffer: in view order, while the buffer lasts
  if (threadIdx.x == 0) {
    int used = 0;
    for (int k = 0; k < K; ++k) {
      const long long need = (long long)vm[k].cells * PV_STRIDE;
      const bool fits = need <= (long long)(stage_floats - used);
      vm[k].off = fits ? used : -1;
      if (fits) used += (int)need;
    }
  }
  __syncthreads();
  // the coordinates of the tile's 64 columns and 16 rows in every view, as float offsets from the view's base: into its staged
  // footprint, or into its grid (below 2^31: hp wp < 2^22, n <= 512), there with the mirroring applied
  for (int i = threadIdx.x; i < K * (TILE_COLS + TILE_ROWS); i += 256) {
    const int k = i / (TILE_COLS + TILE_ROWS), r = i - k * (TILE_COLS + TILE_ROWS);
    const ViewMeta& m = vm[k];
    int* cv = coords + k * PV_COORDS;
    int i0, i1;
    float l;
    if (r < TILE_COLS) {
      FloatCoord{(float)m.wp / (float)w, m.wp}(min(X0 + r, w - 1), &i0, &i1, &l);
      if (m.off >= 0) { i0 = (i0 - m.xlo) * PV_STRIDE; i1 = (i1 - m.xlo) * PV_STRIDE; }
      else { i0 = (m.flip ? m.wp - 1 - i0 : i0) * n; i1 = (m.flip ? m.wp - 1 - i1 : i1) * n; }
      cv[r] = i0; cv[TILE_COLS + r] = i1; cv[2 * TILE_COLS + r] = __float_as_int(l);
    } else {
      const int rr = r - TILE_COLS, rowlen = m.off >= 0 ? m.fw * PV_STRIDE : m.wp * n;
      FloatCoord{(float)m.hp / (float)h, m.hp}(min(Y0 + rr, h - 1), &i0, &i1, &l);
      if (m.off >= 0) { i0 -= m.ylo; i1 -= m.ylo; }
      int* cr = cv + 3 * TILE_COLS;
      cr[rr] = i0 * rowlen; cr[TILE_ROWS + rr] = i1 * rowlen; cr[2 * TILE_ROWS + rr] = __float_as_int(l);
    }
  }

  const int x = min(X0 + lane, w - 1);
  float* pb = probs ? probs + (long long)b * n * h * w : nullptr;
  const long long cstride = (long long)h * w;

  for (int c0 = 0; c0 < n; c0 += PV_CHUNK) {
    const int cn = min(PV_CHUNK, n - c0);
    if (c0) __syncthreads();                      // the previous chunk has been read
    // phase 0: 16 threads per patch, one class each; the classes past n are zero
    for (int k = 0; k < K; ++k) {
      const int off = vm[k].off;
      if (off < 0) continue;
      const float* base = vm[k].base + c0;
      const int wp = vm[k].wp, flip = vm[k].flip, ylo = vm[k].ylo, xlo = vm[k].xlo, fw = vm[k].fw, cells = vm[k].cells;
      const int cc = threadIdx.x & 15;
      for (int p = threadIdx.x >> 4; p < cells; p += 16) {
        const int ry = p / fw, col = xlo + p - ry * fw;
        const long long src = ((long long)(ylo + ry) * wp + (flip ? wp - 1 - col : col)) * n;
        stage[off + p * PV_STRIDE + cc] = cc < cn ? base[src + cc] : 0.f;
      }
    }
    __syncthreads();                              // (the first one publishes the coordinates as well)

    // phase 1, row by row.  -0 is the neutral element of the addition: -0 + v == v for every v, the sign of a zero included
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int row = wave * 4 + j, yr = Y0 + row;
      f32x4 acc[PV_CHUNK / 4];
#pragma unroll
      for (int c = 0; c < PV_CHUNK / 4; ++c) acc[c] = f32x4{-0.f, -0.f, -0.f, -0.f};
      for (int k = 0; k < K; ++k) {
        const int* cv = coords + k * PV_COORDS;
        const int o0 = cv[lane], o1 = cv[TILE_COLS + lane];
        const float lx = __int_as_float(cv[2 * TILE_COLS + lane]);
        const int r0 = cv[3 * TILE_COLS + row], r1 = cv[3 * TILE_COLS + TILE_ROWS + row];
        const float ly = __int_as_float(cv[3 * TILE_COLS + 2 * TILE_ROWS + row]);
        const int off = __builtin_amdgcn_readfirstlane(vm[k].off);
        if (off >= 0) {
          const float* s = stage + off;
          add_view<true>(s + r0 + o0, s + r0 + o1, s + r1 + o0, s + r1 + o1, cn, ly, lx, acc);
        } else {
          const float* s = vm[k].base + c0;
          add_view<false>(s + r0 + o0, s + r0 + o1, s + r1 + o0, s + r1 + o1, cn, ly, lx, acc);
        }
      }
      float bv = c0 ? t_conf[row][lane] : -INFINITY;
      int bc = c0 ? t_lab[row][lane] : 0;
      const bool ok = yr < h && X0 + lane < w;
      float* pp = pb + (long long)c0 * cstride + min(yr, h - 1) * w + x;
#pragma unroll
      for (int c = 0; c < PV_CHUNK; ++c) {
        if (c < cn) {
          const float v = acc[c >> 2][c & 3] * inv_k;
          if (v > bv) { bv = v; bc = c0 + c; }
          if (pb && ok) pp[c * cstride] = v;
        }
      }
      t_conf[row][lane] = bv; t_lab[row][lane] = bc;
    }
  }
  __syncthreads();

  // phase 2: finish_tile, written out -- through the function the scoring instantiation of this kernel (alone) measured
  // 0.7 % slower at twelve views
  if constexpr (S::on) {
    if (labels || conf) store_tile<true>(t_lab, t_conf, b, X0, Y0, xend, h, w, labels, label_bytes, conf);
    int pofs[4], pred[4];
    bool ok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = wave * 4 + j;
      pofs[j] = min(Y0 + row, h - 1) * w + x;
      ok[j] = Y0 + row < h && X0 + lane < w;
      pred[j] = t_lab[row][lane];
    }
    score_tile(sc, reinterpret_cast<uint32_t*>(dyn), n, (long long)b * h * w, pofs, ok, pred);
  } else {
    store_tile<false>(t_lab, t_conf, b, X0, Y0, xend, h, w, labels, label_bytes, conf);
  }
}

// ---- the windows of one image into one label map (sliding-window inference) ----
// scores [B, Nw, hpw * wpw, n]: window k = iy gx + ix of the [oh, ow] plane (tile.h's SlideAxis) ran the network on its own
// hpw x wpw grid.  A pixel of the [h, w] output takes its (up to four) taps in the plane by the coordinate rule; per tap the
// flat four-weight values of the windows that hold it are added in window order (rows outer) and divided by their number; a
// tap of weight zero contributes nothing.  Neither a window's [n, ch, cw] tensor nor the plane is ever written.
// The tile, the lane mapping, the class chunks and add_view are those of seg_predict_views_kernel.  The windows are a
// cross product, so everything is kept per axis: the windows iya..iyb / ixa..ixb hold the tile's plane footprint, each with its
// own run of patch rows / columns under it, and the runs of an axis laid end to end span a staged grid of FH x FW patches
// (PV_CHUNK classes each, at the odd-slot stride) in which window (i, j) owns the block rows(i) x cols(j).  A tile whose
// grid does not fit the buffer reads global memory in the same loop.
constexpr int SW_MAX_WINDOWS = IFSEG_SLIDE_MAX_WINDOWS;
constexpr int SW_META_LDS = 3 * 2 * SW_MAX_WINDOWS * 4 + 16;      // sw_lo, sw_ext, sw_adj, sw_tot
constexpr int SW_STAGE_LIMIT = 65536 - PT_TILE_LDS - SW_META_LDS; // source cells + staged patches

int g_windows_stage_limit = SW_STAGE_LIMIT;

struct Slide {
  SlideAxis y, x;
  int hpw, wpw;
};

// out += wt * (acc / cnt) where wt != 0: a rounded quotient, a rounded product, a rounded sum
__device__ __forceinline__ void add_tap(f32x4 (&out)[PV_CHUNK / 4], const f32x4 (&acc)[PV_CHUNK / 4], float cnt, float wt) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < PV_CHUNK / 4; ++c) {
    const f32x4 v = out[c] + wt * (acc[c] / cnt);
    if (wt != 0.f) out[c] = v;
  }
}

// one pixel's PV_CHUNK classes: plane rows Yt[0..1] (weight 1 - ly2, ly2; wave-uniform), plane columns Xt[0..1] (1 - lx2, lx2).
// VEC: s is the staged grid, adj the runs' offsets in it, rowlen = FW PV_STRIDE; else s is the image's windows in global memory
template <bool VEC>
__device__ __forceinline__ void slide_pixel(const float* s, const Slide& sl, const FloatCoord& cwy, const FloatCoord& cwx,
                                            const int (&adj)[2][SW_MAX_WINDOWS], int iya, int ixa, int rowlen, int n, int cn,
                                            const int (&Yt)[2], float ly2, const int (&Xt)[2], float lx2, bool anyx1,
                                            f32x4 (&out)[PV_CHUNK / 4]) {
  const int cells = sl.hpw * sl.wpw;
  const int nty = ly2 != 0.f ? 2 : 1, ntx = anyx1 ? 2 : 1;
  for (int ty = 0; ty < nty; ++ty) {
    const int Y = Yt[ty], ia = sl.y.first(Y), ib = sl.y.last(Y);
    const float wy = ty ? ly2 : 1.f - ly2;
    for (int tx = 0; tx < ntx; ++tx) {
      const int X = Xt[tx], ja = sl.x.first(X), jb = sl.x.last(X);
      const float wx = tx ? lx2 : 1.f - lx2;
      f32x4 acc[PV_CHUNK / 4];
#pragma unroll
      for (int c = 0; c < PV_CHUNK / 4; ++c) acc[c] = f32x4{-0.f, -0.f, -0.f, -0.f};
      for (int i = ia; i <= ib; ++i) {
        int p0, p1, q0, q1;
        float ly, lx;
        cwy(Y - sl.y.start(i), &p0, &p1, &ly);
        const int rb = VEC ? adj[0][i - iya] * rowlen : i * sl.x.g * cells * n, rl = VEC ? rowlen : sl.wpw * n;
        for (int j = ja; j <= jb; ++j) {
          cwx(X - sl.x.start(j), &q0, &q1, &lx);
          const int cb = VEC ? adj[1][j - ixa] * PV_STRIDE : j * cells * n, cl = VEC ? PV_STRIDE : n;
          const float* r0 = s + (rb + p0 * rl + cb);
          const float* r1 = s + (rb + p1 * rl + cb);
          add_view<VEC>(r0 + q0 * cl, r0 + q1 * cl, r1 + q0 * cl, r1 + q1 * cl, cn, ly, lx, acc);
        }
      }
      add_tap(out, acc, (float)((ib - ia + 1) * (jb - ja + 1)), wy * wx);
    }
  }
}

// The window bookkeeping of one plane under one tile, per axis, by all threads of the workgroup (two barriers inside): the
// plane footprint of the tile's output rows Ya..Yb and columns Xa..Xb, the windows iya.. / ixa.. that hold any of it, per axis
// (0: y, 1: x) and window the run of patches under it (the caller's scratch: sw_lo its first patch, sw_ext their number; sw_tot
// the axis' total) and the runs' places in a grid of FH x FW patches (adj: run offset - first patch).  The grid is staged if
// it fits `room` floats behind `cellsrc` together with its source cells, FH + FW in whole 16-byte slots; those are then
// written -- staged row R / column C comes from patch cellsrc[R] + cellsrc[FH + C] of the image's windows -- and published by
// the caller's next barrier.
struct PlaneTile {
  int iya, ixa, FH, FW;
  long long need;         // floats of the source cells and the grid
  bool staged;            // workgroup-uniform
};
__device__ __forceinline__ PlaneTile plane_tile(const Slide& sl, const FloatCoord& c2y, const FloatCoord& c2x, const FloatCoord& cwy,
                                                const FloatCoord& cwx, int Ya, int Yb, int Xa, int Xb,
                                                int (&sw_lo)[2][SW_MAX_WINDOWS], int (&sw_ext)[2][SW_MAX_WINDOWS],
                                                int (&adj)[2][SW_MAX_WINDOWS], int (&sw_tot)[2], int* cellsrc, int room) {
  const int t = threadIdx.x, cells = sl.hpw * sl.wpw;
  int Ylo, Yhi, Xlo, Xhi;
  footprint(c2y, Ya, Yb, &Ylo, &Yhi);
  footprint(c2x, Xa, Xb, &Xlo, &Xhi);
  const int iya = sl.y.first(Ylo), ny = sl.y.last(Yhi) - iya + 1, ixa = sl.x.first(Xlo), nx = sl.x.last(Xhi) - ixa + 1;
  const bool isx = t >= ny;
  const int ai = isx ? t - ny : t;                                // thread t < ny + nx takes one window of one axis
  if (t < ny + nx) {
    const SlideAxis a = isx ? sl.x : sl.y;
    const int st = a.start((isx ? ixa : iya) + ai), lo = isx ? Xlo : Ylo, hi = isx ? Xhi : Yhi;
    int plo, phi;
    footprint(isx ? cwx : cwy, max(lo, st) - st, min(hi, st + a.e - 1) - st, &plo, &phi);
    sw_lo[isx][ai] = plo; sw_ext[isx][ai] = phi - plo + 1;
  }
  __syncthreads();
  if (t < 2) {
    int used = 0;
    for (int k = 0; k < (t ? nx : ny); ++k) { adj[t][k] = used - sw_lo[t][k]; used += sw_ext[t][k]; }
    sw_tot[t] = used;
  }
  __syncthreads();
  const int FH = sw_tot[0], FW = sw_tot[1];
  const long long need = (long long)FH * FW * PV_STRIDE + ((FH + FW + 3) & ~3);
  const bool staged = need <= (long long)room;
  if (staged && t < ny + nx) {
    const int i = (isx ? ixa : iya) + ai, first = adj[isx][ai] + sw_lo[isx][ai];
    for (int r = 0; r < sw_ext[isx][ai]; ++r)
      cellsrc[(isx ? FH : 0) + first + r] = isx ? i * cells + sw_lo[1][ai] + r : i * sl.x.g * cells + (sw_lo[0][ai] + r) * sl.wpw;
  }
  return {iya, ixa, FH, FW, need, staged};
}

template <typename S>
__global__ __launch_bounds__(256) void seg_predict_windows_kernel(const float* __restrict__ scores, Slide sl, int n, int h, int w,
                                                                  int tiles_x, int tiles_y, void* __restrict__ labels,
                                                                  int label_bytes, float* __restrict__ conf,
                                                                  float* __restrict__ probs, int stage_floats, S sc) {
  // (scoring: the table,) the source cells of the staged rows and columns, then the staged grid: stage_floats in all
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ int t_lab[TILE_ROWS][TILE_COLS];
  __shared__ float t_conf[TILE_ROWS][TILE_COLS];
  // plane_tile's, per axis and window of the tile's range: first patch of its run, their number, run offset - first patch
  __shared__ int sw_lo[2][SW_MAX_WINDOWS], sw_ext[2][SW_MAX_WINDOWS], sw_adj[2][SW_MAX_WINDOWS], sw_tot[2];
  int* cellsrc = reinterpret_cast<int*>(dyn);
  if constexpr (S::on) {
    score_zero(reinterpret_cast<uint32_t*>(dyn), n);              // published by the barriers below
    cellsrc += score_dwords(n);
  }

  const auto [b, X0, Y0, xend, yend, lane, wave] = tile_decode(tiles_x, tiles_y, h, w);
  const FloatCoord c2y{(float)sl.y.o / (float)h, sl.y.o}, c2x{(float)sl.x.o / (float)w, sl.x.o};            // output -> plane
  const FloatCoord cwy{(float)sl.hpw / (float)sl.y.e, sl.hpw}, cwx{(float)sl.wpw / (float)sl.x.e, sl.wpw};  // window -> grid
  const float* sb = scores + (long long)b * sl.y.g * sl.x.g * sl.hpw * sl.wpw * n;

  const PlaneTile pt =
      plane_tile(sl, c2y, c2x, cwy, cwx, Y0, yend - 1, X0, xend - 1, sw_lo, sw_ext, sw_adj, sw_tot, cellsrc, stage_floats);
  const int iya = pt.iya, ixa = pt.ixa, FH = pt.FH, FW = pt.FW;
  const bool staged = pt.staged;
  float* stage = reinterpret_cast<float*>(cellsrc + ((FH + FW + 3) & ~3));
  __syncthreads();

  const int x = min(X0 + lane, w - 1);
  int Xt[2];
  float lx2;
  c2x(x, &Xt[0], &Xt[1], &lx2);
  const bool anyx1 = __ballot(lx2 != 0.f) != 0;
  float* pb = probs ? probs + (long long)b * n * h * w : nullptr;
  const long long cstride = (long long)h * w;

  for (int c0 = 0; c0 < n; c0 += PV_CHUNK) {
    const int cn = min(PV_CHUNK, n - c0);
    if (c0) __syncthreads();                      // the previous chunk has been read
    // phase 0: 16 threads per patch, one class each; the classes past n are zero
    if (staged) {
      const int t = threadIdx.x, cc = t & 15;
      for (int p = t >> 4; p < FH * FW; p += 16) {
        const int R = p / FW, C = p - R * FW;
        stage[p * PV_STRIDE + cc] = cc < cn ? sb[(long long)(cellsrc[R] + cellsrc[FH + C]) * n + c0 + cc] : 0.f;
      }
    }
    __syncthreads();

    // phase 1, row by row
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int row = wave * 4 + j, yr = Y0 + row;
      int Yt[2];
      float ly2;
      c2y(min(yr, h - 1), &Yt[0], &Yt[1], &ly2);
      f32x4 out[PV_CHUNK / 4];
#pragma unroll
      for (int c = 0; c < PV_CHUNK / 4; ++c) out[c] = f32x4{-0.f, -0.f, -0.f, -0.f};
      if (staged) slide_pixel<true>(stage, sl, cwy, cwx, sw_adj, iya, ixa, FW * PV_STRIDE, n, cn, Yt, ly2, Xt, lx2, anyx1, out);
      else slide_pixel<false>(sb + c0, sl, cwy, cwx, sw_adj, iya, ixa, 0, n, cn, Yt, ly2, Xt, lx2, anyx1, out);
      float bv = c0 ? t_conf[row][lane] : -INFINITY;
      int bc = c0 ? t_lab[row][lane] : 0;
      const bool ok = yr < h && X0 + lane < w;
      float* pp = pb + (long long)c0 * cstride + min(yr, h - 1) * w + x;
#pragma unroll
      for (int c = 0; c < PV_CHUNK; ++c) {
        if (c < cn) {
          const float v = out[c >> 2][c & 3];
          if (v > bv) { bv = v; bc = c0 + c; }
          if (pb && ok) pp[c * cstride] = v;
        }
      }
      t_conf[row][lane] = bv; t_lab[row][lane] = bc;
    }
  }
  __syncthreads();

  finish_tile(sc, reinterpret_cast<uint32_t*>(dyn), n, t_lab, t_conf, b, X0, Y0, xend, h, w, labels, label_bytes, conf, lane,
              wave);
}

// ---- K views, each the windows of its own plane, into one label map (multi-scale + flip over sliding-window inference) ----
// View k is seg_predict_windows_kernel's input at its own [oh_k, ow_k] plane and window grid; all views share crop, stride and
// the [h, w] output.  Per pixel and class the view's value is slide_pixel's -- the same function on the same arguments, so one
// unflipped view gives that kernel's bits -- a flipped view sampled at the mirrored output column w - 1 - x.
//   linear   the K values of a class are added in view order and multiplied by inv_k;
//   softmax  every view's value is first normalised over the classes, exp(v - max) / sum with the sum in class order (mmseg's
//            order: slide_inference -> resize -> softmax -> un-flip, averaged over the views).  The normaliser needs all
//            classes of a pixel and view before anything can be accumulated: two passes over the class chunks leave max and
//            sum in LDS (SV_NORM_DWORDS per view), the third recomputes the values -- the same inlined code on the same staged
//            data, contraction off, so the same bits -- normalises and accumulates.
// The tile, the lane mapping and the class chunks are seg_predict_windows_kernel's.  Its per-axis window bookkeeping (plane_tile)
// is done once per view, view after view through one pair of scratch arrays, and what the class loop needs of it stays in LDS:
// per view the runs' offsets (sw_adj), the two scales of its coordinate rules and, for a staged view, the source cells of its
// grid.  (The plane taps of a pixel are one fma and a floor per axis: they are recomputed where they are used, and their LDS
// goes to the normalisers.)  Views are given staging room in view order while the buffer lasts; a view that no longer fits
// reads global memory in the same loop.
// LDS: the linear mode budgets 64 KiB per workgroup as the other kernels do; the softmax mode adds its normalisers (8 KiB per
// view) on top, up to the device's limit (160 KiB on gfx950), and the staging buffer takes what is left.
constexpr int SV_VIEW_DWORDS = 2 * SW_MAX_WINDOWS;                // per view: sw_adj [2][SW_MAX_WINDOWS]
constexpr int SV_NORM_DWORDS = 2 * TILE_ROWS * TILE_COLS;         // per view (softmax): max, then sum, of every pixel
constexpr int SV_META_LDS = 2560;                                 // >= vm + sw_lo + sw_ext + sw_tot
constexpr int SV_LDS_CEILING = 160 * 1024;
constexpr int SV_STAGE_LIMIT = 65536 - PT_TILE_LDS - SV_META_LDS; // the linear mode's: per-view data + staged grids

int g_slide_views_stage_limit = SV_STAGE_LIMIT;

struct SlideView {
  const float* scores;
  Slide sl;
  int flip;
};
struct SlideViewTable {
  SlideView v[PV_MAX_VIEWS];
};

// one view under one tile; off: its first float in the staging buffer (cells, then the grid), < 0 when it reads global memory
struct SlideMeta {
  const float* base;      // the image's windows
  Slide sl;
  float sy, sx, py, px;   // window -> grid and output -> plane scales
  int flip, iya, ixa, FH, FW, off;
};
static_assert(sizeof(SlideMeta) * PV_MAX_VIEWS + 2 * 2 * SW_MAX_WINDOWS * 4 + 16 <= SV_META_LDS, "SV_META_LDS");

// out = view m's merged and resized value of classes c0 .. c0 + cn - 1 at output pixel (y, x), y wave-uniform; vd: the view's
// SV_VIEW_DWORDS, stage: the staging buffer with the chunk's patches in place
__device__ __forceinline__ void slide_view_value(const SlideMeta& m, const int* vd, const float* stage, int n, int c0, int cn,
                                                 int y, int x, int w, f32x4 (&out)[PV_CHUNK / 4]) {
  const Slide sl = m.sl;
  const FloatCoord cwy{m.sy, sl.hpw}, cwx{m.sx, sl.wpw};
  int Yt[2], Xt[2];
  float ly2, lx2;
  FloatCoord{m.py, sl.y.o}(y, &Yt[0], &Yt[1], &ly2);
  // the row is the wave's: so are its plane rows and their weight
  Yt[0] = __builtin_amdgcn_readfirstlane(Yt[0]); Yt[1] = __builtin_amdgcn_readfirstlane(Yt[1]);
  ly2 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ly2)));
  FloatCoord{m.px, sl.x.o}(m.flip ? w - 1 - x : x, &Xt[0], &Xt[1], &lx2);
  const bool anyx1 = __ballot(lx2 != 0.f) != 0;
  const int (&adj)[2][SW_MAX_WINDOWS] = *reinterpret_cast<const int (*)[2][SW_MAX_WINDOWS]>(vd);
  const int iya = __builtin_amdgcn_readfirstlane(m.iya), ixa = __builtin_amdgcn_readfirstlane(m.ixa);
  const int off = __builtin_amdgcn_readfirstlane(m.off);
#pragma unroll
  for (int c = 0; c < PV_CHUNK / 4; ++c) out[c] = f32x4{-0.f, -0.f, -0.f, -0.f};
  if (off >= 0) {
    const int FH = __builtin_amdgcn_readfirstlane(m.FH), FW = __builtin_amdgcn_readfirstlane(m.FW);
    slide_pixel<true>(stage + off + ((FH + FW + 3) & ~3), sl, cwy, cwx, adj, iya, ixa, FW * PV_STRIDE, n, cn, Yt, ly2, Xt, lx2,
                      anyx1, out);
  } else {
    slide_pixel<false>(m.base + c0, sl, cwy, cwx, adj, iya, ixa, 0, n, cn, Yt, ly2, Xt, lx2, anyx1, out);
  }
}

template <typename S>
__global__ __launch_bounds__(256) void seg_predict_slide_views_kernel(SlideViewTable views, int K, float inv_k, int softmax, int n,
                                                                      int h, int w, int tiles_x, int tiles_y,
                                                                      void* __restrict__ labels, int label_bytes,
                                                                      float* __restrict__ conf, float* __restrict__ probs,
                                                                      int stage_floats, S sc) {
  // (scoring: the table,) K * SV_VIEW_DWORDS of per-view data, (softmax: K * SV_NORM_DWORDS of normalisers,) then stage_floats
  // of source cells and staged grids
  extern __shared__ __attribute__((aligned(16))) float dyn[];
  __shared__ int t_lab[TILE_ROWS][TILE_COLS];
  __shared__ float t_conf[TILE_ROWS][TILE_COLS];
  __shared__ SlideMeta vm[PV_MAX_VIEWS];
  // scratch of the view being set up: per axis and window of the tile's range, first patch of its run and their number
  __shared__ int sw_lo[2][SW_MAX_WINDOWS], sw_ext[2][SW_MAX_WINDOWS], sw_tot[2];
  int* vdata = reinterpret_cast<int*>(dyn);
  if constexpr (S::on) {
    score_zero(reinterpret_cast<uint32_t*>(dyn), n);              // published by the barriers below
    vdata += score_dwords(n);
  }
  float* norm = reinterpret_cast<float*>(vdata + K * SV_VIEW_DWORDS);
  float* stage = norm + (softmax ? K * SV_NORM_DWORDS : 0);

  const auto [b, X0, Y0, xend, yend, lane, wave] = tile_decode(tiles_x, tiles_y, h, w);
  const int t = threadIdx.x;

  // thread k takes view k out of the kernel argument (a chain of selects, as in seg_predict_views_kernel)
  if (t < K) {
    SlideView v = views.v[0];
#pragma unroll
    for (int i = 1; i < PV_MAX_VIEWS; ++i)
      if (t == i) v = views.v[i];
    SlideMeta& m = vm[t];
    m.base = v.scores + (long long)b * v.sl.y.g * v.sl.x.g * v.sl.hpw * v.sl.wpw * n;
    m.sl = v.sl;
    m.sy = (float)v.sl.hpw / (float)v.sl.y.e; m.sx = (float)v.sl.wpw / (float)v.sl.x.e;
    m.py = (float)v.sl.y.o / (float)h; m.px = (float)v.sl.x.o / (float)w;
    m.flip = v.flip;
  }
  __syncthreads();

  // plane_tile, view after view; a flipped view is under the mirrored columns of the tile
  int used = 0;
  for (int k = 0; k < K; ++k) {
    const Slide sl = vm[k].sl;
    const int flip = vm[k].flip;
    const FloatCoord c2y{vm[k].py, sl.y.o}, c2x{vm[k].px, sl.x.o};                                          // output -> plane
    const FloatCoord cwy{vm[k].sy, sl.hpw}, cwx{vm[k].sx, sl.wpw};                                          // window -> grid
    int* vd = vdata + k * SV_VIEW_DWORDS;
    int (&adj)[2][SW_MAX_WINDOWS] = *reinterpret_cast<int (*)[2][SW_MAX_WINDOWS]>(vd);
    const auto [iya, ixa, FH, FW, need, staged] =
        plane_tile(sl, c2y, c2x, cwy, cwx, Y0, yend - 1, flip ? w - xend : X0, flip ? w - 1 - X0 : xend - 1, sw_lo, sw_ext, adj,
                   sw_tot, reinterpret_cast<int*>(stage + used), stage_floats - used);
    if (t == 0) {
      SlideMeta& m = vm[k];
      m.iya = iya; m.ixa = ixa; m.FH = FH; m.FW = FW; m.off = staged ? used : -1;
    }
    if (staged) used += (int)need;
    __syncthreads();                              // the scratch is free for the next view; the last one publishes everything
  }

  // phase 0 of a class chunk: 16 threads per patch, one class each; the classes past n are zero
  auto stage_chunk = [&](int c0, int cn) {
    const int cc = t & 15;
    for (int k = 0; k < K; ++k) {
      const int off = vm[k].off;
      if (off < 0) continue;
      const int FH = vm[k].FH, FW = vm[k].FW;
      const int* cellsrc = reinterpret_cast<const int*>(stage + off);
      float* grid = stage + off + ((FH + FW + 3) & ~3);
      const float* sb = vm[k].base + c0;
      for (int p = t >> 4; p < FH * FW; p += 16) {
        const int R = p / FW, C = p - R * FW;
        grid[p * PV_STRIDE + cc] = cc < cn ? sb[(long long)(cellsrc[R] + cellsrc[FH + C]) * n + cc] : 0.f;
      }
    }
  };

  const int x = min(X0 + lane, w - 1);
  // softmax: the maximum of every pixel and view over all classes, then the sum of exp(v - max) in class order
  if (softmax) {
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
#pragma unroll 1
      for (int c0 = 0; c0 < n; c0 += PV_CHUNK) {
        const int cn = min(PV_CHUNK, n - c0);
        __syncthreads();                          // the previous chunk has been read
        stage_chunk(c0, cn);
        __syncthreads();
#pragma unroll 1
        for (int j = 0; j < 4; ++j) {
          const int row = wave * 4 + j;
#pragma unroll 1
          for (int k = 0; k < K; ++k) {
            f32x4 out[PV_CHUNK / 4];
            slide_view_value(vm[k], vdata + k * SV_VIEW_DWORDS, stage, n, c0, cn, min(Y0 + row, h - 1), x, w, out);
            float* nm = norm + k * SV_NORM_DWORDS + row * TILE_COLS + lane;   // the thread's own pixel: no barrier needed
            if (pass == 0) {
              float mx = c0 ? nm[0] : -INFINITY;
#pragma unroll
              for (int c = 0; c < PV_CHUNK; ++c)
                if (c < cn) mx = fmaxf(mx, out[c >> 2][c & 3]);
              nm[0] = mx;
            } else {
              const float mx = nm[0];
              float s = c0 ? nm[TILE_ROWS * TILE_COLS] : 0.f;
#pragma unroll
              for (int c = 0; c < PV_CHUNK; ++c)
                if (c < cn) s += expf(out[c >> 2][c & 3] - mx);
              nm[TILE_ROWS * TILE_COLS] = s;
            }
          }
        }
      }
    }
  }

  float* pb = probs ? probs + (long long)b * n * h * w : nullptr;
  const long long cstride = (long long)h * w;

  for (int c0 = 0; c0 < n; c0 += PV_CHUNK) {
    const int cn = min(PV_CHUNK, n - c0);
    __syncthreads();                              // the previous chunk has been read
    stage_chunk(c0, cn);
    __syncthreads();

    // phase 1, row by row; the view loop adds in view order.  -0 is the neutral element of the addition
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
      const int row = wave * 4 + j, yr = Y0 + row;
      f32x4 acc[PV_CHUNK / 4];
#pragma unroll
      for (int c = 0; c < PV_CHUNK / 4; ++c) acc[c] = f32x4{-0.f, -0.f, -0.f, -0.f};
#pragma unroll 1
      for (int k = 0; k < K; ++k) {
        f32x4 out[PV_CHUNK / 4];
        slide_view_value(vm[k], vdata + k * SV_VIEW_DWORDS, stage, n, c0, cn, min(Y0 + row, h - 1), x, w, out);
        if (softmax) {
          const float* nm = norm + k * SV_NORM_DWORDS + row * TILE_COLS + lane;
          const float mx = nm[0], s = nm[TILE_ROWS * TILE_COLS];
#pragma unroll
          for (int c = 0; c < PV_CHUNK; ++c)
            if (c < cn) out[c >> 2][c & 3] = expf(out[c >> 2][c & 3] - mx) / s;
        }
#pragma unroll
        for (int c = 0; c < PV_CHUNK / 4; ++c) acc[c] += out[c];
      }
      float bv = c0 ? t_conf[row][lane] : -INFINITY;
      int bc = c0 ? t_lab[row][lane] : 0;
      const bool ok = yr < h && X0 + lane < w;
      float* pp = pb + (long long)c0 * cstride + min(yr, h - 1) * w + x;
#pragma unroll
      for (int c = 0; c < PV_CHUNK; ++c) {
        if (c < cn) {
          const float v = acc[c >> 2][c & 3] * inv_k;
          if (v > bv) { bv = v; bc = c0 + c; }
          if (pb && ok) pp[c * cstride] = v;
        }
      }
      t_conf[row][lane] = bv; t_lab[row][lane] = bc;
    }
  }
  __syncthreads();

  finish_tile(sc, reinterpret_cast<uint32_t*>(dyn), n, t_lab, t_conf, b, X0, Y0, xend, h, w, labels, label_bytes, conf, lane,
              wave);
}

// ---- labels from elsewhere (the CRF's argmax, another model) against ground truth ----
// count.h's walk over the label map with the ground truth as its second stream, into the scoring epilogues' table.
template <int LB, int GB>
__global__ __launch_bounds__(256) void seg_areas_kernel(const unsigned char* __restrict__ lab, const unsigned char* __restrict__ gt,
                                                        int head, int groups, int tail, int n, int raw,
                                                        unsigned long long* areas, unsigned long long* tally) {
  __shared__ uint32_t tab[3 * PT_MAX_CLASSES + 2];
  score_zero(tab, n);
  __syncthreads();
  int scored = 0, bad = 0;
  walk_pixels<LB, MapStream<GB>>(lab, gt, head, groups, tail,
                  [&](int pred, int g, bool live) { score_pixel(tab, n, raw, pred, g, live, scored, bad); });
  bins_flush(tab, 3 * n, scored, bad, areas, tally);
}

// ---- which class is taken for which: the confusion matrix of a label map ----
// confusion[c][p] counts the scored pixels of ground-truth class c with predicted label p; column n takes every label outside
// [0, n).  The walk over the two maps is seg_areas_kernel's, the table count.h's under the pair's key = c (n + 1) + p:
//   direct   n (n + 1) <= SC_DIRECT_MAX (n <= 127): uint32 [n][n + 1] in LDS
//   hashed   the matrix does not fit 64 KiB
constexpr int SC_DIRECT_MAX = 16384;     // table entries of the direct regime: 64 KiB
constexpr int SC_STEP_PIXELS = 256 * 16;  // the pixels a workgroup takes per step of the walk

__host__ __device__ inline bool sc_hashed(int n) { return n * (n + 1) > SC_DIRECT_MAX; }
__host__ __device__ inline int sc_dwords(int n) { return sc_hashed(n) ? 2 * SLOTS : n * (n + 1); }

template <int LB, int GB>
__global__ __launch_bounds__(256) void seg_confusion_kernel(const unsigned char* __restrict__ lab, const unsigned char* __restrict__ gt,
                                                            int head, int groups, int tail, int n, int raw,
                                                            unsigned long long* confusion) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ctab[];  // sc_dwords(n)
  const bool hashed = sc_hashed(n);                                // uniform over the grid
  const int dwords = sc_dwords(n);
  table_zero(ctab, hashed, dwords);
  walk_pixels<LB, MapStream<GB>>(lab, gt, head, groups, tail, [&](int pred, int g, bool live) {
    const GtClass t = gt_class(n, raw, g, live);
    const int col = (unsigned)pred < (unsigned)n ? pred : n;
    table_add(ctab, hashed, t.sc ? t.cls * (n + 1) + col : 0, t.sc, confusion);
  });
  table_flush(ctab, hashed, dwords, confusion);
}

// what the scoring entry points refuse on top of their predict counterparts
int score_refusal(const void* gt, int gt_bytes, const unsigned long long* areas, const unsigned long long* tally) {
  if (!gt || !areas || !tally || (gt_bytes != 1 && gt_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if (((size_t)areas & 7) || ((size_t)tally & 7) || ((size_t)gt & (size_t)(gt_bytes - 1))) return IFSEG_ERR_BAD_ARG;
  return 0;
}

// The tile grid of a launch, behind what all four launchers refuse, in this order.  src_ok: the launcher's own look at its
// scores or view table; grids_ok: its patch grids are at least 1 x 1 and small enough; scores: what has to be float-aligned.
// OPT (the scoring launches): labels may be null
struct TileGrid {
  int rc, tiles_x, tiles_y;
  long long blocks;
};
template <bool OPT>
TileGrid launch_grid(bool src_ok, bool grids_ok, const void* scores, int B, int n, int h, int w, const void* labels, int label_bytes,
                     const float* conf, const float* probs) {
  TileGrid g = {0, 0, 0, 0};
  (void)hipGetLastError();
  if (!src_ok) g.rc = IFSEG_ERR_BAD_ARG;
  else if ((!OPT || labels) && (!labels || (label_bytes != 1 && label_bytes != 2))) g.rc = IFSEG_ERR_BAD_ARG;
  else if (n < 1 || n > PT_MAX_CLASSES || (labels && label_bytes == 1 && n > 256)) g.rc = IFSEG_ERR_BAD_ARG;
  else if (B < 1 || !grids_ok || h < 1 || w < 1 || (long long)B * h * w >= (1ll << 31)) g.rc = IFSEG_ERR_BAD_SHAPE;
  // the wide stores of phase 2 want 16-byte aligned bases
  else if (((size_t)labels & 15) || ((size_t)conf & 15) || ((size_t)scores & 3) || ((size_t)probs & 3)) g.rc = IFSEG_ERR_BAD_ARG;
  else if (!tile_grid(h, w, B, &g.tiles_x, &g.tiles_y, &g.blocks)) g.rc = IFSEG_ERR_BAD_SHAPE;
  return g;
}

// the windows of an [oh, ow] plane whose windows ran the network on hpw x wpw grids; false: refused
bool make_slide(int hpw, int wpw, int oh, int ow, int crop_h, int crop_w, int stride_h, int stride_w, Slide* sl) {
  *sl = {{}, {}, hpw, wpw};
  if (hpw < 1 || wpw < 1 || !slide_axis(oh, crop_h, stride_h, &sl->y) || !slide_axis(ow, crop_w, stride_w, &sl->x)) return false;
  const long long nw = (long long)sl->y.g * sl->x.g;
  // offsets inside one image's windows are ints: Nw hpw wpw n < 2^31
  return nw <= SW_MAX_WINDOWS && nw * hpw * wpw < (1ll << 31) / PT_MAX_CLASSES;
}

// ifseg_seg_predict (S = NoScore) and ifseg_seg_score
template <typename S>
int launch_predict(const float* scores, int B, int hp, int wp, int n, int h, int w, void* labels, int label_bytes, float* conf,
                   float* probs, void* stream, S sc) {
  const bool grids_ok = hp >= 1 && wp >= 1 && (long long)hp * wp < (1ll << 31) / PT_MAX_CLASSES;
  const auto [rc, tiles_x, tiles_y, blocks] =
      launch_grid<S::on>(scores != nullptr, grids_ok, scores, B, n, h, w, labels, label_bytes, conf, probs);
  if (rc) return rc;
  // the scoring launches take their table out of the staging budget
  const int table = S::on ? score_dwords(n) * 4 : 0;
  const int lds = stage_bytes(hp, wp, n, h, w, std::min(g_stage_limit, PT_STAGE_LIMIT - table));
  hipLaunchKernelGGL(seg_predict_kernel<S>, dim3((unsigned)blocks), dim3(256), lds + table, (hipStream_t)stream, scores, hp, wp,
                     n, h, w, tiles_x, tiles_y, labels, label_bytes, conf, probs, lds / 4, sc);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

// ifseg_seg_predict_views (S = NoScore) and ifseg_seg_score_views
template <typename S>
int launch_views(const ifseg_predict_view* views, int K, int B, int n, int h, int w, void* labels, int label_bytes, float* conf,
                 float* probs, void* stream, S sc) {
  const auto [rc, tiles_x, tiles_y, blocks] =
      launch_grid<S::on>(views && K >= 1 && K <= PV_MAX_VIEWS, true, nullptr, B, n, h, w, labels, label_bytes, conf, probs);
  if (rc) return rc;
  ViewTable table = {};
  long long need = 0;
  for (int k = 0; k < K; ++k) {
    const ifseg_predict_view& v = views[k];
    if (!v.scores || ((size_t)v.scores & 3)) return IFSEG_ERR_BAD_ARG;
    if (v.hp < 1 || v.wp < 1 || (long long)v.hp * v.wp >= (1ll << 31) / PT_MAX_CLASSES) return IFSEG_ERR_BAD_SHAPE;
    table.v[k] = v;
    table.v[k].flip = v.flip != 0;
    need += footprint_bound(v.hp, v.hp, h, TILE_ROWS, 3) * footprint_bound(v.wp, v.wp, w, TILE_COLS, 3) * PV_STRIDE * 4;
  }
  // (the scoring table and) the coordinates come first; what the limit leaves is the staging buffer
  const int counters = S::on ? score_dwords(n) * 4 : 0;
  const int coords = K * PV_COORDS * 4;
  const int limit = std::min(g_views_stage_limit, PV_STAGE_LIMIT - counters);
  const int stage = (int)std::min<long long>(need, std::max(limit - coords, 0)) & ~15;
  hipLaunchKernelGGL(seg_predict_views_kernel<S>, dim3((unsigned)blocks), dim3(256), counters + coords + stage,
                     (hipStream_t)stream, table, K, (float)(1.0 / K), n, h, w, tiles_x, tiles_y, labels, label_bytes, conf,
                     probs, stage / 4, sc);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

// an upper bound, in bytes, of the source cells and the staged grid of any tile of an [h, w] output under the windows of sl.
// Per axis: the windows that hold any of the tile's plane footprint (a regular grid, + the pulled-back last one), times the
// patches of one window under it
long long slide_stage_bound(const Slide& sl, int h, int w) {
  auto axis_bound = [](const SlideAxis& a, int out, int grid, int tile) {
    const long long plane = footprint_bound(a.o, a.o, out, tile, 3);
    const long long windows = std::min<long long>(a.g, (plane + a.e - 1) / a.s + 2);
    return windows * footprint_bound(grid, grid, a.e, (int)std::min<long long>(plane, a.e), 3);
  };
  const long long fh = axis_bound(sl.y, h, sl.hpw, TILE_ROWS), fw = axis_bound(sl.x, w, sl.wpw, TILE_COLS);
  return (fh * fw * PV_STRIDE + fh + fw + 4) * 4;
}

// ifseg_seg_predict_windows (S = NoScore) and ifseg_seg_score_windows
template <typename S>
int launch_windows(const float* scores, int B, int hpw, int wpw, int n, int oh, int ow, int crop_h, int crop_w, int stride_h,
                   int stride_w, int h, int w, void* labels, int label_bytes, float* conf, float* probs, void* stream, S sc) {
  const auto [rc, tiles_x, tiles_y, blocks] =
      launch_grid<S::on>(scores != nullptr, hpw >= 1 && wpw >= 1, scores, B, n, h, w, labels, label_bytes, conf, probs);
  if (rc) return rc;
  Slide sl;
  if (!make_slide(hpw, wpw, oh, ow, crop_h, crop_w, stride_h, stride_w, &sl)) return IFSEG_ERR_BAD_SHAPE;
  const long long need = slide_stage_bound(sl, h, w);
  const int counters = S::on ? score_dwords(n) * 4 : 0;
  const int limit = std::max(std::min(g_windows_stage_limit, SW_STAGE_LIMIT - counters), 0);
  const int stage = (int)std::min<long long>(need, limit) & ~15;
  hipLaunchKernelGGL(seg_predict_windows_kernel<S>, dim3((unsigned)blocks), dim3(256), counters + stage, (hipStream_t)stream,
                     scores, sl, n, h, w, tiles_x, tiles_y, labels, label_bytes, conf, probs, stage / 4, sc);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

// the most LDS one workgroup of the current device may take, at least the 64 KiB every launch of this file assumes
int device_lds_limit() {
  int dev = 0, lim = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&lim, hipDeviceAttributeMaxSharedMemoryPerBlock, dev) != hipSuccess)
    (void)hipGetLastError();
  return std::min(std::max(lim, 65536), SV_LDS_CEILING);
}

// ifseg_seg_predict_slide_views (S = NoScore) and ifseg_seg_score_slide_views
template <typename S>
int launch_slide_views(const ifseg_slide_view* views, int K, int B, int n, int crop_h, int crop_w, int stride_h, int stride_w, int h,
                       int w, int softmax, void* labels, int label_bytes, float* conf, float* probs, void* stream, S sc) {
  const auto [rc, tiles_x, tiles_y, blocks] =
      launch_grid<S::on>(views && K >= 1 && K <= PV_MAX_VIEWS, true, nullptr, B, n, h, w, labels, label_bytes, conf, probs);
  if (rc) return rc;
  SlideViewTable table = {};
  long long need = 0;
  for (int k = 0; k < K; ++k) {
    const ifseg_slide_view& v = views[k];
    if (!v.scores || ((size_t)v.scores & 3)) return IFSEG_ERR_BAD_ARG;
    Slide sl;
    if (!make_slide(v.hpw, v.wpw, v.oh, v.ow, crop_h, crop_w, stride_h, stride_w, &sl)) return IFSEG_ERR_BAD_SHAPE;
    table.v[k] = {v.scores, sl, v.flip != 0};
    need += slide_stage_bound(sl, h, w);
  }
  // (the scoring table,) the per-view data and the normalisers come first; what the limit leaves is the staging buffer
  const int counters = S::on ? score_dwords(n) * 4 : 0;
  const int norms = softmax ? K * SV_NORM_DWORDS * 4 : 0;
  const int fixed = counters + K * SV_VIEW_DWORDS * 4 + norms;
  const int fixed_lds = PT_TILE_LDS + SV_META_LDS;
  const int total = softmax ? std::min(65536 + norms, device_lds_limit()) : 65536;
  if (fixed_lds + fixed > total) return IFSEG_ERR_BAD_SHAPE;     // a device whose LDS does not hold the normalisers
  const int limit = std::min(g_slide_views_stage_limit, total - fixed_lds - fixed);
  const int stage = (int)std::min<long long>(need, std::max(limit, 0)) & ~15;
  if (fixed_lds + fixed + stage > 65536)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&seg_predict_slide_views_kernel<S>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, fixed + stage);
  hipLaunchKernelGGL(seg_predict_slide_views_kernel<S>, dim3((unsigned)blocks), dim3(256), fixed + stage, (hipStream_t)stream,
                     table, K, (float)(1.0 / K), softmax != 0, n, h, w, tiles_x, tiles_y, labels, label_bytes, conf, probs,
                     stage / 4, sc);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

}  // namespace

extern "C" int ifseg_seg_predict_slide_views_staging(int max_bytes) {
  return swap_limit(g_slide_views_stage_limit, SV_STAGE_LIMIT, max_bytes);
}

extern "C" int ifseg_seg_predict_slide_views(const ifseg_slide_view* views, int K, int B, int n, int crop_h, int crop_w,
                                             int stride_h, int stride_w, int h, int w, int softmax, void* labels, int label_bytes,
                                             float* conf, float* probs, void* stream) {
  return launch_slide_views(views, K, B, n, crop_h, crop_w, stride_h, stride_w, h, w, softmax, labels, label_bytes, conf, probs,
                            stream, NoScore{});
}

extern "C" int ifseg_seg_score_slide_views(const ifseg_slide_view* views, int K, int B, int n, int crop_h, int crop_w, int stride_h,
                                           int stride_w, int h, int w, int softmax, void* labels, int label_bytes, float* conf,
                                           float* probs, const void* gt, int gt_bytes, int raw_labels, unsigned long long* areas,
                                           unsigned long long* tally, void* stream) {
  if (const int rc = score_refusal(gt, gt_bytes, areas, tally)) return rc;
  return launch_slide_views(views, K, B, n, crop_h, crop_w, stride_h, stride_w, h, w, softmax, labels, label_bytes, conf, probs,
                            stream, Score{gt, gt_bytes, raw_labels != 0, areas, tally});
}

extern "C" int ifseg_seg_predict_staging(int max_bytes) { return swap_limit(g_stage_limit, PT_STAGE_LIMIT, max_bytes); }

extern "C" int ifseg_seg_predict(const float* scores, int B, int hp, int wp, int n, int h, int w, void* labels, int label_bytes,
                                 float* conf, float* probs, void* stream) {
  return launch_predict(scores, B, hp, wp, n, h, w, labels, label_bytes, conf, probs, stream, NoScore{});
}

extern "C" int ifseg_seg_score(const float* scores, int B, int hp, int wp, int n, int h, int w, void* labels, int label_bytes,
                               float* conf, float* probs, const void* gt, int gt_bytes, int raw_labels,
                               unsigned long long* areas, unsigned long long* tally, void* stream) {
  if (const int rc = score_refusal(gt, gt_bytes, areas, tally)) return rc;
  return launch_predict(scores, B, hp, wp, n, h, w, labels, label_bytes, conf, probs, stream,
                        Score{gt, gt_bytes, raw_labels != 0, areas, tally});
}

extern "C" int ifseg_seg_predict_views_staging(int max_bytes) {
  return swap_limit(g_views_stage_limit, PV_STAGE_LIMIT, max_bytes);
}

extern "C" int ifseg_seg_predict_views(const ifseg_predict_view* views, int K, int B, int n, int h, int w, void* labels,
                                       int label_bytes, float* conf, float* probs, void* stream) {
  return launch_views(views, K, B, n, h, w, labels, label_bytes, conf, probs, stream, NoScore{});
}

extern "C" int ifseg_seg_score_views(const ifseg_predict_view* views, int K, int B, int n, int h, int w, void* labels,
                                     int label_bytes, float* conf, float* probs, const void* gt, int gt_bytes, int raw_labels,
                                     unsigned long long* areas, unsigned long long* tally, void* stream) {
  if (const int rc = score_refusal(gt, gt_bytes, areas, tally)) return rc;
  return launch_views(views, K, B, n, h, w, labels, label_bytes, conf, probs, stream,
                      Score{gt, gt_bytes, raw_labels != 0, areas, tally});
}

extern "C" int ifseg_seg_predict_windows_staging(int max_bytes) {
  return swap_limit(g_windows_stage_limit, SW_STAGE_LIMIT, max_bytes);
}

extern "C" int ifseg_seg_predict_windows(const float* scores, int B, int hpw, int wpw, int n, int oh, int ow, int crop_h,
                                         int crop_w, int stride_h, int stride_w, int h, int w, void* labels, int label_bytes,
                                         float* conf, float* probs, void* stream) {
  return launch_windows(scores, B, hpw, wpw, n, oh, ow, crop_h, crop_w, stride_h, stride_w, h, w, labels, label_bytes, conf, probs,
                        stream, NoScore{});
}

extern "C" int ifseg_seg_score_windows(const float* scores, int B, int hpw, int wpw, int n, int oh, int ow, int crop_h, int crop_w,
                                       int stride_h, int stride_w, int h, int w, void* labels, int label_bytes, float* conf,
                                       float* probs, const void* gt, int gt_bytes, int raw_labels, unsigned long long* areas,
                                       unsigned long long* tally, void* stream) {
  if (const int rc = score_refusal(gt, gt_bytes, areas, tally)) return rc;
  return launch_windows(scores, B, hpw, wpw, n, oh, ow, crop_h, crop_w, stride_h, stride_w, h, w, labels, label_bytes, conf, probs,
                        stream, Score{gt, gt_bytes, raw_labels != 0, areas, tally});
}

extern "C" int ifseg_seg_areas(const void* labels, int label_bytes, const void* gt, int gt_bytes, long long npix, int n,
                               int raw_labels, unsigned long long* areas, unsigned long long* tally, void* stream) {
  return walk_launch<true, false>({labels, label_bytes, gt, gt_bytes, nullptr}, areas, tally, n, PT_MAX_CLASSES, npix,
                                  [&](auto LB, auto GB, const WalkSplit& w) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_areas_kernel<LB(), GB()>), dim3(w.blocks), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)labels, (const unsigned char*)gt, w.head, w.groups, w.tail, n, raw_labels != 0, areas,
                       tally);
  });
}

extern "C" int ifseg_seg_confusion(const void* labels, int label_bytes, const void* gt, int gt_bytes, long long npix, int n,
                                   int raw_labels, unsigned long long* confusion, void* stream) {
  return walk_launch<true, false>({labels, label_bytes, gt, gt_bytes, nullptr}, confusion, confusion, n, PT_MAX_CLASSES, npix,
                                  [&](auto LB, auto GB, const WalkSplit& w) {
    hipLaunchKernelGGL(HIP_KERNEL_NAME(seg_confusion_kernel<LB(), GB()>), dim3(w.blocks), dim3(256),
                       (size_t)sc_dwords(n) * sizeof(uint32_t), (hipStream_t)stream, (const unsigned char*)labels,
                       (const unsigned char*)gt, w.head, w.groups, w.tail, n, raw_labels != 0, confusion);
  });
}

extern "C" int ifseg_seg_confusion_limit(int which) {
  switch (which) {
    case 0: return SC_DIRECT_MAX;
    case 1: return SLOTS;
    case 2: return SC_STEP_PIXELS;
    case 3: return MAX_BLOCKS;
    default: return IFSEG_ERR_BAD_ARG;
  }
}
