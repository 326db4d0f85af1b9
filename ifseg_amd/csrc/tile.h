// The 16 x 64 tile toolkit of the image-side resampling kernels (predict.hip, imgload.hip, trainload.hip).
//
// A workgroup of 256 threads owns a tile of TILE_ROWS x TILE_COLS destination pixels: lane = x, a wave takes 4 consecutive
// rows, so y (and with it the two source rows and the vertical weight) is wave-uniform.  Source coordinates are monotone in
// the destination, so the tile's first and last pixel bound its source footprint; the footprint is staged in LDS where it fits
// the buffer the host gave the launch and read from global memory otherwise.  Here: the tile decode, the two coordinate rules
// and the footprint on top of them, everything the two uint8 kernels share (staging with aligned dwords, the pixel loop, the
// plane stores, the NaN tile of a poisoned sample, which strong.hip stores too), the label halo of the two kernels that look at
// a label's neighbours (render.hip, pseudo.hip), and the host's grid / bound / staging-limit helpers.
#pragma once
#include <algorithm>
#include "common.h"

namespace tile {

constexpr int TILE_ROWS = 16, TILE_COLS = 64;

struct Tile {
  int b, X0, Y0, xend, yend, lane, wave;          // image, first pixel, one past the last one; wave is wave-uniform
};

// blockIdx.x -> the tile of a [B, h, w] destination cut into tiles_x x tiles_y tiles per image
__device__ __forceinline__ Tile tile_decode(int tiles_x, int tiles_y, int h, int w) {
  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const int X0 = tx * TILE_COLS, Y0 = ty * TILE_ROWS;
  return {b, X0, Y0, min(X0 + TILE_COLS, w), min(Y0 + TILE_ROWS, h), (int)(threadIdx.x & 63),
          __builtin_amdgcn_readfirstlane(threadIdx.x >> 6)};
}

// ---- the two coordinate rules of one axis: destination sample d -> source samples i0, i1 and the weight l of i1 ----
// They are NOT one rule in two notations: the float one is what F.interpolate computes, the integer one rounds its fraction
// once.  evalops.hip and resize.hip keep their own copies, contracted by the compiler in their own contexts.

// bilinear, align_corners=False, in integers: num = max((2 d + 1) in - out, 0), i0 = min(num / (2 out), in - 1).
// (2 d + 1) in - out and 2 out stay below 2^31: the callers refuse 2 in out >= 2^31
struct IntCoord {
  int in, out;
  __device__ __forceinline__ void operator()(int d, int* i0, int* i1, float* l) const {
    const int num = max((2 * d + 1) * in - out, 0), den = 2 * out;
    *i0 = min((int)((unsigned)num / (unsigned)den), in - 1);
    *i1 = min(*i0 + 1, in - 1);
    *l = *i0 == *i1 ? 0.f : (float)(num - *i0 * den) / (float)den;        // IEEE division: the fraction is rounded once
  }
};

// F.interpolate(bilinear, align_corners=False): src = (dst + 0.5) * in/out - 0.5, clamped at 0 (evalops.hip:102-107).  The
// fma is what the compiler contracted the expression to at every call; written out, so that it stays one rule for every caller
struct FloatCoord {
  float scale;                                    // (float)in / (float)out
  int in;
  __device__ __forceinline__ void operator()(int d, int* i0, int* i1, float* l) const {
    const float s = fmaxf(__builtin_fmaf((float)d + 0.5f, scale, -0.5f), 0.f);
    *i0 = min((int)s, in - 1);
    *i1 = min(*i0 + 1, in - 1);
    *l = s - (float)*i0;
  }
};

// the source samples lo..hi under the destination samples first..last of one axis
template <typename Coord>
__device__ __forceinline__ void footprint(const Coord& coord, int first, int last, int* lo, int* hi) {
  int t;
  float tf;
  coord(first, lo, &t, &tf);
  coord(last, &t, hi, &tf);
}

// ---- sliding windows (imgload.hip, predict.hip): mmseg's slide_inference rule on one axis ----
// An axis of o samples under crop c and stride s (1 <= s <= c) carries g = max(o - c + s - 1, 0) / s + 1 windows of
// e = min(c, o) samples; window i starts at max(min(i s + c, o) - c, 0): a regular grid whose last window is pulled back
// inside, so the starts increase strictly and the windows that hold a sample are a contiguous range of indices.
struct SlideAxis {
  int o, s, e, g;
  __host__ __device__ int start(int i) const {
    const int end = i * s + e < o ? i * s + e : o;
    return end - e;
  }
  // the first / last window that holds sample p (0 <= p < o)
  __host__ __device__ int first(int p) const {
    const int i = p < e ? 0 : (p - e) / s + 1;
    return i < g - 1 ? i : g - 1;
  }
  __host__ __device__ int last(int p) const { return p >= o - e ? g - 1 : p / s; }
};

// false for what the rule excludes (and for sizes whose i s + e would leave 31 bits)
inline bool slide_axis(int o, int c, int s, SlideAxis* a) {
  if (o < 1 || c < 1 || s < 1 || s > c || o >= (1 << 30) || c >= (1 << 30)) return false;
  *a = {o, s, std::min(c, o), std::max(o - c + s - 1, 0) / s + 1};
  return true;
}

// ---- uint8 HWC sources -> normalised planes (imgload.hip, trainload.hip) ----
// Dynamic LDS: the [3, 256] table first, the staged footprint behind it.
constexpr int U8_LUT_BYTES = 3 * 256 * 4;
constexpr int U8_STAGE_LIMIT = 65536 - U8_LUT_BYTES;              // 64 KiB of LDS per workgroup in all

// LDS bytes of one staged row of fw pixels: up to 3 bytes of shift in front, whole dwords
template <typename I>
__host__ __device__ inline I u8_rstride(I fw) { return (fw * 3 + 3 + 3) & ~(I)3; }

// where phase 1 reads the image from
struct U8Source {
  const unsigned char* sb;      // the image in global memory
  const unsigned char* row0;    // the first pixel of the footprint there
  const unsigned char* stage;   // the staged footprint
  int W0, ylo, xlo, rstride;
  bool staged;                  // workgroup-uniform
};

// phase 0: the footprint of destination rows yfirst..ylast and columns xfirst..xlast of image sb [H0, W0, 3] goes to LDS with
// ALIGNED dword loads where it fits stage_bytes: a source row is 3 W0 bytes and starts at any byte alignment, so every staged
// row begins at the dword that holds its first byte and keeps its own shift (0..3).  The caller's barrier publishes it
template <typename Coord>
__device__ __forceinline__ U8Source u8_stage(const unsigned char* sb, int W0, const Coord& cy, int yfirst, int ylast,
                                             const Coord& cx, int xfirst, int xlast, unsigned char* stage, int stage_bytes) {
  int ylo, yhi, xlo, xhi;
  footprint(cy, yfirst, ylast, &ylo, &yhi);
  footprint(cx, xfirst, xlast, &xlo, &xhi);
  const int fh = yhi - ylo + 1, fw = xhi - xlo + 1, rstride = u8_rstride(fw);
  const bool staged = (long long)fh * rstride <= (long long)stage_bytes;
  // footprint row ry starts at row0 + ry 3 W0: its shift is that address modulo 4
  const unsigned char* row0 = sb + ((long long)ylo * W0 + xlo) * 3;
  if (staged) {
    const int dpr = rstride >> 2;
    uint32_t* st32 = reinterpret_cast<uint32_t*>(stage);
    for (int i = threadIdx.x; i < fh * dpr; i += 256) {
      const int ry = i / dpr, k = i - ry * dpr;
      const unsigned char* a = row0 + (long long)ry * W0 * 3;
      const int sh = (int)((size_t)a & 3);
      // the dwords that hold at least one byte of the row's fw pixels: up to 3 bytes in front of the first pixel and behind the
      // last one are read with them, also in front of / behind the caller's buffer (an aligned dword never crosses a page)
      if (4 * k < sh + fw * 3) st32[i] = *reinterpret_cast<const uint32_t*>(a - sh + 4 * k);
    }
  }
  return {sb, row0, stage, W0, ylo, xlo, rstride, staged};
}

__device__ __forceinline__ void store_plane(float* out, long long e, bool ok, float v, int, int, int) {
  if (ok) out[e] = v;
}
// bf16: e = flat element index of the lane's pixel; pairs on even e.  The lane on an even e also takes its right neighbour's
// value and stores one dword; the odd element in front of a row's first pair and the even one behind its last leave as halves
__device__ __forceinline__ void store_plane(bf16_t* out, long long e, bool ok, float v, int lane, int x, int xend) {
  const uint32_t h = f2bf(v);
  const uint32_t right = (uint32_t)__shfl_down((int)h, 1);                // every lane takes part
  if (!ok) return;
  if ((e & 1) == 0) {
    if (lane < TILE_COLS - 1 && x + 1 < xend) *reinterpret_cast<uint32_t*>(out + e) = h | (right << 16);
    else out[e] = (bf16_t)h;
  } else if (lane == 0) {
    out[e] = (bf16_t)h;                                                   // (any other odd element left with lane - 1)
  }
}

// a poisoned sample (trainload.hip, strong.hip): NaN in the thread's four pixels of the three planes of an image of a
// [B, 3, P, P] batch.  img0: the image's first element, plane = P P, x = min(X0 + lane, P - 1): the callers hold all three,
// and taking theirs keeps the callers' register counts (recomputed here, the bf16 kernels needed one to three SGPRs more)
template <typename T>
__device__ __forceinline__ void store_nan_tile(T* out, long long img0, long long plane, int P, const Tile& t, int x) {
  const int X0 = t.X0, Y0 = t.Y0, xend = t.xend, lane = t.lane, wave = t.wave;
  const float nanv = __int_as_float(0x7fc00000);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yr = Y0 + wave * 4 + j;
    const bool ok = yr < P && X0 + lane < P;
    const long long erow = img0 + (long long)min(yr, P - 1) * P;
#pragma unroll
    for (int c = 0; c < 3; ++c) store_plane(out, erow + c * plane + x, ok, nanv, lane, x, xend);
  }
}

// the flat four-weight rule on grey levels: one rounded product and three fused multiply-adds, in this order.  These are the
// operations -ffp-contract=fast made of  w00 a + w01 b + w10 d + w11 e  in both kernels; contraction is off and they are
// written out, because which product the compiler leaves unfused depends on the code around the expression, and
// ifseg_train_load promises ifseg_image_load's bits.  (predict.hip's blend is another function: four rounded products.)
__device__ __forceinline__ float blend_u8(float w00, float w01, float w10, float w11, float a, float b, float d, float e) {
#pragma clang fp contract(off)
  return __builtin_fmaf(w11, e, __builtin_fmaf(w10, d, __builtin_fmaf(w00, a, w01 * b)));
}

// the thread's four pixels (rows j = 0..3 of its wave, one x), three channels each.  r0[j] / r1[j]: wave-uniform byte offset of
// the upper / lower source row from `base` (its shift included), o0 / o1: per-lane byte offset of the left / right pixel.
// hook(&r, &g, &b) works on the pixel's grey levels between the resize and the table; the channel reversal comes behind it
template <typename T, typename Ptr, typename Hook>
__device__ __forceinline__ void pixel_loop(Ptr base, const long long (&r0)[4], const long long (&r1)[4], int o0, int o1,
                                           const float (&ly)[4], float lx, const float* lut, bool rev, const Hook& hook, T* out,
                                           const long long (&erow)[4], long long plane, const bool (&ok)[4], int lane, int x,
                                           int xend) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float w00 = (1.f - ly[j]) * (1.f - lx), w01 = (1.f - ly[j]) * lx, w10 = ly[j] * (1.f - lx), w11 = ly[j] * lx;
    int q[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float a = (float)base[r0[j] + o0 + c], b = (float)base[r0[j] + o1 + c];
      const float d = (float)base[r1[j] + o0 + c], e = (float)base[r1[j] + o1 + c];
      q[c] = (int)fminf(fmaxf(floorf(blend_u8(w00, w01, w10, w11, a, b, d, e) + 0.5f), 0.f), 255.f);
    }
    hook(&q[0], &q[1], &q[2]);
#pragma unroll
    for (int c = 0; c < 3; ++c)
      store_plane(out, erow[j] + c * plane + x, ok[j], lut[c * 256 + q[rev ? 2 - c : c]], lane, x, xend);
  }
}

// phase 1 on either source: source rows y0[j], y1[j] and columns x0, x1 of the image, read where u8_stage left them
template <typename T, typename Hook>
__device__ __forceinline__ void u8_pixels(const U8Source& s, const int (&y0)[4], const int (&y1)[4], int x0, int x1,
                                          const float (&ly)[4], float lx, const float* lut, bool rev, const Hook& hook, T* out,
                                          const long long (&erow)[4], long long plane, const bool (&ok)[4], int lane, int x,
                                          int xend) {
  long long r0[4], r1[4];
  if (s.staged) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      r0[j] = (y0[j] - s.ylo) * s.rstride + (int)((size_t)(s.row0 + (long long)(y0[j] - s.ylo) * s.W0 * 3) & 3);
      r1[j] = (y1[j] - s.ylo) * s.rstride + (int)((size_t)(s.row0 + (long long)(y1[j] - s.ylo) * s.W0 * 3) & 3);
    }
    pixel_loop<T>(s.stage, r0, r1, (x0 - s.xlo) * 3, (x1 - s.xlo) * 3, ly, lx, lut, rev, hook, out, erow, plane, ok, lane, x,
                  xend);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) { r0[j] = (long long)y0[j] * s.W0 * 3; r1[j] = (long long)y1[j] * s.W0 * 3; }
    pixel_loop<T>(s.sb, r0, r1, x0 * 3, x1 * 3, ly, lx, lut, rev, hook, out, erow, plane, ok, lane, x, xend);
  }
}

// ---- the label halo of a tile (render.hip, pseudo.hip) ----
// The tile's labels plus the r pixels around it, as shorts in LDS rows of HALO_W; r <= HALO_MAX_R, which the launchers refuse
// beyond.
constexpr int HALO_MAX_R = 4;
constexpr int HALO_W = TILE_COLS + 2 * HALO_MAX_R, HALO_H = TILE_ROWS + 2 * HALO_MAX_R;

// phase 0: halo[hy][hx] = the label at (Y0 - r + hy, X0 - r + hx) of the image that starts at pix0.  The caller's barrier
// publishes it
template <typename L>
__device__ __forceinline__ void halo_stage(const L* labels, long long pix0, const Tile& t, int H, int W, int r, short* halo) {
  const int hw = TILE_COLS + 2 * r;
  for (int i = threadIdx.x; i < (TILE_ROWS + 2 * r) * hw; i += 256) {
    const int hy = i / hw, hx = i - hy * hw;
    // a neighbour outside the image reads the nearest pixel inside, which lies in the same window: it adds no edge
    const int y = min(max(t.Y0 - r + hy, 0), H - 1), x = min(max(t.X0 - r + hx, 0), W - 1);
    halo[hy * HALO_W + hx] = (short)labels[pix0 + (long long)y * W + x];
  }
}

// the tile's own label at row ry, column lane
__device__ __forceinline__ int halo_label(const short* halo, int ry, int lane, int r) { return halo[(ry + r) * HALO_W + lane + r]; }

// whether another label value than l lies within r pixels of it: the (2 r + 1)^2 window
__device__ __forceinline__ bool halo_differs(const short* halo, int ry, int lane, int r, int l) {
  bool edge = false;
  for (int dy = 0; dy <= 2 * r; ++dy)
    for (int dx = 0; dx <= 2 * r; ++dx) edge |= halo[(ry + dy) * HALO_W + lane + dx] != l;
  return edge;
}

// ---- host ----
// the body of an ifseg_*_staging setter: max_bytes < 0 restores the ceiling -> the previous limit
inline int swap_limit(int& limit, int ceiling, int max_bytes) {
  const int prev = limit;
  limit = max_bytes < 0 ? ceiling : std::min(max_bytes, ceiling);
  return prev;
}

// the launch grid of a [B, h, w] destination; false when it does not fit 31 bits
inline bool tile_grid(int h, int w, int B, int* tiles_x, int* tiles_y, long long* blocks) {
  *tiles_x = (w + TILE_COLS - 1) / TILE_COLS;
  *tiles_y = (h + TILE_ROWS - 1) / TILE_ROWS;
  *blocks = (long long)*tiles_x * *tiles_y * B;
  return *blocks < (1ll << 31);
}

// an upper bound of any tile's footprint on an axis of `axis` source samples resized at the ratio in / out: n destination
// samples span at most floor((n - 1) in/out) + 1 source samples, + 1 for the lower / right neighbour, + 1 for the rounding of
// the coordinate (slack 3; a caller whose ratio is itself rounded adds to it)
inline long long footprint_bound(long long axis, long long in, long long out, int n, int slack) {
  return std::min(axis, n * in / out + slack);
}

}  // namespace tile
