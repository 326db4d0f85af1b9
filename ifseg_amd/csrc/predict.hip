// Label maps at image resolution (the inference path of ifseg_amd/predict.py): bilinear resize of the per-patch class
// scores [B, hp*wp, n] to [B, h, w] (align_corners=False, any ratio -- the value rule of seg_eval_kernel in evalops.hip),
// argmax over the classes (first maximum), optionally the winning value and every interpolated value, in one pass: the
// [n, h, w] tensor is only written when the caller asks for it.
//
// A workgroup of 256 threads owns a tile of 16 rows x 64 pixels.
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
#include <algorithm>
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace {

constexpr int PT_ROWS = 16, PT_COLS = 64, PT_MAX_CLASSES = 512;
constexpr int PT_TILE_LDS = PT_ROWS * PT_COLS * 8;                // the label + conf tile of phase 2
constexpr int PT_STAGE_LIMIT = 65536 - PT_TILE_LDS;               // 64 KiB of LDS per workgroup in all

int g_stage_limit = PT_STAGE_LIMIT;

// LDS stride of one patch row of n classes, in floats: a multiple of 4 whose quarter is odd
__host__ __device__ inline int pt_stride(int n) {
  const int q = (n + 3) >> 2;
  return ((q & 1) ? q : q + 1) << 2;
}

// F.interpolate(bilinear, align_corners=False): src = (dst + 0.5) * in/out - 0.5, clamped at 0 (evalops.hip:102-107)
__device__ __forceinline__ void src_coord(int d, float scale, int in, int* i0, int* i1, float* l) {
  const float s = fmaxf(((float)d + 0.5f) * scale - 0.5f, 0.f);
  *i0 = min((int)s, in - 1);
  *i1 = min(*i0 + 1, in - 1);
  *l = s - (float)*i0;
}

struct Best {
  float v;
  int c;
};

// one class of one pixel: the flat four-weight rule, first maximum wins
__device__ __forceinline__ float blend(float w00, float w01, float w10, float w11, float a, float b, float c, float d) {
  return w00 * a + w01 * b + w10 * c + w11 * d;
}

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

__global__ __launch_bounds__(256) void seg_predict_kernel(const float* __restrict__ scores, int hp, int wp, int n, int h, int w,
                                                          int tiles_x, int tiles_y, void* __restrict__ labels, int label_bytes,
                                                          float* __restrict__ conf, float* __restrict__ probs,
                                                          int stage_floats) {
  extern __shared__ __attribute__((aligned(16))) float stage[];
  __shared__ int t_lab[PT_ROWS][PT_COLS];
  __shared__ float t_conf[PT_ROWS][PT_COLS];

  const int tx = blockIdx.x % tiles_x, ty = (blockIdx.x / tiles_x) % tiles_y, b = blockIdx.x / (tiles_x * tiles_y);
  const int X0 = tx * PT_COLS, Y0 = ty * PT_ROWS;
  const int xend = min(X0 + PT_COLS, w), yend = min(Y0 + PT_ROWS, h);
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const float sy = (float)hp / (float)h, sx = (float)wp / (float)w;
  const float* sb = scores + (long long)b * hp * wp * n;

  // the tile's footprint: source coordinates are monotone in the destination, so the first and the last pixel bound it
  int ylo, yhi, xlo, xhi, t0;
  float tf;
  src_coord(Y0, sy, hp, &ylo, &t0, &tf);
  src_coord(yend - 1, sy, hp, &t0, &yhi, &tf);
  src_coord(X0, sx, wp, &xlo, &t0, &tf);
  src_coord(xend - 1, sx, wp, &t0, &xhi, &tf);
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
  src_coord(x, sx, wp, &x0, &x1, &lx);
  int y0[4], y1[4];
  float ly[4];
  bool fresh[4], ok[4];
  int pofs[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yr = Y0 + wave * 4 + j, y = min(yr, h - 1);
    src_coord(y, sy, hp, &y0[j], &y1[j], &ly[j]);
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

  // phase 2: 16 lanes per row; lane k takes the aligned quad at X0 - a + 4k, lanes k < a also one pixel of the last a
  const int r = threadIdx.x >> 4, k = threadIdx.x & 15, y = Y0 + r;
  if (y >= h) return;
  const long long row = ((long long)b * h + y) * w;
  const int a = (int)((row + X0) & 3);
  unsigned char* l8 = (unsigned char*)labels;
  short* l16 = (short*)labels;
  auto put = [&](int xx) {
    const int v = t_lab[r][xx - X0];
    if (label_bytes == 1) l8[row + xx] = (unsigned char)v; else l16[row + xx] = (short)v;
    if (conf) conf[row + xx] = t_conf[r][xx - X0];
  };
  const int xs = X0 - a + 4 * k;
  if (xs >= X0 && xs + 4 <= xend) {
    const int* tl = &t_lab[r][xs - X0];
    if (label_bytes == 1)
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
  if (k < a && X0 + PT_COLS - a + k < xend) put(X0 + PT_COLS - a + k);
}

}  // namespace

extern "C" int ifseg_seg_predict_staging(int max_bytes) {
  const int prev = g_stage_limit;
  g_stage_limit = max_bytes < 0 ? PT_STAGE_LIMIT : (max_bytes < PT_STAGE_LIMIT ? max_bytes : PT_STAGE_LIMIT);
  return prev;
}

extern "C" int ifseg_seg_predict(const float* scores, int B, int hp, int wp, int n, int h, int w, void* labels, int label_bytes,
                                 float* conf, float* probs, void* stream) {
  (void)hipGetLastError();
  if (!scores || !labels || (label_bytes != 1 && label_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if (n < 1 || n > PT_MAX_CLASSES || (label_bytes == 1 && n > 256)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || hp < 1 || wp < 1 || h < 1 || w < 1) return IFSEG_ERR_BAD_SHAPE;
  if ((long long)B * h * w >= (1ll << 31) || (long long)hp * wp >= (1ll << 31) / PT_MAX_CLASSES) return IFSEG_ERR_BAD_SHAPE;
  // the wide stores of phase 2 want 16-byte aligned bases
  if (((size_t)labels & 15) || ((size_t)conf & 15) || ((size_t)scores & 3) || ((size_t)probs & 3)) return IFSEG_ERR_BAD_ARG;
  const int tiles_x = (w + PT_COLS - 1) / PT_COLS, tiles_y = (h + PT_ROWS - 1) / PT_ROWS;
  const long long blocks = (long long)tiles_x * tiles_y * B;
  if (blocks >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  // an upper bound of any tile's footprint: R destination rows span at most floor((R - 1) in/out) + 1 source rows, + 1 for the
  // lower neighbour, + 1 for the rounding of the coordinate
  const long long fh = std::min<long long>(hp, (long long)PT_ROWS * hp / h + 3), fw = std::min<long long>(wp, (long long)PT_COLS * wp / w + 3);
  const long long need = fh * fw * pt_stride(n) * 4;
  const int lds = (int)std::min<long long>(need, g_stage_limit) & ~15;
  hipLaunchKernelGGL(seg_predict_kernel, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, scores, hp, wp, n, h, w,
                     tiles_x, tiles_y, labels, label_bytes, conf, probs, lds / 4);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
