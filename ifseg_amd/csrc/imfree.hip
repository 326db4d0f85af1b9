// Image-free training samples on the device (the `rand_k-L-R` artificial image of data/mm_data/segmentation_dataset.py:303-345
// and its collater layout :85-107): a random sh x sw class map per sample, nearest-resized to the patch grid (EmbeddingBag ids /
// ends of the class names, prev_output_tokens) and to the image (text2seg_target).  ifseg_amd/artificial.py holds the same stream
// and the same index rule in plain torch / numpy: the kernels are compared against it bit for bit.
//
//   ifseg_imfree_draw    shapes, coarse  <- splitmix64(seed + (ordinal << 32) + i)                 one launch
//   ifseg_imfree_expand  ids, ends, prev_output_tokens (one workgroup per sample: the scan)         two launches
//                        text2seg_target (the bandwidth part: B * (S_h * S_w + 1) * 8 bytes)
//
// Every launch shape depends on the arguments only (never on drawn data), nothing is read back: capturable into a HIP graph;
// with the ordinal in a device word a replayed graph draws new images.  The counter stream and the ordinal check: common.h.
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace {

// PyTorch's `nearest` source index (UpSampleKernel.cpp nearest_idx: floorf(dst * scale), scale = (float)in / (float)out, in fp32).
// The integer rule (dst * in) / out is NOT the same map: in = 84, out = 40 or 640 differ.
__device__ __forceinline__ int nearest_src(int dst, float scale, int in) {
  return min((int)floorf((float)dst * scale), in - 1);
}
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(256) void imfree_draw_kernel(unsigned long long seed, unsigned long long first, const long long* first_dev,
                                                          int l, int r, int nseg, int* shapes, int* coarse) {
  const int b = blockIdx.y, cs = (r - 1) * (r - 1);
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= (unsigned)cs) return;
  const unsigned long long base = stream_base(seed, first_dev ? (unsigned long long)*first_dev : first, b);
  const int sh = l + draw_below(base, 0, r - l), sw = l + draw_below(base, 1, r - l);
  if (i == 0) {
    shapes[2 * b] = sh;
    shapes[2 * b + 1] = sw;
  }
  coarse[(long long)b * cs + i] = i < (unsigned)(sh * sw) ? draw_below(base, 2 + i, nseg) : 0;
}

// One workgroup per sample: low-res map on the hp x wp grid, prev_output_tokens, the inclusive scan of the name lengths (256 bags
// per pass, the running total carried from pass to pass), the bags' tokens at their scanned positions and `pad` behind them.
// A class outside [0, nseg] and a name length outside [0, Lmax] are clamped: no write can leave ids[b, 0 : P * Lmax).
__global__ __launch_bounds__(256) void imfree_bags_kernel(const int* shapes, const int* coarse, int max_side, const long long* name_ids,
                                                          const int* name_len, int nseg, int Lmax, int hp, int wp, long long seg0,
                                                          long long bos, long long pad, long long* ids, long long* ends,
                                                          long long* prev) {
  __shared__ int wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int P = hp * wp, W = P * Lmax;
  const int sh = clampi(shapes[2 * b], 1, max_side), sw = clampi(shapes[2 * b + 1], 1, max_side);
  const float scale_h = (float)sh / (float)hp, scale_w = (float)sw / (float)wp;
  const int* cm = coarse + (long long)b * max_side * max_side;
  long long* ids_b = ids + (long long)b * W;
  long long* prev_b = prev + (long long)b * (P + 1);
  if (tid == 0) prev_b[0] = bos;
  int carry = 0;
  for (int base = 0; base < P; base += 256) {
    const int p = base + tid;
    int cls = 0, len = 0;
    if (p < P) {
      const int py = p / wp, px = p - py * wp;
      cls = clampi(cm[nearest_src(py, scale_h, sh) * sw + nearest_src(px, scale_w, sw)], 0, nseg);
      len = clampi(name_len[cls], 0, Lmax);
      prev_b[1 + p] = seg0 + cls;
    }
    int v = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o);
      if (lane >= o) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int woff = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int s = wsum[w];
      woff += w < wave ? s : 0;
      total += s;
    }
    if (p < P) {
      const int incl = carry + woff + v, start = incl - len;
      ends[(long long)b * P + p] = incl;
      for (int k = 0; k < len; ++k) ids_b[start + k] = name_ids[(long long)cls * Lmax + k];
    }
    carry += total;
    __syncthreads();      // wsum is rewritten by the next pass
  }
  for (int j = carry + tid; j < W; j += 256) ids_b[j] = pad;
}

// text2seg_target[b] = seg0 + coarse[iy(y)][ix(x)] for the S_h x S_w pixels, then eos.  A row holds S_h * S_w + 1 elements (odd),
// so rows alternate between 16-byte aligned and not: the first element of a misaligned row and the last element of a row whose
// remainder is odd are written alone, everything between as 16-byte stores (two elements per lane, consecutive lanes consecutive).
// The clamped coarse map (16 bit) and the per-column source index (8 bit) live in LDS; the row index costs one multiply per pair.
constexpr int TGT_PAIRS = 8;      // 16-byte stores per thread: 32 KiB of the row per workgroup
__global__ __launch_bounds__(256) void imfree_target_kernel(const int* shapes, const int* coarse, int max_side, int nseg, int S_h, int S_w,
                                                            long long seg0, long long eos, long long* target) {
  extern __shared__ __align__(16) unsigned char smem[];
  unsigned short* cm = reinterpret_cast<unsigned short*>(smem);
  unsigned char* ixt = smem + ((max_side * max_side * 2 + 15) & ~15);
  const int b = blockIdx.y, tid = threadIdx.x;
  const int sh = clampi(shapes[2 * b], 1, max_side), sw = clampi(shapes[2 * b + 1], 1, max_side);
  const int* src = coarse + (long long)b * max_side * max_side;
  for (int i = tid; i < sh * sw; i += 256) cm[i] = (unsigned short)clampi(src[i], 0, nseg);
  const float scale_h = (float)sh / (float)S_h, scale_w = (float)sw / (float)S_w;
  for (int x = tid; x < S_w; x += 256) ixt[x] = (unsigned char)nearest_src(x, scale_w, sw);
  __syncthreads();
  const int N = S_h * S_w + 1;
  long long* row = target + (long long)b * N;
  const int head = (int)((reinterpret_cast<uintptr_t>(row) >> 3) & 1);
  const int npairs = (N - head) >> 1;
  if (blockIdx.x == 0) {
    if (tid == 0 && head) row[0] = seg0 + cm[ixt[0]];                 // pixel (0, 0): source row 0
    if (tid == 1 && ((N - head) & 1)) row[N - 1] = eos;
  }
#pragma unroll
  for (int j = 0; j < TGT_PAIRS; ++j) {
    const int k = (blockIdx.x * TGT_PAIRS + j) * 256 + tid;
    if (k >= npairs) break;
    const int e = head + 2 * k;                                        // e + 1 <= N - 1
    const int y = e / S_w, x = e - y * S_w;
    const int r0 = nearest_src(y, scale_h, sh) * sw;
    longlong2 v;
    v.x = seg0 + cm[r0 + ixt[x]];
    if (e + 1 == N - 1)
      v.y = eos;
    else if (x + 1 < S_w)
      v.y = seg0 + cm[r0 + ixt[x + 1]];
    else
      v.y = seg0 + cm[nearest_src(y + 1, scale_h, sh) * sw + ixt[0]];
    *reinterpret_cast<longlong2*>(row + e) = v;
  }
}

}  // namespace

extern "C" int ifseg_imfree_draw(unsigned long long seed, long long first_ordinal, const long long* first_ordinal_dev, int B, int l,
                                 int r, int nseg, int* shapes, int* coarse, void* stream) {
  (void)hipGetLastError();
  if (l < 1 || l >= r || r > 129 || nseg < 1 || nseg > 65535) return IFSEG_ERR_BAD_ARG;
  if (!first_ordinal_dev && !ordinals_ok(first_ordinal, B)) return IFSEG_ERR_BAD_ARG;
  if (B <= 0) return 0;
  if (B > 65535) return IFSEG_ERR_BAD_SHAPE;
  const int cs = (r - 1) * (r - 1);
  hipLaunchKernelGGL(imfree_draw_kernel, dim3((cs + 255) / 256, B), dim3(256), 0, (hipStream_t)stream, seed,
                     (unsigned long long)first_ordinal, first_ordinal_dev, l, r, nseg, shapes, coarse);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_imfree_expand(const int* shapes, const int* coarse, int max_side, const long long* name_ids, const int* name_len,
                                   int nseg, int Lmax, int B, int hp, int wp, long long seg_id_offset, long long bos, long long eos,
                                   long long pad, long long* ids, long long* ends, long long* prev_output_tokens,
                                   long long* text2seg_target, void* stream) {
  (void)hipGetLastError();
  if (max_side < 1 || max_side > 128 || nseg < 1 || nseg > 65535 || Lmax < 1 || Lmax > 16) return IFSEG_ERR_BAD_ARG;
  if (hp < 1 || wp < 1 || (long long)hp * wp > 4096) return IFSEG_ERR_BAD_SHAPE;
  if (B <= 0) return 0;
  if (B > 65535) return IFSEG_ERR_BAD_SHAPE;
  const int S_h = 16 * hp, S_w = 16 * wp;
  const size_t lds = (size_t)((max_side * max_side * 2 + 15) & ~15) + (size_t)S_w;
  if (lds > 64 * 1024) return IFSEG_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(imfree_bags_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, shapes, coarse, max_side, name_ids, name_len, nseg,
                     Lmax, hp, wp, seg_id_offset, bos, pad, ids, ends, prev_output_tokens);
  IFSEG_CHECK_LAUNCH();
  const int npairs = (S_h * S_w + 1) / 2;      // of an aligned row; a misaligned one has as many
  hipLaunchKernelGGL(imfree_target_kernel, dim3((npairs + TGT_PAIRS * 256 - 1) / (TGT_PAIRS * 256), B), dim3(256), lds,
                     (hipStream_t)stream, shapes, coarse, max_side, nseg, S_h, S_w, seg_id_offset, eos, text2seg_target);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
