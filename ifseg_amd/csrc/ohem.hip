// Online hard example mining for the fused segmentation loss (gfx950): mmseg's OHEMPixelSampler with `thresh` given, as a
// producer of the uint8 weight plane ifseg_seg_loss_tiles_weighted reads.  criterions/seg_criterion.py states the rule
// (hardness_reference, ohem_reference); include/ifseg_hip.h the entry points.
//
//   seg_hardness_kernel   the front half of loss.hip's tile kernel, from seg_tile.h: one workgroup per low-res cell = one 16 x 16
//                         pixel tile, the 3 x 3 cells staged in LDS at an odd row stride, the four-tap value(c), one
//                         online-softmax walk -> p = softmax(v)[y] clamped to <= 1, or -1 on a pixel that is no class, as an
//                         fp32 plane [B, H*W].  The [B, H*W, nseg] scores are never built.
//   the select            an exact k-th smallest over the candidates (bit patterns 0 .. 0x3F800000) of the whole batch by a
//                         most-significant-digit radix select: three digits of 10 bits over the 30 significant key bits.
//                         Four launches, nothing read back:
//                           ohem_hist_kernel<0|1|2>   a walk over the plane; a workgroup counts digit D of the keys that share
//                                                     the digits already picked in count.h's direct LDS table (1024 bins, 4 KiB)
//                                                     and flushes its non-zero bins with 64-bit atomics.  Every workgroup redoes
//                                                     the prefix scan of the previous digit's histogram; workgroup 0 writes what
//                                                     it picked to the state words for the launch after the next.
//                           ohem_apply_kernel         picks the last digit, tau = max(thresh, k-th), writes the plane and info
//                         The counters are integers: the result is bit-reproducible.
// Workspace (uint64 [OHEM_WORK_WORDS], zeroed once when it is allocated): three histograms and 16 state words.  A launch zeroes
// only what no workgroup of the same launch reads: pass 0 the histograms of digits 1 and 2, pass 1 the below-thresh counter it has
// just copied, the apply launch the histogram of digit 0; the last workgroup of the apply launch to have read the state and the
// third histogram zeroes those and the second -- so a call leaves the workspace as it found it, every word zero.
#include <string.h>
#include "count.h"
#include "seg_tile.h"

namespace {

using namespace count;
using namespace seg_tile;

__global__ __launch_bounds__(256) void seg_hardness_kernel(const bf16_t* logits, int ldl, long long lbs, const long long* target,
                                                           long long tbs, int hp, int wp, int W, int nseg, long long seg0,
                                                           long long pad_id, long long eos_id, float* hardness, long long hbs) {
  extern __shared__ float dyn[];
  const int ls = nseg | 1;
  float* sLog = dyn;                         // [9][ls]
  __shared__ float sWY[TS][3], sWX[TS][3];
  const int tid = threadIdx.x;
  const int ncell = hp * wp;
  const int b = blockIdx.x / ncell, cell = blockIdx.x % ncell;
  const int cy = cell / wp, cx = cell % wp;

  stage_cells(sLog, ls, logits, ldl, lbs, b, cy, cx, hp, wp, nseg);
  stage_weights(sWY, sWX, cy, cx, hp, wp);
  __syncthreads();

  const int py = tid >> 4, px = tid & 15;
  const Taps value(ls, sWY, sWX, py, px);
  const long long pix = (long long)(cy * TS + py) * W + (cx * TS + px);
  const long long tg = target[b * tbs + pix];
  const bool valid = is_class(tg, seg0, nseg, pad_id, eos_id);
  const int label = valid ? (int)(tg - seg0) : 0;
  // p = exp(v_y - lse) as exp(v_y - m) / sum.  The plane feeds an order statistic and must sit within 4 e of the specification,
  // e a fraction of an ulp of p at 150 classes: the accurate expf, the sum of up to 512 terms kept in fp64 (an fp32 running sum
  // alone measured 4.3 e at 150 classes) and the one exponential of the result in fp64.  Not on the step's critical path.
  float m = -INFINITY, vl = 0.f;
  double sum = 0.0;
  for (int c = 0; c < nseg; ++c) {
    const float v = value(sLog, c);
    if (v > m) { sum = sum * exp((double)(m - v)) + 1.0; m = v; }   // (rare: it scales the whole sum, so in fp64 as well)
    else sum += (double)expf(v - m);
    if (c == label) vl = v;
  }
  hardness[b * hbs + pix] = valid ? fminf((float)(exp((double)(vl - m)) / sum), 1.f) : -1.f;
}

// ---- the select ----
constexpr int DIGIT_BITS = 10;
constexpr int BINS = 1 << DIGIT_BITS;          // 1024: 4 KiB of uint32 in LDS, count.h's direct regime
constexpr uint32_t KEY_MAX = 0x3F800000u;      // bits of 1.0f: a candidate is 0 <= v <= 1 with the sign bit clear
constexpr int STATE = 3 * BINS;                // the state words behind the three histograms
// state words (uint64)
constexpr int S_BELOW_T = 0;   // pass 0 counts the candidates below thresh here; pass 1 copies it to S_BT and clears it
constexpr int S_NVALID = 1;    // the number of candidates (pass 1)
constexpr int S_D0 = 2;        // the picked first digit, the candidates below its bin, the rank left inside it (pass 1)
constexpr int S_LOW0 = 3;
constexpr int S_K1 = 4;
constexpr int S_BT = 5;
constexpr int S_D1 = 6;        // the same for the second digit (pass 2); S_LOW1 counts the candidates below (D0, D1)
constexpr int S_LOW1 = 7;
constexpr int S_K2 = 8;
constexpr int S_DONE = 9;      // the workgroups of the apply launch that have read the state (the last one zeroes it)
constexpr int OHEM_WORK_WORDS = STATE + 16;  // == hip.OHEM_WORK_WORDS

typedef unsigned long long u64;

// the smallest bin d with hist[0] + .. + hist[d] > k, and the sum below it; every lane of the workgroup gets both.
// total <= k (an empty histogram): d = 0, low = 0.
__device__ __forceinline__ void pick_digit(const u64* hist, u64 k, u64* scan /* LDS [256] */, u64* pick /* LDS [2] */, int* d,
                                           u64* low) {
  const int tid = threadIdx.x;
  u64 h[4], t = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) { h[i] = hist[4 * tid + i]; t += h[i]; }
  if (tid < 2) pick[tid] = 0;
  scan[tid] = t;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const u64 v = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += v;
    __syncthreads();
  }
  u64 ex = scan[tid] - t;
  if (ex <= k && k < ex + t) {                 // at most one lane
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (k < ex + h[i]) { pick[0] = (u64)(4 * tid + i); pick[1] = ex; break; }
      ex += h[i];
    }
  }
  __syncthreads();
  *d = (int)pick[0];
  *low = pick[1];
  __syncthreads();
}

__device__ __forceinline__ u64 kth_rank(u64 nvalid, long long min_kept, int B) {
  const u64 want = (u64)min_kept * (u64)B;     // min_kept < 2^40, B < 2^20 (the host's checks)
  return nvalid ? (want < nvalid - 1 ? want : nvalid - 1) : 0;
}

// PASS 0: the first digit of every candidate, and the candidates below thresh
// PASS 1: picks the first digit; the second digit of the candidates inside it
// PASS 2: picks the second digit; the third digit of the candidates inside (D0, D1)
template <int PASS>
__global__ __launch_bounds__(256) void ohem_hist_kernel(const float* __restrict__ hardness, long long total, int B,
                                                        uint32_t thresh_bits, long long min_kept, u64* work) {
  __shared__ __attribute__((aligned(16))) uint32_t tab[BINS];
  __shared__ u64 sScan[256], sPick[2];
  u64* state = work + STATE;
  const int tid = threadIdx.x;
  table_zero(tab, false, BINS);
  uint32_t prefix = 0;                          // the digits picked so far, in place
  if constexpr (PASS == 0) {
    if (blockIdx.x == 0)
      for (int i = tid; i < 2 * BINS; i += 256) work[BINS + i] = 0;
  } else if constexpr (PASS == 1) {
    u64 nvalid = 0;
    for (int i = tid; i < BINS; i += 256) nvalid += work[i];
    // the total of the first histogram: sScan is free until pick_digit
    sScan[tid] = nvalid;
    __syncthreads();
    if (tid == 0) {
      u64 s = 0;
      for (int i = 0; i < 256; ++i) s += sScan[i];
      sPick[0] = s;
    }
    __syncthreads();
    nvalid = sPick[0];
    __syncthreads();
    int d0;
    u64 low0;
    const u64 k = kth_rank(nvalid, min_kept, B);
    pick_digit(work, k, sScan, sPick, &d0, &low0);
    prefix = (uint32_t)d0 << (2 * DIGIT_BITS);
    if (blockIdx.x == 0 && tid == 0) {
      state[S_NVALID] = nvalid;
      state[S_D0] = (u64)d0;
      state[S_LOW0] = low0;
      state[S_K1] = k - low0;
      state[S_BT] = state[S_BELOW_T];
      state[S_BELOW_T] = 0;
    }
  } else {
    const int d0 = (int)state[S_D0];
    const u64 k1 = state[S_K1], low0 = state[S_LOW0];
    int d1;
    u64 low1;
    pick_digit(work + BINS, k1, sScan, sPick, &d1, &low1);
    prefix = (uint32_t)d0 << (2 * DIGIT_BITS) | (uint32_t)d1 << DIGIT_BITS;
    if (blockIdx.x == 0 && tid == 0) {
      state[S_D1] = (u64)d1;
      state[S_LOW1] = low0 + low1;
      state[S_K2] = k1 - low1;
    }
  }
  constexpr int SHIFT = (2 - PASS) * DIGIT_BITS;
  int below = 0;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // whole (converged) waves reach table_add: the loop's bound is the wave's
  for (long long base = (long long)blockIdx.x * 256 + wave * 64; base < total; base += (long long)gridDim.x * 256) {
    const long long i = base + lane;
    const uint32_t key = i < total ? __float_as_uint(hardness[i]) : 0xffffffffu;
    bool on = key <= KEY_MAX;
    if constexpr (PASS == 0) below += on && key < thresh_bits;
    else on = on && (key >> (SHIFT + DIGIT_BITS)) == (prefix >> (SHIFT + DIGIT_BITS));
    table_add(tab, false, (int)((key >> SHIFT) & (BINS - 1)), on, work + PASS * BINS);
  }
  if constexpr (PASS == 0) {
#pragma unroll
    for (int o = 32; o; o >>= 1) below += __shfl_xor(below, o);
    if (lane == 0 && below) atomicAdd(&state[S_BELOW_T], (u64)below);
  }
  table_flush(tab, false, BINS, work + PASS * BINS);
}

__global__ __launch_bounds__(256) void ohem_apply_kernel(const float* __restrict__ hardness, long long total, uint32_t thresh_bits,
                                                         const unsigned char* __restrict__ weight, unsigned char* __restrict__ out,
                                                         long long* info, u64* work) {
  __shared__ u64 sScan[256], sPick[2];
  u64* state = work + STATE;
  const int tid = threadIdx.x;
  const u64 nvalid = state[S_NVALID];
  int d2;
  u64 low2;
  pick_digit(work + 2 * BINS, state[S_K2], sScan, sPick, &d2, &low2);
  const uint32_t kth = nvalid ? ((uint32_t)state[S_D0] << (2 * DIGIT_BITS) | (uint32_t)state[S_D1] << DIGIT_BITS | (uint32_t)d2) : 0u;
  const uint32_t tau = thresh_bits > kth ? thresh_bits : kth;
  if (blockIdx.x == 0) {
    // nobody reads the first histogram in this launch: cleared for the next call
    for (int i = tid; i < BINS; i += 256) work[i] = 0;
    if (tid == 0) {
      info[0] = (long long)nvalid;
      // the candidates below tau: counted by pass 0 when thresh decides, else the sums below the three picked bins
      info[1] = (long long)(!nvalid ? 0 : thresh_bits > kth ? state[S_BT] : state[S_LOW1] + low2);
      info[2] = (long long)tau;
      info[3] = (long long)kth;
    }
  }
  // every read of the state and of the last histogram lies above this line: the last workgroup to get here zeroes them (and the
  // second histogram), so that the workspace is all zeros again after the call.  An integer count, no waiting.
  __shared__ int sLast;
  __syncthreads();
  if (tid == 0) {
    __threadfence();
    sLast = atomicAdd(&state[S_DONE], (u64)1) == (u64)gridDim.x - 1;
  }
  __syncthreads();
  if (sLast) {
    __threadfence();
    for (int i = tid; i < 2 * BINS + 16; i += 256) work[BINS + i] = 0;
  }
  for (long long i = (long long)blockIdx.x * 256 + tid; i < total; i += (long long)gridDim.x * 256) {
    const uint32_t key = __float_as_uint(hardness[i]);
    const bool keep = key <= KEY_MAX && key < tau;   // strict: the pixels that tie with the k-th value are dropped
    out[i] = keep ? (weight ? weight[i] : (unsigned char)255) : (unsigned char)0;
  }
}

}  // namespace

extern "C" int ifseg_seg_hardness(const void* logits, int ldl, long long logits_bs, const long long* target, long long target_bs,
                                  int B, int hp, int wp, int H, int W, int nseg, long long seg_id_offset, long long pad_id,
                                  long long eos_id, float* hardness, long long hardness_bs, void* stream) {
  (void)hipGetLastError();
  if (!hardness || ((size_t)hardness & 3)) return IFSEG_ERR_BAD_ARG;
  if (const int rc = check_tile_args(logits, ldl, logits_bs, target, target_bs, B, hp, wp, H, W, nseg)) return rc;
  if (hardness_bs < (long long)H * W) return IFSEG_ERR_BAD_ARG;
  const size_t dyn = (size_t)(9 * (nseg | 1)) * 4;
  hipLaunchKernelGGL(seg_hardness_kernel, dim3(B * hp * wp), dim3(256), dyn, (hipStream_t)stream, (const bf16_t*)logits, ldl,
                     logits_bs, target, target_bs, hp, wp, W, nseg, seg_id_offset, pad_id, eos_id, hardness, hardness_bs);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_ohem_select(const float* hardness, int B, long long n, float thresh, long long min_kept,
                                 const unsigned char* weight, unsigned char* out, long long* info,
                                 unsigned long long* work, void* stream) {
  (void)hipGetLastError();
  if (!hardness || !out || !info || !work || ((size_t)hardness & 3) || ((size_t)info & 7) || ((size_t)work & 7))
    return IFSEG_ERR_BAD_ARG;
  if (!(thresh >= 0.f && thresh <= 1.f) || min_kept < 0 || min_kept >= (1ll << 40)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || B >= (1 << 20) || n < 1 || (long long)B * n >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  const long long total = (long long)B * n;
  uint32_t tb;
  thresh += 0.f;                                // -0.0 -> +0.0
  memcpy(&tb, &thresh, 4);
  const int blocks = (int)std::min<long long>(std::max<long long>((total + 1023) / 1024, 1), MAX_BLOCKS);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(ohem_hist_kernel<0>, dim3(blocks), dim3(256), 0, s, hardness, total, B, tb, min_kept, work);
  IFSEG_CHECK_LAUNCH();
  hipLaunchKernelGGL(ohem_hist_kernel<1>, dim3(blocks), dim3(256), 0, s, hardness, total, B, tb, min_kept, work);
  IFSEG_CHECK_LAUNCH();
  hipLaunchKernelGGL(ohem_hist_kernel<2>, dim3(blocks), dim3(256), 0, s, hardness, total, B, tb, min_kept, work);
  IFSEG_CHECK_LAUNCH();
  hipLaunchKernelGGL(ohem_apply_kernel, dim3(blocks), dim3(256), 0, s, hardness, total, tb, weight, out, info, work);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
