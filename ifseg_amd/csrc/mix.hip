// ClassMix / CutMix of a labelled (source) batch into a pseudo-labelled (destination) batch on the device (ifseg_amd/augment.py,
// "the batch mix", is the specification, bit for bit).  Both batches in train_load's layout and of one B and P: images
// [B, 3, P, P] (fp32 or bf16), target int64 [B, P*P + 1], optionally a uint8 weight plane [B, P*P].
//
//   ifseg_mix_draw    records int32 [B, 16] <- the source targets and splitmix64(seed + (ordinal << 32) + slot)     one launch
//                     One workgroup of 1024 threads per sample.  "class": the presence of every class in LDS (plain flags: a
//                     lane stores only what nobody has marked yet), wave 0 packs the present classes in ascending order, and
//                     one thread runs the partial Fisher-Yates over at most 255 of them and writes the record.  "box": no
//                     target is read.
//   ifseg_mix_apply   one launch, grid (runs of a sample, B): a thread owns MX_RUN consecutive pixels of one sample -- they lie
//                     in one image row, P being a multiple of 16 -- and moves three image planes, the int64 target and the uint8
//                     weight: the source's where the record selects the pixel, else the destination's.  Images as 16-byte
//                     pieces selected bit-wise (a copy: NaN payloads survive).  A target row is P*P + 1 entries long, so rows of
//                     odd b start 8 bytes off a 16-byte boundary: targets move as 16-byte pieces at 8-byte alignment.
//                     out may BE the destination (the same pointers): a thread reads every destination element before it
//                     writes that element, and no other thread touches it.
// The class of a source pixel: c = target - seg_id_offset in 64 bits, a class only if 0 <= c < nseg ('unknown', a poisoned -1
// and seg_id_offset + 2^32 + 3 have none).  No address depends on a record or on a target's value beyond that test.
// No scratch buffer, no memset, static launch shapes, nothing read back.
// The counter stream, the ordinal check and the byte-range overlap test are common.h's.
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace {

constexpr int MX_MAX_P = 4096;
constexpr int MX_RUN = 8;                        // pixels per thread of the apply kernel
constexpr int MX_SLOT_BOX = 28, MX_SLOT_CLASS = 32;
enum { M_BITS = 0, M_Y0 = 8, M_X0, M_Y1, M_X1, M_PRESENT, M_CHOSEN };

// the class of a target value, or -1
__device__ __forceinline__ int mix_class(long long t, long long seg0, int nseg) {
  const unsigned long long c = (unsigned long long)t - (unsigned long long)seg0;
  return c < (unsigned long long)nseg ? (int)c : -1;
}

// Presence needs no count: a lane looks (the lanes of one address are served by one broadcast read) and only a class nobody
// has marked yet is written, by however many lanes meet it at once -- all of them store the same 1.  (count.h's pre-aggregated
// atomic add was measured first: a wave that crosses block edges of a piecewise-constant map sends its second and third
// class as 32 atomics to one address each, and the draw of a 512 x 512 map of 32 x 32 blocks took twice as long as that of
// a map of independent pixels.)
__device__ __forceinline__ void mark_seen(uint32_t* seen, int c) {
  if (__hip_atomic_load(&seen[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0)
    __hip_atomic_store(&seen[c], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct __attribute__((packed, aligned(8))) I64x2 {       // two targets at an 8-byte boundary
  long long v[2];
};

// ------------------------------------------------------------------------------------------------------------- draw
constexpr int MX_DRAW_THREADS = 1024, MX_DRAW_PAIRS = 8;

__global__ __launch_bounds__(MX_DRAW_THREADS) void mix_draw_kernel(const long long* __restrict__ src_target, unsigned long long seed,
                                                       unsigned long long first, int P, int nseg, long long seg0, int box,
                                                       int* __restrict__ records) {
  __shared__ uint32_t seen[256];                // 1: the class is present
  __shared__ int list[256];                     // the present classes, ascending, then partly shuffled
  __shared__ int pick[128];                     // j of step i
  __shared__ uint32_t bits[8];
  __shared__ int npresent;
  const int b = blockIdx.x, tid = threadIdx.x;
  const unsigned long long base = stream_base(seed, first, b);
  int* rec = records + (long long)b * 16;
  if (box) {
    if (tid < 16) {
      const int bh = P / 4 + draw_below(base, MX_SLOT_BOX, (unsigned)(P / 2 + 1));
      const int bw = P / 4 + draw_below(base, MX_SLOT_BOX + 1, (unsigned)(P / 2 + 1));
      const int y0 = draw_below(base, MX_SLOT_BOX + 2, (unsigned)(P - bh + 1));
      const int x0 = draw_below(base, MX_SLOT_BOX + 3, (unsigned)(P - bw + 1));
      rec[tid] = tid == M_Y0 ? y0 : tid == M_X0 ? x0 : tid == M_Y1 ? y0 + bh : tid == M_X1 ? x0 + bw : 0;
    }
    return;
  }
  if (tid < 256) seen[tid] = 0;
  if (tid < 8) bits[tid] = 0;
  __syncthreads();
  // One workgroup reads its sample's whole row, so what counts is the bytes it keeps in flight: a lane takes pairs of targets
  // (16 bytes at the row's 8-byte alignment), MX_DRAW_PAIRS of them per step.  P*P is a multiple of 256, so a pair is inside
  // the row or outside as a whole.
  const long long n = (long long)P * P;
  const long long* row = src_target + (long long)b * (n + 1);
  for (long long i0 = 0; i0 < n; i0 += 2 * MX_DRAW_THREADS * MX_DRAW_PAIRS) {
    long long t[2 * MX_DRAW_PAIRS];
    bool live[MX_DRAW_PAIRS];
#pragma unroll
    for (int k = 0; k < MX_DRAW_PAIRS; ++k) {
      const long long i = i0 + 2 * (k * MX_DRAW_THREADS + tid);
      live[k] = i < n;
      I64x2 v = {{0, 0}};
      if (live[k]) v = *reinterpret_cast<const I64x2*>(row + i);
      t[2 * k] = v.v[0];
      t[2 * k + 1] = v.v[1];
    }
#pragma unroll
    for (int k = 0; k < 2 * MX_DRAW_PAIRS; ++k) {
      const int c = live[k >> 1] ? mix_class(t[k], seg0, nseg) : -1;
      if (c >= 0) mark_seen(seen, c);
    }
  }
  __syncthreads();
  if (tid < 64) {                               // wave 0: the present classes in ascending order
    int have = 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = r * 64 + tid;
      const bool on = c < nseg && seen[c] != 0;
      const unsigned long long m = __ballot(on);
      if (on) list[have + __popcll(m & ((1ull << tid) - 1))] = c;
      have += (int)__popcll(m);
    }
    if (tid == 0) npresent = have;
  }
  __syncthreads();
  const int np = npresent, m = (np + 1) / 2;
  if (tid < m) pick[tid] = tid + draw_below(base, MX_SLOT_CLASS + tid, (unsigned)(np - tid));
  __syncthreads();
  if (tid == 0) {
    for (int i = 0; i < m; ++i) {
      const int j = pick[i], ci = list[i], cj = list[j];
      list[i] = cj;
      list[j] = ci;
      bits[cj >> 5] |= 1u << (cj & 31);
    }
  }
  __syncthreads();
  if (tid < 16) rec[tid] = tid < 8 ? (int)bits[tid] : tid == M_PRESENT ? np : tid == M_CHOSEN ? m : 0;
}

// ------------------------------------------------------------------------------------------------------------- apply

template <int EB>
__global__ __launch_bounds__(256) void mix_apply_kernel(const int* __restrict__ records, const unsigned char* __restrict__ src_img,
                                                        const long long* __restrict__ src_tgt,
                                                        const unsigned char* __restrict__ src_w,
                                                        const unsigned char* dst_img, const long long* dst_tgt,
                                                        const unsigned char* dst_w, int P, int nseg, long long seg0,
                                                        unsigned char* out_img, long long* out_tgt, unsigned char* out_w) {
  __shared__ unsigned char chosen[256];         // chosen[c] = 1: class c is pasted
  const int b = blockIdx.y, tid = threadIdx.x;
  const int* rec = records + (long long)b * 16;
  chosen[tid] = tid < nseg ? (unsigned char)(((unsigned)rec[M_BITS + (tid >> 5)] >> (tid & 31)) & 1u) : 0;
  const int y0 = rec[M_Y0], x0 = rec[M_X0], y1 = rec[M_Y1], x1 = rec[M_X1];
  __syncthreads();
  const long long n = (long long)P * P;
  const long long* st = src_tgt + (long long)b * (n + 1);
  const long long* dt = dst_tgt + (long long)b * (n + 1);
  long long* ot = out_tgt + (long long)b * (n + 1);
  if (blockIdx.x == 0 && tid == 0) ot[n] = dt[n];                                  // EOS: the destination's
  const long long p0 = ((long long)blockIdx.x * 256 + tid) * MX_RUN;               // the run's first pixel
  if (p0 >= n) return;
  const int y = (int)(p0 / P), xb = (int)(p0 - (long long)y * P);
  const bool yin = y >= y0 && y < y1;

  // every load in front of every store: with out = the destination a thread has read all it overwrites
  long long sv[MX_RUN], dv[MX_RUN];
#pragma unroll
  for (int q = 0; q < MX_RUN / 2; ++q) {
    const I64x2 s = *reinterpret_cast<const I64x2*>(st + p0 + 2 * q);
    const I64x2 d = *reinterpret_cast<const I64x2*>(dt + p0 + 2 * q);
    sv[2 * q] = s.v[0]; sv[2 * q + 1] = s.v[1];
    dv[2 * q] = d.v[0]; dv[2 * q + 1] = d.v[1];
  }
  constexpr int NV = MX_RUN * EB / 16;          // 16-byte pieces of a run in one plane: 2 (fp32) or 1 (bf16)
  const long long e0 = ((long long)b * 3 * n + p0) * EB;                           // byte offset in plane 0 of sample b
  uint4 si[3][NV], di[3][NV];
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      si[c][v] = *reinterpret_cast<const uint4*>(src_img + e0 + (long long)c * n * EB + 16 * v);
      di[c][v] = *reinterpret_cast<const uint4*>(dst_img + e0 + (long long)c * n * EB + 16 * v);
    }
  const long long w0 = (long long)b * n + p0;
  uint2 sw = make_uint2(0xffffffffu, 0xffffffffu), dw = sw;                        // a missing plane reads as 255
  if (src_w) sw = *reinterpret_cast<const uint2*>(src_w + w0);
  if (dst_w) dw = *reinterpret_cast<const uint2*>(dst_w + w0);

  bool sel[MX_RUN];
#pragma unroll
  for (int k = 0; k < MX_RUN; ++k) {
    const int c = mix_class(sv[k], seg0, nseg);
    const int x = xb + k;
    sel[k] = (c >= 0 && chosen[max(c, 0)] != 0) || (yin && x >= x0 && x < x1);
  }

#pragma unroll
  for (int q = 0; q < MX_RUN / 2; ++q) {
    I64x2 o;
    o.v[0] = sel[2 * q] ? sv[2 * q] : dv[2 * q];
    o.v[1] = sel[2 * q + 1] ? sv[2 * q + 1] : dv[2 * q + 1];
    *reinterpret_cast<I64x2*>(ot + p0 + 2 * q) = o;
  }
  // images as dwords under a bit mask: a copy, whatever the bits say
  uint32_t mask[4 * NV];
#pragma unroll
  for (int w = 0; w < 4 * NV; ++w)
    mask[w] = EB == 4 ? (sel[w] ? 0xffffffffu : 0u) : ((sel[2 * w] ? 0xffffu : 0u) | (sel[2 * w + 1] ? 0xffff0000u : 0u));
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      const uint4 s = si[c][v], d = di[c][v];
      uint4 o;
      o.x = (s.x & mask[4 * v]) | (d.x & ~mask[4 * v]);
      o.y = (s.y & mask[4 * v + 1]) | (d.y & ~mask[4 * v + 1]);
      o.z = (s.z & mask[4 * v + 2]) | (d.z & ~mask[4 * v + 2]);
      o.w = (s.w & mask[4 * v + 3]) | (d.w & ~mask[4 * v + 3]);
      *reinterpret_cast<uint4*>(out_img + e0 + (long long)c * n * EB + 16 * v) = o;
    }
  if (out_w) {
    uint32_t m[2];
#pragma unroll
    for (int w = 0; w < 2; ++w)
      m[w] = (sel[4 * w] ? 0xffu : 0u) | (sel[4 * w + 1] ? 0xff00u : 0u) | (sel[4 * w + 2] ? 0xff0000u : 0u) |
             (sel[4 * w + 3] ? 0xff000000u : 0u);
    *reinterpret_cast<uint2*>(out_w + w0) = make_uint2((sw.x & m[0]) | (dw.x & ~m[0]), (sw.y & m[1]) | (dw.y & ~m[1]));
  }
}

}  // namespace

extern "C" int ifseg_mix_draw(const long long* src_target, int B, int P, int nseg, long long seg_id_offset,
                              unsigned long long seed, long long first_ordinal, int box, int* records, void* stream) {
  (void)hipGetLastError();
  if (!src_target || !records || ((size_t)src_target & 7) || ((size_t)records & 3)) return IFSEG_ERR_BAD_ARG;
  if (nseg < 1 || nseg > 255 || (box != 0 && box != 1)) return IFSEG_ERR_BAD_ARG;
  if (!ordinals_ok(first_ordinal, B)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || B > 65535 || P < 16 || P % 16 || P > MX_MAX_P) return IFSEG_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(mix_draw_kernel, dim3(B), dim3(MX_DRAW_THREADS), 0, (hipStream_t)stream, src_target, seed,
                     (unsigned long long)first_ordinal, P, nseg, seg_id_offset, box, records);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_mix_apply(const int* records, const void* src_images, const long long* src_target, const void* src_weight,
                               const void* dst_images, const long long* dst_target, const void* dst_weight, int B, int P,
                               int nseg, long long seg_id_offset, int elem_bytes, void* out_images, long long* out_target,
                               void* out_weight, void* stream) {
  (void)hipGetLastError();
  if (!records || !src_images || !src_target || !dst_images || !dst_target || !out_images || !out_target) return IFSEG_ERR_BAD_ARG;
  if ((elem_bytes != 4 && elem_bytes != 2) || nseg < 1 || nseg > 255) return IFSEG_ERR_BAD_ARG;
  if ((!out_weight) != (!src_weight && !dst_weight)) return IFSEG_ERR_BAD_ARG;    // a plane comes out iff one goes in
  if (((size_t)records & 3) || (((size_t)src_images | (size_t)dst_images | (size_t)out_images) & 15) ||
      (((size_t)src_target | (size_t)dst_target | (size_t)out_target) & 7) ||
      (((size_t)src_weight | (size_t)dst_weight | (size_t)out_weight) & 7))
    return IFSEG_ERR_BAD_ARG;
  if (B < 1 || B > 65535 || P < 16 || P % 16 || P > MX_MAX_P) return IFSEG_ERR_BAD_SHAPE;
  const long long n = (long long)P * P;
  if ((long long)B * 3 * n >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  // an output may be the destination tensor it replaces, pointer for pointer; it shares no byte with anything else
  const long long nb[3] = {(long long)B * 3 * n * elem_bytes, (long long)B * (n + 1) * 8, (long long)B * n};
  const void* outs[3] = {out_images, out_target, out_weight};
  const void* srcs[3] = {src_images, src_target, src_weight};
  const void* dsts[3] = {dst_images, dst_target, dst_weight};
  for (int i = 0; i < 3; ++i) {
    if (overlaps(outs[i], nb[i], records, (long long)B * 16 * 4)) return IFSEG_ERR_BAD_ARG;
    for (int j = 0; j < 3; ++j) {
      if (overlaps(outs[i], nb[i], srcs[j], nb[j])) return IFSEG_ERR_BAD_ARG;
      if (overlaps(outs[i], nb[i], dsts[j], nb[j]) && !(i == j && outs[i] == dsts[j])) return IFSEG_ERR_BAD_ARG;
      if (j > i && overlaps(outs[i], nb[i], outs[j], nb[j])) return IFSEG_ERR_BAD_ARG;
    }
  }
  const dim3 grid((unsigned)((n / MX_RUN + 255) / 256), (unsigned)B);
#define MIX_APPLY(EB)                                                                                                          \
  hipLaunchKernelGGL(mix_apply_kernel<EB>, grid, dim3(256), 0, (hipStream_t)stream, records, (const unsigned char*)src_images, \
                     src_target, (const unsigned char*)src_weight, (const unsigned char*)dst_images, dst_target,               \
                     (const unsigned char*)dst_weight, P, nseg, seg_id_offset, (unsigned char*)out_images, out_target,         \
                     (unsigned char*)out_weight)
  if (elem_bytes == 4) MIX_APPLY(4);
  else MIX_APPLY(2);
#undef MIX_APPLY
  IFSEG_CHECK_LAUNCH();
  return 0;
}
