// The two ends of "attention with a bias somebody else computed" (torch.ops.ifseg.attention_bias), gfx950.
//
//   ifseg_attn_bias_pack : an ordinary [H, T, S] bias tensor (fp32 or bf16, strided rows / heads)  ->  the dense bf16 operand
//                          D [H, Tp, Sp] of csrc/attention_bi.hip (padding and causally masked pairs -inf)
//   ifseg_attn_dbias_sum : the slabs [ng, H, T, Sp] of sum_b dS that ifseg_attn_bwd_bi writes  ->  one [H, T, S] gradient
//
// Both are single passes over HBM with nothing to reuse: a thread owns one 16-byte piece (8 bf16) of a padded row, a
// workgroup of 256 threads owns 8 consecutive rows (a flat index over rows x pieces, so that short rows still fill the
// lanes).  The padded side (Sp % 32 == 0, 16-byte aligned base) always moves as 16-byte words; the plain tensor on the
// other side moves as 16-byte words where the piece lies inside the row and its address is 16-byte aligned, element by
// element otherwise (S % 8 != 0 tails, odd strides, offset views).  No LDS, no atomics: the sum runs over the slabs in
// slab order in fp32, bit-reproducible.
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace {

constexpr int ROWS_PER_WG = 8;
constexpr unsigned BF_NEG_INF2 = 0xff80ff80u;       // two bf16 -inf

struct PackArgs {
  const void* bias;            // [H][T][S] elements, last dimension contiguous; nullptr = zero bias
  long long hs, rs;            // head / row stride in elements
  int f32, H, T, S, Sp, Tp, causal, P;
  bf16_t* D;
};

// the "tail-first" causal order of attn_dense_bias_kernel: P grid tokens first, the tail behind them; a tail key is visible
// to every grid query
// (written as selects on bit operations, applied to the value with one more select: the short-circuit form of
// attn_dense_bias_kernel, `if (masked) v[e] = -inf` unrolled eight times, came out of hipcc 7 with the assignment missing for
// e = 1..7 -- an empty exec region in the ISA, masked entries left finite on the GPU)
__device__ __forceinline__ bool causal_masked(int i, int j, int P) {
  const bool above = j > i, grid_key = j < P;
  return (i >= P) ? (grid_key | above) : (grid_key & above);
}

__global__ __launch_bounds__(256) void attn_bias_pack_kernel(PackArgs a) {
  const int nch = a.Sp >> 3;
  const int row0 = blockIdx.x * ROWS_PER_WG;                  // row = h * Tp + i; Tp % 8 == 0: a workgroup stays inside a head
  const int h = row0 / a.Tp, i0 = row0 - h * a.Tp;
  for (int idx = threadIdx.x; idx < ROWS_PER_WG * nch; idx += 256) {
    const int r = idx / nch, c = idx - r * nch;
    const int i = i0 + r, j0 = c * 8;
    uint4 o = make_uint4(BF_NEG_INF2, BF_NEG_INF2, BF_NEG_INF2, BF_NEG_INF2);
    if (i < a.T && j0 < a.S) {
      float v[8];
      const int n = min(8, a.S - j0);
      if (!a.bias) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
      } else if (a.f32) {
        const float* p = reinterpret_cast<const float*>(a.bias) + (long long)h * a.hs + (long long)i * a.rs + j0;
        if (n == 8 && ((size_t)p & 15) == 0) {
          const float4 x0 = *reinterpret_cast<const float4*>(p), x1 = *reinterpret_cast<const float4*>(p + 4);
          v[0] = x0.x; v[1] = x0.y; v[2] = x0.z; v[3] = x0.w; v[4] = x1.x; v[5] = x1.y; v[6] = x1.z; v[7] = x1.w;
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = e < n ? p[e] : 0.f;
        }
      } else {
        const bf16_t* p = reinterpret_cast<const bf16_t*>(a.bias) + (long long)h * a.hs + (long long)i * a.rs + j0;
        if (n == 8 && ((size_t)p & 15) == 0) {
          U128 u;
          u.v = *reinterpret_cast<const uint4*>(p);
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = bf2f(u.h[e]);
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) v[e] = e < n ? bf2f(p[e]) : 0.f;
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = j0 + e;
        const bool masked = (j >= a.S) | ((a.causal != 0) & causal_masked(i, j, a.P));
        v[e] = masked ? -INFINITY : v[e];
      }
      o = make_uint4(pack2bf(v[0], v[1]), pack2bf(v[2], v[3]), pack2bf(v[4], v[5]), pack2bf(v[6], v[7]));
    }
    *reinterpret_cast<uint4*>(a.D + ((long long)h * a.Tp + i) * a.Sp + j0) = o;
  }
}

struct SumArgs {
  const bf16_t* dbias;         // [ng][H][T][Sp]
  long long gs;                // H * T * Sp
  void* out;                   // [H][T][S] elements, last dimension contiguous
  long long hs, rs;
  int f32, ng, H, T, S, Sp, rows;
};

__global__ __launch_bounds__(256) void attn_dbias_sum_kernel(SumArgs a) {
  const int nch = (a.S + 7) >> 3;
  const int row0 = blockIdx.x * ROWS_PER_WG;                  // row = h * T + i
  for (int idx = threadIdx.x; idx < ROWS_PER_WG * nch; idx += 256) {
    const int r = idx / nch, c = idx - r * nch;
    const int row = row0 + r, j0 = c * 8;
    if (row >= a.rows) break;
    const bf16_t* src = a.dbias + (long long)row * a.Sp + j0;
    float acc[8];
    {
      U128 u;
      u.v = *reinterpret_cast<const uint4*>(src);
#pragma unroll
      for (int e = 0; e < 4; ++e) { acc[2 * e] = bflo(u.w[e]); acc[2 * e + 1] = bfhi(u.w[e]); }
    }
#pragma unroll 4
    for (int g = 1; g < a.ng; ++g) {
      U128 u;
      u.v = *reinterpret_cast<const uint4*>(src + g * a.gs);
#pragma unroll
      for (int e = 0; e < 4; ++e) { acc[2 * e] += bflo(u.w[e]); acc[2 * e + 1] += bfhi(u.w[e]); }
    }
    const int h = row / a.T, i = row - h * a.T;
    const int n = min(8, a.S - j0);
    const long long off = (long long)h * a.hs + (long long)i * a.rs + j0;
    if (a.f32) {
      float* p = reinterpret_cast<float*>(a.out) + off;
      if (n == 8 && ((size_t)p & 15) == 0) {
        *reinterpret_cast<float4*>(p) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        *reinterpret_cast<float4*>(p + 4) = make_float4(acc[4], acc[5], acc[6], acc[7]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) if (e < n) p[e] = acc[e];
      }
    } else {
      bf16_t* p = reinterpret_cast<bf16_t*>(a.out) + off;
      if (n == 8 && ((size_t)p & 15) == 0) {
        *reinterpret_cast<uint4*>(p) = make_uint4(pack2bf(acc[0], acc[1]), pack2bf(acc[2], acc[3]), pack2bf(acc[4], acc[5]),
                                                  pack2bf(acc[6], acc[7]));
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) if (e < n) p[e] = f2bf(acc[e]);
      }
    }
  }
}

}  // namespace

extern "C" int ifseg_attn_bias_pack(const void* bias, int bias_is_f32, long long head_stride, long long row_stride, int H,
                                    int T, int S, int causal, int P, void* D, int Sp, int Tp, void* stream) {
  (void)hipGetLastError();
  if (!D || H <= 0 || T <= 0 || S <= 0 || (Sp & 31) || (Tp & 31) || Sp < S || Tp < T) return IFSEG_ERR_BAD_ARG;
  if (((size_t)D & 15) || ((size_t)bias & (bias_is_f32 ? 3 : 1))) return IFSEG_ERR_BAD_ARG;
  if (causal && (P < 0 || (P & 63) || P > T || P > S)) return IFSEG_ERR_BAD_SHAPE;
  if ((long long)H * Tp / ROWS_PER_WG >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  PackArgs a{};
  a.bias = bias; a.hs = head_stride; a.rs = row_stride; a.f32 = bias_is_f32 ? 1 : 0;
  a.H = H; a.T = T; a.S = S; a.Sp = Sp; a.Tp = Tp; a.causal = causal ? 1 : 0; a.P = causal ? P : S;
  a.D = (bf16_t*)D;
  hipLaunchKernelGGL(attn_bias_pack_kernel, dim3((unsigned)((long long)H * Tp / ROWS_PER_WG)), dim3(256), 0, (hipStream_t)stream, a);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_attn_dbias_sum(const void* dbias, int ng, int H, int T, int S, int Sp, void* out, int out_is_f32,
                                    long long head_stride, long long row_stride, void* stream) {
  (void)hipGetLastError();
  if (!dbias || !out || ng <= 0 || H <= 0 || T <= 0 || S <= 0 || (Sp & 31) || Sp < S) return IFSEG_ERR_BAD_ARG;
  if (((size_t)dbias & 15) || ((size_t)out & (out_is_f32 ? 3 : 1))) return IFSEG_ERR_BAD_ARG;
  if ((long long)H * T >= (1ll << 31) - ROWS_PER_WG) return IFSEG_ERR_BAD_SHAPE;
  SumArgs a{};
  a.dbias = (const bf16_t*)dbias; a.gs = (long long)H * T * Sp; a.out = out; a.hs = head_stride; a.rs = row_stride;
  a.f32 = out_is_f32 ? 1 : 0; a.ng = ng; a.H = H; a.T = T; a.S = S; a.Sp = Sp; a.rows = H * T;
  hipLaunchKernelGGL(attn_dbias_sum_kernel, dim3((unsigned)((a.rows + ROWS_PER_WG - 1) / ROWS_PER_WG)), dim3(256), 0,
                     (hipStream_t)stream, a);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
