// Flat-arena optimizer kernels (gfx950): global grad-norm and a fused
// clip + Adam(W) + bf16 write-back, one launch over the whole parameter arena;
// with Trainer(store_ema=True) the same launch also steps the averaged teacher
// (fairseq/models/ema/ema.py:134-167), and ema_swap_kernel exchanges the two.
// Reference semantics: trainer.py:865-907 (multiply_grads, clip_grad_norm 1.0,
// optimizer.step) with fairseq/optim/adam.py:158-240 (decoupled weight decay,
// bias-corrected step) and fp16_optimizer.py:96-222 (fp32 master copy).
#include "common.h"
#include "../../include/ifseg_hip.h"

namespace {

__global__ __launch_bounds__(256) void sumsq_bf16_kernel(const bf16_t* g, long long n, float* part) {
  __shared__ float red[4];
  float acc = 0.f;
  const long long stride = (long long)gridDim.x * blockDim.x * 8;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 8; i < n; i += stride) {
    if (i + 7 < n) {
      uint4 u = *reinterpret_cast<const uint4*>(g + i);
      const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) { const float a = bflo(w[e]), b = bfhi(w[e]); acc += a * a + b * b; }
    } else {
      for (long long k = i; k < n; ++k) { const float a = bf2f(g[k]); acc += a * a; }
    }
  }
  acc = warp_sum(acc);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

__global__ void finish_norm_kernel(const float* part, int nparts, float* out_sumsq) {
  float acc = 0.f;
  for (int i = threadIdx.x; i < nparts; i += 64) acc += part[i];
  acc = warp_sum(acc);
  if (threadIdx.x == 0) out_sumsq[0] = acc;
}

// e' = fma(rest, q, round32(e * decay)): fairseq's `ema.mul_(decay); ema.add_(param.float(), alpha=1 - decay)` element for element
// (models/ema/ema.py:164-165 with ema_fp32 on a 16-bit model; ifseg_amd/ema.py is the specification).  Contraction is off in
// here and the one fma is written out: the product must be rounded before it enters the sum.
__device__ __forceinline__ float ema_mix(float e, float q, float decay, float rest) {
#pragma clang fp contract(off)
  return __builtin_fmaf(rest, q, e * decay);
}

// p32, m, v: fp32 masters; g: bf16 grads; p16: bf16 model copy.  gscale multiplies
// every gradient (world/sample_size factor); the clip coefficient is derived on
// device from *sumsq (of the unscaled grads) so there is no host sync.
// EMA: the teacher (e32 fp32, e16 its bf16 rounding) takes a step towards the bf16 weight this launch has just produced, from
// registers.  (decay, rest) == (1, 0) neither loads nor stores it: how a captured step sits out the off-updates of
// ema_update_freq.  The Adam lines are the same text for both instantiations (bit-equal: tests/test_ema_gpu.py).
template <bool EMA>
__global__ __launch_bounds__(256) void adam_kernel(float* p32, const bf16_t* g, float* m, float* v, bf16_t* p16,
                                                   long long n, float lr, float beta1, float beta2, float eps, float wd,
                                                   float bc1, float bc2, float gscale, float max_norm,
                                                   const float* sumsq, int* overflow, const float* hyper,
                                                   float* e32, bf16_t* e16, float decay, float rest) {
  if (hyper) {      // per-update scalars from device memory (a captured step replays with the current schedule)
    lr = hyper[0]; bc1 = hyper[1]; bc2 = hyper[2]; gscale = hyper[3];
    if (EMA) { decay = hyper[4]; rest = hyper[5]; }
  }
  float coef = gscale;
  if (sumsq && !isfinite(sumsq[0])) {
    // trainer.py:895-904: a NaN / Inf gradient norm must not reach the fp32 masters or the Adam moments
    // (fminf(1, NaN) would evaluate to 1 and apply the poisoned step): skip the update, raise the flag
    // (and the teacher stays with it: trainer.py:961-964 steps the EMA only after a successful update)
    if (overflow && blockIdx.x == 0 && threadIdx.x == 0) overflow[0] = 1;
    return;
  }
  if (max_norm > 0.f && sumsq) {
    const float norm = sqrtf(sumsq[0]) * gscale;
    coef *= fminf(1.f, max_norm / (norm + 1e-6f));
  }
  const float step_size = lr * sqrtf(bc2) / bc1;
  const bool ema = EMA && !(decay == 1.f && rest == 0.f);       // uniform
  const long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      float4 P = *reinterpret_cast<float4*>(p32 + i), M = *reinterpret_cast<float4*>(m + i), V = *reinterpret_cast<float4*>(v + i);
      uint2 gw = *reinterpret_cast<const uint2*>(g + i);
      float pp[4] = {P.x, P.y, P.z, P.w}, mm[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
      const float gg[4] = {bflo(gw.x) * coef, bfhi(gw.x) * coef, bflo(gw.y) * coef, bfhi(gw.y) * coef};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        mm[e] = mm[e] * beta1 + gg[e] * (1.f - beta1);
        vv[e] = vv[e] * beta2 + gg[e] * gg[e] * (1.f - beta2);
        const float denom = sqrtf(vv[e]) + eps;
        pp[e] = pp[e] - wd * lr * pp[e];
        pp[e] = pp[e] - step_size * mm[e] / denom;
      }
      const uint2 pw = make_uint2(pack2bf(pp[0], pp[1]), pack2bf(pp[2], pp[3]));
      *reinterpret_cast<float4*>(p32 + i) = make_float4(pp[0], pp[1], pp[2], pp[3]);
      *reinterpret_cast<float4*>(m + i) = make_float4(mm[0], mm[1], mm[2], mm[3]);
      *reinterpret_cast<float4*>(v + i) = make_float4(vv[0], vv[1], vv[2], vv[3]);
      *reinterpret_cast<uint2*>(p16 + i) = pw;
      if (ema) {
        const float4 E = *reinterpret_cast<const float4*>(e32 + i);
        const float e0 = ema_mix(E.x, bflo(pw.x), decay, rest), e1 = ema_mix(E.y, bfhi(pw.x), decay, rest);
        const float e2 = ema_mix(E.z, bflo(pw.y), decay, rest), e3 = ema_mix(E.w, bfhi(pw.y), decay, rest);
        *reinterpret_cast<float4*>(e32 + i) = make_float4(e0, e1, e2, e3);
        *reinterpret_cast<uint2*>(e16 + i) = make_uint2(pack2bf(e0, e1), pack2bf(e2, e3));
      }
    } else {
      for (long long k = i; k < n; ++k) {
        const float gk = bf2f(g[k]) * coef;
        const float mk = m[k] * beta1 + gk * (1.f - beta1), vk = v[k] * beta2 + gk * gk * (1.f - beta2);
        float pk = p32[k];
        pk -= wd * lr * pk;
        pk -= step_size * mk / (sqrtf(vk) + eps);
        const bf16_t qk = f2bf(pk);
        p32[k] = pk; m[k] = mk; v[k] = vk; p16[k] = qk;
        if (ema) {
          const float ek = ema_mix(e32[k], bf2f(qk), decay, rest);
          e32[k] = ek; e16[k] = f2bf(ek);
        }
      }
    }
  }
}

// p32 <-> e32 and p16 <-> e16 in place: every element has one owner (a thread reads both sides of it, then writes both), so
// nothing is staged
__global__ __launch_bounds__(256) void ema_swap_kernel(float* p32, bf16_t* p16, float* e32, bf16_t* e16, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x * 4;
  for (long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 3 < n) {
      const float4 P = *reinterpret_cast<const float4*>(p32 + i), E = *reinterpret_cast<const float4*>(e32 + i);
      const uint2 p = *reinterpret_cast<const uint2*>(p16 + i), e = *reinterpret_cast<const uint2*>(e16 + i);
      *reinterpret_cast<float4*>(p32 + i) = E;
      *reinterpret_cast<float4*>(e32 + i) = P;
      *reinterpret_cast<uint2*>(p16 + i) = e;
      *reinterpret_cast<uint2*>(e16 + i) = p;
    } else {
      for (long long k = i; k < n; ++k) {
        const float a = p32[k], b = e32[k];
        const bf16_t c = p16[k], d = e16[k];
        p32[k] = b; e32[k] = a; p16[k] = d; e16[k] = c;
      }
    }
  }
}

// the refusals the two Adam entries share: the kernel reads and writes p32 / m / v as float4 and g / p16 as uint2
inline int check_adam_args(const float* p32, const void* g, const float* m, const float* v, const void* p16) {
  if (!p32 || !g || !m || !v || !p16) return IFSEG_ERR_BAD_ARG;
  if (((size_t)p32 & 15) || ((size_t)m & 15) || ((size_t)v & 15) || ((size_t)g & 7) || ((size_t)p16 & 7)) return IFSEG_ERR_BAD_ARG;
  return 0;
}

}  // namespace

extern "C" int ifseg_grad_sumsq_bf16(const void* g, long long n, float* workspace /* >= 1024 floats */,
                                     float* out_sumsq, void* stream) {
  (void)hipGetLastError();
  if (!g || !workspace || !out_sumsq || ((size_t)g & 15) || ((size_t)workspace & 3) || ((size_t)out_sumsq & 3) || n < 0)
    return IFSEG_ERR_BAD_ARG;     // (n == 0: no block reads g, every part is 0 and so is the sum)
  const int nblk = 1024;
  hipLaunchKernelGGL(sumsq_bf16_kernel, dim3(nblk), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)g, n, workspace);
  hipLaunchKernelGGL(finish_norm_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, workspace, nblk, out_sumsq);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_adam_step(float* p32, const void* g, float* m, float* v, void* p16, long long n, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                               float max_norm, const float* sumsq, int* overflow, const float* hyper, void* stream) {
  (void)hipGetLastError();
  if (n <= 0) return 0;
  if (const int rc = check_adam_args(p32, g, m, v, p16)) return rc;
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  // grid: two blocks per CU.  Sweep on MI355X over 109 M parameters (tools/adam_bench.py, profiles/round6_adam_grid.txt): 256 blocks
  // 789 us, 512: 573, 768: 578, 1024: 588, 1536: 618, 2048 (until round 6): 620, 4096: 620 -- 5.33 TB/s against a torch copy's 5.0
  hipLaunchKernelGGL(adam_kernel<false>, dim3(512), dim3(256), 0, (hipStream_t)stream, p32, (const bf16_t*)g, m, v,
                     (bf16_t*)p16, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_scale, max_norm, sumsq, overflow, hyper,
                     (float*)nullptr, (bf16_t*)nullptr, 1.f, 0.f);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_adam_ema_step(float* p32, const void* g, float* m, float* v, void* p16, float* e32, void* e16,
                                   long long n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                   float grad_scale, float max_norm, const float* sumsq, int* overflow, const float* hyper,
                                   float ema_decay, float ema_rest, void* stream) {
  (void)hipGetLastError();
  if (n <= 0) return 0;
  if (const int rc = check_adam_args(p32, g, m, v, p16)) return rc;
  if (!e32 || !e16 || ((size_t)e32 & 15) || ((size_t)e16 & 7)) return IFSEG_ERR_BAD_ARG;
  const float bc1 = 1.f - powf(beta1, (float)step), bc2 = 1.f - powf(beta2, (float)step);
  // the grid of ifseg_adam_step: the same sweep with 40 instead of 30 bytes per element
  hipLaunchKernelGGL(adam_kernel<true>, dim3(512), dim3(256), 0, (hipStream_t)stream, p32, (const bf16_t*)g, m, v,
                     (bf16_t*)p16, n, lr, beta1, beta2, eps, weight_decay, bc1, bc2, grad_scale, max_norm, sumsq, overflow, hyper,
                     e32, (bf16_t*)e16, ema_decay, ema_rest);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_ema_swap(float* p32, void* p16, float* e32, void* e16, long long n, void* stream) {
  (void)hipGetLastError();
  if (n <= 0) return 0;
  if (!p32 || !p16 || !e32 || !e16) return IFSEG_ERR_BAD_ARG;
  const long long want = (n + 1023) / 1024;         // 256 threads x 4 elements per block and sweep
  hipLaunchKernelGGL(ema_swap_kernel, dim3((unsigned)(want < 512 ? want : 512)), dim3(256), 0, (hipStream_t)stream, p32,
                     (bf16_t*)p16, e32, (bf16_t*)e16, n);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
