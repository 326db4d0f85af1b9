// The photometric chain on grey levels (mmseg PhotoMetricDistortion; ifseg_amd/augment.py `photometric` is the specification,
// bit for bit): brightness; contrast if mode = 1; saturation; hue; contrast if mode = 0.  In registers, integers throughout,
// and convert() as ONE fp32 operation.  Shared by trainload.hip (behind the resize) and strong.hip (on the grey levels recovered
// from a normalised batch).
#pragma once
#include "common.h"

namespace photo {

constexpr int HSV_D = 7650;

// convert(x, alpha, 0) and convert(x, 1, beta): one fp32 operation each, nothing for the compiler to contract
__device__ __forceinline__ int cvt_mul(int x, float a) { return (int)fminf(fmaxf((float)x * a, 0.f), 255.f); }
__device__ __forceinline__ int cvt_add(int x, float b) { return (int)fminf(fmaxf((float)x + b, 0.f), 255.f); }

__device__ __forceinline__ void rgb_to_hsv8(int r, int g, int b, int* H, int* S, int* V) {
  const int v = max(r, max(g, b)), d = v - min(r, min(g, b));
  *V = v;
  *S = v ? (int)((unsigned)(510 * d + v) / (unsigned)(2 * v)) : 0;
  if (d == 0) { *H = 0; return; }
  int x, off;
  if (v == r) { x = g - b; off = 0; }
  else if (v == g) { x = b - r; off = 60; }
  else { x = r - g; off = 120; }
  const int n = 30 * x + (off + 180) * d;                   // + 180 d: positive, and a whole turn
  *H = (int)((unsigned)(2 * n + d) / (unsigned)(2 * d)) % 180;
}

__device__ __forceinline__ int hsv_rd(int n) { return (int)((unsigned)(2 * n + HSV_D) / (unsigned)(2 * HSV_D)); }

__device__ __forceinline__ void hsv8_to_rgb(int H, int S, int V, int* r, int* g, int* b) {
  const int sec = H / 30, f = H - 30 * sec;
  const int p = hsv_rd(30 * V * (255 - S)), q = hsv_rd(V * (HSV_D - S * f)), t = hsv_rd(V * (HSV_D - S * (30 - f)));
  *r = sec == 0 || sec == 5 ? V : (sec == 1 ? q : (sec == 4 ? t : p));
  *g = sec == 1 || sec == 2 ? V : (sec == 0 ? t : (sec == 3 ? q : p));
  *b = sec == 3 || sec == 4 ? V : (sec == 2 ? t : (sec == 5 ? q : p));
}

struct Photo {
  int bright, contrast, sat, hue, mode, delta;      // delta already in [0, 180)
  float beta, alpha_c, alpha_s;
};

__device__ __forceinline__ void photometric(const Photo& ph, int* r, int* g, int* b) {
  if (ph.bright) { *r = cvt_add(*r, ph.beta); *g = cvt_add(*g, ph.beta); *b = cvt_add(*b, ph.beta); }
  if (ph.contrast && ph.mode == 1) { *r = cvt_mul(*r, ph.alpha_c); *g = cvt_mul(*g, ph.alpha_c); *b = cvt_mul(*b, ph.alpha_c); }
  if (ph.sat) {
    int H, S, V;
    rgb_to_hsv8(*r, *g, *b, &H, &S, &V);
    hsv8_to_rgb(H, cvt_mul(S, ph.alpha_s), V, r, g, b);
  }
  if (ph.hue) {
    int H, S, V;
    rgb_to_hsv8(*r, *g, *b, &H, &S, &V);
    H += ph.delta;
    hsv8_to_rgb(H >= 180 ? H - 180 : H, S, V, r, g, b);
  }
  if (ph.contrast && ph.mode == 0) { *r = cvt_mul(*r, ph.alpha_c); *g = cvt_mul(*g, ph.alpha_c); *b = cvt_mul(*b, ph.alpha_c); }
}

}  // namespace photo
