// The photometric chain on grey levels (mmseg PhotoMetricDistortion; ifseg_amd/augment.py `photometric` is the specification,
// bit for bit): brightness; contrast if mode = 1; saturation; hue; contrast if mode = 0.  In registers, integers throughout,
// and convert() as ONE fp32 operation.  Shared by trainload.hip (behind the resize) and strong.hip (on the grey levels recovered
// from a normalised batch), and with it the nine record words that drive it: how they are drawn, read back and validated.
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

// ---- the photometric part of a record: nine consecutive int32 words, wherever the record keeps them ----
enum { PH_BRIGHT, PH_CONTRAST, PH_SAT, PH_HUE, PH_MODE, PH_BETA, PH_ALPHA_C, PH_ALPHA_S, PH_DELTA };
// drawn from five consecutive slots of the sample's stream (common.h): bits 1 brightness on, 2 mode, 3 contrast on, 4 saturation
// on, 5 hue on of the first, the four "on" bits ANDed with `gate`; beta, alpha_c, alpha_s, delta of the other four
__device__ __forceinline__ void photo_draw(int* w, unsigned long long base, unsigned slot, int gate) {
  const unsigned bits = draw32(base, slot);
  w[PH_BRIGHT] = gate & (bits >> 1);
  w[PH_MODE] = (bits >> 2) & 1;
  w[PH_CONTRAST] = gate & (bits >> 3);
  w[PH_SAT] = gate & (bits >> 4);
  w[PH_HUE] = gate & (bits >> 5);
  // exact in fp32: integers below 2^24 times a power of two
  w[PH_BETA] = __float_as_int((float)((int)(draw32(base, slot + 1) >> 9) - (1 << 22)) * (1.f / 131072.f));
  w[PH_ALPHA_C] = __float_as_int((float)((1 << 22) + (int)(draw32(base, slot + 2) >> 9)) * (1.f / 8388608.f));
  w[PH_ALPHA_S] = __float_as_int((float)((1 << 22) + (int)(draw32(base, slot + 3) >> 9)) * (1.f / 8388608.f));
  w[PH_DELTA] = draw_below(base, slot + 4, 36u) - 18;
}
// as the chain takes them: delta reduced mod 180, whatever its sign
__device__ __forceinline__ Photo photo_read(const int* w) {
  Photo ph;
  ph.bright = w[PH_BRIGHT]; ph.contrast = w[PH_CONTRAST]; ph.sat = w[PH_SAT]; ph.hue = w[PH_HUE]; ph.mode = w[PH_MODE];
  ph.delta = (w[PH_DELTA] % 180 + 180) % 180;
  ph.beta = __int_as_float(w[PH_BETA]); ph.alpha_c = __int_as_float(w[PH_ALPHA_C]); ph.alpha_s = __int_as_float(w[PH_ALPHA_S]);
  return ph;
}
// the five flags in {0, 1} and the three floats finite (strong.hip refuses a record that fails; trainload.hip does not ask)
__device__ __forceinline__ bool photo_valid(const int* w) {
  bool bad = false;
#pragma unroll
  for (int i = PH_BRIGHT; i <= PH_MODE; ++i) bad |= (unsigned)w[i] > 1u;
#pragma unroll
  for (int i = PH_BETA; i <= PH_ALPHA_S; ++i) bad |= (w[i] & 0x7f800000) == 0x7f800000;
  return !bad;
}

}  // namespace photo
