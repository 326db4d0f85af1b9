// The reference's TRAINING transform on the device (ifseg_amd/augment.py is the specification, bit for bit): raw uint8 images
// [H0, W0, 3] and raw uint8 label maps [H0, W0] of any size -> patch_images [B, 3, P, P] (fp32 or bf16) and target int64
// [B, P*P + 1] in the collater's layout.  mmseg's Resize(ratio_range) / RandomCrop(cat_max_ratio) / RandomFlip /
// PhotoMetricDistortion of data/mm_data/segmentation_dataset.py:157-163, as a pure function of (seed, sample ordinal).
//
//   ifseg_train_draw   records int32 [B, 16] <- splitmix64(seed + (ordinal << 32) + slot)       one memset node + one launch
//                      One workgroup per (sample, crop candidate k = 0..9): the class histogram of the candidate's P x P window
//                      of the nearest-resized label map in LDS (integer atomics, so arrival order cannot matter), its verdict
//                      4 max < 3 P^2 into slot 15 of the record with ONE global integer atomicAdd that also counts the
//                      arrivals; the workgroup that arrives tenth holds all ten verdicts in the value the atomic returned,
//                      picks the first good candidate (else candidate 10) and writes the record.
//   ifseg_train_load   one launch per batch whatever the source shapes, csrc/imgload.hip's shape and code (tile.h): a 256-thread
//                      workgroup owns a 16 x 64 output tile, a thread a pixel with its three channels.  The source footprint of
//                      the tile is staged in LDS with aligned dword loads where it fits, else read from global memory.  Per
//                      pixel: 12 byte taps -> grey levels q -> the photometric chain in registers, tile.h's pixel hook (integers,
//                      and convert() as ONE fp32 operation) -> table -> three coalesced plane stores (bf16: pairs); one nearest
//                      label tap -> one int64 target store.
//                      A record that does not hold a P x P window (only a caller's own records can) poisons its sample: NaN
//                      images and target -1, nothing is read through it.
// No scratch buffer, static launch shapes, nothing read back.
// The counter stream and the ordinal check: common.h; words 6..14 of a record, drawn and read back: photo.h; the NaN tile: tile.h.
#include "tile.h"
#include "photo.h"
#include "../../include/ifseg_hip.h"

namespace {

using namespace tile;
using namespace photo;

constexpr int TL_CANDIDATES = 10;                 // the checked ones; candidate 10 is taken unchecked
constexpr int TL_MAX_P = 4096;

int g_tl_stage_limit = U8_STAGE_LIMIT;

constexpr unsigned TL_SLOT_PHOTO = 23;             // bit 0 of its first draw is the flip
enum { R_NEW_H, R_NEW_W, R_OFF_H, R_OFF_W, R_K, R_FLIP, R_PHOTO, R_ZERO = 15 };      // R_PHOTO: photo.h's nine words

// a record that holds no P x P window of its H0 x W0 source, or whose resize leaves the 31 bits of tile.h's integer rule
__host__ __device__ __forceinline__ bool no_window(int nh, int nw, int offh, int offw, int H0, int W0, int P) {
  return nh < P || nw < P || offh < 0 || offw < 0 || offh > nh - P || offw > nw - P || 2ll * H0 * nh >= (1ll << 31) ||
         2ll * W0 * nw >= (1ll << 31);
}

__device__ __forceinline__ int remap_class(int x, int nseg, int raw) {
  if (raw) x = (x == 0 || x == 255) ? nseg : x - 1;
  return min(x, nseg);
}

// (new_h, new_w) of a source of H0 x W0 whose short side becomes ns: the long side is (2 ns long + s) / (2 s)
__device__ __forceinline__ void resized_size(int H0, int W0, int ns, int* nh, int* nw) {
  const long long s = min(H0, W0);
  const int lg = (int)min((2ll * ns * max(H0, W0) + s) / (2 * s), (long long)0x7fffffff);
  *nh = H0 <= W0 ? ns : lg;
  *nw = H0 <= W0 ? lg : ns;
}

// ------------------------------------------------------------------------------------------------------------- draw
__global__ __launch_bounds__(256) void train_draw_kernel(const ifseg_train_src* __restrict__ tab, unsigned long long seed,
                                                         unsigned long long first, int P, int nseg, int raw, int lo2, int span2,
                                                         int enable, int* __restrict__ params) {
  extern __shared__ int tl_draw_smem[];
  int* hist = tl_draw_smem;             // [256]
  int* red = hist + 256;                // [4]
  int* syt = red + 4;                   // [P] source row of window row y, times W0 -- fits 31 bits: H0 W0 < 2^31 is checked
  int* sxt = syt + P;                   // [P]
  const int b = blockIdx.y, k = blockIdx.x, tid = threadIdx.x;
  const ifseg_train_src s = tab[b];
  const unsigned long long base = stream_base(seed, first, b);
  const unsigned t0 = draw32(base, 0);
  const int ns = max(P, (int)(((unsigned long long)P * (((unsigned long long)lo2 << 32) + (unsigned long long)span2 * t0)) >> 33));
  int nh, nw;
  resized_size(s.H0, s.W0, ns, &nh, &nw);
  const int oh = draw_below(base, 1 + 2 * k, (unsigned)(nh - P + 1));
  const int ow = draw_below(base, 2 + 2 * k, (unsigned)(nw - P + 1));
  hist[tid] = 0;
  for (int i = tid; i < P; i += 256) {
    syt[i] = min((int)((long long)(oh + i) * s.H0 / nh), s.H0 - 1) * s.W0;
    sxt[i] = min((int)((long long)(ow + i) * s.W0 / nw), s.W0 - 1);
  }
  __syncthreads();
  const unsigned char* lab = (const unsigned char*)s.label;
  const int n = P * P;
  for (int i = tid; i < n; i += 256) {
    const int y = i / P, x = i - y * P;
    const int c = remap_class(lab[(long long)syt[y] + sxt[x]], nseg, raw);
    // large flat regions are the rule in a label map: a wave of one class sends one atomic
    const int c0 = __builtin_amdgcn_readfirstlane(c);
    const unsigned long long act = __ballot(1);
    if (__all(c == c0)) {
      if ((int)(threadIdx.x & 63) == __ffsll((long long)act) - 1) atomicAdd(&hist[c0], (int)__popcll(act));
    } else {
      atomicAdd(&hist[c], 1);
    }
  }
  __syncthreads();
  int mx = hist[tid];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = max(mx, __shfl_xor(mx, o));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid != 0) return;
  mx = max(max(red[0], red[1]), max(red[2], red[3]));
  const int ok = 4ll * mx < 3ll * n ? 1 : 0;                 // implies more than one class
  int* rec = params + (long long)b * 16;
  const int old = atomicAdd(&rec[R_ZERO], (1 << 16) | (ok << k));
  if ((old >> 16) != TL_CANDIDATES - 1) return;
  // the tenth arrival: `old` carries the nine other verdicts (distinct bits: the sum is their union)
  const int mask = (old | (ok << k)) & ((1 << TL_CANDIDATES) - 1);
  const int kk = mask ? __ffs(mask) - 1 : TL_CANDIDATES;
  rec[R_NEW_H] = nh;
  rec[R_NEW_W] = nw;
  rec[R_OFF_H] = draw_below(base, 1 + 2 * kk, (unsigned)(nh - P + 1));
  rec[R_OFF_W] = draw_below(base, 2 + 2 * kk, (unsigned)(nw - P + 1));
  rec[R_K] = kk;
  rec[R_FLIP] = (enable & 1) & draw32(base, TL_SLOT_PHOTO);
  photo_draw(rec + R_PHOTO, base, TL_SLOT_PHOTO, (enable >> 1) & 1);
  rec[R_ZERO] = 0;
}

// ------------------------------------------------------------------------------------------------------------- load
template <typename T>
__global__ __launch_bounds__(256) void train_load_kernel(const ifseg_train_src* __restrict__ tab, const int* __restrict__ params,
                                                         int P, int tiles_x, int tiles_y, int nseg, int raw, long long seg0,
                                                         long long eos, const float* __restrict__ lut_g, int rev,
                                                         T* __restrict__ out, long long* __restrict__ target, int stage_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* lut = reinterpret_cast<float*>(smem);

  const Tile t = tile_decode(tiles_x, tiles_y, P, P);
  const auto [b, X0, Y0, xend, yend, lane, wave] = t;
  const ifseg_train_src s = tab[b];
  const int* rec = params + (long long)b * 16;
  const int H0 = s.H0, W0 = s.W0, nh = rec[R_NEW_H], nw = rec[R_NEW_W], offh = rec[R_OFF_H], offw = rec[R_OFF_W];
  const bool flip = rec[R_FLIP] != 0;
  const Photo ph = photo_read(rec + R_PHOTO);               // not validated: any words make some chain, none an address

  const long long plane = (long long)P * P;
  long long* tgt = target + (long long)b * (plane + 1);
  if (blockIdx.x % (tiles_x * tiles_y) == 0 && threadIdx.x == 0) tgt[plane] = eos;

  const int x = min(X0 + lane, P - 1);
  if (no_window(nh, nw, offh, offw, H0, W0, P)) {           // workgroup-uniform
    store_nan_tile(out, (long long)b * 3 * plane, plane, P, t, x);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int yr = Y0 + wave * 4 + j;
      if (yr < P && X0 + lane < P) tgt[(long long)yr * P + x] = -1;
    }
    return;
  }

  for (int i = threadIdx.x; i < 768; i += 256) lut[i] = lut_g[i];

  // the tile's footprint in the source: window pixel (y, x) is pixel (offh + y, offw + xs) of the resized image, xs = x or its
  // mirror.  (2 d + 1) in - out and 2 out stay below 2^31: a record with 2 in out >= 2^31 was poisoned above
  const IntCoord cy{H0, nh}, cx{W0, nw};
  const U8Source src = u8_stage((const unsigned char*)s.image, W0, cy, offh + Y0, offh + yend - 1, cx,
                                offw + (flip ? P - xend : X0), offw + (flip ? P - 1 - X0 : xend - 1), smem + U8_LUT_BYTES,
                                stage_bytes);
  __syncthreads();

  const int xs = offw + (flip ? P - 1 - x : x);
  int x0, x1;
  float lx;
  cx(xs, &x0, &x1, &lx);
  const int lsx = min((int)((long long)xs * W0 / nw), W0 - 1);
  int y0[4], y1[4];
  float ly[4];
  bool ok[4];
  long long erow[4];
  const unsigned char* lab = (const unsigned char*)s.label;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yr = Y0 + wave * 4 + j, y = min(yr, P - 1);
    cy(offh + y, &y0[j], &y1[j], &ly[j]);
    ok[j] = yr < P && X0 + lane < P;
    erow[j] = (long long)b * 3 * plane + (long long)y * P;
    if (ok[j]) {
      const int lsy = min((int)((long long)(offh + y) * H0 / nh), H0 - 1);
      tgt[(long long)y * P + x] = seg0 + remap_class(lab[(long long)lsy * W0 + lsx], nseg, raw);
    }
  }
  u8_pixels(src, y0, y1, x0, x1, ly, lx, lut, rev != 0, [&ph](int* r, int* g, int* b) { photometric(ph, r, g, b); }, out, erow,
            plane, ok, lane, x, xend);
}

// ------------------------------------------------------------------------------------------------------------- plane
// a uint8 plane that travels with the label map (per-pixel loss weights): train_load_kernel's label tap on the plane's own
// bytes.  One 16 x 64 tile per workgroup, lane = x, plain byte stores; a record train_load_kernel would poison writes 0.
__global__ __launch_bounds__(256) void train_plane_kernel(const ifseg_train_src* __restrict__ tab, const int* __restrict__ params,
                                                          int P, int tiles_x, int tiles_y, unsigned char* __restrict__ out) {
  const auto [b, X0, Y0, xend, yend, lane, wave] = tile_decode(tiles_x, tiles_y, P, P);
  const ifseg_train_src s = tab[b];
  const int* rec = params + (long long)b * 16;
  const int H0 = s.H0, W0 = s.W0, nh = rec[R_NEW_H], nw = rec[R_NEW_W], offh = rec[R_OFF_H], offw = rec[R_OFF_W];
  const bool flip = rec[R_FLIP] != 0;
  const bool bad = no_window(nh, nw, offh, offw, H0, W0, P);                     // workgroup-uniform
  const int x = X0 + lane;
  if (x >= xend) return;
  const unsigned char* src = (const unsigned char*)s.label;
  unsigned char* o = out + (long long)b * P * P;
  const int xs = offw + (flip ? P - 1 - x : x);
  const int lsx = bad ? 0 : min((int)((long long)xs * W0 / nw), W0 - 1);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int y = Y0 + wave * 4 + j;
    if (y >= yend) break;
    unsigned char v = 0;
    if (!bad) {
      const int lsy = min((int)((long long)(offh + y) * H0 / nh), H0 - 1);
      v = src[(long long)lsy * W0 + lsx];
    }
    o[(long long)y * P + x] = v;
  }
}

// what both entry points ask of the host copy of the table
int check_table(const ifseg_train_src* th, int B, bool want_images, long long max_short) {
  const long long lim = 1ll << 31;
  for (int b = 0; b < B; ++b) {
    if (!th[b].label || (want_images && !th[b].image)) return IFSEG_ERR_BAD_ARG;
    const long long H0 = th[b].H0, W0 = th[b].W0;
    if (H0 < 1 || W0 < 1 || H0 * W0 * 3 >= lim) return IFSEG_ERR_BAD_SHAPE;
    if (max_short) {
      // the largest resized size this source can be drawn to
      const long long s = std::min(H0, W0), lg = (2 * max_short * std::max(H0, W0) + s) / (2 * s);
      if (2 * s * max_short >= lim || 2 * std::max(H0, W0) * lg >= lim) return IFSEG_ERR_BAD_SHAPE;
    }
  }
  return 0;
}

// the records a caller holds in host memory (may be NULL): one that does not hold a P x P window is refused before the launch
int check_records(const ifseg_train_src* th, const int* params_host, int B, int P) {
  if (!params_host) return 0;
  for (int b = 0; b < B; ++b) {
    const int* r = params_host + 16 * b;
    if (no_window(r[R_NEW_H], r[R_NEW_W], r[R_OFF_H], r[R_OFF_W], th[b].H0, th[b].W0, P)) return IFSEG_ERR_BAD_SHAPE;
  }
  return 0;
}

}  // namespace

extern "C" int ifseg_train_draw(const ifseg_train_src* table_host, const ifseg_train_src* table, int B, int P, int nseg,
                                int raw_labels, unsigned long long seed, long long first_ordinal, int ratio_lo2, int ratio_span2,
                                int enable, int* params, void* stream) {
  (void)hipGetLastError();
  if (!table_host || !table || !params || ((size_t)params & 3) || ((size_t)table & 7)) return IFSEG_ERR_BAD_ARG;
  if (nseg < 1 || nseg > 255 || ratio_lo2 < 0 || ratio_span2 < 0 || ratio_lo2 + ratio_span2 > 64) return IFSEG_ERR_BAD_ARG;
  if (!ordinals_ok(first_ordinal, B)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || B > 65535 || P < 16 || P % 16 || P > TL_MAX_P) return IFSEG_ERR_BAD_SHAPE;
  const long long max_short = std::max<long long>(P, ((long long)P * (ratio_lo2 + ratio_span2)) >> 1);
  if (int rc = check_table(table_host, B, false, max_short)) return rc;
  // slot 15 of every record collects the verdicts: zero before the launch, zero again behind it
  hipError_t e = hipMemsetAsync(params, 0, (size_t)B * 16 * sizeof(int), (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  const size_t lds = (size_t)(256 + 4 + 2 * P) * sizeof(int);
  hipLaunchKernelGGL(train_draw_kernel, dim3(TL_CANDIDATES, B), dim3(256), lds, (hipStream_t)stream, table, seed,
                     (unsigned long long)first_ordinal, P, nseg, raw_labels, ratio_lo2, ratio_span2, enable, params);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_train_load_staging(int max_bytes) { return swap_limit(g_tl_stage_limit, U8_STAGE_LIMIT, max_bytes); }

extern "C" int ifseg_train_load(const ifseg_train_src* table_host, const ifseg_train_src* table, const int* params,
                                const int* params_host, int B, int P, int nseg, int raw_labels, long long seg_id_offset,
                                long long eos, const float* lut, int reverse_channels, void* out, int out_bytes,
                                long long* target, void* stream) {
  (void)hipGetLastError();
  if (!table_host || !table || !params || !lut || !out || !target || (out_bytes != 4 && out_bytes != 2)) return IFSEG_ERR_BAD_ARG;
  if (((size_t)out & 15) || ((size_t)lut & 3) || ((size_t)target & 7) || ((size_t)params & 3) || ((size_t)table & 7))
    return IFSEG_ERR_BAD_ARG;
  if (nseg < 1 || nseg > 255) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || P < 16 || P % 16 || P > TL_MAX_P) return IFSEG_ERR_BAD_SHAPE;
  const long long lim = 1ll << 31;
  if ((long long)B * 3 * P * P >= lim) return IFSEG_ERR_BAD_SHAPE;
  if (int rc = check_table(table_host, B, true, 0)) return rc;
  if (int rc = check_records(table_host, params_host, B, P)) return rc;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(P, P, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  // the resized short side is at least P, so a step of the window is at most s / P source samples on either axis (the long
  // side's rounding adds less than one sample over a tile): tile.h's bound at the ratio s / P, + 1 for the long side
  long long need = 0;
  for (int b = 0; b < B; ++b) {
    const long long H0 = table_host[b].H0, W0 = table_host[b].W0, s = std::min(H0, W0);
    need = std::max(need, footprint_bound(H0, s, P, TILE_ROWS, 4) * u8_rstride(footprint_bound(W0, s, P, TILE_COLS, 4)));
  }
  const int stage = need > g_tl_stage_limit ? g_tl_stage_limit & ~15 : (int)((need + 15) & ~15ll);
  const int lds = U8_LUT_BYTES + stage;
  if (out_bytes == 4)
    hipLaunchKernelGGL(train_load_kernel<float>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, table, params, P,
                       tiles_x, tiles_y, nseg, raw_labels, seg_id_offset, eos, lut, reverse_channels, (float*)out, target, stage);
  else
    hipLaunchKernelGGL(train_load_kernel<bf16_t>, dim3((unsigned)blocks), dim3(256), lds, (hipStream_t)stream, table, params, P,
                       tiles_x, tiles_y, nseg, raw_labels, seg_id_offset, eos, lut, reverse_channels, (bf16_t*)out, target, stage);
  IFSEG_CHECK_LAUNCH();
  return 0;
}

extern "C" int ifseg_train_load_plane(const ifseg_train_src* table_host, const ifseg_train_src* table, const int* params,
                                      const int* params_host, int B, int P, void* out, void* stream) {
  (void)hipGetLastError();
  if (!table_host || !table || !params || !out || ((size_t)params & 3) || ((size_t)table & 7)) return IFSEG_ERR_BAD_ARG;
  if (B < 1 || P < 1 || P > TL_MAX_P) return IFSEG_ERR_BAD_SHAPE;              // any P: no 16-pixel patch grid behind a plane
  if ((long long)B * P * P >= (1ll << 31)) return IFSEG_ERR_BAD_SHAPE;
  if (int rc = check_table(table_host, B, false, 0)) return rc;
  if (int rc = check_records(table_host, params_host, B, P)) return rc;
  int tiles_x, tiles_y;
  long long blocks;
  if (!tile_grid(P, P, B, &tiles_x, &tiles_y, &blocks)) return IFSEG_ERR_BAD_SHAPE;
  hipLaunchKernelGGL(train_plane_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, table, params, P, tiles_x,
                     tiles_y, (unsigned char*)out);
  IFSEG_CHECK_LAUNCH();
  return 0;
}
