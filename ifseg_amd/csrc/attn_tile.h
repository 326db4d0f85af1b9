// Device helpers shared by the two attention kernel generations (attention.hip, attention_bi.hip): the swizzled 128-byte-row
// LDS tile image, the prologue-fragment marker, the -gain V scaling and the bf16 epilogue of a 32 x 32 accumulator tile.
// Helpers that only one generation uses (kx_off, stage_table, the db_* family, the buffer-DMA staging) stay in their file.
#pragma once
#include "common.h"

namespace {

constexpr float NEG_INF = -INFINITY;
constexpr float LOG2E = 1.4426950408889634f;

// LDS images that are read BOTH row-wise (ds_read_b128: 16 rows x one 16-byte chunk per lane group) and transposed
// (ds_read_b64_tr_b16: 4 consecutive rows x one 64-byte granule): the chunk index is XOR-ed with a bit-rotated row id so
// that 16 consecutive rows hit 16 different 16-byte slots of the 256-byte bank line AND 4 consecutive rows hit 4 different
// 64-byte bank quarters.
// V / dO tile, and every [32][64] bf16 operand tile and [32][32] fp32 bias tile of the batch-inner kernels: 128-byte rows
// (8 chunks, two rows per bank line).  vx_swz is the chunk XOR of row r, vx_off the byte offset of (row, byte column);
// vx_off spells the XOR out: through vx_swz the dK/dV kernels of both files allocate registers differently.
__device__ __forceinline__ int vx_off(int r, int colbyte) {
  const int u = r >> 1, hsw = ((u & 1) << 2) | ((u >> 1) & 3);
  return r * 128 + ((((colbyte >> 4) ^ hsw) & 7) << 4) + (colbyte & 15);
}
__device__ __forceinline__ int vx_swz(int r) { const int u = r >> 1; return ((u & 1) << 2) | ((u >> 1) & 3); }

// Marks a register fragment as used here.  Fragments loaded from global memory in a kernel prologue and first read
// inside the main loop leave their loads "pending" at the loop header in the compiler's wait-count model; it then puts
// s_waitcnt vmcnt(N) with small N in front of their uses INSIDE the loop, and from the second iteration on those waits
// hit the loop's own prefetch (global loads / LDS-DMA for the next tile), serialising it with the MFMAs.
__device__ __forceinline__ void consume_frag(const bf16x8& f) {
  typedef __attribute__((__vector_size__(4 * sizeof(unsigned)))) unsigned u32x4_t;
  asm volatile("" :: "v"(__builtin_bit_cast(u32x4_t, f)));
}

// eight bf16 times f, rounded back to bf16 (the dK/dV kernels' -gain V operand)
__device__ __forceinline__ uint4 scale_bf16x8(uint4 v, float f) {
  unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    w[i] = pack2bf(__uint_as_float(w[i] << 16) * f, __uint_as_float(w[i] & 0xffff0000u) * f);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// Epilogue of a 32 x 32 accumulator tile whose row (query / key) is the lane: element r of lane (half, x) is column
// (r&3) + 8*(r>>2) + 4*half, i.e. 8-byte runs.  The two lanes of a row exchange one run each (v_permlane32_swap), so
// that every lane stores 16 contiguous bytes: half as many store instructions (the store tail is issue-bound).
__device__ __forceinline__ void store_tile_bf16(bf16_t* rowp, const f32x16& acc, float scale, int half, bool valid) {
#pragma unroll
  for (int rgp = 0; rgp < 2; ++rgp) {
    const int e0 = rgp * 8, e1 = rgp * 8 + 4;
    const unsigned x0 = pack2bf(acc[e0] * scale, acc[e0 + 1] * scale), x1 = pack2bf(acc[e0 + 2] * scale, acc[e0 + 3] * scale);
    const unsigned y0 = pack2bf(acc[e1] * scale, acc[e1 + 1] * scale), y1 = pack2bf(acc[e1 + 2] * scale, acc[e1 + 3] * scale);
    const auto p0 = __builtin_amdgcn_permlane32_swap(x0, y0, false, false);
    const auto p1 = __builtin_amdgcn_permlane32_swap(x1, y1, false, false);
    // lanes 0..31: columns 16*rgp .. +7 (own run, partner's run); lanes 32..63: columns 16*rgp + 8 .. +15
    if (valid) *reinterpret_cast<uint4*>(rowp + 16 * rgp + 8 * half) = make_uint4(p0[0], p1[0], p0[1], p1[1]);
  }
}

}  // namespace
