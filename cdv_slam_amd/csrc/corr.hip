// corr.hip -- altcorr: patch-to-frame local correlation + bilinear blend, gfx950.
//
// Reference: cdvslam/altcorr/correlation_kernel.cu:82-136 (27.5 M threads per level, each doing 24
// strided 2-byte loads from channel-planar maps), :213-232 (raw 8x8 volume written to HBM and re-read
// by four ATen slice-multiply-add passes), then torch.stack of the two levels (slam.py:323).
//
// Here (cdv_corr_fused): ONE launch for both pyramid levels.  One wave per edge:
//   * the union window of the 9 patch pixels (<= 16 x 12 feature pixels, typically 10 x 11) is packed densely into the
//     16 pixel slots of the MFMA A operand, loaded straight from a CHANNELS-LAST padded feature ring (one pixel = C
//     contiguous halves, so a lane's 8 k-values are one 16-byte buffer load; the descriptor's range check and the zero
//     margins give the reference's out-of-bounds rule -- no LDS staging of the inputs, no masks);
//   * the 3x3xC patch tile is the B operand (9 of 16 columns used), one 16-byte load from the pixel-major tile;
//   * v_mfma_f32_16x16x32_f16 produces 16 window pixels x 9 patch pixels per instruction (f32 accumulate);
//   * every window group of a level is requested before its first MFMA, the level-1 request flies under the level-0
//     blend (two dependent memory round trips per edge: indices + coordinates, then patch tile + windows);
//   * the raw volume lives only in LDS (f16 like the reference's, 3.7 KB per wave, conflict-free row stride); the
//     8x8 -> 7x7 bilinear blend of every patch pixel reads it back with its own sub-pixel offset, separably;
//   * the [882]-half row of the edge is staged in LDS (over the raw volume) and leaves as 16-byte-per-lane stores.
// corr_fused2_kernel is the product kernel (C <= 32: CDV-SLAM's DIMF = 24); corr_wide_kernel serves C up to 128 (DPVO).
// Algorithmic HBM bytes per edge: 1764 out + 72 coords + 16 idx (+ the feature maps once): DESIGN.md.
// (The rings and tiles it reads are kept by rings.hip; the reference-shaped per-level operators are altcorr_fwd.hip.)
#include <math.h>
#include <stdlib.h>

#include "cdv_common.h"
#include "cdv_graph.h"
#include "cdv_parts.h"

CDV_STAMP_TU(corr)

// ablation switches of the diagnostic build (make STAMPS=1, env CDV_CORR_EXP): compiled out of the product library
#ifdef CDV_STAMPS
#define CDV_EXP(bit) ((exp & (bit)) != 0)
#else
#define CDV_EXP(bit) false
#endif

namespace {

// HBM layout of the feature rings the fused kernel gathers from ("padded channels-last"; written by rings.hip):
//   [slot][H + 2*PADY][W + 2*PADX][C] f16, zero margins.  A 16 x 12 window box whose origin is clamped to
//   [-PADX, W] x [-PADY, H] never leaves the allocation, and everything it reads outside the image is the
//   zero the reference's out-of-bounds rule asks for (correlation_kernel.cu:122) -- no per-lane bounds
//   tests, no masks in the kernel.
constexpr int PADX = CDV_FMAP_PADX;             // 16
constexpr int PADY = CDV_FMAP_PADY;             // 12

// Per-wave LDS: the raw correlation volume of ONE level in f16 (the reference's raw volume is f16 too,
// correlation_kernel.cu:207) + the staged output row of the edge.
constexpr int RAW_ROWS = 12;                    // window rows the fast path holds (typical: 10-11 / 8-9)
constexpr int NQ_MAX = 8;                       // 16-pixel groups of the densely packed window kept in registers at a time (144 pixels; typical
                                                // windows: 110-121 / 81 pixels; larger ones take a second round): 78 VGPRs,
                                                // 6 waves per SIMD
// halfs per patch pixel: 102 dwords = 6 (mod 32), so the 16 lanes of a ds_write_b64 group (patch pixels n = 0..15 of
// one MFMA D tile, 2 banks each) cover all 32 banks exactly once (with the earlier 100 dwords the stores were 3-way
// conflicted: 112 of 296 LDS cycles per edge)
constexpr int RAW_MSH = RAW_ROWS * 16 + 12;
constexpr int RAW_HALFS = 9 * RAW_MSH;          // 1836
constexpr int CW = 4;                           // waves (= edges) per workgroup of the product kernel; the waves are independent (no barrier)
constexpr int OUT_POLICY = 16;                  // cache policy of the product kernel's output stores: sc1 (write-through)
constexpr int OUT_HALFS = 896;                  // the staged output row: 882 halfs, linear (the copy-out needs no index math)
constexpr int WAVE_LDS_BYTES = RAW_HALFS * 2 + OUT_HALFS * 2;  // wide kernel: raw volume + staged row
// product kernel: the staged row re-uses the raw volume (written after the last blend has read it); the D-tile lanes
// that are not patch pixels (n >= 9) store into a 512-byte dump on the banks the same lanes of a full 16-row layout
// would use
constexpr int DUMP_OFF_B = 3712;                // >= RAW_HALFS * 2, a multiple of 128 B (bank 0)
constexpr int WAVE_LDS2_BYTES = DUMP_OFF_B + 512;
static_assert(RAW_HALFS * 2 <= DUMP_OFF_B && OUT_HALFS * 2 <= RAW_HALFS * 2, "LDS layout");

typedef _Float16 cdv_half4 __attribute__((ext_vector_type(4)));
typedef _Float16 cdv_half2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void wave_lds_sync() {
  // LDS operations of one wave execute in order; this only has to stop the compiler from moving the
  // reads above the writes and to wait for outstanding DS ops.  (Not a workgroup-scope release fence: that one
  // also drains vmcnt, i.e. waits for the window loads of the NEXT level that are meant to fly under the blend.)
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// all-reduce (min or max) of an int over the 16 lanes of a DPP row by rotation (row_ror 8,4,2,1): the DPP operand is
// folded into the min / max itself (one VALU instruction per step; integers need no NaN canonicalisation).  The
// s_nop covers the two wait states between a VALU write and a DPP read of the same register.
template <bool IS_MIN>
__device__ __forceinline__ int row16_reduce_i32(int v) {
#define CDV_ROR(n)                                                                                             \
  if (IS_MIN) asm volatile("s_nop 1\n\tv_min_i32_dpp %0, %1, %1 row_ror:" #n " row_mask:0xf bank_mask:0xf" : "=v"(v) : "0"(v)); \
  else asm volatile("s_nop 1\n\tv_max_i32_dpp %0, %1, %1 row_ror:" #n " row_mask:0xf bank_mask:0xf" : "=v"(v) : "0"(v));
  CDV_ROR(8) CDV_ROR(4) CDV_ROR(2) CDV_ROR(1)
#undef CDV_ROR
  return v;
}

// the four extremes the window boxes need (min / max of x and of y) with the four rotation chains interleaved: every
// DPP read is three instructions behind the write of its register, so no wait states (s_nop) are needed at all
__device__ __forceinline__ void row16_minmax4(int x, int y, int& xmin, int& xmax, int& ymin, int& ymax) {
  int a = x, b = x, c = y, d = y;
#define CDV_STEP(n)                                                                                  \
  asm volatile("v_min_i32_dpp %0, %0, %0 row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"               \
               "v_max_i32_dpp %1, %1, %1 row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"               \
               "v_min_i32_dpp %2, %2, %2 row_ror:" #n " row_mask:0xf bank_mask:0xf\n\t"               \
               "v_max_i32_dpp %3, %3, %3 row_ror:" #n " row_mask:0xf bank_mask:0xf"                    \
               : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
  asm volatile("s_nop 1" ::: "memory");   // the copies above may be the instructions right before the first DPP read
  CDV_STEP(8) CDV_STEP(4) CDV_STEP(2) CDV_STEP(1)
#undef CDV_STEP
  xmin = a; xmax = b; ymin = c; ymax = d;
}

struct LevelParams {
  const _Float16* fmap;  // [slots][H + 2 PADY][W + 2 PADX][C]
  int H, W;
  float inv_scale;       // 1 / scale, scale a power of two: x * inv_scale == x / scale exactly (slam.py:321-322)
  int shift;             // log2(scale / scale of level 0) >= 0: floor(x / scale) == floor(x / scale0) >> shift
};

// wave-uniform window box of one level (all members live in SGPRs)
struct Box {
  int x0, y0;        // unclamped origin of the union window of the 9 patch pixels
  int Wb, Hb;        // extent
  bool fast;         // fits the 16 x RAW_ROWS tile
  int stride;        // halfs between window rows of the raw volume in LDS (dense: Wb; per-pixel path: 16)
  bool outside;      // fast && entirely outside the padded image: the level is all zeros
  int x0c, y0c;      // origin clamped into the padded map
};

__device__ __forceinline__ int floor_clamped(float v) {
  return (int)fminf(fmaxf(floorf(v), -1.0e6f), 1.0e6f);
}

// ixmin .. iymax: extreme floor(coordinate / scale) over the 9 patch pixels (floor is monotone, so the extreme pixels
// give the extreme integer coordinates)
__device__ __forceinline__ Box make_box(int ixmin, int ixmax, int iymin, int iymax, const LevelParams& LP) {
  Box b;
  b.x0 = ixmin - 3;   // slam.py:321-322, correlation_kernel.cu:107-110
  b.y0 = iymin - 3;
  b.Wb = ixmax + 4 - b.x0 + 1;
  b.Hb = iymax + 4 - b.y0 + 1;
  b.fast = (b.Wb <= 16) && (b.Hb <= RAW_ROWS);
  b.stride = b.fast ? b.Wb : 16;
  b.x0c = min(max(b.x0, -PADX), LP.W);
  b.y0c = min(max(b.y0, -PADY), LP.H);
  b.outside = (b.x0c != b.x0) || (b.y0c != b.y0);  // a clamped <=16 x <=12 box lies entirely in the margin
  return b;
}

// D[window pixel n][patch pixel m] = sum_c window[n][c] * patch[m][c]; lane (m = lane & 15, g = lane >> 4)
// receives the 4 consecutive window pixels n = 4g .. 4g+3 of row t: one 8-byte LDS store of 4 halfs.
template <int KS>
__device__ __forceinline__ void mfma_row_store(const cdv_half8 (&win)[KS], const cdv_half8 (&pat)[KS],
                                               _Float16* __restrict__ raw_lane, int t) {
  cdv_float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < KS; s++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(win[s], pat[s], acc, 0, 0, 0);
  cdv_half4 h = {(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};
  *reinterpret_cast<cdv_half4*>(raw_lane + t * 16) = h;
}

// per-lane blend geometry of one level: lane = 7 m + xo
struct BlendGeo {
  int hb;         // BYTE offset of the half raw[m][by][bx + xo]
  int stride_b;   // bytes between window rows
  cdv_half2 wx;   // (1 - dx, dx): horizontal taps, dx rounded to f16 as the reference casts it before blending
  float dy;       // vertical sub-pixel offset (rounded to f16 likewise)
};

__device__ __forceinline__ BlendGeo blend_geo(float xm, float ym, int m, int xo, const LevelParams& LP,
                                              const Box& b, bool per_pixel) {
  BlendGeo g;
  const float x = xm * LP.inv_scale, y = ym * LP.inv_scale;
  const float fxf = floorf(x), fyf = floorf(y);
  const float dx = (float)(_Float16)(x - fxf);   // correlation_kernel.cu:223-224
  g.wx = cdv_half2{(_Float16)(1.0f - dx), (_Float16)dx};
  g.dy = (float)(_Float16)(y - fyf);
  const int bx = per_pixel ? 0 : floor_clamped(x) - 3 - b.x0;
  const int by = per_pixel ? 0 : floor_clamped(y) - 3 - b.y0;
  g.hb = 2 * (m * RAW_MSH + __mul24(by, b.stride) + bx + xo);   // |by| is small: not the quarter-rate v_mul_lo_u32
  g.stride_b = 2 * b.stride;
  return g;
}

// 8x8 -> 7x7 bilinear blend, separable.  The pair (c0, c1) of a window row starts at an arbitrary half offset; a
// 4-byte LDS read at an odd half offset is an UNALIGNED access (very slow on the LDS), so the two aligned dwords
// around it are read (one ds_read2_b32) and funnel-shifted (v_alignbit) into the pair; the horizontal tap is one
// v_dot2_f32_f16 (exact f16 products, f32 sum).  5 VALU + 1 LDS instruction per window row.
__device__ __forceinline__ float dot2_f16(uint32_t pair, uint32_t w) {
  // v_dot2_f32_f16 with a literal zero accumulator (the compiler's pick, v_dot2c, needs a v_mov 0 every time)
  float r;
  asm("v_dot2_f32_f16 %0, %1, %2, 0" : "=v"(r) : "v"(pair), "v"(w));
  return r;
}

// The vertical tap and the rounding of the result to f16 are written as one expression, (f16)fma(dy, h1 - h0, h0): the
// compiler emits v_fma_mixlo/hi_f16 (f32 arithmetic, ONE rounding to f16) in every kernel that inlines this.
// (The wide kernel keeps float results and rounds when it packs them: its conditionally blended, zero-initialised f16
// results were mis-assembled into v_fma_mixhi_f16 chains by the compiler -- every second value wrong.)
template <typename TR>
__device__ __forceinline__ void blend_level(const _Float16* __restrict__ raw, const BlendGeo& g, TR (&res)[7]) {
  const char* rb = reinterpret_cast<const char*>(raw);   // raw is 16-byte aligned
  float h[8];
  // even and odd rows keep their own aligned LDS pointer and funnel shift: two rows further down the byte offset
  // moves by 2 stride_b = 4 stride, a multiple of 4, so neither alignment changes -- 3 VALU per row
  // (pointer add, v_alignbit, v_dot2)
  const int hb1 = g.hb + g.stride_b;
  const char* p0 = rb + (g.hb & ~3);
  const char* p1 = rb + (hb1 & ~3);
  const unsigned s0 = (unsigned)g.hb << 3, s1 = (unsigned)hb1 << 3;   // shift = low 5 bits: 0 or 16
  const int step2 = 2 * g.stride_b;
  const uint32_t wxb = __builtin_bit_cast(uint32_t, g.wx);
#pragma unroll
  for (int r = 0; r < 8; r++) {
    const uint32_t* pd = reinterpret_cast<const uint32_t*>((r & 1) ? p1 : p0);
    const uint32_t lo = pd[0], hi = pd[1];           // hi is unused when the pair is dword aligned (stays in the wave's LDS)
    const uint32_t pr = __builtin_amdgcn_alignbit(hi, lo, (r & 1) ? s1 : s0);
    h[r] = dot2_f16(pr, wxb);
    if (r & 1) p1 += step2; else p0 += step2;
  }
#pragma unroll
  for (int yo = 0; yo < 7; yo++) res[yo] = (TR)__builtin_fmaf(g.dy, h[yo + 1] - h[yo], h[yo]);
}

// wide reprojection footprint (strong zoom / rotation): every patch pixel gets its own 8x8 window; two
// window rows share one MFMA (pixels 0-7 | 8-15), only column m of D is kept.  Rare: compact, not tuned.
// (xv, yv): the coordinates of patch pixel m are in lane LM * m
template <int KS, int LM = 1>
__device__ __forceinline__ void slow_level(const LevelParams& LP, int64_t jslot, float xv, float yv,
                                           const cdv_half8 (&pat)[KS], _Float16* __restrict__ raw, int lane, int C) {
  const int n = lane & 15, g = lane >> 4;
  const int Wp = LP.W + 2 * PADX, Hp = LP.H + 2 * PADY;
  const _Float16* fbase = LP.fmap + (size_t)jslot * Hp * Wp * C;
#pragma unroll 1   // rare path: kept rolled, so that it adds no registers to the kernel (occupancy of the common path)
  for (int m = 0; m < 9; m++) {
    const float xm = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xv), LM * m));
    const float ym = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(yv), LM * m));
    const int x0 = floor_clamped(xm * LP.inv_scale) - 3, y0 = floor_clamped(ym * LP.inv_scale) - 3;
    const int x0c = min(max(x0, -PADX), LP.W), y0c = min(max(y0, -PADY), LP.H);
    const bool outside = (x0c != x0) || (y0c != y0);
#pragma unroll 1
    for (int t2 = 0; t2 < 4; t2++) {
      const int py = y0c + PADY + 2 * t2 + (n >> 3), px = x0c + PADX + (n & 7);
      cdv_float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < KS; s++) {
        const int chg = min(32 * s + 8 * g, C - 8);  // lanes of the k padding re-read real (finite) data
        const cdv_half8 v = *reinterpret_cast<const cdv_half8*>(fbase + ((size_t)py * Wp + px) * C + chg);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(v, pat[s], acc, 0, 0, 0);
      }
      if (n == m) {
        const int row = 2 * t2 + (g >> 1), col = 4 * (g & 1);
        cdv_half4 h = {(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};
        if (outside) h = cdv_half4{0, 0, 0, 0};
        *reinterpret_cast<cdv_half4*>(raw + m * RAW_MSH + row * 16 + col) = h;
      }
    }
  }
}

// a level that contributes nothing (window entirely off the padded map, invalid indices): the raw volume is zeroed and
// the blend runs as always -- no per-value selects, no zero-initialised result registers on the common path
__device__ __forceinline__ void zero_raw(_Float16* __restrict__ raw, int lane) {
  typedef uint32_t cdv_u32x4z __attribute__((ext_vector_type(4)));
  const cdv_u32x4z z = {0u, 0u, 0u, 0u};
  for (int i = lane; i < RAW_HALFS / 8; i += 64) reinterpret_cast<cdv_u32x4z*>(raw)[i] = z;
}

// ---- wide feature vectors (DPVO, C = 128; KS = C / 32 k-steps): one 16-pixel tile per window row ---------------
template <int KS>
__global__ __launch_bounds__(256) void corr_wide_kernel(const _Float16* __restrict__ gmap, LevelParams L0,
                                                         LevelParams L1, const float* __restrict__ coords,
                                                         const int64_t* __restrict__ kk,
                                                         const int64_t* __restrict__ jj,
                                                         const int32_t* __restrict__ order,
                                                         _Float16* __restrict__ out, int E, int64_t Ng, int64_t slots,
                                                         int C, int nlev, int64_t kmod, int64_t jmod, uint32_t kmagic,
                                                         uint32_t jmagic, int gmap_pm,
                                                         int exp) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  _Float16* raw = reinterpret_cast<_Float16*>(smem_raw + (size_t)wave * WAVE_LDS_BYTES);
  _Float16* outT = raw + RAW_HALFS;
  const int p = blockIdx.x * 4 + wave;
  if (p >= E) return;  // no block-wide barriers below: waves are independent
  const int e = order ? __builtin_amdgcn_readfirstlane(order[p]) : p;   // wave-uniform: scalar loads below
  CDV_STAMP(corr, p, 0);

  // ---- round trip 1: indices (scalar) and the 18 coordinates ----------------------------------------
  int64_t kpatch = kk[e], jslot = jj[e];
  // index % modulus (slam.py:319-320) with the host's reciprocal: q = mulhi(x, ceil(2^32 / d)) is x / d or one more
  // for 0 <= x < 2^31, so one correction step; the 64-bit division the compiler would emit is ~150 scalar instructions
  if (kmod > 0 && kpatch >= 0 && kpatch < ((int64_t)1 << 31)) {
    const uint32_t x = (uint32_t)kpatch, d = (uint32_t)kmod;
    const uint32_t q = __builtin_amdgcn_readfirstlane((int)__umulhi(x, kmagic));
    const int32_t r = (int32_t)(x - q * d);
    kpatch = (d == 1u) ? 0 : (r < 0 ? r + (int32_t)d : r);
  }
  if (jmod > 0 && jslot >= 0 && jslot < ((int64_t)1 << 31)) {
    const uint32_t x = (uint32_t)jslot, d = (uint32_t)jmod;
    const uint32_t q = __builtin_amdgcn_readfirstlane((int)__umulhi(x, jmagic));
    const int32_t r = (int32_t)(x - q * d);
    jslot = (d == 1u) ? 0 : (r < 0 ? r + (int32_t)d : r);
  }
  const bool idx_ok = kpatch >= 0 && kpatch < Ng && jslot >= 0 && jslot < slots;
  if (!idx_ok) { kpatch = 0; jslot = 0; }  // reference behaviour is undefined here; stay in bounds
  if (CDV_EXP(16)) jslot = 0;                 // experiment bit 4: every edge reads map slot 0 (L2-resident)
  const float* cptr = coords + (size_t)e * 18;
  const int mm = lane < 9 ? lane : 0;       // row 0 of the wave: lanes 0..8 own patch pixel m, 9..15 mirror 0
  const int bm = min(lane / 7, 8), bxo = lane - 7 * (lane / 7);  // blend role of this lane: (m, x offset)
  // ONE vector load for the 18 coordinates (lane l < 18 holds value l), handed to the lanes that need them through
  // the LDS crossbar (ds_bpermute): the vector-memory pipe is the busy one in this kernel
  const int cval = __float_as_int(cptr[min(lane, 17)]);
  const float xv = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * mm, cval));
  const float yv = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (9 + mm), cval));
  const float xb = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * bm, cval));
  const float yb = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (9 + bm), cval));
  // integer pixel coordinates at level 0 per lane, their extremes over the patch (DPP row reductions), and from
  // those -- all scalar from here -- the window boxes of both levels (level 1: an arithmetic shift)
  const int ixl = floor_clamped(xv * L0.inv_scale), iyl = floor_clamped(yv * L0.inv_scale);
  const int ixmin = __builtin_amdgcn_readfirstlane(row16_reduce_i32<true>(ixl));
  const int ixmax = __builtin_amdgcn_readfirstlane(row16_reduce_i32<false>(ixl));
  const int iymin = __builtin_amdgcn_readfirstlane(row16_reduce_i32<true>(iyl));
  const int iymax = __builtin_amdgcn_readfirstlane(row16_reduce_i32<false>(iyl));
  const Box b0 = make_box(ixmin, ixmax, iymin, iymax, L0);
  const int sh1 = nlev == 2 ? L1.shift : 0;
  const Box b1 = make_box(ixmin >> sh1, ixmax >> sh1, iymin >> sh1, iymax >> sh1, nlev == 2 ? L1 : L0);
  CDV_STAMP(corr, p, 1);

  const int n = lane & 15, g = lane >> 4;
  // per-lane byte offset inside a window row: pixel n, channel group g (the k-padding group re-reads real,
  // finite data: its products meet the zero k-slots of the patch fragment)
  // ---- round trip 2: patch tile (MFMA B operand) ------------------------------------------------------
  cdv_half8 pat[KS];
  if (gmap_pm) {
    // pixel-major tiles [9][C]: one 16-byte buffer load per k-step; the descriptor covers exactly this tile, so the
    // lanes that are not patch pixels (n >= 9) and the k padding (forced offset) read zeros from the range check
    typedef int cdv_i32x4p __attribute__((ext_vector_type(4)));
    const unsigned tile_b = 9u * (unsigned)C * 2u;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<char*>(reinterpret_cast<const char*>(gmap) + (size_t)kpatch * tile_b), (short)0, (int)tile_b, 0x00020000);
#pragma unroll
    for (int s = 0; s < KS; s++) {
      const int chg = 32 * s + 8 * g;
      const unsigned voff = (chg < C) ? (unsigned)(n * C + chg) * 2u : 0x40000000u;
      pat[s] = __builtin_bit_cast(cdv_half8, (cdv_i32x4p)__builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, 0, 0));
    }
  } else {
    const _Float16* gp = gmap + (size_t)kpatch * C * 9 + (n < 9 ? n : 0);
#pragma unroll
    for (int s = 0; s < KS; s++) {
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int ch = 32 * s + 8 * g + j;
        const _Float16 v = gp[min(ch, C - 1) * 9];
        pat[s][j] = (n < 9 && ch < C) ? v : (_Float16)0.f;
      }
    }
  }

  float res0[7], res1[7];
#pragma unroll
  for (int i = 0; i < 7; i++) { res0[i] = 0.f; res1[i] = 0.f; }
  // lanes n >= 9 of the D tile are not patch pixels: they store into the (not yet used) staging area instead of
  // being masked off (no EXEC save/restore around every store)
  _Float16* raw_lane = (n < 9) ? raw + n * RAW_MSH + 4 * g : outT + ((n - 9) * 4 + g) * 4;

  // wide feature vectors (DPVO, C = 128): rows in batches of 2 to stay inside the register file
  for (int lev = 0; lev < nlev; lev++) {
    const LevelParams& LP = lev == 0 ? L0 : L1;
    Box b = lev == 0 ? b0 : b1;
    b.stride = 16;  // this path stores one 16-pixel tile per window row
    const int Wp = LP.W + 2 * PADX, Hp = LP.H + 2 * PADY;
    if (lev == 1) wave_lds_sync();
    if (b.fast && !b.outside) {
      const _Float16* fb = LP.fmap + (((size_t)jslot * Hp + (b.y0c + PADY)) * Wp + (b.x0c + PADX)) * C;
      for (int t = 0; t < b.Hb; t++) {
        cdv_half8 wa[KS];
#pragma unroll
        for (int s = 0; s < KS; s++)
          wa[s] = *reinterpret_cast<const cdv_half8*>(fb + ((size_t)t * Wp + n) * C + min(32 * s + 8 * g, C - 8));
        cdv_float4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KS; s++) acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wa[s], pat[s], acc, 0, 0, 0);
        if (n < 9) {
          cdv_half4 h = {(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};
          *reinterpret_cast<cdv_half4*>(raw_lane + t * 16) = h;
        }
      }
    } else if (!b.fast) {
      slow_level<KS>(LP, jslot, xv, yv, pat, raw, lane, C);
    }
    wave_lds_sync();
    if (!(b.fast && b.outside)) {
      const BlendGeo gg = blend_geo(xb, yb, bm, bxo, LP, b, !b.fast);
      if (lev == 0) blend_level(raw, gg, res0); else blend_level(raw, gg, res1);
    }
  }

  // ---- stage the edge's output row [x][y][m][lev] in LDS, then 256-byte coalesced stores ------------
  if (lane < 63 && !CDV_EXP(512)) {
    if (nlev == 2) {
      uint32_t* o32 = reinterpret_cast<uint32_t*>(outT) + bxo * 63 + bm;   // dword (x, y, m) = 63 x + 9 y + m
#pragma unroll
      for (int yo = 0; yo < 7; yo++) {
        const _Float16 h0 = idx_ok ? (_Float16)res0[yo] : (_Float16)0.f;
        const _Float16 h1 = idx_ok ? (_Float16)res1[yo] : (_Float16)0.f;
        const uint32_t lo = __builtin_bit_cast(unsigned short, h0), hi = __builtin_bit_cast(unsigned short, h1);
        o32[yo * 9] = lo | (hi << 16);
      }
    } else {
#pragma unroll
      for (int yo = 0; yo < 7; yo++) outT[(bxo * 7 + yo) * 9 + bm] = idx_ok ? (_Float16)res0[yo] : (_Float16)0.f;
    }
  }
  wave_lds_sync();
  CDV_STAMP(corr, p, 7);
  if (!CDV_EXP(2)) {                             // experiment bit 1: no global store
  if (nlev == 2) {
    // 441 dwords: two 16-byte-per-lane stores (256 + 184 dwords) and one last dword.  The row starts on a 4-byte
    // boundary only (1764 B per edge); global memory takes the unaligned 16-byte accesses.
    const uint32_t* src = reinterpret_cast<const uint32_t*>(outT);
    uint32_t* dst = reinterpret_cast<uint32_t*>(out) + (size_t)e * 441;
    typedef uint32_t cdv_u32x4 __attribute__((ext_vector_type(4)));
    typedef uint32_t cdv_u32x4u __attribute__((ext_vector_type(4), aligned(4)));
    const cdv_u32x4 v0 = *reinterpret_cast<const cdv_u32x4*>(src + 4 * lane);
    *reinterpret_cast<cdv_u32x4u*>(dst + 4 * lane) = v0;
    if (lane < 46) {
      const cdv_u32x4 v1 = *reinterpret_cast<const cdv_u32x4*>(src + 256 + 4 * lane);
      *reinterpret_cast<cdv_u32x4u*>(dst + 256 + 4 * lane) = v1;
    }
    if (lane == 63) dst[440] = src[440];
  } else {
    _Float16* dst = out + (size_t)e * 441;
#pragma unroll
    for (int i = 0; i < 7; i++) {
      const int t = i * 64 + lane;
      if (t < 441) dst[t] = outT[t];
    }
  }
  }
  CDV_STAMP(corr, p, 8);
}

// ---- the product kernel (C <= 32) ------------------------------------------------------
// One wave per edge, both levels (header of this file); built around what bounds it on MI355X -- not bytes and not one saturated unit, but the serial chain of one wave (6 waves per SIMD;
// ~14,000 cycles per edge of which ~1,600 are its VALU issue) and the scalar unit the four SIMDs of a CU share:
//   * every argument the first instructions need sits at the front of ONE argument struct (one scalar load, not six
//     dependent ones); strides, pitches and the (biased) ring bases are precomputed by the host;
//   * the coordinate load is issued before the index loads are waited for (one memory round trip, not two);
//   * indices are handled in 32-bit scalar arithmetic (a 64-bit compare is a VALU instruction on this ISA);
//   * window addressing in float arithmetic, 3 VALU per load (see CDV_LD1);
//   * no result selects: a level that contributes nothing gets a zeroed raw volume, both levels of one output dword
//     are ONE v_cvt_pk_f16_f32;
//   * workgroup b runs on XCD b % 8: XCD x takes the x-th contiguous eighth of the edge list (the edges of one target
//     frame are neighbours in the list, so a frame's windows meet in one L2 instead of eight).
struct CorrLevel {
  const char* base_m;   // ring base MINUS 0x4B000000 bytes (the float-bit-pattern offsets of the window loads carry that bias)
  int H, W;
  float inv_scale;
  int shift;
  uint32_t pitch;       // bytes per padded row
  uint32_t slot_bytes;  // bytes per slot
};
struct CorrArgs2 {
  const float* coords;
  const int64_t* kk;
  const int64_t* jj;
  const int32_t* order;
  int E;
  uint32_t kmod, jmod, kmagic, jmagic;
  uint32_t Ng, slots;
  const char* gmap;     // tiles, f16: pixel-major [Ng][9][C] (gmap_pm) or the reference's planar [Ng][C][3][3]
  _Float16* out;
  CorrLevel L0, L1;
  int C;
  int gmap_pm;
  int exp;
  // one-level launches only: output element (e, t) at out[e * out_pitch + t * out_stride + out_off] (inside the row of a
  // two-level result), and edges whose coordinates equal coords_ref * ref_mul bit for bit are skipped (their values are
  // in place already: cdv_corr_level_checked_interleaved)
  int out_stride, out_off, out_pitch;   // out_pitch: halves from one edge's row to the next
  const float* coords_ref;
  float ref_mul;
  // packed per-edge input stream in PROCESSING order (written by the index build next to `order`): record p =
  // {18 coords, edge id, patch-ring index, frame-ring index (0xFFFFFFFF: invalid), ...} -- cdv_graph.h CORR_REC_WORDS
  const uint32_t* rec;
  // != NULL: the number of edges is *dynE (include/cdvslam_hip.h CDV_DYN_E); E above bounds it and sized the launch
  const int32_t* dynE;
};

constexpr uint32_t FBIAS = 0x4B000000u;   // bit pattern of 2^23

__device__ __forceinline__ LevelParams level_params(const CorrLevel& L) {
  return LevelParams{reinterpret_cast<const _Float16*>(L.base_m + (size_t)FBIAS), L.H, L.W, L.inv_scale, L.shift};
}

// one edge; its first round trip (coordinates: lane l < 18 holds value l; ring indices already reduced and checked)
// was issued by the caller
// what the caller's first round trip brought: either the 18 coordinates spread over the lanes (cval: lane l < 18 holds
// value l; the box is then found here), or -- from the packed input stream -- this lane's blend coordinates directly and
// the wave-uniform extremes of floor(x), floor(y) over the patch (level 0) as scalars
struct EdgeCoords {
  int cval;
  float xb, yb;
  int ixmin, ixmax, iymin, iymax;
};

template <int CC, int NLEV, bool REC>
__device__ __forceinline__ void corr_edge(const CorrArgs2& a, int p, int e, const EdgeCoords& ec, uint32_t kq, uint32_t jq,
                                          bool idx_ok, int lane, _Float16* __restrict__ raw, _Float16* __restrict__ outT) {
  CDV_STAMP(corr, p, 0);
  const int C = CC ? CC : a.C;
#ifdef CDV_STAMPS
  const int exp = a.exp;
#endif
  const int mm = lane < 9 ? lane : 0;       // row 0 of the wave: lanes 0..8 own patch pixel m, 9..15 mirror 0
  const int bm = min(lane / 7, 8), bxo = lane - 7 * (lane / 7);  // blend role of this lane: (m, x offset)
  const int n = lane & 15, g = lane >> 4;
  if (!idx_ok) { kq = 0u; jq = 0u; }  // reference behaviour is undefined here; stay in bounds, emit zeros
  if (CDV_EXP(16)) jq = 0u;
  const int64_t jslot = (int64_t)jq;

  // ---- patch tile (MFMA B operand): one 16-byte buffer load; the descriptor covers exactly this tile, so the lanes
  // that are not patch pixels (n >= 9) and the k padding (forced offset) read zeros from the range check
  typedef int cdv_i32x4 __attribute__((ext_vector_type(4)));
  cdv_half8 pat[1];
  if (a.gmap_pm) {
    const unsigned tile_b = 9u * (unsigned)C * 2u;
    const auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(a.gmap) + (size_t)(kq * tile_b), (short)0,
                                                      (int)tile_b, 0x00020000);   // tiles are below 4 GB (host check)
    const unsigned voff = (8 * g < C) ? (unsigned)(n * C + 8 * g) * 2u : 0x40000000u;
    pat[0] = __builtin_bit_cast(cdv_half8, (cdv_i32x4)__builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, 0, 0));
  } else {
    // the reference's planar tiles [Ng][C][3][3] (cdv_corr_fused on tensors nobody converted): eight strided gathers
    const _Float16* gp = reinterpret_cast<const _Float16*>(a.gmap) + (size_t)kq * C * 9 + (n < 9 ? n : 0);
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const int ch = 8 * g + j;
      const _Float16 v = gp[min(ch, C - 1) * 9];
      pat[0][j] = (n < 9 && ch < C) ? v : (_Float16)0.f;
    }
  }

  const LevelParams L0 = level_params(a.L0), L1 = level_params(NLEV == 2 ? a.L1 : a.L0);
  float xv, yv, xb, yb;
  int ixmin, ixmax, iymin, iymax;
  if (REC) {
    // the stream brought this lane's blend coordinates and the box extremes: nothing to exchange between lanes.  (The
    // per-pixel path below -- rare -- is the only user of (xv, yv) and picks pixel m's pair from lane 7 m.)
    xb = ec.xb; yb = ec.yb;
    xv = xb; yv = yb;      // patch pixel m sits in lane 7 m (slow_level<1, 7>)
    ixmin = ec.ixmin; ixmax = ec.ixmax; iymin = ec.iymin; iymax = ec.iymax;
  } else {
    const int cval = ec.cval;
    xv = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * mm, cval));
    yv = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (9 + mm), cval));
    xb = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * bm, cval));
    yb = __int_as_float(__builtin_amdgcn_ds_bpermute(4 * (9 + bm), cval));
    const int ixl = floor_clamped(xv * L0.inv_scale), iyl = floor_clamped(yv * L0.inv_scale);
    int vxmin, vxmax, vymin, vymax;
    row16_minmax4(ixl, iyl, vxmin, vxmax, vymin, vymax);
    ixmin = __builtin_amdgcn_readfirstlane(vxmin); ixmax = __builtin_amdgcn_readfirstlane(vxmax);
    iymin = __builtin_amdgcn_readfirstlane(vymin); iymax = __builtin_amdgcn_readfirstlane(vymax);
  }
  const Box b0 = make_box(ixmin, ixmax, iymin, iymax, L0);
  const int sh1 = NLEV == 2 ? L1.shift : 0;
  const Box b1 = make_box(ixmin >> sh1, ixmax >> sh1, iymin >> sh1, iymax >> sh1, L1);
  CDV_STAMP(corr, p, 1);

  _Float16 res0[7], res1[7];
  // lanes n >= 9 of the D tile are not patch pixels: they store into the dump area instead of being masked off
  // (no EXEC save/restore around every store)
  _Float16* raw_lane = (n < 9) ? raw + n * RAW_MSH + 4 * g
                               : reinterpret_cast<_Float16*>(reinterpret_cast<char*>(raw) + DUMP_OFF_B +
                                                             4 * ((n * (RAW_MSH / 2) + 2 * g) & 31));

  // ---- round trip 2: EVERY window group of a level is requested before its first MFMA; the level-1 request goes out
  // as soon as level 0 has left the registers and flies under the level-0 blend -------------------------------------
  const unsigned CB = (unsigned)C * 2u;                              // bytes per pixel
  const char* r0 = a.L0.base_m + (size_t)(jq * a.L0.slot_bytes + (unsigned)(b0.y0c + PADY) * a.L0.pitch +
                                          (unsigned)(b0.x0c + PADX) * CB);   // rings are below 4 GB (host check)
  const CorrLevel& A1 = NLEV == 2 ? a.L1 : a.L0;
  const char* r1 = A1.base_m + (size_t)(jq * A1.slot_bytes + (unsigned)(b1.y0c + PADY) * A1.pitch +
                                        (unsigned)(b1.x0c + PADX) * CB);
  const unsigned pitch0 = a.L0.pitch, pitch1 = A1.pitch;
  cdv_half8 w[NQ_MAX][1];
  const bool do0 = b0.fast && !b0.outside && idx_ok;
  const bool do1 = NLEV == 2 && b1.fast && !b1.outside && idx_ok;
  const int nq0 = (b0.Wb * b0.Hb + 15) >> 4, nq1 = (b1.Wb * b1.Hb + 15) >> 4;
  // Window addressing in float arithmetic (exact: every value is an integer below 2^24).  The union window is packed
  // DENSELY into the 16 pixel slots of the MFMA A operand: slot n of group q is window pixel P = 16 q + n, in window
  // row floor((P + 0.5) / Wb) -- (P + 0.5) / Wb stays 0.5 / 16 away from every integer, far beyond the rounding of the
  // reciprocal -- at byte offset row * (pitch - Wb CB) + P CB (+ channel group).  (t, b) = ((P + 0.5) / Wb,
  // P CB + group + 2^23) advance together with one v_pk_add_f32 per group; the 2^23 makes the low mantissa bits of
  // fma(row, wrap, b) the integer offset itself, so the float's BIT PATTERN is the buffer offset (no conversion): the
  // descriptor base is biased by -0x4B000000 (host) and its size by +0x4B000000.  The range check of the descriptor
  // returns zeros past the last window row; the k-padding lanes start from 2^25 (always out of range).
  typedef float cdv_f32x2 __attribute__((ext_vector_type(2)));
  const float nhalf = (float)n + 0.5f;
  const float lanebase = (8 * g < C) ? (float)((unsigned)n * CB + (unsigned)(8 * g) * 2u) + 8388608.0f : 33554432.0f;
  // Groups per level: a FIXED number is requested and multiplied without any test -- 8 at level 0 (windows up to 128
  // pixels: 10 x 10 ... 11 x 11, what a patch at roughly its own scale gives), 6 at level 1 (up to 96: 8 x 8 ... 9 x 10).
  // Groups past the window lie past its last row, where the descriptor's range check returns zeros without touching
  // memory, and their products land in raw-volume rows nobody reads.  With the count known at compile time the waits
  // between the loads and the matrix instructions are progressive (vmcnt(n) instead of vmcnt(0): the first MFMA starts
  // when the first group has arrived), and the 2 x 2 tested chains of the earlier version (a compare and a branch per
  // group, four times per edge) are gone.  Larger windows (strong zoom) finish in a rolled tail loop, one group at a
  // time through one register set.
  constexpr int NQF0 = 8, NQF1 = 6;
#define CDV2_LOAD_SETUP(BX, RB, PITCH)                                                             \
    const unsigned Wb_ = (unsigned)(BX).Wb, pitch_ = (PITCH);                                      \
    const auto rsrc_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(RB), (short)0,          \
                                                         (int)((unsigned)(BX).Hb * pitch_ + FBIAS), 0x00020000); \
    const float invW_ = __builtin_amdgcn_rcpf((float)Wb_);                                         \
    const float wrapf_ = (float)(pitch_ - Wb_ * CB);                                               \
    const cdv_f32x2 dtb_ = {16.0f * invW_, (float)(16u * CB)};
#define CDV2_LD1(q)                                                                                \
    {                                                                                              \
      const float vf_ = __builtin_fmaf(__builtin_floorf(tb_[0]), wrapf_, tb_[1]);                  \
      const cdv_i32x4 v_ = __builtin_amdgcn_raw_buffer_load_b128(rsrc_, __float_as_int(vf_), 0, 0); \
      w[q][0] = __builtin_bit_cast(cdv_half8, v_);                                                 \
      tb_ += dtb_;                                                                                 \
    }
  // NQF - 1 groups unconditionally, the NQF-th if the window has it (level 0: 7 groups for 93 % of the edges of the
  // synthetic stream, 8 for 4 %; level 1: 4 or 5 for 72 %, 6 for 28 %)
#define CDV2_LOAD_FIXED(BX, RB, PITCH, NQF, NQ)                                                    \
  {                                                                                                \
    CDV2_LOAD_SETUP(BX, RB, PITCH)                                                                 \
    cdv_f32x2 tb_ = {nhalf * invW_, lanebase};                                                     \
    CDV2_LD1(0) CDV2_LD1(1) CDV2_LD1(2) CDV2_LD1(3) CDV2_LD1(4)                                    \
    if (NQF > 6) { CDV2_LD1(5) CDV2_LD1(6) }                                                       \
    if ((NQ) >= (NQF)) { CDV2_LD1(NQF - 1) }                                                       \
  }
#define CDV2_MF1(WQ, q)                                                                            \
    {                                                                                              \
      cdv_float4 acc = {0.f, 0.f, 0.f, 0.f};                                                       \
      acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(WQ, pat[0], acc, 0, 0, 0);                      \
      cdv_half4 h = {(_Float16)acc[0], (_Float16)acc[1], (_Float16)acc[2], (_Float16)acc[3]};      \
      *reinterpret_cast<cdv_half4*>(raw_lane + (q) * 16) = h;                                      \
    }
  // (scheduling barriers between pairs of groups: left alone, the scheduler runs all matrix instructions first and keeps
  // eight accumulators alive)
#define CDV2_MF2(qa, qb) CDV2_MF1(w[qa][0], qa) CDV2_MF1(w[qb][0], qb) __builtin_amdgcn_sched_barrier(0);
#define CDV2_MFMA_FIXED(NQF, NQ)                                                                   \
  {                                                                                                \
    CDV2_MF2(0, 1) CDV2_MF2(2, 3)                                                                  \
    if (NQF > 6) { CDV2_MF2(4, 5) CDV2_MF1(w[6][0], 6) } else { CDV2_MF1(w[4][0], 4) }             \
    if ((NQ) >= (NQF)) { CDV2_MF1(w[NQF - 1][0], NQF - 1) }                                        \
  }
  // groups NQF .. NQ - 1 of a large window, rolled (rare)
#define CDV2_TAIL(BX, RB, PITCH, NQF, NQ)                                                          \
  if ((NQ) > (NQF)) {                                                                              \
    CDV2_LOAD_SETUP(BX, RB, PITCH)                                                                 \
    cdv_f32x2 tb_ = {(nhalf + (float)(16 * (NQF))) * invW_, lanebase + (float)(16u * (unsigned)(NQF) * CB)}; \
    _Pragma("unroll 1") for (int q_ = (NQF); q_ < (NQ); q_++) {                                    \
      const float vf_ = __builtin_fmaf(__builtin_floorf(tb_[0]), wrapf_, tb_[1]);                  \
      const cdv_i32x4 v_ = __builtin_amdgcn_raw_buffer_load_b128(rsrc_, __float_as_int(vf_), 0, 0); \
      tb_ += dtb_;                                                                                 \
      CDV2_MF1(__builtin_bit_cast(cdv_half8, v_), q_)                                              \
    }                                                                                              \
  }
  if (do0 && !CDV_EXP(1)) CDV2_LOAD_FIXED(b0, r0, pitch0, NQF0, nq0)
  const BlendGeo g0 = blend_geo(xb, yb, bm, bxo, L0, b0, !b0.fast);
  const BlendGeo g1 = blend_geo(xb, yb, bm, bxo, L1, b1, !b1.fast);
  CDV_STAMP(corr, p, 2);
  if (do0 && !CDV_EXP(256)) {
    CDV2_MFMA_FIXED(NQF0, nq0)
    CDV2_TAIL(b0, r0, pitch0, NQF0, nq0)
  } else if (!b0.fast && idx_ok) {
    slow_level<1, REC ? 7 : 1>(L0, jslot, xv, yv, pat, raw, lane, C);
  } else {
    zero_raw(raw, lane);
  }
  __builtin_amdgcn_sched_barrier(0);   // the level-1 request reuses the window registers: not before level 0 has left them
  if (do1 && !CDV_EXP(1)) CDV2_LOAD_FIXED(b1, r1, pitch1, NQF1, nq1)
  wave_lds_sync();
  CDV_STAMP(corr, p, 3);
  if (!CDV_EXP(128)) blend_level(raw, g0, res0);
  CDV_STAMP(corr, p, 4);
  if (NLEV == 2) {
    wave_lds_sync();
    if (do1 && !CDV_EXP(256)) {
      CDV2_MFMA_FIXED(NQF1, nq1)
      CDV2_TAIL(b1, r1, pitch1, NQF1, nq1)
    } else if (!b1.fast && idx_ok) {
      slow_level<1, REC ? 7 : 1>(L1, jslot, xv, yv, pat, raw, lane, C);
    } else {
      zero_raw(raw, lane);
    }
    wave_lds_sync();
    CDV_STAMP(corr, p, 5);
    if (!CDV_EXP(128)) blend_level(raw, g1, res1);
    CDV_STAMP(corr, p, 6);
  }
#undef CDV2_LOAD_FIXED
#undef CDV2_LOAD_SETUP
#undef CDV2_LD1
#undef CDV2_MF1
#undef CDV2_MF2
#undef CDV2_MFMA_FIXED
#undef CDV2_TAIL

  // ---- stage the edge's output row [x][y][m][lev] in LDS, then 16-byte-per-lane stores ------------------------------
  wave_lds_sync();   // the row overwrites the raw volume: keep the stores behind the last blend's reads
  if (lane < 63 && !CDV_EXP(512)) {
    if (NLEV == 2) {
      uint32_t* o32 = reinterpret_cast<uint32_t*>(outT) + __mul24(bxo, 63) + bm;   // dword (x, y, m) = 63 x + 9 y + m (24-bit multiply: full rate)
#pragma unroll
      for (int yo = 0; yo < 7; yo++) {
        const cdv_half2 h = {res0[yo], res1[yo]};
        o32[yo * 9] = __builtin_bit_cast(uint32_t, h);
      }
    } else {
#pragma unroll
      for (int yo = 0; yo < 7; yo++) outT[(bxo * 7 + yo) * 9 + bm] = res0[yo];
    }
  }
  wave_lds_sync();
  CDV_STAMP(corr, p, 7);
  if (!CDV_EXP(2)) {
    if (NLEV == 2) {
      // 441 dwords: two 16-byte-per-lane stores (256 + 184 dwords) and one last dword.  The row starts on a 4-byte
      // boundary only (1764 B per edge); global memory takes the unaligned 16-byte accesses.
      const uint32_t* src = reinterpret_cast<const uint32_t*>(outT);
      uint32_t* dst = reinterpret_cast<uint32_t*>(a.out) + (size_t)e * 441;
      typedef uint32_t cdv_u32x4 __attribute__((ext_vector_type(4)));
      const cdv_u32x4 v0 = *reinterpret_cast<const cdv_u32x4*>(src + 4 * lane);
      // the output row leaves written through (sc1: the line is dropped from this XCD's L2 instead of staying there -- 84 MB of
      // output per launch that nobody of this launch reads again pushed the feature maps out of the 4 MB L2s; round 5, measured
      // back to back on the default / stress workloads: 38.4-38.9 -> 37.6 us, 70.5-71.2 -> 69.2-69.4 us; nt (2): the same)
      typedef int cdv_i32x4s __attribute__((ext_vector_type(4)));
      const auto rso = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<char*>(dst), (short)0, 1768, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b128((cdv_i32x4s)v0, rso, 16 * lane, 0, OUT_POLICY);
      if (lane < 46) {
        const cdv_u32x4 v1 = *reinterpret_cast<const cdv_u32x4*>(src + 256 + 4 * lane);
        __builtin_amdgcn_raw_buffer_store_b128((cdv_i32x4s)v1, rso, 1024 + 16 * lane, 0, OUT_POLICY);
      }
      if (lane == 63) __builtin_amdgcn_raw_buffer_store_b32((int)src[440], rso, 1760, 0, OUT_POLICY);
    } else {
      _Float16* dst = a.out + (size_t)e * a.out_pitch + a.out_off;
#pragma unroll
      for (int i = 0; i < 7; i++) {
        const int t = i * 64 + lane;
        if (t < 441) dst[t * a.out_stride] = outT[t];
      }
    }
  }
  CDV_STAMP(corr, p, 8);
}

// index % modulus (slam.py:319-320) with the host's reciprocal: q = mulhi(x, ceil(2^32 / d)) is x / d or one more
// for 0 <= x < 2^31, so one correction step.  Returns false for an index outside its ring (or not a 31-bit value).
__device__ __forceinline__ bool ring_index(int64_t v64, uint32_t mod, uint32_t magic, uint32_t limit, uint32_t& q) {
  q = (uint32_t)v64;
  const bool small = (uint32_t)(v64 >> 32) == 0u && q < 0x80000000u;
  if (mod > 1u) {
    const int32_t r = (int32_t)(q - __umulhi(q, magic) * mod);
    q = (uint32_t)(r < 0 ? r + (int32_t)mod : r);
  } else if (mod == 1u) {
    q = 0u;
  }
  return small && q < limit;
}

// The four leading arguments are what a wave needs to find its edge and request its record: one scalar load, and no second
// one for the grid size (gridDim.x lives in the hidden arguments; `eighth` = gridDim.x / 8 comes from the host).  (Round 5:
// with -amdgpu-kernarg-preload-count=4 these arguments arrive in scalar registers at wave launch and the record request
// goes out with no kernel-argument load in front of it at all -- measured next to this build and to the one before it
// (two dependent scalar round trips): 36.3-37.6 us back to back for all three, no difference.  The kernel is not bound by
// the length of one wave's chain of round trips; the preload flag is not used.)
template <int CC, int NLEV, bool REC = false>
__global__ __launch_bounds__(64 * CW) void corr_fused2_kernel(const uint32_t* __restrict__ rec_h, const int32_t* __restrict__ dynE_h,
                                                          int E_h, int eighth_h, const CorrArgs2 a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  _Float16* raw = reinterpret_cast<_Float16*>(smem_raw + (size_t)wave * WAVE_LDS2_BYTES);
  _Float16* outT = raw;   // the staged output row takes the place of the raw volume once both blends are done
  // workgroup b runs on XCD b % 8 and takes CW consecutive edges of the b % 8-th contiguous eighth of the list.  (Round 5,
  // 2 / 3 edges per wave with the next record requested behind the current edge's window loads: 77 registers instead of 62
  // (70 without machine LICM), six (seven) waves per SIMD instead of eight: 40.5 (39.3) against 37.7 us back to back -- the
  // hidden round trip buys what the lost waves cost, no more; forced to 64 registers it spills 43 values: 79 us.  Workgroups
  // of 8 / 16 waves instead of 4: 1 % / 5 % slower.  DESIGN.md section 3.)
  int E = E_h, eighth = eighth_h;
  if (REC && dynE_h) {    // sizes on the device: the contiguous eighths are those of the ACTUAL list, not of the launch
    E = min(__builtin_amdgcn_readfirstlane(*dynE_h), E_h);
    eighth = (E + 8 * CW - 1) / (8 * CW);
    if (((int)blockIdx.x >> 3) >= eighth) return;
  }
  const int p0 = (((int)blockIdx.x & 7) * eighth + ((int)blockIdx.x >> 3)) * CW + wave;
  if (p0 >= E) return;  // no block-wide barriers below: waves are independent
  if (REC) {
    // ---- ONE round trip: record p0 of the packed input stream the index build wrote in processing order -- the 18
    // coordinates as one vector load, edge id and ring indices as scalar loads of the same line (no order[] -> coords /
    // kk / jj indirection: one dependent memory round trip less per wave, no index arithmetic)
    const uint32_t* r = rec_h + (size_t)p0 * cdv::CORR_REC_WORDS;
    const int bm = min(lane / 7, 8);
    EdgeCoords ec;
    ec.cval = 0;
    ec.xb = __int_as_float((int)r[bm]);          // two gathers from the record's one or two cache lines: each lane gets
    ec.yb = __int_as_float((int)r[9 + bm]);      // the coordinates of ITS patch pixel, no cross-lane exchange
    const int e = (int)r[18];
    const uint32_t kq = r[19], jq = r[20];
    const int bx = (int)r[21], by = (int)r[22];   // extremes of floor(x), floor(y): (max << 16) | (min & 0xffff)
    ec.ixmin = (int)(short)(bx & 0xffff); ec.ixmax = bx >> 16;
    ec.iymin = (int)(short)(by & 0xffff); ec.iymax = by >> 16;
    corr_edge<CC, NLEV, true>(a, p0, e, ec, kq, jq, jq != 0xFFFFFFFFu, lane, raw, outT);
    return;
  }
  // ---- round trip 1: the 18 coordinates (one vector load) and the two indices (scalar loads) -----------------------
  const int e = a.order ? __builtin_amdgcn_readfirstlane(a.order[p0]) : p0;   // wave-uniform
  const int cval = __float_as_int(a.coords[(size_t)e * 18 + min(lane, 17)]);
  if (NLEV == 1 && a.coords_ref) {   // this edge's level is in place if it was computed from these very coordinates
    const float r = a.coords_ref[(size_t)e * 18 + min(lane, 17)] * a.ref_mul;
    if (__all(lane >= 18 || __float_as_int(r) == cval)) return;
  }
  uint32_t kq, jq;
  const bool k_ok = ring_index(a.kk[e], a.kmod, a.kmagic, a.Ng, kq);
  const bool j_ok = ring_index(a.jj[e], a.jmod, a.jmagic, a.slots, jq);
  EdgeCoords ec;
  ec.cval = cval;
  corr_edge<CC, NLEV, false>(a, p0, e, ec, kq, jq, k_ok && j_ok, lane, raw, outT);
}

// Host-side arguments of one fused launch.  What an entry point does not set keeps the value of the plain two-level call
// over coords / kk / jj: a dense [E][882] result, no reference coordinates, no record stream, edge count on the host.
struct FusedCall {
  const void *gmap = nullptr, *fmap0_nhwc = nullptr, *fmap1_nhwc = nullptr;
  const float *coords = nullptr, *coords_ref = nullptr;
  const int64_t *kk = nullptr, *jj = nullptr;
  const int32_t *order = nullptr, *dynE = nullptr;
  const uint32_t* rec = nullptr;
  void *out = nullptr, *stream = nullptr;
  int64_t E = 0, Ng = 0, slots = 0, kmod = 0, jmod = 0;
  int C = 0, H0 = 0, W0 = 0, H1 = 0, W1 = 0, nlev = 2, gmap_pixel_major = 0;
  float scale0 = 0.f, scale1 = 0.f, ref_mul = 1.0f;
  int out_stride = 1, out_off = 0, out_pitch = 441;   // CorrArgs2: where element t of edge e goes
};

template <int CC, int NLEV, bool REC>
void launch_fused(int blocks, size_t smem2, hipStream_t s, const CorrArgs2& a) {
  hipLaunchKernelGGL((corr_fused2_kernel<CC, NLEV, REC>), dim3(blocks), dim3(64 * CW), smem2, s, a.rec, a.dynE, a.E, blocks >> 3, a);
}

int corr_fused_impl(const FusedCall& c) {
  const int C = c.C, nlev = c.nlev;
  CDV_REQUIRE(nlev == 1 || nlev == 2, CDV_ERR_ARG, "cdv_corr_fused: nlev must be 1 or 2");
  CDV_REQUIRE(C % 8 == 0 && C > 0 && C <= 128, CDV_ERR_UNSUPPORTED, "cdv_corr_fused: C must be a multiple of 8, <= 128");
  CDV_REQUIRE(c.E >= 0 && c.E < ((int64_t)1 << 31), CDV_ERR_ARG, "cdv_corr_fused: E out of range");
  int ex0 = 0, ex1 = 0;
  CDV_REQUIRE(c.scale0 > 0.f && frexpf(c.scale0, &ex0) == 0.5f && (nlev == 1 || (c.scale1 > 0.f && frexpf(c.scale1, &ex1) == 0.5f)),
              CDV_ERR_UNSUPPORTED, "cdv_corr_fused: pyramid scales must be powers of two (1 and 4 in SLAM.corr)");
  CDV_REQUIRE(c.fmap0_nhwc != nullptr && (nlev == 1 || c.fmap1_nhwc != nullptr), CDV_ERR_ARG, "cdv_corr_fused: NULL map");
  CDV_REQUIRE_ALIGNED(c.fmap0_nhwc, 16, "cdv_corr_fused: fmap0_nhwc must be 16-byte aligned");
  CDV_REQUIRE_ALIGNED(nlev == 2 ? c.fmap1_nhwc : nullptr, 16, "cdv_corr_fused: fmap1_nhwc must be 16-byte aligned");
  CDV_REQUIRE_ALIGNED(c.gmap_pixel_major ? c.gmap : nullptr, 16, "cdv_corr_fused: pixel-major gmap must be 16-byte aligned");
  CDV_REQUIRE_ALIGNED(c.out, 4, "cdv_corr_fused: out must be 4-byte aligned");
  CDV_REQUIRE(cdv_fmap_padded_elems(c.slots, C, c.H0, c.W0) * 2 < ((size_t)1 << 32) &&
                  (nlev == 1 || cdv_fmap_padded_elems(c.slots, C, c.H1, c.W1) * 2 < ((size_t)1 << 32)),
              CDV_ERR_UNSUPPORTED, "cdv_corr_fused: a feature ring of 4 GB or more");
  CDV_REQUIRE(c.kmod >= 0 && c.jmod >= 0 && c.kmod < ((int64_t)1 << 31) && c.jmod < ((int64_t)1 << 31), CDV_ERR_ARG,
              "cdv_corr_fused: kmod / jmod out of range");
  const uint32_t kmagic = cdv_magic_u32(c.kmod), jmagic = cdv_magic_u32(c.jmod);
  if (c.E == 0) return CDV_OK;
  CDV_REQUIRE(nlev == 1 || ex1 >= ex0, CDV_ERR_UNSUPPORTED, "cdv_corr_fused: level 1 must not be finer than level 0");
  static const int exp = getenv("CDV_CORR_EXP") ? atoi(getenv("CDV_CORR_EXP")) : 0;  // diagnostics only
  hipStream_t s = (hipStream_t)c.stream;
  if (C <= 32) {
    CDV_REQUIRE(c.Ng < ((int64_t)1 << 31) && c.slots < ((int64_t)1 << 31) && (size_t)c.Ng * 9 * (size_t)C * 2 < ((size_t)1 << 32),
                CDV_ERR_UNSUPPORTED, "cdv_corr_fused: 4 GB or more of patch tiles");
    auto level = [&](const void* ring, int H, int W, float scale, int shift) {
      const uint32_t pitch = (uint32_t)(W + 2 * PADX) * (uint32_t)C * 2u;
      return CorrLevel{(const char*)ring - (size_t)FBIAS, H, W, 1.0f / scale, shift, pitch, pitch * (uint32_t)(H + 2 * PADY)};
    };
    const CorrLevel A0 = level(c.fmap0_nhwc, c.H0, c.W0, c.scale0, 0);
    const CorrArgs2 a{c.coords, c.kk, c.jj, c.order, (int)c.E, (uint32_t)c.kmod, (uint32_t)c.jmod, kmagic, jmagic, (uint32_t)c.Ng,
                      (uint32_t)c.slots, (const char*)c.gmap, (_Float16*)c.out, A0,
                      nlev == 2 ? level(c.fmap1_nhwc, c.H1, c.W1, c.scale1, ex1 - ex0) : A0, C, c.gmap_pixel_major, exp,
                      c.out_stride, c.out_off, c.out_pitch, c.coords_ref, c.ref_mul, c.rec, c.dynE};
    const int blocks = 8 * (int)cdv_div_up(c.E, 8 * CW);   // a multiple of 8: the kernel deals contiguous eighths to the XCDs
    const size_t smem2 = (size_t)CW * WAVE_LDS2_BYTES;
    if (c.rec) {   // packed input stream in processing order (cdv_corr_fused_stream)
      CDV_REQUIRE(nlev == 2 && c.coords_ref == nullptr, CDV_ERR_UNSUPPORTED, "cdv_corr_fused_stream: two fused levels only");
      C == 24 ? launch_fused<24, 2, true>(blocks, smem2, s, a) : launch_fused<0, 2, true>(blocks, smem2, s, a);
    } else if (nlev == 2) {
      C == 24 ? launch_fused<24, 2, false>(blocks, smem2, s, a) : launch_fused<0, 2, false>(blocks, smem2, s, a);
    } else {   // one level per call: what an unchanged slam.py issues (slam.py:316-323), twice per update
      C == 24 ? launch_fused<24, 1, false>(blocks, smem2, s, a) : launch_fused<0, 1, false>(blocks, smem2, s, a);
    }
  } else {
    CDV_REQUIRE(c.out_stride == 1 && c.out_off == 0 && c.coords_ref == nullptr, CDV_ERR_UNSUPPORTED,
                "cdv_corr_fused: checked calls need C <= 32");
    LevelParams L0{(const _Float16*)c.fmap0_nhwc, c.H0, c.W0, 1.0f / c.scale0, 0};
    LevelParams L1{(const _Float16*)c.fmap1_nhwc, c.H1, c.W1, nlev == 2 ? 1.0f / c.scale1 : 1.0f, nlev == 2 ? ex1 - ex0 : 0};
    hipLaunchKernelGGL(corr_wide_kernel<4>, dim3(cdv_div_up(c.E, 4)), dim3(256), 4 * (size_t)WAVE_LDS_BYTES, s, (const _Float16*)c.gmap,
                       L0, L1, c.coords, c.kk, c.jj, c.order, (_Float16*)c.out, (int)c.E, c.Ng, c.slots, C, nlev, c.kmod, c.jmod,
                       kmagic, jmagic, c.gmap_pixel_major, exp);
  }
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

}  // namespace

extern "C" int cdv_corr_fused(const void* gmap, const void* fmap0_nhwc, const void* fmap1_nhwc, const float* coords,
                              const int64_t* kk, const int64_t* jj, const int32_t* order, void* out, int64_t E,
                              int64_t Ng, int64_t slots, int C, int H0, int W0, int H1, int W1, float scale0,
                              float scale1, int nlev, int64_t kmod, int64_t jmod, int gmap_pixel_major, void* stream) {
  FusedCall c;
  c.gmap = gmap; c.fmap0_nhwc = fmap0_nhwc; c.fmap1_nhwc = fmap1_nhwc; c.out = out; c.E = E; c.Ng = Ng; c.slots = slots;
  c.C = C; c.H0 = H0; c.W0 = W0; c.H1 = H1; c.W1 = W1; c.scale0 = scale0; c.scale1 = scale1;
  c.gmap_pixel_major = gmap_pixel_major; c.stream = stream;
  c.coords = coords; c.kk = kk; c.jj = jj; c.order = order; c.nlev = nlev; c.kmod = kmod; c.jmod = jmod;
  return corr_fused_impl(c);
}

extern "C" int cdv_corr_fused_stream(const void* gmap, const void* fmap0_nhwc, const void* fmap1_nhwc, const void* records,
                                     void* out, int64_t E, int64_t Ng, int64_t slots, int C, int H0, int W0, int H1, int W1,
                                     float scale0, float scale1, int gmap_pixel_major, void* stream) {
  CDV_REQUIRE(records != nullptr, CDV_ERR_ARG, "cdv_corr_fused_stream: NULL record stream");
  CDV_REQUIRE(C <= 32, CDV_ERR_UNSUPPORTED, "cdv_corr_fused_stream: C must be <= 32");
  FusedCall c;
  c.gmap = gmap; c.fmap0_nhwc = fmap0_nhwc; c.fmap1_nhwc = fmap1_nhwc; c.out = out; c.E = E; c.Ng = Ng; c.slots = slots;
  c.C = C; c.H0 = H0; c.W0 = W0; c.H1 = H1; c.W1 = W1; c.scale0 = scale0; c.scale1 = scale1;
  c.gmap_pixel_major = gmap_pixel_major; c.stream = stream;
  c.rec = (const uint32_t*)records;
  return corr_fused_impl(c);
}

// cdv_corr_fused_stream with the number of edges on the device: *dyn_E edges (at most E_bound, which sizes the launch)
extern "C" int cdv_corr_fused_stream_dyn(const void* gmap, const void* fmap0_nhwc, const void* fmap1_nhwc, const void* records,
                                         void* out, int64_t E_bound, const int32_t* dyn, int64_t Ng, int64_t slots, int C, int H0,
                                         int W0, int H1, int W1, float scale0, float scale1, int gmap_pixel_major, void* stream) {
  CDV_REQUIRE(records != nullptr && dyn != nullptr, CDV_ERR_ARG, "cdv_corr_fused_stream_dyn: NULL record stream / dynamic block");
  CDV_REQUIRE(C <= 32, CDV_ERR_UNSUPPORTED, "cdv_corr_fused_stream_dyn: C must be <= 32");
  FusedCall c;
  c.gmap = gmap; c.fmap0_nhwc = fmap0_nhwc; c.fmap1_nhwc = fmap1_nhwc; c.out = out; c.E = E_bound; c.Ng = Ng; c.slots = slots;
  c.C = C; c.H0 = H0; c.W0 = W0; c.H1 = H1; c.W1 = W1; c.scale0 = scale0; c.scale1 = scale1;
  c.gmap_pixel_major = gmap_pixel_major; c.stream = stream;
  c.rec = (const uint32_t*)records; c.dynE = dyn + CDV_DYN_E;
  return corr_fused_impl(c);
}

// ONE level of the INTERLEAVED two-level result of cdv_corr_fused ([E][441][2] halves: what SLAM.corr's torch.stack(..., -1)
// produces), level `level` of element t of edge e at out[e * 882 + 2 t + level]; an edge whose coordinates equal
// coords_ref * ref_mul bit for bit is skipped (its values are in place already)
extern "C" int cdv_corr_level_checked_interleaved(const void* gmap, const void* fmap_nhwc, const float* coords,
                                                  const float* coords_ref, float ref_mul, const int64_t* kk, const int64_t* jj,
                                                  void* out, int level, int64_t E, int64_t Ng, int64_t slots, int C, int H, int W,
                                                  float scale, int64_t kmod, int64_t jmod, int gmap_pixel_major, void* stream) {
  CDV_REQUIRE(level == 0 || level == 1, CDV_ERR_ARG, "cdv_corr_level_checked_interleaved: level must be 0 or 1");
  CDV_REQUIRE(coords_ref != nullptr && out != nullptr, CDV_ERR_ARG, "cdv_corr_level_checked_interleaved: NULL argument");
  CDV_REQUIRE(C <= 32, CDV_ERR_UNSUPPORTED, "cdv_corr_level_checked_interleaved: C must be <= 32");
  FusedCall c;
  c.gmap = gmap; c.fmap0_nhwc = fmap_nhwc; c.out = out; c.E = E; c.Ng = Ng; c.slots = slots;
  c.C = C; c.H0 = H; c.W0 = W; c.scale0 = scale; c.scale1 = 1.0f;
  c.gmap_pixel_major = gmap_pixel_major; c.stream = stream;
  c.coords = coords; c.kk = kk; c.jj = jj; c.nlev = 1; c.kmod = kmod; c.jmod = jmod;
  c.out_stride = 2; c.out_off = level; c.out_pitch = 882; c.coords_ref = coords_ref; c.ref_mul = ref_mul;
  return corr_fused_impl(c);
}
