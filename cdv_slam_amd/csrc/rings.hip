// rings.hip -- upkeep of the two layouts the fused correlation (corr.hip) gathers from: the padded channels-last feature
// rings [slot][H + 2 PADY][W + 2 PADX][C] (zero margins; why: the layout comment in corr.hip) and the pixel-major patch
// tiles [Ng][9][C].
//
// Reference: slam.py:680-682 writes a new frame's tiles and maps into the PLANAR rings gmap_ / fmap1_ / fmap2_ (level 1:
// F.avg_pool2d(fmap, 4, 4)) and correlation_kernel.cu:82-136 reads those with strided 2-byte loads.  Here:
//   * cdv_frame_ingest / cdv_fmap_ingest: one launch writes the frame into both channels-last rings (4x4 pool included),
//     optionally the planar rings too, and converts the frame's tiles (body: cdv_parts.h, shared with the update prologue);
//   * cdv_fmap_to_nhwc / cdv_gmap_to_pixel_major: whole-range conversions of planar tensors somebody else owns;
//   * cdv_fmap_sync_nhwc / cdv_shadows_sync: a planar ring an unchanged slam.py writes with torch ops is kept in step with
//     its channels-last shadow by fingerprinting every slot and converting only the ones that changed (normally one).
#include "cdv_parts.h"

namespace {

// ---- layout kernels -----------------------------------------------------------------------------------
// planar [N][C][H][W] -> padded channels-last [N][H+2PADY][W+2PADX][C] (interior only; the margins are
// zeroed once at allocation); one thread per (pixel, 8-channel group): 8 strided 2-byte reads (coalesced
// across the wave along W), one 16-byte write.
__global__ __launch_bounds__(256) void nchw_to_nhwc_kernel(const _Float16* __restrict__ src,
                                                           _Float16* __restrict__ dst, int64_t first, int64_t count,
                                                           int C, int H, int W) {
  const int G = C / 8;
  const int64_t total = count * H * W * G;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    // x fastest so that the planar reads of a wave are contiguous
    int64_t t = idx;
    const int xw = (int)(t % W); t /= W;
    const int gq = (int)(t % G); t /= G;
    const int yh = (int)(t % H); t /= H;
    const int64_t nslot = first + t;
    cdv_half8 v;
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = src[((nslot * C + 8 * gq + j) * H + yh) * W + xw];
    *reinterpret_cast<cdv_half8*>(dst + ((nslot * (H + 2 * cdv::PART_PADY) + yh + cdv::PART_PADY) * (W + 2 * cdv::PART_PADX) +
                                         xw + cdv::PART_PADX) * C + 8 * gq) = v;
  }
}

// ---- a planar ring whose writer is somebody else (the reference's slam.py writes fmap1_[:, n % mem] with torch ops) kept
// in step with its channels-last shadow WITHOUT converting all of it every frame: pass 1 fingerprints every slot of the
// planar ring (a read of the ring: 21 MB at level 0), pass 2 converts only the slots whose fingerprint differs from
// the one taken at the previous sync (normally ONE).  Fingerprint = FP_PARTS position-keyed 64-bit sums per slot.
constexpr int FP_PARTS = 16;      // workgroups (and partial sums) per slot

__device__ __forceinline__ void fingerprint_body(const uint32_t* __restrict__ src, int64_t words_per_slot,
                                                 uint64_t* __restrict__ fp, int bid) {
  const int slot = bid / FP_PARTS, part = bid % FP_PARTS;
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const u32x4* p = reinterpret_cast<const u32x4*>(src + (size_t)slot * words_per_slot);
  const int64_t n4 = words_per_slot / 4;        // slots are multiples of 16 bytes (C % 8 == 0)
  uint64_t acc = 0;
  for (int64_t i = (int64_t)part * 256 + threadIdx.x; i < n4; i += (int64_t)FP_PARTS * 256) {
    const u32x4 v = p[i];
    const uint64_t key = 0x9E3779B97F4A7C15ull + 2ull * (uint64_t)i;           // odd, different for every position
    acc += ((uint64_t)v[0] | ((uint64_t)v[1] << 32)) * key;
    acc += ((uint64_t)v[2] | ((uint64_t)v[3] << 32)) * (key ^ 0xD6E8FEB86659FD92ull);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  __shared__ uint64_t sw[4];
  if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) fp[(size_t)slot * FP_PARTS + part] = (sw[0] + sw[1]) + (sw[2] + sw[3]) + 1ull;   // never 0 = "no fingerprint yet"
}

__global__ __launch_bounds__(256) void fmap_fingerprint_kernel(const uint32_t* __restrict__ src, int64_t words_per_slot,
                                                               uint64_t* __restrict__ fp) {
  fingerprint_body(src, words_per_slot, fp, (int)blockIdx.x);
}

__device__ __forceinline__ void dirty_body(const _Float16* __restrict__ src, _Float16* __restrict__ dst, int C, int H, int W,
                                           const uint64_t* __restrict__ fp_new, const uint64_t* __restrict__ fp_old,
                                           int wg_per_slot, int32_t* __restrict__ n_dirty, int bid) {
  const int64_t nslot = bid / wg_per_slot;
  const int wg = bid % wg_per_slot;
  bool same = true;
#pragma unroll
  for (int i = 0; i < FP_PARTS; i++) same = same && fp_new[nslot * FP_PARTS + i] == fp_old[nslot * FP_PARTS + i];
  if (same) return;                                  // workgroup-uniform
  if (wg == 0 && threadIdx.x == 0 && n_dirty) atomicAdd(n_dirty, 1);
  const int G = C / 8;
  const int64_t total = (int64_t)H * W * G;
  for (int64_t idx = (int64_t)wg * 256 + threadIdx.x; idx < total; idx += (int64_t)wg_per_slot * 256) {
    int64_t t = idx;
    const int xw = (int)(t % W); t /= W;
    const int gq = (int)(t % G); t /= G;
    const int yh = (int)t;
    cdv_half8 v;
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = src[((nslot * C + 8 * gq + j) * H + yh) * W + xw];
    *reinterpret_cast<cdv_half8*>(dst + ((nslot * (H + 2 * cdv::PART_PADY) + yh + cdv::PART_PADY) * (W + 2 * cdv::PART_PADX) +
                                         xw + cdv::PART_PADX) * C + 8 * gq) = v;
  }
}

__global__ __launch_bounds__(256) void nchw_to_nhwc_dirty_kernel(const _Float16* __restrict__ src,
                                                                 _Float16* __restrict__ dst, int C, int H, int W,
                                                                 const uint64_t* __restrict__ fp_new,
                                                                 const uint64_t* __restrict__ fp_old, int wg_per_slot,
                                                                 int32_t* __restrict__ n_dirty) {
  dirty_body(src, dst, C, H, W, fp_new, fp_old, wg_per_slot, n_dirty, (int)blockIdx.x);
}

// ---- the same two passes for SEVERAL rings at once, the tiles' conversion riding the second (cdv_shadows_sync): what an
// unchanged slam.py needs in front of its correlation -- both pyramid levels' shadows and the tile shadow in step -- is five
// launches through the single-ring entry points and two here.  Same bodies, same bytes.
struct ShadowJob {
  const _Float16* src; _Float16* dst;
  uint64_t *fp_new; const uint64_t* fp_old;
  int32_t* n_dirty;
  int64_t words_per_slot;
  int C, H, W, wg_per_slot, fp_blocks, cv_blocks;
};
struct ShadowJobs {
  ShadowJob j[2];
  int n;
  const _Float16* g_src; _Float16* g_dst;     // tiles (NULL: none)
  int64_t g_count;
  int g_C, g_blocks;
};

__global__ __launch_bounds__(256) void shadows_fingerprint_kernel(const ShadowJobs J) {
  int b = (int)blockIdx.x;
  for (int q = 0; q < J.n; q++) {               // workgroup-uniform
    if (b < J.j[q].fp_blocks) {
      fingerprint_body(reinterpret_cast<const uint32_t*>(J.j[q].src), J.j[q].words_per_slot, J.j[q].fp_new, b);
      return;
    }
    b -= J.j[q].fp_blocks;
  }
}

__global__ __launch_bounds__(256) void shadows_convert_kernel(const ShadowJobs J) {
  int b = (int)blockIdx.x;
  for (int q = 0; q < J.n; q++) {
    const ShadowJob& s = J.j[q];
    if (b < s.cv_blocks) {
      dirty_body(s.src, s.dst, s.C, s.H, s.W, s.fp_new, s.fp_old, s.wg_per_slot, s.n_dirty, b);
      return;
    }
    b -= s.cv_blocks;
  }
  if (J.g_src) cdv::gmap_pm_convert(J.g_src, J.g_dst, 0, J.g_count, J.g_C, (int64_t)b * 256 + threadIdx.x, (int64_t)J.g_blocks * 256);
}

__global__ __launch_bounds__(256) void gmap_pm_kernel(const _Float16* __restrict__ src, _Float16* __restrict__ dst,
                                                      int64_t first, int64_t count, int C) {
  cdv::gmap_pm_convert(src, dst, first, count, C, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                       (int64_t)gridDim.x * blockDim.x);
}

// feature-map ring write + 4x4 pool (+ the frame's patch tiles): body in cdv_parts.h
__global__ __launch_bounds__(256) void fmap_ingest_kernel(cdv::IngestArgs a) {
  cdv::ingest_body(a, (int)blockIdx.x, (int)blockDim.x, (int)threadIdx.x);
}

}  // namespace

extern "C" size_t cdv_fmap_padded_elems(int64_t slots, int C, int H, int W) {
  return (size_t)slots * (size_t)(H + 2 * cdv::PART_PADY) * (size_t)(W + 2 * cdv::PART_PADX) * (size_t)C;
}

extern "C" int cdv_fmap_to_nhwc(const void* src_nchw, void* dst_nhwc, int64_t N, int C, int H, int W, int64_t first,
                                int64_t count, void* stream) {
  CDV_REQUIRE(C % 8 == 0 && C > 0, CDV_ERR_ARG, "cdv_fmap_to_nhwc: C must be a multiple of 8");
  CDV_REQUIRE(first >= 0 && count >= 0 && first + count <= N, CDV_ERR_ARG, "cdv_fmap_to_nhwc: slot range");
  CDV_REQUIRE_ALIGNED(dst_nhwc, 16, "cdv_fmap_to_nhwc: dst_nhwc must be 16-byte aligned");
  if (count == 0) return CDV_OK;
  const int64_t total = count * H * W * (C / 8);
  const int blocks = cdv_div_up(total, 256) < 16384 ? cdv_div_up(total, 256) : 16384;
  hipLaunchKernelGGL(nchw_to_nhwc_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const _Float16*)src_nchw,
                     (_Float16*)dst_nhwc, first, count, C, H, W);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

extern "C" size_t cdv_fmap_sync_workspace_bytes(int64_t N) {
  return (size_t)(2 * (N > 0 ? N : 1) * FP_PARTS) * sizeof(uint64_t) + 64;
}

extern "C" int cdv_fmap_sync_nhwc(const void* src_nchw, void* dst_nhwc, int64_t N, int C, int H, int W, void* ws,
                                  int parity, void* stream) {
  CDV_REQUIRE(C % 8 == 0 && C > 0, CDV_ERR_ARG, "cdv_fmap_sync_nhwc: C must be a multiple of 8");
  CDV_REQUIRE(src_nchw && dst_nhwc && ws && N >= 0 && H > 0 && W > 0, CDV_ERR_ARG, "cdv_fmap_sync_nhwc: bad argument");
  CDV_REQUIRE_ALIGNED(dst_nhwc, 16, "cdv_fmap_sync_nhwc: dst_nhwc must be 16-byte aligned");
  CDV_REQUIRE_ALIGNED(src_nchw, 4, "cdv_fmap_sync_nhwc: src_nchw must be 4-byte aligned");
  CDV_REQUIRE_ALIGNED(ws, 16, "cdv_fmap_sync_nhwc: ws must be 16-byte aligned");
  if (N == 0) return CDV_OK;
  uint64_t* fp = (uint64_t*)ws;
  uint64_t* fp_new = fp + (size_t)(parity & 1) * N * FP_PARTS;
  const uint64_t* fp_old = fp + (size_t)((parity & 1) ^ 1) * N * FP_PARTS;
  int32_t* n_dirty = (int32_t*)(fp + 2 * (size_t)N * FP_PARTS);
  const int64_t words = (int64_t)C * H * W / 2;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(fmap_fingerprint_kernel, dim3((unsigned)(N * FP_PARTS)), dim3(256), 0, s, (const uint32_t*)src_nchw,
                     words, fp_new);
  const int wg_per_slot = (int)(cdv_div_up((int64_t)H * W * (C / 8), 256) < 64 ? cdv_div_up((int64_t)H * W * (C / 8), 256) : 64);
  hipLaunchKernelGGL(nchw_to_nhwc_dirty_kernel, dim3((unsigned)(N * wg_per_slot)), dim3(256), 0, s, (const _Float16*)src_nchw,
                     (_Float16*)dst_nhwc, C, H, W, fp_new, fp_old, wg_per_slot, n_dirty);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

extern "C" int cdv_shadows_sync(const cdv_shadow_ring* rings, int n_rings, const void* gmap_planar, void* gmap_pm, int64_t Ng,
                                int C_tiles, void* stream) {
  CDV_REQUIRE(n_rings >= 0 && n_rings <= 2 && (n_rings == 0 || rings != nullptr), CDV_ERR_ARG, "cdv_shadows_sync: 0 to 2 rings");
  const bool do_g = gmap_planar != nullptr && gmap_pm != nullptr && Ng > 0;
  CDV_REQUIRE(!do_g || (C_tiles % 8 == 0 && C_tiles > 0), CDV_ERR_ARG, "cdv_shadows_sync: C of the tiles must be a multiple of 8");
  CDV_REQUIRE_ALIGNED(gmap_pm, 16, "cdv_shadows_sync: gmap_pm must be 16-byte aligned");
  for (int q = 0; q < n_rings; q++) {
    CDV_REQUIRE_ALIGNED(rings[q].dst_nhwc, 16, "cdv_shadows_sync: dst_nhwc must be 16-byte aligned");
    CDV_REQUIRE_ALIGNED(rings[q].src_nchw, 4, "cdv_shadows_sync: src_nchw must be 4-byte aligned");
    CDV_REQUIRE_ALIGNED(rings[q].ws, 16, "cdv_shadows_sync: ws must be 16-byte aligned");
  }
  ShadowJobs J;
  J.n = 0;
  int fp_total = 0, cv_total = 0;
  for (int q = 0; q < n_rings; q++) {
    const cdv_shadow_ring& r = rings[q];
    CDV_REQUIRE(r.C % 8 == 0 && r.C > 0 && r.src_nchw && r.dst_nhwc && r.ws && r.N >= 0 && r.H > 0 && r.W > 0, CDV_ERR_ARG,
                "cdv_shadows_sync: bad ring");
    if (r.N == 0) continue;
    ShadowJob& s = J.j[J.n++];
    uint64_t* fp = (uint64_t*)r.ws;
    s.src = (const _Float16*)r.src_nchw; s.dst = (_Float16*)r.dst_nhwc;
    s.fp_new = fp + (size_t)(r.parity & 1) * r.N * FP_PARTS;
    s.fp_old = fp + (size_t)((r.parity & 1) ^ 1) * r.N * FP_PARTS;
    s.n_dirty = (int32_t*)(fp + 2 * (size_t)r.N * FP_PARTS);
    s.words_per_slot = (int64_t)r.C * r.H * r.W / 2;
    s.C = r.C; s.H = r.H; s.W = r.W;
    const int64_t per = cdv_div_up((int64_t)r.H * r.W * (r.C / 8), 256);
    s.wg_per_slot = (int)(per < 64 ? per : 64);
    s.fp_blocks = (int)(r.N * FP_PARTS);
    s.cv_blocks = (int)(r.N * s.wg_per_slot);
    fp_total += s.fp_blocks; cv_total += s.cv_blocks;
  }
  J.g_src = do_g ? (const _Float16*)gmap_planar : nullptr;
  J.g_dst = (_Float16*)gmap_pm;
  J.g_count = Ng; J.g_C = C_tiles;
  const int64_t gtotal = do_g ? Ng * 9 * (C_tiles / 8) : 0;
  J.g_blocks = (int)(cdv_div_up(gtotal, 256) < 16384 ? cdv_div_up(gtotal, 256) : 16384);
  if (!do_g) J.g_blocks = 0;
  hipStream_t s = (hipStream_t)stream;
  if (fp_total > 0) hipLaunchKernelGGL(shadows_fingerprint_kernel, dim3((unsigned)fp_total), dim3(256), 0, s, J);
  if (cv_total + J.g_blocks > 0)
    hipLaunchKernelGGL(shadows_convert_kernel, dim3((unsigned)(cv_total + J.g_blocks)), dim3(256), 0, s, J);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

extern "C" int cdv_frame_ingest(const void* fmap_chw, void* fmap1_nhwc, void* fmap2_nhwc, void* fmap1_nchw,
                                void* fmap2_nchw, int slot, int C, int H, int W, const void* gmap_planar, void* gmap_pm,
                                int64_t Ng, int64_t gmap_first, int64_t gmap_count, void* stream) {
  CDV_REQUIRE(C % 8 == 0 && C > 0, CDV_ERR_ARG, "cdv_fmap_ingest: C must be a multiple of 8");
  CDV_REQUIRE(H % 4 == 0 && W % 4 == 0, CDV_ERR_ARG, "cdv_fmap_ingest: H and W must be multiples of 4");
  CDV_REQUIRE(slot >= 0, CDV_ERR_ARG, "cdv_fmap_ingest: slot");
  CDV_REQUIRE_ALIGNED(fmap1_nhwc, 16, "cdv_fmap_ingest: fmap1_nhwc must be 16-byte aligned");
  CDV_REQUIRE_ALIGNED(fmap2_nhwc, 16, "cdv_fmap_ingest: fmap2_nhwc must be 16-byte aligned");
  CDV_REQUIRE_ALIGNED(gmap_pm, 16, "cdv_frame_ingest: gmap_pm must be 16-byte aligned");
  const bool do_g = gmap_planar != nullptr && gmap_pm != nullptr && gmap_count > 0;
  CDV_REQUIRE(!do_g || (gmap_first >= 0 && gmap_first + gmap_count <= Ng), CDV_ERR_ARG, "cdv_frame_ingest: tile range");
  const int64_t total = (int64_t)(H / 4) * (W / 4) * (C / 8) * 16;   // one thread per pixel and 8-channel group
  const int blocks = cdv_div_up(total, 256);
  const int gblocks = do_g ? (int)cdv_div_up(gmap_count * 9 * (C / 8), 256) : 0;
  const cdv::IngestArgs a{(const _Float16*)fmap_chw, (_Float16*)fmap1_nhwc, (_Float16*)fmap2_nhwc, (_Float16*)fmap1_nchw,
                          (_Float16*)fmap2_nchw, slot, C, H, W, (const _Float16*)gmap_planar, (_Float16*)gmap_pm,
                          gmap_first, gmap_count, blocks, gblocks};
  hipLaunchKernelGGL(fmap_ingest_kernel, dim3(blocks + gblocks), dim3(256), 0, (hipStream_t)stream, a);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

extern "C" int cdv_fmap_ingest(const void* fmap_chw, void* fmap1_nhwc, void* fmap2_nhwc, void* fmap1_nchw,
                               void* fmap2_nchw, int slot, int C, int H, int W, void* stream) {
  return cdv_frame_ingest(fmap_chw, fmap1_nhwc, fmap2_nhwc, fmap1_nchw, fmap2_nchw, slot, C, H, W, nullptr, nullptr, 0,
                          0, 0, stream);
}

extern "C" int cdv_gmap_to_pixel_major(const void* gmap_planar, void* gmap_pm, int64_t Ng, int C, int64_t first,
                                       int64_t count, void* stream) {
  CDV_REQUIRE(C % 8 == 0 && C > 0, CDV_ERR_ARG, "cdv_gmap_to_pixel_major: C must be a multiple of 8");
  CDV_REQUIRE(first >= 0 && count >= 0 && first + count <= Ng, CDV_ERR_ARG, "cdv_gmap_to_pixel_major: tile range");
  CDV_REQUIRE_ALIGNED(gmap_pm, 16, "cdv_gmap_to_pixel_major: gmap_pm must be 16-byte aligned");
  if (count == 0) return CDV_OK;
  const int64_t total = count * 9 * (C / 8);
  const int blocks = cdv_div_up(total, 256) < 16384 ? cdv_div_up(total, 256) : 16384;
  hipLaunchKernelGGL(gmap_pm_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const _Float16*)gmap_planar,
                     (_Float16*)gmap_pm, first, count, C);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}
