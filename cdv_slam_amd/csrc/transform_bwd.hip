// transform_bwd.hip -- vector-Jacobian product of the fused pops.transform (reproject.hip: cdv_transform), gfx950.
//
// The reference differentiates projective_ops.py:53-69 through a dozen autograd nodes (iproj, the gathers, lietorch Inv / Mul /
// Act4 and their *_backward kernels, proj) that scatter with float atomics.  Here the forward is recomputed per edge from the
// inputs (nothing is saved by cdv_transform) and the two scatters -- into the pose rows and into the patches -- are sums with
// one owner per output word, a fixed order and no float atomics (DESIGN.md "The projective_ops backward"):
//
//   poses    few keys (n ~ 15), long segments (tens of thousands of edges per frame): NO index.  The edges are cut into slabs of
//            whole 64-edge tiles; one wave per slab computes its edges (lane = edge), adds the contributions of each frame in
//            the tile with a fixed shuffle tree and the tiles in ascending order into an LDS row per frame, and leaves
//            [slab][frame][6] partial sums; the gather launch adds the slabs of a frame in slab order.
//   patches  many keys, short segments: count / scan / fill / order on kk as corr_bwd.hip does it (integer atomics for the
//            slots, then every edge finds its rank among its segment's edge ids: ascending edge order); one lane per output
//            word walks its segment over the per-edge words the edge pass left in the workspace.
//
// Convention of the pose gradient: the left-perturbation row vector in words 0..5 of the 7-word row, word 6 zero (lie_bwd.hip).
#include "cdv_common.h"
// No multiply-add contraction (as lie_bwd.hip): an edge's contribution is the same bits whichever outputs are asked for.
#pragma clang fp contract(off)
#include "cdv_se3.h"

namespace {

// (kernel names carry the file's prefix, tfb_: corr_bwd.hip has a zero / scan / fill / order of its own)
constexpr int TILE = 64;              // edges per tile = lanes per wave
constexpr int MAX_SLABS = 1024;       // pose partial sums: at most this many slabs ...
constexpr int MIN_SLABS = 16;
constexpr int SLAB_WORDS = 16384;     // ... and about this many frames x slabs (the partials are written in full)
constexpr int MAX_FRAMES = 1024;      // an LDS row of 6 floats per frame
constexpr int SCAN_THREADS = 1024;
constexpr int GTHREADS = 256;

struct Geometry {
  int64_t tiles;
  int slabs, tiles_per_slab;
};

// launch geometry of the edge pass from the shapes alone
Geometry geometry(int64_t E, int64_t n) {
  Geometry g;
  g.tiles = (E + TILE - 1) / TILE;
  int64_t cap = SLAB_WORDS / (n > 0 ? n : 1);
  cap = cap < MIN_SLABS ? MIN_SLABS : cap > MAX_SLABS ? MAX_SLABS : cap;
  g.tiles_per_slab = (int)((g.tiles + cap - 1) / cap);
  if (g.tiles_per_slab < 1) g.tiles_per_slab = 1;
  g.slabs = (int)((g.tiles + g.tiles_per_slab - 1) / g.tiles_per_slab);
  return g;
}

size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }

struct Layout {
  size_t partial, pw, cnt, off, cursor, tmp, sorted, total;
};

Layout layout(int64_t E, int64_t n, int64_t m, int P) {
  const Geometry g = geometry(E, n);
  Layout L;
  size_t at = 0;
  L.partial = at; at += align16((size_t)g.slabs * (size_t)n * 6 * sizeof(float));
  L.pw = at;      at += align16((size_t)E * 3 * P * P * sizeof(float));
  L.cnt = at;     at += align16((size_t)(m + 1) * sizeof(int));
  L.off = at;     at += align16((size_t)(m + 1) * sizeof(int));
  L.cursor = at;  at += align16((size_t)(m + 1) * sizeof(int));
  L.tmp = at;     at += align16((size_t)E * sizeof(int));
  L.sorted = at;  at += align16((size_t)E * sizeof(int));
  L.total = at;
  return L;
}

struct Args {
  const float *poses, *patches, *intr, *grad;
  const int64_t *ii, *jj, *kk;
  int64_t E, n, m;
  int e2pp, need_poses, need_patches, tiles_per_slab;
  float* partial;   // [slabs][n][6]
  float* pw;        // [E][3 P P]: the edge's words of dpatches[kk[e]]
  int* cnt;         // [m]: edges per patch
};

// ---- the edge pass: one wave per slab of tiles, lane = edge ------------------------------------------------------------
template <int P>
__global__ __launch_bounds__(TILE) void tfb_edge_kernel(const Args A) {
  constexpr int PP = P * P;
  extern __shared__ float s_acc[];                 // [n][6]
  const int lane = threadIdx.x;
  const int n6 = (int)A.n * 6;
  if (A.need_poses) {
    for (int i = lane; i < n6; i += TILE) s_acc[i] = 0.f;
    __syncthreads();
  }
  const int64_t t0 = (int64_t)blockIdx.x * A.tiles_per_slab;
  for (int64_t tile = t0; tile < t0 + A.tiles_per_slab && tile * TILE < A.E; tile++) {
    const int64_t e = tile * TILE + lane;
    int64_t ix = 0, jx = 0, kx = 0;
    bool in = e < A.E;
    if (in) {
      ix = A.ii[e]; jx = A.jj[e]; kx = A.kk[e];
      // an edge that names a frame or a patch outside the arrays contributes nothing (and touches nothing)
      in = ix >= 0 && ix < A.n && jx >= 0 && jx < A.n && kx >= 0 && kx < A.m;
    }
    float a[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, b[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (in) {
      // The recomputation runs in float64 and rounds once per word: behind a pose step Z = 1 + t_z d is a difference of nearly
      // equal numbers, D and D^2 carry its relative error (50 u in float32 at Z = 0.04), and the gradient is what is left of it.
      // Gij = Gj * Gi^-1, re-normalised on every load as transform_body has it (cdv_parts.h tf_relative)
      double Pi[7], Pj[7], Pinv[7], G[7], t[3], q[4], R[9];
#pragma unroll
      for (int c = 0; c < 7; c++) { Pi[c] = (double)A.poses[7 * ix + c]; Pj[c] = (double)A.poses[7 * jx + c]; }
      cdv::lt_se3_inv(Pi, Pinv);
      cdv::lt_se3_mul(Pj, Pinv, G);
      cdv::lt_se3_load(G, t, q);
      cdv::lt_quat_to_R(q, R);
      const double fxi = A.intr[4 * ix + 0], fyi = A.intr[4 * ix + 1], cxi = A.intr[4 * ix + 2], cyi = A.intr[4 * ix + 3];
      const double fxj = A.intr[4 * jx + 0], fyj = A.intr[4 * jx + 1];
      const double rfxi = 1.0 / fxi, rfyi = 1.0 / fyi;
      const float* pk = A.patches + kx * 3 * PP;
      const float* g = A.grad + e * 2 * PP;
      float* pw = A.pw + e * 3 * PP;
      double ad[6] = {0., 0., 0., 0., 0., 0.}, bd[6];
#pragma unroll
      for (int p = 0; p < PP; p++) {
        const double gu = A.e2pp ? g[p] : g[2 * p], gv = A.e2pp ? g[PP + p] : g[2 * p + 1];
        double X0[4], X1[4];
        X0[0] = ((double)pk[p] - cxi) * rfxi;      // iproj, projective_ops.py:19-29
        X0[1] = ((double)pk[PP + p] - cyi) * rfyi;
        X0[2] = 1.0;
        X0[3] = pk[2 * PP + p];
        cdv::lt_act4_loaded(t, q, X0, X1);
        const double Z = X1[2];
        const double D = 1.0 / fmax(Z, 0.1);       // proj, projective_ops.py:43; the clamp passes no gradient below 0.1
        double qb[3];
        qb[0] = fxj * D * gu;
        qb[1] = fyj * D * gv;
        qb[2] = Z >= 0.1 ? -(D * D) * (fxj * X1[0] * gu + fyj * X1[1] * gv) : 0.0;
        // act4: dX = dq [[q_w I, -[q_xyz]x], [0]]  (lie_bwd.hip)
        double c[3];
        cdv::cross3(X1, qb, c);
        ad[0] += X1[3] * qb[0]; ad[1] += X1[3] * qb[1]; ad[2] += X1[3] * qb[2];
        ad[3] += c[0]; ad[4] += c[1]; ad[5] += c[2];
        if (A.need_patches) {                      // dX0 = dq M(G), through iproj
          double r[3];
          cdv::mat3T_vec(R, qb, r);
          pw[p] = (float)(r[0] * rfxi);
          pw[PP + p] = (float)(r[1] * rfyi);
          pw[2 * PP + p] = (float)(qb[0] * t[0] + qb[1] * t[1] + qb[2] * t[2]);
        }
      }
      cdv::lt_se3_adjT_loaded(t, R, ad, bd);       // a . Ad(G): mul then inv of the table, Ad(Gj) Ad(Gi^-1) = Ad(G)
#pragma unroll
      for (int c = 0; c < 6; c++) { a[c] = (float)ad[c]; b[c] = (float)-bd[c]; }
      if (A.need_patches) atomicAdd(A.cnt + kx, 1);
    }
    if (!A.need_poses) continue;
    // every frame named in the tile: its lanes' a (as target) and b (as source) through one fixed shuffle tree, then onto the
    // frame's LDS row -- tiles in ascending order
    const int jk = in ? (int)jx : -1, ik = in ? (int)ix : -1;
    unsigned long long todo_j = __ballot(in), todo_i = todo_j;
    while (todo_j | todo_i) {                       // wave-uniform
      const int key = todo_j ? __shfl(jk, __ffsll((long long)todo_j) - 1) : __shfl(ik, __ffsll((long long)todo_i) - 1);
      const bool mj = jk == key, mi = ik == key;
      float v[6];
#pragma unroll
      for (int c = 0; c < 6; c++) {
        v[c] = (mj ? a[c] : 0.f) + (mi ? b[c] : 0.f);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o);
      }
      if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 6; c++) s_acc[key * 6 + c] += v[c];
      }
      todo_j &= ~__ballot(mj);
      todo_i &= ~__ballot(mi);
    }
  }
  if (A.need_poses) {
    __syncthreads();
    float* out = A.partial + (int64_t)blockIdx.x * n6;
    for (int i = lane; i < n6; i += TILE) out[i] = s_acc[i];
  }
}

// ---- the patch index: count (in the edge pass) / scan / fill / order, as corr_bwd.hip ------------------------------------
__global__ __launch_bounds__(256) void tfb_zero_kernel(int* __restrict__ cnt, int64_t K) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < K) cnt[i] = 0;
}

// off[k] = edges of the patches before k, off[K] = their number; cursor = off
__global__ __launch_bounds__(SCAN_THREADS) void tfb_scan_kernel(const int* __restrict__ cnt, int* __restrict__ off,
                                                            int* __restrict__ cursor, int64_t K) {
  __shared__ int s_sum[SCAN_THREADS];
  const int t = threadIdx.x;
  const int64_t per = (K + SCAN_THREADS - 1) / SCAN_THREADS;
  const int64_t lo = min((int64_t)t * per, K), hi = min(lo + per, K);
  int sum = 0;
  for (int64_t i = lo; i < hi; i++) sum += cnt[i];
  s_sum[t] = sum;
  __syncthreads();
  for (int o = 1; o < SCAN_THREADS; o <<= 1) {
    const int add = t >= o ? s_sum[t - o] : 0;
    __syncthreads();
    s_sum[t] += add;
    __syncthreads();
  }
  int run = s_sum[t] - sum;
  for (int64_t i = lo; i < hi; i++) {
    off[i] = run;
    cursor[i] = run;
    run += cnt[i];
  }
  if (t == SCAN_THREADS - 1) off[K] = s_sum[t];
}

__device__ __forceinline__ int patch_key(const Args& A, int64_t e) {
  const int64_t ix = A.ii[e], jx = A.jj[e], kx = A.kk[e];
  return (ix >= 0 && ix < A.n && jx >= 0 && jx < A.n && kx >= 0 && kx < A.m) ? (int)kx : -1;
}

__global__ __launch_bounds__(256) void tfb_fill_kernel(const Args A, int* __restrict__ cursor, int* __restrict__ tmp) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= A.E) return;
  const int key = patch_key(A, e);
  if (key >= 0) tmp[atomicAdd(cursor + key, 1)] = (int)e;
}

// rank of an edge among its patch's edges = number of smaller edge ids in the segment (short: the edges of one patch)
__global__ __launch_bounds__(256) void tfb_order_kernel(const Args A, const int* __restrict__ off, const int* __restrict__ tmp,
                                                    int* __restrict__ sorted) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= A.E) return;
  const int key = patch_key(A, e);
  if (key < 0) return;
  const int lo = off[key], hi = off[key + 1];
  int rank = 0;
  for (int j = lo; j < hi; j++) rank += tmp[j] < (int)e;
  sorted[lo + rank] = (int)e;
}

// ---- the gather: blocks [0, pose_blocks) own the pose rows (one wave per frame), the others the patch words ---------------
__global__ __launch_bounds__(GTHREADS) void tfb_gather_kernel(const Args A, int slabs, int pose_blocks, int PP3,
                                                          const int* __restrict__ off, const int* __restrict__ sorted,
                                                          float* __restrict__ dposes, float* __restrict__ dpatches) {
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < pose_blocks) {
    const int lane = tid & 63;
    const int64_t f = (int64_t)blockIdx.x * (GTHREADS / 64) + (tid >> 6);
    if (f >= A.n) return;                            // wave-uniform
    float v[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = lane; s < slabs; s += 64) {         // slabs of a lane in ascending order, then the fixed tree over lanes
      const float* p = A.partial + ((int64_t)s * A.n + f) * 6;
#pragma unroll
      for (int c = 0; c < 6; c++) v[c] += p[c];
    }
#pragma unroll
    for (int c = 0; c < 6; c++) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v[c] += __shfl_xor(v[c], o);
    }
    if (lane < 7) {
      float w = 0.f;
#pragma unroll
      for (int c = 0; c < 6; c++) w = lane == c ? v[c] : w;
      dposes[f * 7 + lane] = w;
    }
    return;
  }
  const int64_t idx = (int64_t)((int)blockIdx.x - pose_blocks) * GTHREADS + tid;
  if (idx >= A.m * PP3) return;
  const int64_t k = idx / PP3;
  const int w = (int)(idx - k * PP3);
  float sum = 0.f;
  for (int j = off[k]; j < off[k + 1]; j++) sum += A.pw[(int64_t)sorted[j] * PP3 + w];
  dpatches[idx] = sum;
}

__global__ __launch_bounds__(256) void tfb_zero_f32_kernel(float* __restrict__ p, int64_t K) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < K) p[i] = 0.f;
}

}  // namespace

extern "C" size_t cdv_transform_bwd_workspace_bytes(int64_t E, int64_t n, int64_t m, int P) {
  if (E < 0 || n < 0 || m < 0 || (P != 1 && P != 3)) return 0;
  return layout(E, n, m, P).total;
}

extern "C" int cdv_transform_bwd(const cdv_transform_bwd_args* args, void* stream) {
  CDV_REQUIRE(args != nullptr, CDV_ERR_ARG, "cdv_transform_bwd: args is NULL");
  const cdv_transform_bwd_args r = *args;
  const float *poses = r.poses, *patches = r.patches, *intrinsics = r.intrinsics, *grad_coords = r.grad_coords;
  const int64_t *ii = r.ii, *jj = r.jj, *kk = r.kk;
  const int64_t E = r.E, n = r.n, m = r.m;
  const int P = r.P, flags = r.flags;
  float *dposes = r.dposes, *dpatches = r.dpatches;
  void* workspace = r.workspace;
  CDV_REQUIRE(P == 3 || P == 1, CDV_ERR_UNSUPPORTED, "cdv_transform_bwd: patch size P must be 3 or 1");
  CDV_REQUIRE(!(flags & CDV_TF_TONLY), CDV_ERR_UNSUPPORTED, "cdv_transform_bwd: the translation-only transform has no backward");
  CDV_REQUIRE((flags & ~(CDV_TF_LAYOUT_E2PP | CDV_TF_TONLY)) == 0, CDV_ERR_ARG, "cdv_transform_bwd: unknown flag");
  CDV_REQUIRE(E >= 0 && n >= 0 && m >= 0, CDV_ERR_ARG, "cdv_transform_bwd: E, n, m must not be negative");
  CDV_REQUIRE(E <= ((int64_t)1 << 30) && m < ((int64_t)1 << 31) / 27, CDV_ERR_ARG, "cdv_transform_bwd: E or m beyond 32-bit edge ids");
  CDV_REQUIRE(n <= MAX_FRAMES || !dposes, CDV_ERR_UNSUPPORTED,
              "cdv_transform_bwd: the pose gradient is served for at most 1024 frames (one LDS row per frame)");
  hipStream_t s = (hipStream_t)stream;
  const int PP3 = 3 * P * P;
  if (!dposes && !dpatches) return CDV_OK;
  if (E == 0) {
    if (dposes && n > 0) hipLaunchKernelGGL(tfb_zero_f32_kernel, dim3(cdv_div_up(n * 7, 256)), dim3(256), 0, s, dposes, n * 7);
    if (dpatches && m > 0)
      hipLaunchKernelGGL(tfb_zero_f32_kernel, dim3(cdv_div_up(m * PP3, 256)), dim3(256), 0, s, dpatches, m * PP3);
    CDV_LAUNCH_CHECK();
    return CDV_OK;
  }
  CDV_REQUIRE(workspace != nullptr, CDV_ERR_ARG, "cdv_transform_bwd: workspace is NULL");
  CDV_REQUIRE_ALIGNED(workspace, 16, "cdv_transform_bwd: workspace must be 16-byte aligned");
  CDV_REQUIRE(poses && patches && intrinsics && ii && jj && kk && grad_coords, CDV_ERR_ARG,
              "cdv_transform_bwd: an input pointer is NULL");
  const Geometry g = geometry(E, n);
  const Layout L = layout(E, n, m, P);
  char* ws = (char*)workspace;
  int* cnt = (int*)(ws + L.cnt);
  int* off = (int*)(ws + L.off);
  int* cursor = (int*)(ws + L.cursor);
  int* tmp = (int*)(ws + L.tmp);
  int* sorted = (int*)(ws + L.sorted);
  Args A{poses, patches, intrinsics, grad_coords, ii, jj, kk, E, n, m, (flags & CDV_TF_LAYOUT_E2PP) ? 1 : 0,
         dposes ? 1 : 0, dpatches ? 1 : 0, g.tiles_per_slab, (float*)(ws + L.partial), (float*)(ws + L.pw), cnt};
  if (dpatches) hipLaunchKernelGGL(tfb_zero_kernel, dim3(cdv_div_up(m + 1, 256)), dim3(256), 0, s, cnt, m + 1);
  const size_t lds = dposes ? (size_t)n * 6 * sizeof(float) : 0;
  if (P == 3)
    hipLaunchKernelGGL(tfb_edge_kernel<3>, dim3(g.slabs), dim3(TILE), lds, s, A);
  else
    hipLaunchKernelGGL(tfb_edge_kernel<1>, dim3(g.slabs), dim3(TILE), lds, s, A);
  if (dpatches) {
    hipLaunchKernelGGL(tfb_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, cnt, off, cursor, m);
    hipLaunchKernelGGL(tfb_fill_kernel, dim3(cdv_div_up(E, 256)), dim3(256), 0, s, A, cursor, tmp);
    hipLaunchKernelGGL(tfb_order_kernel, dim3(cdv_div_up(E, 256)), dim3(256), 0, s, A, off, tmp, sorted);
  }
  const int pose_blocks = dposes ? cdv_div_up(n, GTHREADS / 64) : 0;
  const int patch_blocks = dpatches ? cdv_div_up(m * PP3, GTHREADS) : 0;
  if (pose_blocks + patch_blocks > 0)
    hipLaunchKernelGGL(tfb_gather_kernel, dim3(pose_blocks + patch_blocks), dim3(GTHREADS), 0, s, A, g.slabs, pose_blocks, PP3, off,
                       sorted, dposes, dpatches);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}
