// corr_bwd.hip -- the altcorr backward passes (training): cuda_corr.backward (correlation_kernel.cu:139-190, :236-285)
// and cuda_corr.patchify_backward (:49-80, :310-333) as destination gathers.
//
// The reference scatters every product with a float atomic add.  Here every output element is owned by one lane that
// sums its contributions in a fixed order and stores once, so the result is bitwise reproducible and needs neither a
// zero-fill nor float atomics.  Both ops are the same six launches on one stream (no host synchronisation, so a call
// can be captured into a graph):
//   1. zero     the per-key counters of the index
//   2. count    every entry (an edge, or a window) bumps the counter of its key (integer atomics)
//   3. scan     one workgroup: exclusive scan of the counts -> segment offsets, and the fill cursors in place
//   4. fill     every entry takes a slot of its key's segment (integer atomics: slot order is arbitrary)
//   5. order    every entry finds its rank among its segment's ids and stores itself there: ascending ids
//   6. gather   one workgroup per destination block walks its segments in ascending id order and stores once
//
// Keys.  A window (D x D pixels, D = 2r+2, top-left corner (y0, x0)) is binned by the BX x BY tile of its corner, in a
// tile grid shifted by S = ceil((D-1)/B) tiles per axis so that corners up to D-1 pixels above / left of the map get a
// bin too.  Output tile (oy, ox) reads the bins of tile rows floor((oy BY - D + 1) / BY) + SY .. oy + SY (likewise
// columns), row by row, each segment in ascending id: one fixed order per output element.  Windows wholly off the map, and edges with
// an index outside [0, N1) / [0, N2), get no key and contribute nothing (the forward gives them zero).
//
// The correlation's two gradients share one index (keys [0, N1): the edges of each fmap1 tile, keys N1..: the (edge,
// patch pixel) windows of each fmap2 frame) and one gather launch with two workgroup roles.
#include "cdv_common.h"

namespace {

constexpr int BTHREADS = 64;    // one wave per gather workgroup: one lane per pixel of a BX x BY tile, BX BY = 64
// tile shapes: the correlation's 8 x 8 windows (r 3) meet most lanes of an 8 x 8 tile; patchify's small windows
// (2x2 .. 4x4) leave most tiles empty, where 32 x 2 tiles store 128-B row segments of the (mostly zero) gradient
constexpr int CORR_BX = 8, CORR_BY = 8, PATCH_BX = 32, PATCH_BY = 2;
constexpr int CCH = 32;         // channels per gather workgroup (register accumulators per lane)
constexpr int SCAN_THREADS = 1024;
constexpr int ENTRY_BLOCKS_MAX = 16384;

__device__ __forceinline__ int clamp_floor(float v) { return (int)fminf(fmaxf(floorf(v), -1.0e6f), 1.0e6f); }

__host__ __device__ __forceinline__ int floor_div(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the tile grid of one map: BX x BY tiles, TY x TX bins per frame, shifts SY, SX
struct Tiles {
  int BX, BY, SY, SX, TY, TX, OTY, OTX;
};

__host__ __device__ inline Tiles make_tiles(int H, int W, int D, int BX, int BY) {
  Tiles t;
  t.BX = BX;
  t.BY = BY;
  t.SY = (D - 1 + BY - 1) / BY;
  t.SX = (D - 1 + BX - 1) / BX;
  t.TY = (H - 1) / BY + t.SY + 1;
  t.TX = (W - 1) / BX + t.SX + 1;
  t.OTY = (H + BY - 1) / BY;
  t.OTX = (W + BX - 1) / BX;
  return t;
}

// bin of a D x D window with corner (y0, x0) on an H x W map, or -1 when it misses the map
__device__ __forceinline__ int window_bin(int y0, int x0, int D, int H, int W, const Tiles& t) {
  if (y0 + D <= 0 || y0 >= H || x0 + D <= 0 || x0 >= W) return -1;
  return (floor_div(y0, t.BY) + t.SY) * t.TX + floor_div(x0, t.BX) + t.SX;
}

// ---- the two problems' entries: id and key -------------------------------------------------------------------------
struct CorrIdx {
  const float* coords;  // [M][2][P][P]
  const int64_t* us;
  const int64_t* vs;
  int64_t M, N1, N2;
  int P, H2, W2, R;
  Tiles t;
  // entries [0, M): edge m, key us[m]; entries [M, M + M P^2): window (m, q), key N1 + bin
  __device__ __forceinline__ int64_t n_entries() const { return M + M * P * P; }
  __device__ __forceinline__ void entry(int64_t e, int& id, int& key) const {
    const int PP = P * P;
    const int64_t m = e < M ? e : (e - M) / PP;
    const int64_t ix = us[m], jx = vs[m];
    key = -1;
    if (e < M) {
      id = (int)m;
      if (ix >= 0 && ix < N1 && jx >= 0 && jx < N2) key = (int)ix;
      return;
    }
    const int q = (int)((e - M) % PP);
    id = (int)(m * PP + q);
    if (!(ix >= 0 && ix < N1 && jx >= 0 && jx < N2)) return;
    const int D = 2 * R + 2;
    const int x0 = clamp_floor(coords[m * 2 * PP + q]) - R, y0 = clamp_floor(coords[(m * 2 + 1) * PP + q]) - R;
    const int b = window_bin(y0, x0, D, H2, W2, t);
    if (b >= 0) key = (int)(N1 + (jx * t.TY * t.TX) + b);
  }
};

struct PatchIdx {
  const float* coords;  // [B][M][2]
  int64_t M;
  int B, H, W, R;
  Tiles t;
  __device__ __forceinline__ int64_t n_entries() const { return (int64_t)B * M; }
  __device__ __forceinline__ void entry(int64_t e, int& id, int& key) const {
    id = (int)e;
    const int bb = (int)(e / M);
    const int D = 2 * R + 2;
    const int x0 = clamp_floor(coords[e * 2 + 0]) - R, y0 = clamp_floor(coords[e * 2 + 1]) - R;
    const int b = window_bin(y0, x0, D, H, W, t);
    key = b < 0 ? -1 : bb * t.TY * t.TX + b;
  }
};

// workspace: [cnt / cursor K][off K + 1][tmp E][sorted E] int32
struct Index {
  int* cnt;
  int* off;
  int* tmp;
  int* sorted;
};

__host__ inline Index carve(void* ws, int64_t K, int64_t E) {
  Index x;
  x.cnt = (int*)ws;
  x.off = x.cnt + K;
  x.tmp = x.off + K + 1;
  x.sorted = x.tmp + E;
  return x;
}

__host__ inline size_t index_bytes(int64_t K, int64_t E) { return (size_t)(K + K + 1 + E + E) * sizeof(int) + 256; }

__global__ __launch_bounds__(256) void zero_kernel(int* __restrict__ cnt, int64_t K) {
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x)
    cnt[k] = 0;
}

template <class Prob>
__global__ __launch_bounds__(256) void count_kernel(const Prob pr, int* __restrict__ cnt) {
  const int64_t E = pr.n_entries();
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    int id, key;
    pr.entry(e, id, key);
    if (key >= 0) atomicAdd(cnt + key, 1);
  }
}

// one workgroup: off[k] = sum of cnt[< k], off[K] = total; cnt[k] becomes the fill cursor off[k]
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(int* __restrict__ cnt, int* __restrict__ off, int64_t K) {
  __shared__ int wsum[SCAN_THREADS / CDV_WAVE];
  __shared__ int carry_s;
  const int tid = threadIdx.x, lane = tid & (CDV_WAVE - 1), w = tid / CDV_WAVE;
  if (tid == 0) carry_s = 0;
  __syncthreads();
  for (int64_t base = 0; base < K; base += SCAN_THREADS) {
    const int64_t k = base + tid;
    const int v = k < K ? cnt[k] : 0;
    int incl = v;
#pragma unroll
    for (int d = 1; d < CDV_WAVE; d <<= 1) {
      const int o = __shfl_up(incl, d, CDV_WAVE);
      if (lane >= d) incl += o;
    }
    if (lane == CDV_WAVE - 1) wsum[w] = incl;
    __syncthreads();
    int before = carry_s;
    for (int j = 0; j < w; j++) before += wsum[j];
    const int ex = before + incl - v;
    if (k < K) {
      off[k] = ex;
      cnt[k] = ex;
    }
    __syncthreads();
    if (tid == SCAN_THREADS - 1) carry_s = ex + v;
    __syncthreads();
  }
  if (tid == 0) off[K] = carry_s;
}

template <class Prob>
__global__ __launch_bounds__(256) void fill_kernel(const Prob pr, int* __restrict__ cursor, int* __restrict__ tmp) {
  const int64_t E = pr.n_entries();
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    int id, key;
    pr.entry(e, id, key);
    if (key >= 0) tmp[atomicAdd(cursor + key, 1)] = id;
  }
}

// rank of an id among its segment = number of smaller ids in it (ids are distinct): the segment in ascending order
template <class Prob>
__global__ __launch_bounds__(256) void order_kernel(const Prob pr, const int* __restrict__ off,
                                                    const int* __restrict__ tmp, int* __restrict__ sorted) {
  const int64_t E = pr.n_entries();
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < E; e += (int64_t)gridDim.x * blockDim.x) {
    int id, key;
    pr.entry(e, id, key);
    if (key < 0) continue;
    const int lo = off[key], hi = off[key + 1];
    int rank = 0;
    for (int j = lo; j < hi; j++) rank += tmp[j] < id;
    sorted[lo + rank] = id;
  }
}

// ---- the correlation's window gradient, recomputed where it is needed ------------------------------------------------
// gw[A][B] of edge m at patch pixel q: the adjoint of the forward's blend out[xo][yo] = sum_ab w_ab c[yo + a][xo + b]
// (corr_generic_kernel), grad [M][D-1 (x)][D-1 (y)][P][P]; fixed order of the four terms
__device__ __forceinline__ float window_grad(const float* __restrict__ grad, int64_t m, int q, int PP, int D, int A,
                                             int B, float dx, float dy) {
  const int d = D - 1;
  const float* g = grad + m * (int64_t)d * d * PP + q;
  float s = 0.f;
  if (A < d && B < d) s += (1.f - dx) * (1.f - dy) * g[((int64_t)B * d + A) * PP];
  if (A < d && B >= 1) s += dx * (1.f - dy) * g[((int64_t)(B - 1) * d + A) * PP];
  if (A >= 1 && B < d) s += (1.f - dx) * dy * g[((int64_t)B * d + A - 1) * PP];
  if (A >= 1 && B >= 1) s += dx * dy * g[((int64_t)(B - 1) * d + A - 1) * PP];
  return s;
}

struct CorrGather {
  const float* fmap1;  // [N1][C][P][P]
  const float* fmap2;  // [N2][C][H2][W2]
  const float* grad;   // [M][D-1][D-1][P][P]
  float* g1;           // fmap1_grad or NULL
  float* g2;           // fmap2_grad or NULL
  int nwg1, groups1;   // role 1: N1 x groups1 workgroups (BTHREADS (c, q) outputs each)
  int chunks2;         // role 2: N2 x OTY x OTX x chunks2 workgroups
  int nwg2;
  int C;
};

__global__ __launch_bounds__(BTHREADS) void corr_gather_kernel(const CorrIdx ix, const CorrGather G,
                                                               const int* __restrict__ off,
                                                               const int* __restrict__ sorted) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x;
  const int P = ix.P, PP = P * P, R = ix.R, D = 2 * R + 2, DD = D * D, C = G.C;
  const int H2 = ix.H2, W2 = ix.W2;
  if ((int)blockIdx.x < G.nwg1) {
    // ---- role 1: fmap1_grad[n1][c][q] = sum over the edges of tile n1 (ascending) and the window of q
    const int64_t n1 = blockIdx.x / G.groups1;
    const int o = (blockIdx.x % G.groups1) * BTHREADS + tid;
    const bool active = o < C * PP;
    const int c = active ? o / PP : 0, q = active ? o % PP : 0;
    float* gw = lds;                            // [PP][D][D]
    int* org = (int*)(lds + (size_t)PP * DD);   // [PP][2] window corners (y0, x0)
    float acc = 0.f;
    const int lo = off[n1], hi = off[n1 + 1];
    for (int j = lo; j < hi; j++) {
      const int64_t m = sorted[j];
      __syncthreads();
      for (int t = tid; t < PP * DD; t += BTHREADS) {
        const int qq = t / DD, A = (t / D) % D, B = t % D;
        const float x = ix.coords[m * 2 * PP + qq], y = ix.coords[(m * 2 + 1) * PP + qq];
        gw[t] = window_grad(G.grad, m, qq, PP, D, A, B, x - floorf(x), y - floorf(y));
      }
      for (int t = tid; t < PP; t += BTHREADS) {
        org[2 * t] = clamp_floor(ix.coords[(m * 2 + 1) * PP + t]) - R;
        org[2 * t + 1] = clamp_floor(ix.coords[m * 2 * PP + t]) - R;
      }
      __syncthreads();
      if (active) {
        const int y0 = org[2 * q], x0 = org[2 * q + 1];
        const float* f2 = G.fmap2 + (ix.vs[m] * C + c) * (int64_t)H2 * W2;
        const float* w = gw + q * DD;
        for (int A = 0; A < D; A++) {
          const int i1 = y0 + A;
          if (i1 < 0 || i1 >= H2) continue;
          for (int B = 0; B < D; B++) {
            const int j1 = x0 + B;
            if (j1 >= 0 && j1 < W2) acc += w[A * D + B] * f2[(int64_t)i1 * W2 + j1];
          }
        }
      }
    }
    if (active) G.g1[(n1 * C + c) * PP + q] = acc;
    return;
  }
  // ---- role 2: fmap2_grad, one lane per pixel of a BX x BY tile, CCH channels
  int r = blockIdx.x - G.nwg1;
  if (r >= G.nwg2) return;   // the idle workgroup of an empty grid
  const Tiles& t = ix.t;
  const int ch = r % G.chunks2; r /= G.chunks2;
  const int ox = r % t.OTX; r /= t.OTX;
  const int oy = r % t.OTY; r /= t.OTY;
  const int64_t n2 = r;
  const int py = oy * t.BY + tid / t.BX, px = ox * t.BX + tid % t.BX;
  const bool inside = py < H2 && px < W2;
  const int c0 = ch * CCH, cc = C - c0 < CCH ? C - c0 : CCH;
  float acc[CCH];
#pragma unroll
  for (int k = 0; k < CCH; k++) acc[k] = 0.f;
  const int ty0 = floor_div(oy * t.BY - D + 1, t.BY) + t.SY, tx0 = floor_div(ox * t.BX - D + 1, t.BX) + t.SX;
  for (int ty = ty0 < 0 ? 0 : ty0; ty <= oy + t.SY && ty < t.TY; ty++)
    for (int tx = tx0 < 0 ? 0 : tx0; tx <= ox + t.SX && tx < t.TX; tx++) {
      const int64_t key = ix.N1 + (n2 * t.TY + ty) * t.TX + tx;
      const int lo = off[key], hi = off[key + 1];
      for (int j = lo; j < hi; j++) {
        const int id = sorted[j];
        const int64_t m = id / PP;
        const int q = id % PP;
        const float x = ix.coords[m * 2 * PP + q], y = ix.coords[(m * 2 + 1) * PP + q];
        const int A = py - (clamp_floor(y) - R), B = px - (clamp_floor(x) - R);
        if (!inside || A < 0 || A >= D || B < 0 || B >= D) continue;
        const float g = window_grad(G.grad, m, q, PP, D, A, B, x - floorf(x), y - floorf(y));
        const float* f1 = G.fmap1 + (ix.us[m] * C + c0) * (int64_t)PP + q;
#pragma unroll
        for (int k = 0; k < CCH; k++)
          if (k < cc) acc[k] += g * f1[(int64_t)k * PP];
      }
    }
  if (!inside) return;
#pragma unroll
  for (int k = 0; k < CCH; k++)
    if (k < cc) G.g2[((n2 * C + c0 + k) * H2 + py) * (int64_t)W2 + px] = acc[k];
}

// net_grad[b][c][py][px] = sum over the patches whose window covers the pixel (ascending b M + m) of patch_grad
template <typename T>
__global__ __launch_bounds__(BTHREADS) void patchify_gather_kernel(const PatchIdx ix, const T* __restrict__ pg,
                                                                   T* __restrict__ out, int C, int chunks,
                                                                   const int* __restrict__ off,
                                                                   const int* __restrict__ sorted) {
  const int tid = threadIdx.x;
  const int R = ix.R, D = 2 * R + 2, H = ix.H, W = ix.W;
  const Tiles& t = ix.t;
  int r = blockIdx.x;
  const int ch = r % chunks; r /= chunks;
  const int ox = r % t.OTX; r /= t.OTX;
  const int oy = r % t.OTY; r /= t.OTY;
  const int64_t bb = r;
  const int py = oy * t.BY + tid / t.BX, px = ox * t.BX + tid % t.BX;
  const bool inside = py < H && px < W;
  const int c0 = ch * CCH, cc = C - c0 < CCH ? C - c0 : CCH;
  float acc[CCH];
#pragma unroll
  for (int k = 0; k < CCH; k++) acc[k] = 0.f;
  const int ty0 = floor_div(oy * t.BY - D + 1, t.BY) + t.SY, tx0 = floor_div(ox * t.BX - D + 1, t.BX) + t.SX;
  for (int ty = ty0 < 0 ? 0 : ty0; ty <= oy + t.SY && ty < t.TY; ty++)
    for (int tx = tx0 < 0 ? 0 : tx0; tx <= ox + t.SX && tx < t.TX; tx++) {
      const int64_t key = (bb * t.TY + ty) * t.TX + tx;
      const int lo = off[key], hi = off[key + 1];
      for (int j = lo; j < hi; j++) {
        const int64_t e = sorted[j];
        const int A = py - (clamp_floor(ix.coords[e * 2 + 1]) - R), B = px - (clamp_floor(ix.coords[e * 2]) - R);
        if (!inside || A < 0 || A >= D || B < 0 || B >= D) continue;
        const T* p = pg + ((e * C + c0) * D + A) * (int64_t)D + B;
#pragma unroll
        for (int k = 0; k < CCH; k++)
          if (k < cc) acc[k] += (float)p[(int64_t)k * D * D];
      }
    }
  if (!inside) return;
#pragma unroll
  for (int k = 0; k < CCH; k++)
    if (k < cc) out[((bb * C + c0 + k) * H + py) * (int64_t)W + px] = (T)acc[k];
}

inline int entry_blocks(int64_t E) {
  const int64_t b = (E + 255) / 256;
  return b < 1 ? 1 : (b > ENTRY_BLOCKS_MAX ? ENTRY_BLOCKS_MAX : (int)b);
}

template <class Prob>
int build_index(const Prob& pr, Index x, int64_t K, int64_t E, hipStream_t s) {
  hipLaunchKernelGGL(zero_kernel, dim3(entry_blocks(K)), dim3(256), 0, s, x.cnt, K);
  hipLaunchKernelGGL(count_kernel<Prob>, dim3(entry_blocks(E)), dim3(256), 0, s, pr, x.cnt);
  hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, x.cnt, x.off, K);
  hipLaunchKernelGGL(fill_kernel<Prob>, dim3(entry_blocks(E)), dim3(256), 0, s, pr, x.cnt, x.tmp);
  hipLaunchKernelGGL(order_kernel<Prob>, dim3(entry_blocks(E)), dim3(256), 0, s, pr, x.off, x.tmp, x.sorted);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

// the keys and entries of one correlation backward (shapes only)
inline void corr_sizes(int64_t M, int64_t N1, int64_t N2, int P, int H2, int W2, int radius, int64_t& K, int64_t& E) {
  const Tiles t = make_tiles(H2, W2, 2 * radius + 2, CORR_BX, CORR_BY);
  K = N1 + N2 * t.TY * t.TX;
  E = M + M * P * P;
}

inline void patchify_sizes(int B, int64_t M, int H, int W, int radius, int64_t& K, int64_t& E) {
  const Tiles t = make_tiles(H, W, 2 * radius + 2, PATCH_BX, PATCH_BY);
  K = (int64_t)B * t.TY * t.TX;
  E = (int64_t)B * M;
}

constexpr int64_t INDEX_MAX = ((int64_t)1 << 31) - 1;

}  // namespace

extern "C" size_t cdv_corr_bwd_workspace_bytes(int64_t M, int64_t N1, int64_t N2, int P, int H2, int W2, int radius) {
  if (M < 0 || N1 < 0 || N2 < 0 || P <= 0 || H2 <= 0 || W2 <= 0 || radius < 0) return 0;
  int64_t K, E;
  corr_sizes(M, N1, N2, P, H2, W2, radius, K, E);
  return index_bytes(K, E);
}

extern "C" int cdv_corr_bwd(const float* fmap1, const float* fmap2, const float* coords, const int64_t* us,
                            const int64_t* vs, const float* grad, float* fmap1_grad, float* fmap2_grad, void* workspace,
                            int64_t M, int64_t N1, int64_t N2, int C, int P, int H2, int W2, int radius,
                            void* stream) {
  CDV_REQUIRE(C > 0 && P > 0 && radius >= 0 && H2 > 0 && W2 > 0 && M >= 0 && N1 >= 0 && N2 >= 0, CDV_ERR_ARG,
              "cdv_corr_bwd: bad shape");
  CDV_REQUIRE(fmap1 && fmap2 && workspace && (M == 0 || (coords && us && vs && grad)), CDV_ERR_ARG,
              "cdv_corr_bwd: NULL argument");
  const int D = 2 * radius + 2, PP = P * P;
  int64_t K, E;
  corr_sizes(M, N1, N2, P, H2, W2, radius, K, E);
  CDV_REQUIRE(K + 1 < INDEX_MAX && E < INDEX_MAX && M * PP < INDEX_MAX, CDV_ERR_ARG, "cdv_corr_bwd: too many entries");
  const size_t lds = (size_t)PP * D * D * sizeof(float) + 2 * (size_t)PP * sizeof(int);
  CDV_REQUIRE(lds <= 60 * 1024, CDV_ERR_UNSUPPORTED, "cdv_corr_bwd: P^2 (2r+2)^2 window gradient exceeds LDS");
  CDV_REQUIRE(fmap1_grad == nullptr || N1 * ((C * PP + BTHREADS - 1) / BTHREADS) < INDEX_MAX, CDV_ERR_ARG,
              "cdv_corr_bwd: too many fmap1 tiles");
  hipStream_t s = (hipStream_t)stream;
  CorrIdx ix;
  ix.coords = coords; ix.us = us; ix.vs = vs;
  ix.M = M; ix.N1 = N1; ix.N2 = N2;
  ix.P = P; ix.H2 = H2; ix.W2 = W2; ix.R = radius;
  ix.t = make_tiles(H2, W2, D, CORR_BX, CORR_BY);
  const Index x = carve(workspace, K, E);
  int rc = build_index(ix, x, K, E, s);
  if (rc != CDV_OK) return rc;
  CorrGather G;
  G.fmap1 = fmap1; G.fmap2 = fmap2; G.grad = grad; G.g1 = fmap1_grad; G.g2 = fmap2_grad; G.C = C;
  G.groups1 = (C * PP + BTHREADS - 1) / BTHREADS;
  G.nwg1 = fmap1_grad ? (int)(N1 * G.groups1) : 0;
  G.chunks2 = (C + CCH - 1) / CCH;
  const int64_t nwg2 = fmap2_grad ? N2 * ix.t.OTY * ix.t.OTX * G.chunks2 : 0;
  CDV_REQUIRE(G.nwg1 + nwg2 < INDEX_MAX, CDV_ERR_ARG, "cdv_corr_bwd: grid too large");
  G.nwg2 = (int)nwg2;
  const int64_t blocks = G.nwg1 + nwg2;
  // the sixth launch always runs (an empty grid gets one idle workgroup): a fixed launch count per call
  hipLaunchKernelGGL(corr_gather_kernel, dim3(blocks > 0 ? (unsigned)blocks : 1u), dim3(BTHREADS),
                     G.nwg1 > 0 ? lds : 0, s, ix, G, x.off, x.sorted);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

extern "C" size_t cdv_patchify_bwd_workspace_bytes(int B, int64_t M, int H, int W, int radius) {
  if (B < 0 || M < 0 || H <= 0 || W <= 0 || radius < 0) return 0;
  int64_t K, E;
  patchify_sizes(B, M, H, W, radius, K, E);
  return index_bytes(K, E);
}

extern "C" int cdv_patchify_bwd(const void* patch_grad, const float* coords, void* net_grad, void* workspace, int B,
                                int64_t M, int C, int H, int W, int radius, int dtype, void* stream) {
  CDV_REQUIRE(dtype == CDV_F16 || dtype == CDV_F32, CDV_ERR_UNSUPPORTED, "cdv_patchify_bwd: dtype must be f16 or f32");
  CDV_REQUIRE(B >= 0 && M >= 0 && C > 0 && H > 0 && W > 0 && radius >= 0, CDV_ERR_ARG, "cdv_patchify_bwd: bad shape");
  CDV_REQUIRE(net_grad && workspace && (B * M == 0 || (patch_grad && coords)), CDV_ERR_ARG,
              "cdv_patchify_bwd: NULL argument");
  if (B == 0) return CDV_OK;
  int64_t K, E;
  patchify_sizes(B, M, H, W, radius, K, E);
  CDV_REQUIRE(K + 1 < INDEX_MAX && E < INDEX_MAX, CDV_ERR_ARG, "cdv_patchify_bwd: too many entries");
  hipStream_t s = (hipStream_t)stream;
  PatchIdx ix;
  ix.coords = coords; ix.M = M; ix.B = B; ix.H = H; ix.W = W; ix.R = radius;
  ix.t = make_tiles(H, W, 2 * radius + 2, PATCH_BX, PATCH_BY);
  const Index x = carve(workspace, K, E);
  int rc = build_index(ix, x, K, E, s);
  if (rc != CDV_OK) return rc;
  const int chunks = (C + CCH - 1) / CCH;
  const int64_t blocks = (int64_t)B * ix.t.OTY * ix.t.OTX * chunks;
  CDV_REQUIRE(blocks < INDEX_MAX, CDV_ERR_ARG, "cdv_patchify_bwd: grid too large");
  if (dtype == CDV_F16)
    hipLaunchKernelGGL(patchify_gather_kernel<_Float16>, dim3((unsigned)blocks), dim3(BTHREADS), 0, s, ix,
                       (const _Float16*)patch_grad, (_Float16*)net_grad, C, chunks, x.off, x.sorted);
  else
    hipLaunchKernelGGL(patchify_gather_kernel<float>, dim3((unsigned)blocks), dim3(BTHREADS), 0, s, ix,
                       (const float*)patch_grad, (float*)net_grad, C, chunks, x.off, x.sorted);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}
