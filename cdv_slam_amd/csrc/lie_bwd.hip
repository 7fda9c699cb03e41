// lie_bwd.hip -- vector-Jacobian products of the batched SO3 / SE3 ops of lie.hip (lietorch_backends.*_backward), gfx950.
//
// Convention (DESIGN.md "The lietorch backward"): the gradient of a scalar L with respect to a group element X is the row
// vector dL/d eps at eps = 0 of L(Exp(eps) X), stored in the first K words of an N-word row (the last word is zero); the
// incoming gradient of a group-valued output is read the same way.  Tangents and points carry ordinary gradients.
//
// One lane per row of `grad`, fixed-size math in registers on cdv_se3.h.  One operand may be GROUPED: it has n / m rows and
// row i of the call uses its row i / m (one pose against its m points).  The kernel reads that row where it lies and writes
// the operand's gradient as [n / m] rows: every lane leaves its contribution in LDS, and one owner per output word adds the
// m of them in ascending row order.  No float atomics: the same bits at every run.
#include "cdv_common.h"
// No multiply-add contraction anywhere in this file, cdv_se3.h as compiled here included: contraction is decided per kernel
// after inlining, and a row's gradient must be the same bits whichever instantiation (grouped or not) computes it.
#pragma clang fp contract(off)
#include "cdv_se3.h"

namespace {

enum { OP_EXP = 0, OP_LOG, OP_INV, OP_MUL, OP_ADJ, OP_ADJT, OP_ACT, OP_ACT4, OP_MATRIX };
enum { GRP_NONE = 0, GRP_X = 1, GRP_Y = 2 };
enum { NEED_X = 1, NEED_Y = 2 };
constexpr int THREADS = 256;
constexpr int MAX_REP = 64;

// widths of the rows of an op: the inputs as stored, the incoming gradient as stored, and of each input's gradient the
// words that carry values (`k`) and the words stored (`w`: a group element's gradient is padded to N with a zero)
template <bool SE3, int OP>
struct Shape {
  static constexpr int N = SE3 ? 7 : 4, K = SE3 ? 6 : 3;
  static constexpr bool binary = OP == OP_MUL || OP == OP_ADJ || OP == OP_ADJT || OP == OP_ACT || OP == OP_ACT4;
  static constexpr int x = OP == OP_EXP ? K : N;
  static constexpr int y = OP == OP_MUL ? N : (OP == OP_ADJ || OP == OP_ADJT) ? K : OP == OP_ACT ? 3 : OP == OP_ACT4 ? 4 : 0;
  static constexpr bool group_out = OP == OP_EXP || OP == OP_INV || OP == OP_MUL;
  static constexpr int g = group_out ? N : OP == OP_ACT ? 3 : OP == OP_ACT4 ? 4 : K;
  static constexpr int gk = group_out ? K : g;     // words of the incoming gradient that are read
  static constexpr int xk = K, xw = OP == OP_EXP ? K : N;
  static constexpr int yk = OP == OP_MUL ? K : y, yw = y;
};

// (R, t) of a loaded element; t = 0 for SO3
template <typename T, bool SE3>
__device__ __forceinline__ void load_Rt(const T* X, T* R, T* t) {
  T q[4];
  if constexpr (SE3) {
    cdv::lt_se3_load(X, t, q);
  } else {
    t[0] = t[1] = t[2] = T(0);
    cdv::lt_quat_load(X, q);
  }
  cdv::lt_quat_to_R(q, R);
}

// row . Ad(X):  SO3 R^T row;  SE3 (R^T u, R^T (u x t + w))
template <typename T, bool SE3>
__device__ __forceinline__ void row_times_Ad(const T* R, const T* t, const T* row, T* o) {
  if constexpr (SE3) cdv::lt_se3_adjT_loaded(t, R, row, o); else cdv::mat3T_vec(R, row, o);
}

// Ad(X) a:  SO3 R a;  SE3 (R a1 + t x R a2, R a2)
template <typename T, bool SE3>
__device__ __forceinline__ void Ad_times(const T* R, const T* t, const T* a, T* o) {
  cdv::mat3_vec(R, a, o);
  if constexpr (SE3) {
    T c[3];
    cdv::mat3_vec(R, a + 3, o + 3);
    cdv::cross3(t, o + 3, c);
    o[0] += c[0]; o[1] += c[1]; o[2] += c[2];
  }
}

// the vector-Jacobian products of one row.  g: the incoming gradient's gk words; xr / yr: the inputs as stored; gx / gy: the
// xk / yk value words of the inputs' gradients (only those that `need` names are computed).
template <typename T, bool SE3, int OP>
__device__ __forceinline__ void lie_vjp(const T* g, const T* xr, const T* yr, int need, T* gx, T* gy) {
  constexpr int K = SE3 ? 6 : 3;
  if constexpr (OP == OP_EXP) {              // da = dX . Jl(a)
    if constexpr (SE3) {
      cdv::lt_se3_row_times_left_jacobian(xr, g, gx);
    } else {
      T J[9];
      cdv::lt_so3_left_jacobian(xr, J);
      cdv::mat3T_vec(J, g, gx);
    }
  } else if constexpr (OP == OP_LOG) {       // dX = da . Jl^-1(Log X)
    T a[K];
    if constexpr (SE3) {
      cdv::lt_se3_log(xr, a);
      cdv::lt_se3_row_times_left_jacobian_inverse(a, g, gx);
    } else {
      T Ji[9];
      cdv::lt_so3_log(xr, a);
      cdv::lt_so3_left_jacobian_inverse(a, Ji);
      cdv::mat3T_vec(Ji, g, gx);
    }
  } else {
    T R[9], t[3];
    load_Rt<T, SE3>(xr, R, t);
    if constexpr (OP == OP_INV) {            // dX = -dY . Ad(X^-1) = -(R u, t x R u + R w)
      cdv::mat3_vec(R, g, gx);
      if constexpr (SE3) {
        T c[3];
        cdv::mat3_vec(R, g + 3, gx + 3);
        cdv::cross3(t, gx, c);
        gx[3] += c[0]; gx[4] += c[1]; gx[5] += c[2];
      }
#pragma unroll
      for (int c = 0; c < K; c++) gx[c] = -gx[c];
    } else if constexpr (OP == OP_MUL) {     // dX = dZ, dY = dZ . Ad(X)
#pragma unroll
      for (int c = 0; c < K; c++) gx[c] = g[c];
      if (need & NEED_Y) row_times_Ad<T, SE3>(R, t, g, gy);
    } else if constexpr (OP == OP_ADJ) {     // b = Ad(X) a:  da = db . Ad(X), dX = -db . ad(b)
      if (need & NEED_Y) row_times_Ad<T, SE3>(R, t, g, gy);
      if (need & NEED_X) {
        T b[K];
        Ad_times<T, SE3>(R, t, yr, b);
        cdv::lt_neg_row_times_ad<T, SE3>(g, b, gx);
      }
    } else if constexpr (OP == OP_ADJT) {    // b = Ad(X)^T a, c = Ad(X) db:  da = c^T, dX = -a . ad(c)
      Ad_times<T, SE3>(R, t, g, gy);
      if (need & NEED_X) cdv::lt_neg_row_times_ad<T, SE3>(yr, gy, gx);
    } else {                                 // q = X p:  dp = dq . M, dX = dq . d(Exp(eps) q) / d eps
      T q[3], c[3];
      cdv::mat3_vec(R, yr, q);
      T w = T(1);
      if constexpr (OP == OP_ACT4) w = yr[3];
      if constexpr (SE3) { q[0] += w * t[0]; q[1] += w * t[1]; q[2] += w * t[2]; }
      if (need & NEED_Y) {
        cdv::mat3T_vec(R, g, gy);
        if constexpr (OP == OP_ACT4) gy[3] = g[3] + (SE3 ? g[0] * t[0] + g[1] * t[1] + g[2] * t[2] : T(0));
      }
      cdv::cross3(q, g, c);                  // -dq . [q]x
      if constexpr (SE3) {
        gx[0] = w * g[0]; gx[1] = w * g[1]; gx[2] = w * g[2];
        gx[3] = c[0]; gx[4] = c[1]; gx[5] = c[2];
      } else {
        gx[0] = c[0]; gx[1] = c[1]; gx[2] = c[2];
      }
    }
  }
}

// GRP_NONE: lane = row.  GRP_X / GRP_Y: a workgroup serves `groups` = THREADS / m whole groups (groups * m lanes work), so
// that every sum stays inside it.
template <typename T, bool SE3, int OP, int GRP>
__global__ __launch_bounds__(THREADS) void lie_bwd_kernel(int64_t n, int m, int need, const T* __restrict__ grad,
                                                          const T* __restrict__ x, const T* __restrict__ y,
                                                          T* __restrict__ dx, T* __restrict__ dy) {
  using S = Shape<SE3, OP>;
  const int lane = threadIdx.x;
  const int groups = GRP == GRP_NONE ? 0 : THREADS / m;
  const int64_t first_group = (int64_t)blockIdx.x * groups;
  const int64_t row = GRP == GRP_NONE ? (int64_t)blockIdx.x * THREADS + lane : first_group * m + lane;
  const bool active = row < n && (GRP == GRP_NONE || lane < groups * m);
  const int64_t shared_row = GRP == GRP_NONE ? row : first_group + lane / m;
  const int64_t xrow = GRP == GRP_X ? shared_row : row, yrow = GRP == GRP_Y ? shared_row : row;

  T gx[S::xk], gy[S::yk > 0 ? S::yk : 1];
  if (active) {
    T g[S::gk], xr[S::x], yr[S::y > 0 ? S::y : 1];
#pragma unroll
    for (int c = 0; c < S::gk; c++) g[c] = grad[S::g * row + c];
#pragma unroll
    for (int c = 0; c < S::x; c++) xr[c] = x[S::x * xrow + c];
#pragma unroll
    for (int c = 0; c < S::y; c++) yr[c] = y[S::y * yrow + c];
    lie_vjp<T, SE3, OP>(g, xr, yr, need, gx, gy);
    if (GRP != GRP_X && (need & NEED_X)) {
#pragma unroll
      for (int c = 0; c < S::xw; c++) dx[S::xw * row + c] = c < S::xk ? gx[c] : T(0);
    }
    if (S::binary && GRP != GRP_Y && (need & NEED_Y)) {
#pragma unroll
      for (int c = 0; c < S::yw; c++) dy[S::yw * row + c] = c < S::yk ? gy[c] : T(0);
    }
  }
  if constexpr (GRP != GRP_NONE) {
    constexpr int SK = GRP == GRP_X ? S::xk : S::yk, SW = GRP == GRP_X ? S::xw : S::yw;
    if (!(need & (GRP == GRP_X ? NEED_X : NEED_Y))) return;      // the same for every lane
    __shared__ T part[6 * THREADS];                               // [word][lane]
    if (active) {
#pragma unroll
      for (int c = 0; c < SK; c++) part[c * THREADS + lane] = GRP == GRP_X ? gx[c] : gy[c];
    }
    __syncthreads();
    T* out = GRP == GRP_X ? dx : dy;
    const int64_t n_groups = n / m;
    for (int idx = lane; idx < groups * SW; idx += THREADS) {
      const int gl = idx / SW, c = idx - gl * SW;
      if (first_group + gl >= n_groups) break;
      T sum = T(0);
      if (c < SK) {
        const T* p = part + c * THREADS + gl * m;
        sum = p[0];
        for (int j = 1; j < m; j++) sum += p[j];
      }
      out[(first_group + gl) * SW + c] = sum;
    }
  }
}

template <typename T, bool SE3, int OP>
void launch_one(int grp, int64_t n, int m, int need, const T* grad, const T* x, const T* y, T* dx, T* dy, hipStream_t s) {
  if (grp == GRP_NONE) {
    hipLaunchKernelGGL((lie_bwd_kernel<T, SE3, OP, GRP_NONE>), dim3(cdv_div_up(n, THREADS)), dim3(THREADS), 0, s, n, 1, need,
                       grad, x, y, dx, dy);
    return;
  }
  if constexpr (Shape<SE3, OP>::binary) {
    const int blocks = cdv_div_up(n / m, THREADS / m);
    if (grp == GRP_X)
      hipLaunchKernelGGL((lie_bwd_kernel<T, SE3, OP, GRP_X>), dim3(blocks), dim3(THREADS), 0, s, n, m, need, grad, x, y, dx, dy);
    else
      hipLaunchKernelGGL((lie_bwd_kernel<T, SE3, OP, GRP_Y>), dim3(blocks), dim3(THREADS), 0, s, n, m, need, grad, x, y, dx, dy);
  }
}

template <typename T, bool SE3>
int launch_bwd(const cdv_lie_bwd_args& a, int grp, int m, hipStream_t s) {
#define CDV_LIE_BWD_CASE(O)                                                                                          \
  case O:                                                                                                            \
    launch_one<T, SE3, O>(grp, a.n, m, a.need, (const T*)a.grad, (const T*)a.x, (const T*)a.y, (T*)a.dx, (T*)a.dy, s); \
    break;
  switch (a.op) {
    CDV_LIE_BWD_CASE(OP_EXP)
    CDV_LIE_BWD_CASE(OP_LOG)
    CDV_LIE_BWD_CASE(OP_INV)
    CDV_LIE_BWD_CASE(OP_MUL)
    CDV_LIE_BWD_CASE(OP_ADJ)
    CDV_LIE_BWD_CASE(OP_ADJT)
    CDV_LIE_BWD_CASE(OP_ACT)
    CDV_LIE_BWD_CASE(OP_ACT4)
  }
#undef CDV_LIE_BWD_CASE
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

}  // namespace

extern "C" int cdv_lie_bwd(const cdv_lie_bwd_args* args, void* stream) {
  CDV_REQUIRE(args != nullptr, CDV_ERR_ARG, "cdv_lie_bwd: args is NULL");
  const cdv_lie_bwd_args a = *args;
  CDV_REQUIRE(a.group == 1 || a.group == 3, CDV_ERR_UNSUPPORTED,
              "cdv_lie_bwd: only SO3 (1) and SE3 (3) are served; RxSO3/Sim3 are out of scope");
  CDV_REQUIRE(a.dtype == CDV_F32 || a.dtype == CDV_F64, CDV_ERR_UNSUPPORTED, "cdv_lie_bwd: dtype must be f32 or f64");
  CDV_REQUIRE(a.op != OP_MATRIX, CDV_ERR_ARG, "cdv_lie_bwd: as_matrix has no backward");
  CDV_REQUIRE(a.op >= OP_EXP && a.op <= OP_ACT4, CDV_ERR_ARG, "cdv_lie_bwd: unknown op");
  const bool binary = a.op >= OP_MUL;
  CDV_REQUIRE(a.n >= 0 && a.rep_x >= 1 && a.rep_y >= 1, CDV_ERR_ARG, "cdv_lie_bwd: n >= 0 and rep >= 1");
  CDV_REQUIRE(a.rep_x == 1 || a.rep_y == 1, CDV_ERR_ARG, "cdv_lie_bwd: at most one grouped operand");
  CDV_REQUIRE(a.rep_x <= MAX_REP && a.rep_y <= MAX_REP, CDV_ERR_ARG,
              "cdv_lie_bwd: a grouped operand repeats at most 64 times (expand it and sum outside)");
  CDV_REQUIRE(a.n % a.rep_x == 0 && a.n % a.rep_y == 0, CDV_ERR_ARG, "cdv_lie_bwd: n must be a multiple of rep");
  CDV_REQUIRE(binary || (a.rep_x == 1 && a.rep_y == 1), CDV_ERR_ARG, "cdv_lie_bwd: a grouped operand needs a binary op");
  const int need = a.need & (binary ? (NEED_X | NEED_Y) : NEED_X);
  if (a.n == 0) return CDV_OK;               // nothing to write: an empty tensor's pointer may be NULL
  CDV_REQUIRE(!(need & NEED_X) || a.dx != nullptr, CDV_ERR_ARG, "cdv_lie_bwd: dx is needed and NULL");
  CDV_REQUIRE(!(need & NEED_Y) || a.dy != nullptr, CDV_ERR_ARG, "cdv_lie_bwd: dy is needed and NULL");
  if (need == 0) return CDV_OK;
  CDV_REQUIRE(a.grad != nullptr && a.x != nullptr && (!binary || a.y != nullptr), CDV_ERR_ARG,
              "cdv_lie_bwd: grad, x (and y of a binary op) must be given");
  cdv_lie_bwd_args b = a;
  b.need = need;
  const int grp = a.rep_x > 1 ? GRP_X : a.rep_y > 1 ? GRP_Y : GRP_NONE;
  const int m = (int)(a.rep_x > 1 ? a.rep_x : a.rep_y);
  hipStream_t s = (hipStream_t)stream;
  if (a.dtype == CDV_F32) return a.group == 3 ? launch_bwd<float, true>(b, grp, m, s) : launch_bwd<float, false>(b, grp, m, s);
  return a.group == 3 ? launch_bwd<double, true>(b, grp, m, s) : launch_bwd<double, false>(b, grp, m, s);
}
