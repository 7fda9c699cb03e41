// altcorr_fwd.hip -- the reference-shaped per-level forward operators of altcorr (their backward passes: corr_bwd.hip).
//
// Reference: cuda_corr.forward = corr_forward_kernel (correlation_kernel.cu:82-136) plus the four slice-multiply-add
// passes of corr_cuda_forward (:193-233), here one pass (cdv_corr_fwd: planar layouts, any C / P / radius, f16 or f32);
// cuda_corr.patchify_forward (:16-47, :288-308) as cdv_patchify_fwd; altcorr.patchify with its blend (correlation.py:51-71)
// as cdv_patchify_blend, and several such calls on one set of patch centres as cdv_patchify_multi (net_cdv.py:355-374).
// None of these is on the hot path: the two-level correlation of an update is cdv_corr_fused (corr.hip).
#include "cdv_common.h"

namespace {

// ---- generic per-level kernel: planar layouts, any C / P / radius, f16 or f32 ----------------------
template <typename T>
__global__ __launch_bounds__(256) void corr_generic_kernel(const T* __restrict__ fmap1, const T* __restrict__ fmap2,
                                                           const float* __restrict__ coords,
                                                           const int64_t* __restrict__ us,
                                                           const int64_t* __restrict__ vs, T* __restrict__ out,
                                                           int64_t M, int64_t N1, int64_t N2, int C, int P, int H2,
                                                           int W2, int R) {
  const int D1 = 2 * R + 1;
  const int64_t total = M * D1 * D1 * P * P;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = idx;
    const int j0 = (int)(t % P); t /= P;
    const int i0 = (int)(t % P); t /= P;
    const int yo = (int)(t % D1); t /= D1;
    const int xo = (int)(t % D1); t /= D1;
    const int64_t m = t;
    const int64_t ix = us[m], jx = vs[m];
    const float x = coords[((m * 2 + 0) * P + i0) * P + j0];
    const float y = coords[((m * 2 + 1) * P + i0) * P + j0];
    const float fxf = floorf(x), fyf = floorf(y);
    const float dx = (float)(T)(x - fxf), dy = (float)(T)(y - fyf);
    const int fx = (int)fminf(fmaxf(fxf, -1.0e6f), 1.0e6f), fy = (int)fminf(fmaxf(fyf, -1.0e6f), 1.0e6f);
    float c[2][2];
    const bool idx_ok = ix >= 0 && ix < N1 && jx >= 0 && jx < N2;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int i1 = fy + yo + a - R, j1 = fx + xo + b - R;
        float s = 0.f;
        if (idx_ok && i1 >= 0 && i1 < H2 && j1 >= 0 && j1 < W2) {
          const T* p1 = fmap1 + ((ix * C) * P + i0) * P + j0;
          const T* p2 = fmap2 + ((jx * C) * (int64_t)H2 + i1) * W2 + j1;
          for (int ch = 0; ch < C; ch++) s += (float)p1[(int64_t)ch * P * P] * (float)p2[(int64_t)ch * H2 * W2];
        }
        c[a][b] = s;
      }
    const float v = (1.f - dx) * (1.f - dy) * c[0][0] + dx * (1.f - dy) * c[0][1] + (1.f - dx) * dy * c[1][0] +
                    dx * dy * c[1][1];
    out[idx] = (T)v;
  }
}

// patchify forward (correlation_kernel.cu:16-47): gather (2R+2)^2 tiles, zero when OOB
template <typename T>
__global__ __launch_bounds__(256) void patchify_kernel(const T* __restrict__ net, const float* __restrict__ coords,
                                                       T* __restrict__ patches, int B, int64_t M, int C, int H, int W,
                                                       int R) {
  const int D = 2 * R + 2;
  const int64_t total = (int64_t)B * M * C * D * D;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = idx;
    const int b2 = (int)(t % D); t /= D;
    const int a2 = (int)(t % D); t /= D;
    const int ch = (int)(t % C); t /= C;
    const int64_t m = t % M; t /= M;
    const int bb = (int)t;
    const float x = coords[(bb * M + m) * 2 + 0], y = coords[(bb * M + m) * 2 + 1];
    const int i = (int)fminf(fmaxf(floorf(y), -1.0e6f), 1.0e6f) + (a2 - R);
    const int j = (int)fminf(fmaxf(floorf(x), -1.0e6f), 1.0e6f) + (b2 - R);
    T v = (T)0.f;
    if (i >= 0 && i < H && j >= 0 && j < W) v = net[(((int64_t)bb * C + ch) * H + i) * W + j];
    patches[idx] = v;
  }
}

// altcorr.patchify(net, coords, radius, mode) (correlation.py:51-71) in one pass: mode 1 = 'bilinear' (the (2r+2)^2
// gather of patchify_forward blended to (2r+1)^2 with the sub-pixel offset of the patch centre, in the reference's
// operation order x00 + x01 + x10 + x11), mode 2 = 'upperleft' (the 1x1 corner tile).  Out-of-image taps are zero.
// (the blend multiplies float32 offsets into the tile, so torch's type promotion makes the 'bilinear' result float32
// whatever the map's dtype; 'upperleft' is a slice and keeps the dtype)
template <typename T>
__global__ __launch_bounds__(256) void patchify_blend_kernel(const T* __restrict__ net, const float* __restrict__ coords,
                                                             void* __restrict__ outv, int B, int64_t M, int C, int H,
                                                             int W, int R, int mode) {
  const int d = (mode == 2) ? 1 : 2 * R + 1;
  const int64_t total = (int64_t)B * M * C * d * d;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
       idx += (int64_t)gridDim.x * blockDim.x) {
    int64_t t = idx;
    const int b2 = (int)(t % d); t /= d;
    const int a2 = (int)(t % d); t /= d;
    const int ch = (int)(t % C); t /= C;
    const int64_t m = t % M; t /= M;
    const int bb = (int)t;
    const float x = coords[(bb * M + m) * 2 + 0], y = coords[(bb * M + m) * 2 + 1];
    const float fxf = floorf(x), fyf = floorf(y);
    const int i0 = (int)fminf(fmaxf(fyf, -1.0e6f), 1.0e6f) + (a2 - R);
    const int j0 = (int)fminf(fmaxf(fxf, -1.0e6f), 1.0e6f) + (b2 - R);
    const T* np = net + ((int64_t)bb * C + ch) * H * W;
    auto tap = [&](int i, int j) -> T { return (i >= 0 && i < H && j >= 0 && j < W) ? np[(int64_t)i * W + j] : (T)0.f; };
    if (mode == 2) {
      reinterpret_cast<T*>(outv)[idx] = tap(i0, j0);
    } else {
      const float dx = x - fxf, dy = y - fyf;   // correlation.py:58-66, same operation order
      const float x00 = (1.0f - dy) * (1.0f - dx) * (float)tap(i0, j0);
      const float x01 = (1.0f - dy) * dx * (float)tap(i0, j0 + 1);
      const float x10 = dy * (1.0f - dx) * (float)tap(i0 + 1, j0);
      const float x11 = dy * dx * (float)tap(i0 + 1, j0 + 1);
      reinterpret_cast<float*>(outv)[idx] = ((x00 + x01) + x10) + x11;
    }
  }
}

// Several altcorr.patchify calls on ONE set of patch centres in one launch: a new frame's imap / gmap / colour / patch
// tiles (net_cdv.py:355-374).  Job j reads its own map at (coords + o_j) * s_j -- the scaling the reference applies with
// torch ops before each call (scale_f2i * coords, 4 * (coords + 0.5)), same two float operations -- with its own radius,
// mode and dtype; workgroups [first[j], first[j + 1]) belong to job j.
struct PatchifyJobs {
  cdv_patchify_job j[CDV_MAX_PATCHIFY_JOBS];
  int first[CDV_MAX_PATCHIFY_JOBS + 1];
  int n_jobs;
};

template <typename T>
__device__ __forceinline__ void patchify_job_body(const cdv_patchify_job& J, const float* __restrict__ coords, int64_t M,
                                                  int64_t idx0, int64_t stride) {
  const int R = J.radius, mode = J.mode, C = J.C, H = J.H, W = J.W;
  const int d = (mode == 2) ? 1 : 2 * R + 1;
  const int64_t total = M * C * d * d;
  const T* net = reinterpret_cast<const T*>(J.net);
  for (int64_t idx = idx0; idx < total; idx += stride) {
    int64_t t = idx;
    const int b2 = (int)(t % d); t /= d;
    const int a2 = (int)(t % d); t /= d;
    const int ch = (int)(t % C); t /= C;
    const int64_t m = t;
    const float x = (coords[m * 2 + 0] + J.ox) * J.sx, y = (coords[m * 2 + 1] + J.oy) * J.sy;
    const float fxf = floorf(x), fyf = floorf(y);
    const int i0 = (int)fminf(fmaxf(fyf, -1.0e6f), 1.0e6f) + (a2 - R);
    const int j0 = (int)fminf(fmaxf(fxf, -1.0e6f), 1.0e6f) + (b2 - R);
    const T* np = net + (int64_t)ch * H * W;
    auto tap = [&](int i, int j) -> T { return (i >= 0 && i < H && j >= 0 && j < W) ? np[(int64_t)i * W + j] : (T)0.f; };
    if (mode == 2) {
      reinterpret_cast<T*>(J.out)[idx] = tap(i0, j0);
    } else {
      const float dx = x - fxf, dy = y - fyf;   // correlation.py:58-66, same operation order
      const float x00 = (1.0f - dy) * (1.0f - dx) * (float)tap(i0, j0);
      const float x01 = (1.0f - dy) * dx * (float)tap(i0, j0 + 1);
      const float x10 = dy * (1.0f - dx) * (float)tap(i0 + 1, j0);
      const float x11 = dy * dx * (float)tap(i0 + 1, j0 + 1);
      reinterpret_cast<float*>(J.out)[idx] = ((x00 + x01) + x10) + x11;
    }
  }
}

__global__ __launch_bounds__(256) void patchify_multi_kernel(const PatchifyJobs P, const float* __restrict__ coords,
                                                             int64_t M) {
  int ji = 0;
  while (ji + 1 < P.n_jobs && (int)blockIdx.x >= P.first[ji + 1]) ji++;
  const cdv_patchify_job& J = P.j[ji];
  const int nb = P.first[ji + 1] - P.first[ji];
  const int64_t idx0 = (int64_t)((int)blockIdx.x - P.first[ji]) * 256 + threadIdx.x, stride = (int64_t)nb * 256;
  if (J.dtype == CDV_F16) patchify_job_body<_Float16>(J, coords, M, idx0, stride);
  else patchify_job_body<float>(J, coords, M, idx0, stride);
}

}  // namespace

extern "C" int cdv_patchify_multi(const cdv_patchify_job* jobs, int n_jobs, const float* coords, int64_t M, void* stream) {
  CDV_REQUIRE(n_jobs >= 0 && n_jobs <= CDV_MAX_PATCHIFY_JOBS, CDV_ERR_ARG, "cdv_patchify_multi: too many jobs");
  if (n_jobs == 0 || M == 0) return CDV_OK;
  CDV_REQUIRE(jobs != nullptr && coords != nullptr && M > 0, CDV_ERR_ARG, "cdv_patchify_multi: NULL argument");
  PatchifyJobs P;
  P.n_jobs = n_jobs;
  P.first[0] = 0;
  for (int i = 0; i < n_jobs; i++) {
    const cdv_patchify_job& J = jobs[i];
    CDV_REQUIRE(J.dtype == CDV_F16 || J.dtype == CDV_F32, CDV_ERR_UNSUPPORTED, "cdv_patchify_multi: dtype must be f16 or f32");
    CDV_REQUIRE(J.mode == 1 || J.mode == 2, CDV_ERR_ARG, "cdv_patchify_multi: mode 1 (bilinear) or 2 (upperleft)");
    CDV_REQUIRE(J.net && J.out && J.C > 0 && J.H > 0 && J.W > 0 && J.radius >= 0, CDV_ERR_ARG, "cdv_patchify_multi: bad job");
    const int d = (J.mode == 2) ? 1 : 2 * J.radius + 1;
    const int64_t total = M * J.C * d * d;
    P.j[i] = J;
    P.first[i + 1] = P.first[i] + (int)(cdv_div_up(total, 256) < 4096 ? cdv_div_up(total, 256) : 4096);
  }
  hipLaunchKernelGGL(patchify_multi_kernel, dim3(P.first[n_jobs]), dim3(256), 0, (hipStream_t)stream, P, coords, M);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

extern "C" int cdv_patchify_blend(const void* net, const float* coords, void* out, int B, int64_t M, int C, int H, int W,
                                  int radius, int mode, int dtype, void* stream) {
  CDV_REQUIRE(dtype == CDV_F16 || dtype == CDV_F32, CDV_ERR_UNSUPPORTED, "cdv_patchify_blend: dtype must be f16 or f32");
  CDV_REQUIRE(mode == 1 || mode == 2, CDV_ERR_ARG, "cdv_patchify_blend: mode 1 (bilinear) or 2 (upperleft)");
  const int d = (mode == 2) ? 1 : 2 * radius + 1;
  const int64_t total = (int64_t)B * M * C * d * d;
  if (total == 0) return CDV_OK;
  const int blocks = cdv_div_up(total, 256) < 16384 ? cdv_div_up(total, 256) : 16384;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == CDV_F16)
    hipLaunchKernelGGL(patchify_blend_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, (const _Float16*)net, coords, out,
                       B, M, C, H, W, radius, mode);
  else
    hipLaunchKernelGGL(patchify_blend_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)net, coords, out, B, M,
                       C, H, W, radius, mode);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

extern "C" int cdv_corr_fwd(const void* fmap1, const void* fmap2, const float* coords, const int64_t* us,
                            const int64_t* vs, void* out, int64_t M, int64_t N1, int64_t N2, int C, int P, int H2,
                            int W2, int radius, int dtype, void* stream) {
  CDV_REQUIRE(dtype == CDV_F16 || dtype == CDV_F32, CDV_ERR_UNSUPPORTED, "cdv_corr_fwd: dtype must be f16 or f32");
  CDV_REQUIRE(C > 0 && P > 0 && radius >= 0 && H2 > 0 && W2 > 0, CDV_ERR_ARG, "cdv_corr_fwd: bad shape");
  if (M == 0) return CDV_OK;
  const int D1 = 2 * radius + 1;
  const int64_t total = M * D1 * D1 * P * P;
  const int blocks = cdv_div_up(total, 256) < 65536 ? cdv_div_up(total, 256) : 65536;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == CDV_F16)
    hipLaunchKernelGGL(corr_generic_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, (const _Float16*)fmap1,
                       (const _Float16*)fmap2, coords, us, vs, (_Float16*)out, M, N1, N2, C, P, H2, W2, radius);
  else
    hipLaunchKernelGGL(corr_generic_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)fmap1,
                       (const float*)fmap2, coords, us, vs, (float*)out, M, N1, N2, C, P, H2, W2, radius);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}

extern "C" int cdv_patchify_fwd(const void* net, const float* coords, void* patches, int B, int64_t M, int C, int H,
                                int W, int radius, int dtype, void* stream) {
  CDV_REQUIRE(dtype == CDV_F16 || dtype == CDV_F32, CDV_ERR_UNSUPPORTED, "cdv_patchify_fwd: dtype must be f16 or f32");
  const int D = 2 * radius + 2;
  const int64_t total = (int64_t)B * M * C * D * D;
  if (total == 0) return CDV_OK;
  const int blocks = cdv_div_up(total, 256) < 16384 ? cdv_div_up(total, 256) : 16384;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == CDV_F16)
    hipLaunchKernelGGL(patchify_kernel<_Float16>, dim3(blocks), dim3(256), 0, s, (const _Float16*)net, coords,
                       (_Float16*)patches, B, M, C, H, W, radius);
  else
    hipLaunchKernelGGL(patchify_kernel<float>, dim3(blocks), dim3(256), 0, s, (const float*)net, coords,
                       (float*)patches, B, M, C, H, W, radius);
  CDV_LAUNCH_CHECK();
  return CDV_OK;
}
