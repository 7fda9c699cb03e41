// ba.hip -- fastba: Schur-reduced Gauss-Newton bundle adjustment over the patch graph, gfx950: the entry point
// cdv_ba_forward (replaces cuda_ba.forward, cdvslam/fastba/ba.cpp:31-45, ba_cuda.cu:462-611).  Top to bottom: the host
// record of a workspace, cdv_ba_workspace_*, the argument checks, zeroing when the workspace is fresh, the dispatch to one
// of three *_iteration functions, and the status words.  No kernel but the zeroing one lives here.
//
// Dispatch on the number of free poses N:
//   1 <= N <= 10    ba_win.hip   two launches per iteration, no float atomics, bitwise reproducible
//   10 < N <= 32    ba_mid.hip   three launches per iteration, the same properties
//   N > 32 (<=1024) ba_big.hip   dense E in HBM, Schur products on the matrix cores, blocked multi-workgroup Cholesky; one
//                                owner and a fixed order for every sum there too
//   N = 0           ba_big.hip   patch + q + retract: depths alone.

#include <atomic>
#include <mutex>
#include <unordered_map>

#include "cdv_ba.h"

using namespace cdv;

namespace {

struct WsState {
  bool valid = false;
  int64_t U_max = 0;
  int N = 0;
  size_t bytes = 0;
  int32_t token = 0;  // last hand-off tag handed to a launch on this workspace (window path)
};
// What the library remembers about a bundle-adjustment workspace, by workspace ADDRESS.  Who sets a field and what clears it:
//   st        written by every cdv_ba_forward that gets past its size checks (valid from then on: the accumulators in the
//             workspace are zero for this (U_max, N, bytes)); reset by cdv_ba_workspace_init, after which the next call
//             zeroes again and cdv_ba_status answers that no call has run
//   counters  set by cdv_ba_bind_status_counters (NULL unbinds), survives cdv_ba_workspace_init
//   ppf       set by cdv_ba_set_patches_per_frame (0 forgets), survives cdv_ba_workspace_init
// Binding counters or ppf on an address without state makes an entry whose st.valid is false.  cdv_workspace_forget erases
// the entry and with it every field.
struct BaWsEntry {
  WsState st;
  int32_t* counters = nullptr;
  int ppf = 0;
};
std::mutex g_ws_mutex;
std::unordered_map<const void*, BaWsEntry> g_ws;
std::atomic<int> g_handoff_test{0};                        // cdv_ba_test_handoff: fault injection for the in-launch hand-offs

// what a workspace's first call zeroes (accumulators, status words, hand-off words), as a kernel
__global__ __launch_bounds__(256) void ba_zero_kernel(uint32_t* __restrict__ p, int64_t n4) {
  typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
  const int64_t nv = n4 >> 2;
  u32x4* p4 = reinterpret_cast<u32x4*>(p);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) p4[i] = u32x4{0u, 0u, 0u, 0u};
  if (blockIdx.x == 0 && threadIdx.x < (n4 & 3)) p[4 * nv + threadIdx.x] = 0u;
}

}  // namespace

// The library remembers, per workspace ADDRESS, that it has initialised the accumulators in it.  A caller that frees a
// workspace and later gets the same address back from its allocator (torch's caching allocator does that) must say so,
// or stale bytes would be taken for zeroed accumulators.
extern "C" void cdv_workspace_forget(const void* ws) {
  {
    std::lock_guard<std::mutex> lk(g_ws_mutex);
    g_ws.erase(ws);
  }
  cdv_graph_forget(ws);
}

// Explicit initialisation (instead of "the first time the library sees this address"): whoever allocates a workspace says so.
// The bundle-adjustment workspace needs nothing but to be unknown to the library: the first cdv_ba_forward then zeroes what
// it keeps zero; the status counters stay bound across a re-initialisation.
extern "C" int cdv_ba_workspace_init(void* ba_ws, void* stream) {
  (void)stream;
  CDV_REQUIRE(ba_ws != nullptr, CDV_ERR_ARG, "cdv_ba_workspace_init: workspace is NULL");
  std::lock_guard<std::mutex> lk(g_ws_mutex);
  auto it = g_ws.find(ba_ws);
  if (it != g_ws.end()) it->second.st = WsState{};
  return CDV_OK;
}

extern "C" size_t cdv_ba_workspace_bytes(int64_t E_max, int64_t U_max, int N_max) {
  if (E_max < 1) E_max = 1;
  if (U_max < 1) U_max = 1;
  if (N_max < 1) N_max = 1;
  if (N_max > BA_NBIG) N_max = BA_NBIG;
  return ba_layout(U_max, N_max, E_max).total;
}

// Arguments of one call, as the two entry points hand them on.  What an entry point does not set keeps the value of the plain
// cdv_ba_forward: no debug dump, the window on the host, the index looked up here.
struct BaCall {
  float *poses = nullptr, *patches = nullptr;
  const float *intrinsics = nullptr, *target = nullptr, *weight = nullptr, *lmbda = nullptr;
  const int64_t *ii = nullptr, *jj = nullptr, *kk = nullptr;
  int64_t E = 0;
  int P = 0, t0 = 0, t1 = 0, iterations = 0;
  const void* graph_ws = nullptr;
  const GraphInfo* graph = nullptr;   // the caller's snapshot of graph_ws, when it has taken one for its own checks
  void* ba_ws = nullptr;
  size_t ba_ws_bytes = 0;
  int64_t U_max = 0;
  float* dbg = nullptr;
  void* stream = nullptr;
  const int32_t* dyn = nullptr;
};

static int ba_forward_impl(const BaCall& c) {
  const int64_t E = c.E, U_max = c.U_max;
  const int P = c.P, t0 = c.t0, iterations = c.iterations;
  void* const ba_ws = c.ba_ws;
  const int N = c.t1 - t0;
  CDV_REQUIRE(N >= 0, CDV_ERR_ARG, "cdv_ba_forward: t1 < t0");
  CDV_REQUIRE(N <= BA_NBIG, CDV_ERR_UNSUPPORTED, "cdv_ba_forward: more than 1024 free poses");
  const bool big = N > BA_NMAX;   // global BA: panel-sparse Schur products + blocked multi-workgroup Cholesky
  CDV_REQUIRE(P == 3 || P == 1, CDV_ERR_UNSUPPORTED, "cdv_ba_forward: patch size P must be 3 or 1");
  CDV_REQUIRE(E >= 0 && E < ((int64_t)1 << 31), CDV_ERR_ARG, "cdv_ba_forward: E out of range");
  CDV_REQUIRE_ALIGNED(c.target, 8, "cdv_ba_forward: target must be 8-byte aligned");      // a row is loaded as one float2
  CDV_REQUIRE_ALIGNED(c.weight, 8, "cdv_ba_forward: weight must be 8-byte aligned");
  CDV_REQUIRE_ALIGNED(ba_ws, 16, "cdv_ba_forward: ba_ws must be 16-byte aligned");
  if (E == 0 || iterations <= 0) return CDV_OK;
  GraphInfo gi_here;   // ONE snapshot of the index registry per call: layout, form and capacity describe the same build
  if (!c.graph) CDV_REQUIRE(cdv_graph_info(c.graph_ws, &gi_here), CDV_ERR_ARG, "cdv_ba_forward: graph_ws has no built graph");
  const GraphInfo& gi = c.graph ? *c.graph : gi_here;
  CDV_REQUIRE(gi.L.E_max >= E, CDV_ERR_ARG, "cdv_ba_forward: graph was built for fewer edges");
  const GraphView gv = graph_view((void*)c.graph_ws, gi.L);
  CDV_REQUIRE(U_max >= 1, CDV_ERR_ARG, "cdv_ba_forward: U_max must be >= 1");
  const BaLayout L = ba_layout(U_max, N > 0 ? N : 1, E);
  CDV_REQUIRE(L.total <= c.ba_ws_bytes, CDV_ERR_WORKSPACE, "cdv_ba_forward: workspace too small for (U_max, N)");
  char* b = (char*)ba_ws;
  int32_t* info = (int32_t*)(b + L.info);
  hipStream_t s = (hipStream_t)c.stream;

  // The accumulators are zeroed once per (workspace, U_max, N): afterwards the solve / retract kernels leave
  // them zero, so the steady-state call enqueues no memset.
  bool fresh;
  int32_t token_base = 0;
  int32_t* counters = nullptr;
  int ppf_hint = 0;
  {
    std::lock_guard<std::mutex> lk(g_ws_mutex);
    BaWsEntry& w = g_ws[ba_ws];
    WsState& st = w.st;
    fresh = !(st.valid && st.U_max == U_max && st.N == N && st.bytes == c.ba_ws_bytes);
    token_base = (fresh || st.token > 0x7ffffff0 - 4 * iterations) ? 0 : st.token;
    st.valid = true; st.U_max = U_max; st.N = N; st.bytes = c.ba_ws_bytes;
    st.token = token_base + iterations;
    counters = w.counters;
    ppf_hint = w.ppf;
  }
  // the slab paths: two launches per iteration, no float atomics (ba_win.hip up to 10 free poses, ba_mid.hip up to 32)
  const bool window = N >= 1 && N <= MID_N;
  const bool table = gi.table;
  CDV_REQUIRE(!table || window, CDV_ERR_UNSUPPORTED,
              "cdv_ba_forward: graph_ws holds a patch table (cdv_graph_build_table), which serves 1 .. 32 free poses; build "
              "the ranked index (cdv_graph_build_edges) for the global bundle adjustment");
  if (fresh) {   // (zeroing KERNELS, not hipMemsetAsync: a first call made under stream capture leaves kernel nodes only)
    const auto zero = [&](void* p, size_t bytes) {   // every area starts 256-byte aligned (ba_layout) and is a multiple of 4 bytes
      const size_t n4 = bytes / 4;
      if (n4 == 0) return;
      const int grid = (int)(cdv_div_up((int64_t)n4, 1024) < 4096 ? cdv_div_up((int64_t)n4, 1024) : 4096);
      hipLaunchKernelGGL(ba_zero_kernel, dim3(grid), dim3(256), 0, s, (uint32_t*)p, (int64_t)n4);
    };
    if (!window) zero(b + L.sy, L.zero_bytes);   // the window path keeps no accumulators
    zero(info, sizeof(int32_t) * 16 + sizeof(uint64_t) * MID_GRAN);
    if (window) zero(b + L.hand, sizeof(int32_t) * HAND_WORDS);   // token 0, no flag set
    if (big) zero(b + L.xgran, sizeof(uint64_t) * (size_t)L.npad);   // no granule carries a token
  }
  if (window) {
    BaWinArgs wa;
    wa.poses = c.poses; wa.patches = c.patches; wa.intr = c.intrinsics; wa.target = c.target; wa.weight = c.weight; wa.lmbda = c.lmbda;
    wa.ii = c.ii; wa.P = P; wa.t0 = t0; wa.N = N;
    wa.gmeta = gv.meta; wa.koff_u = gv.koff_u; wa.kx = gv.kx;
    wa.tdeg = gv.tdeg; wa.tplo = gv.tplo; wa.tkid = gv.tkid; wa.tab_cap = 0;
    if (table) {   // patch table: rows are slots, the overflow CSR stands where the CSR records do
      wa.prec = gv.tprec; wa.pell = gv.ttab; wa.ell_chunks = 0x7fffffff;
      wa.tab_cap = (int)gi.tab_cap;
      CDV_REQUIRE(wa.tab_cap >= 1 && wa.tab_cap <= U_max, CDV_ERR_ARG,
                  "cdv_ba_forward: U_max must be at least the capacity of the patch table in graph_ws");
    } else {
      wa.prec = gv.prec; wa.pell = gv.pell; wa.ell_chunks = (int)gi.L.ell_chunks;
    }
    wa.has_ii = gi.has_ii ? 1 : 0;
    wa.slabs = (float*)(b + L.slabs); wa.ared = (float*)(b + L.ared);
    wa.arrive = (int32_t*)(b + L.hand);
    wa.granX = reinterpret_cast<uint64_t*>(info + 16);
    wa.Cg = (float*)(b + L.C); wa.ug = (float*)(b + L.u); wa.qg = (float*)(b + L.q); wa.Edg = (float*)(b + L.Ed);
    wa.dXg = (float*)(b + L.dX);
    wa.U_stride = (int)L.U_stride; wa.U_max = (int)L.U_max; wa.n_ck_cap = (int)L.n_ck;
    wa.info = info; wa.counters = counters;
    wa.test = g_handoff_test.load();
    wa.dyn = c.dyn;
    // wide chunks cut per frame (ba_mid.hip): only when a frame's patches really are ppf consecutive table slots
    // ... and only when the per-frame cut does not need more slabs than the workspace holds (one per 16 rows of U_max): a
    // frame of fewer than 16 patches would be a workgroup -- and a slab -- of its own (ppf 4, 8, 12: tab_cap / ppf > n_ck)
    wa.ppf = 0;
    if (table && N > WIN_N && ppf_hint >= 4 && ppf_hint % 4 == 0 && wa.tab_cap % ppf_hint == 0 &&
        (int64_t)(wa.tab_cap / ppf_hint) * cdv_ba_mid_wide_per_frame(ppf_hint) <= L.n_ck)
      wa.ppf = ppf_hint;
    for (int itr = 0; itr < iterations; itr++) {
      wa.dbg = (c.dbg && itr == 0) ? c.dbg : nullptr;
      wa.first = itr == 0 ? 1 : 0;
      wa.token = token_base + 1 + itr;
      const int rc = N <= WIN_N ? cdv_ba_window_iteration(wa, s) : cdv_ba_mid_iteration(wa, s);
      if (rc != CDV_OK) return rc;
    }
    return CDV_OK;
  }

  BaDenseArgs da;
  da.poses = c.poses; da.patches = c.patches; da.intr = c.intrinsics; da.target = c.target; da.weight = c.weight; da.lmbda = c.lmbda;
  da.ii = c.ii; da.jj = c.jj; da.kk = c.kk; da.E = E; da.P = P; da.t0 = t0; da.N = N;
  da.gmeta = gv.meta; da.prec = gv.prec; da.koff_u = gv.koff_u; da.kx = gv.kx;
  da.sy = (float*)(b + L.sy); da.dXg = (float*)(b + L.dX); da.Cg = (float*)(b + L.C); da.ug = (float*)(b + L.u);
  da.qg = (float*)(b + L.q); da.Edg = (float*)(b + L.Ed);
  da.cmask = big ? (uint32_t*)(b + L.cmask) : nullptr;
  da.Abig = (float*)(b + L.Abig); da.xgran = (uint64_t*)(b + L.xgran); da.fctl = (int32_t*)(b + L.fctl); da.ltg = (float*)(b + L.ltg);
  da.ptab = (int32_t*)(b + L.ptab); da.pdiag = (float*)(b + L.pdiag); da.pkeys = (int64_t*)(b + L.pkeys);
  da.pgraph = b + L.pgraph; da.pgraph_bytes = L.pgraph_bytes;
  da.E_max = L.E_max; da.pair_range = L.pair_range; da.pair_cap = L.pair_cap;
  da.U_stride = L.U_stride; da.U_max = L.U_max; da.sy_stride = L.sy_stride; da.npad = L.npad;
  da.info = info; da.counters = counters;
  da.test = g_handoff_test.load();
  if (big) {
    const int rc = cdv_ba_dense_pair_index(da, fresh, s);
    if (rc != CDV_OK) return rc;
  }
  for (int itr = 0; itr < iterations; itr++) {
    da.dbg = (c.dbg && itr == 0) ? c.dbg : nullptr;
    da.first = itr == 0 ? 1 : 0;
    da.token = token_base + 1 + itr;
    const int rc = cdv_ba_dense_iteration(da, s);
    if (rc != CDV_OK) return rc;
  }
  return CDV_OK;
}

extern "C" int cdv_ba_forward(float* poses, float* patches, const float* intrinsics, const float* target,
                              const float* weight, const float* lmbda, const int64_t* ii, const int64_t* jj,
                              const int64_t* kk, int64_t E, int P, int t0, int t1, int iterations,
                              const void* graph_ws, void* ba_ws, size_t ba_ws_bytes, int64_t U_max, float* dbg,
                              void* stream) {
  BaCall c;
  c.poses = poses; c.patches = patches; c.intrinsics = intrinsics; c.target = target; c.weight = weight; c.lmbda = lmbda;
  c.ii = ii; c.jj = jj; c.kk = kk; c.E = E; c.P = P; c.t0 = t0; c.t1 = t1; c.iterations = iterations;
  c.graph_ws = graph_ws; c.ba_ws = ba_ws; c.ba_ws_bytes = ba_ws_bytes; c.U_max = U_max; c.dbg = dbg; c.stream = stream;
  return ba_forward_impl(c);
}

// cdv_ba_forward with the window on the device: the free poses are [dyn[CDV_DYN_T0], + dyn[CDV_DYN_NFREE]) with
// dyn[CDV_DYN_NFREE] <= N_max <= 32 (the optimisation window of a frame stream, slam.py:512-513: known to the device only
// when the keyframe decision stays there; N_max picks the path -- <= 10 the window kernels, <= 32 ba_mid.hip's -- and the
// kernels then work on whatever the block says, e.g. the 7 free poses of a stream's first update inside launches laid out
// for 22); E_bound sizes the workspace, the index in graph_ws must be a patch table.
extern "C" int cdv_ba_forward_dyn(float* poses, float* patches, const float* intrinsics, const float* target, const float* weight,
                                  const float* lmbda, const int64_t* ii, const int64_t* jj, const int64_t* kk, int64_t E_bound,
                                  int P, int N_max, const int32_t* dyn, int iterations, const void* graph_ws, void* ba_ws,
                                  size_t ba_ws_bytes, int64_t U_max, void* stream) {
  CDV_REQUIRE(dyn != nullptr, CDV_ERR_ARG, "cdv_ba_forward_dyn: NULL dynamic block");
  CDV_REQUIRE(N_max >= 1 && N_max <= MID_N, CDV_ERR_UNSUPPORTED, "cdv_ba_forward_dyn: 1 <= N_max <= 32 free poses");
  GraphInfo gi;
  CDV_REQUIRE(cdv_graph_info(graph_ws, &gi) && gi.table, CDV_ERR_UNSUPPORTED, "cdv_ba_forward_dyn: graph_ws must hold a patch table");
  BaCall c;
  c.poses = poses; c.patches = patches; c.intrinsics = intrinsics; c.target = target; c.weight = weight; c.lmbda = lmbda;
  c.ii = ii; c.jj = jj; c.kk = kk; c.E = E_bound; c.P = P; c.t0 = 0; c.t1 = N_max; c.iterations = iterations;
  c.graph_ws = graph_ws; c.graph = &gi; c.ba_ws = ba_ws; c.ba_ws_bytes = ba_ws_bytes; c.U_max = U_max; c.stream = stream;
  c.dyn = dyn;
  return ba_forward_impl(c);
}

// ---------------------------------------------------------------------------------------------------------
// status of a workspace
// ---------------------------------------------------------------------------------------------------------

// Fault injection for the in-launch hand-offs (tests only; process-wide, read by the next cdv_ba_forward calls):
//   0 off; 1 the solver of the N <= 32 paths stalls BEFORE its commit (the retract workgroups abandon: nothing is applied) --
//   on the global path the back substitution withholds one block's solution (its readers time out: nothing is applied);
//   2 the solver stalls AFTER its commit (the retract workgroups lose their patience, learn that the solution is coming and
//   wait on: the update is applied as usual; the global path has no such in-launch commit and runs undisturbed);  3 (global path) a diagonal block of the factorisation launch never raises its flag
//   (everybody who needs it times out, the launch drains, nothing is applied).  The waits are shortened so that a test takes
//   milliseconds.
extern "C" int cdv_ba_test_handoff(int mode) {
  CDV_REQUIRE(mode >= 0 && mode <= 3, CDV_ERR_ARG, "cdv_ba_test_handoff: mode 0 .. 3");
  g_handoff_test.store(mode);
  return CDV_OK;
}

// PPF of cuda_ba.forward (fastba/ba.cpp:31-45 passes the patches per frame; the reference's kernels only use it in the
// block-sparse E of eff_impl): a hint that lets the 10 < N <= 32 path cut its workgroups' patch ranges per frame when the
// patch table's capacity is a multiple of it.  0 forgets the hint.  Results do not depend on it beyond summation order.
extern "C" int cdv_ba_set_patches_per_frame(void* ba_ws, int patches_per_frame) {
  CDV_REQUIRE(ba_ws != nullptr && patches_per_frame >= 0, CDV_ERR_ARG, "cdv_ba_set_patches_per_frame: arguments");
  std::lock_guard<std::mutex> lk(g_ws_mutex);
  g_ws[ba_ws].ppf = patches_per_frame;
  return CDV_OK;
}

extern "C" int cdv_ba_bind_status_counters(void* ba_ws, int32_t* counters) {
  CDV_REQUIRE(ba_ws != nullptr, CDV_ERR_ARG, "cdv_ba_bind_status_counters: workspace is NULL");
  std::lock_guard<std::mutex> lk(g_ws_mutex);
  g_ws[ba_ws].counters = counters;
  return CDV_OK;
}

extern "C" int cdv_ba_status(const void* ba_ws, int32_t* info_host, void* stream) {
  CDV_REQUIRE(ba_ws != nullptr && info_host != nullptr, CDV_ERR_ARG, "cdv_ba_status: NULL argument");
  WsState st;
  {
    std::lock_guard<std::mutex> lk(g_ws_mutex);
    auto it = g_ws.find(ba_ws);
    CDV_REQUIRE(it != g_ws.end() && it->second.st.valid, CDV_ERR_ARG, "cdv_ba_status: no cdv_ba_forward has run on this workspace");
    st = it->second.st;
  }
  const BaLayout L = ba_layout(st.U_max, st.N > 0 ? st.N : 1);
  CDV_HIP_CHECK(hipMemcpyAsync(info_host, (const char*)ba_ws + L.info, 4 * sizeof(int32_t), hipMemcpyDeviceToHost,
                               (hipStream_t)stream));
  CDV_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
  if (info_host[BI_GRAPH]) {
    cdv_set_error(CDV_ERR_GRAPH_RANGE, "bundle adjustment skipped: the patch-graph index reported a patch-id range beyond its capacity");
    return CDV_ERR_GRAPH_RANGE;
  }
  if (info_host[BI_OVERFLOW]) {
    cdv_set_error(CDV_ERR_BA_OVERFLOW, "bundle adjustment skipped: more unique patches than U_max");
    return CDV_ERR_BA_OVERFLOW;
  }
  if (info_host[BI_HANDOFF]) {
    cdv_set_error(CDV_ERR_BA_HANDOFF, "bundle adjustment: an in-launch hand-off timed out, the update was not applied");
    return CDV_ERR_BA_HANDOFF;
  }
  if (info_host[BI_CHOL]) {
    cdv_set_error(CDV_ERR_BA_NOT_SPD, "bundle adjustment: the reduced system is not positive definite (Cholesky pivot <= 0)");
    return CDV_ERR_BA_NOT_SPD;
  }
  return CDV_OK;
}
