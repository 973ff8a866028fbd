// lmm_hip.hip — device context + C ABI of include/lmm/lmm_hip.h for the MI355X (gfx950) LMM solver: context
// create / destroy, flat allocation and upload, the lmmhip_solve dispatch, setters, getters, the component labelling
// and the profile exports.  The engines, the resident mirror and the step glue are in lmm_hip_maxmin.hip,
// lmm_hip_fair.hip, lmm_hip_resident.hip and lmm_hip_step.hip (lmm_ctx.hpp).
//
// Kernels: lmm_maxmin_kernels.hpp (System::lmm_solve, maxmin.cpp:487-693) and lmm_fb_kernels.hpp
// (FairBottleneck::bottleneck_solve, fair_bottleneck.cpp:23-153); layout in lmm_dev.hpp.
// All arithmetic is fp64; device code is compiled with -ffp-contract=off so every a*b+c rounds like the
// reference (the FairBottleneck `value == bound` test is exact).
#include <cstring>

#include "lmm_ctx.hpp"
#include "lmm_common_kernels.hpp"
#include "lmm_cc_kernels.hpp"
#include "lmm_scan.hpp"

void free_owner(lmmhip_ctx* c) {
  c->fair.owner_allocs.clear();
  c->fair.owner = FbOwner{};
  c->fair.owner_ready = false;
}

static void free_all(lmmhip_ctx* c) {
  c->allocs.clear();
  free_owner(c);
  c->d = Dev{};
  c->uploaded = false;
  c->fair.f = FbFields{};
  c->fair.fbd_cap = 0;
  c->fair.shard_xnb = nullptr;
  c->res_flat = false;
}

const char* lmmhip_last_error(void) { return g_err.c_str(); }

int lmmhip_device_count(void) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    g_err = std::string("hipGetDeviceCount: ") + hipGetErrorString(e);
    return 0;
  }
  return n;
}

int lmmhip_ctx_create(int device, lmmhip_ctx** out) {
  if (!out)
    return fail(LMMHIP_E_ARG, "null out");
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0)
    return fail(LMMHIP_E_NODEVICE, "no HIP device visible (the MI355X path has no CPU fallback)");
  auto* c = new lmmhip_ctx;
  if (device < 0) {
    if (hipGetDevice(&device) != hipSuccess)
      device = 0;
  }
  c->device = device;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess)
    e = hipDeviceGetAttribute(&c->n_cu, hipDeviceAttributeMultiprocessorCount, device);
  if (e == hipSuccess)
    e = hipStreamCreateWithFlags(&c->own_stream.p, hipStreamNonBlocking);
  c->stream = c->own_stream.p;
  if (e == hipSuccess)
    e = hipHostMalloc((void**)&c->h_ctl.p, 4 * CTL_WORDS * sizeof(int32_t), hipHostMallocDefault);
  if (e == hipSuccess)
    e = hipHostMalloc((void**)&c->h_rdv.p, 64, hipHostMallocMapped);
  if (e == hipSuccess)
    e = hipHostGetDevicePointer((void**)&c->d_rdv, c->h_rdv.p, 0);
  if (e == hipSuccess)
    e = hipEventCreateWithFlags(&c->ev_poll[0].p, hipEventDisableTiming);
  if (e == hipSuccess)
    e = hipEventCreateWithFlags(&c->ev_poll[1].p, hipEventDisableTiming);
  if (e == hipSuccess)
    e = hipEventCreate(&c->ev0.p);
  if (e == hipSuccess)
    e = hipEventCreate(&c->ev1.p);
  if (e != hipSuccess) {
    delete c;  // (its members release what was created)
    return fail(LMMHIP_E_HIP, std::string("context creation: ") + hipGetErrorString(e));
  }
  persist_ctx_ref(device, +1);
  *out = c;
  return 0;
}

int lmmhip_ctx_destroy(lmmhip_ctx* c) {
  if (!c)
    return 0;
  (void)hipSetDevice(c->device);
  if (c->stream)
    (void)hipStreamSynchronize(c->stream);
  if (c->own_stream.p && c->own_stream.p != c->stream)
    (void)hipStreamSynchronize(c->own_stream.p);
  for (const Stream& st : c->retired_streams)  // a persistent launch whose rendezvous closed: its late workgroups
    (void)hipStreamSynchronize(st.p);         // still read the barrier words
  persist_ctx_ref(c->device, -1);
  delete c;
  return 0;
}

static int alloc_flat_exact(lmmhip_ctx* c, int64_t nV, int64_t nC, int64_t nnz, int64_t nch, FlatBufs* o) {
  free_all(c);
  Dev& d = c->d;
  FbFields& f = c->fair.f;
  d.nV = int32_t(nV);
  d.nC = int32_t(nC);
  d.nnz = nnz;
  uint32_t *vp, *cp, *crow1, *crow2;
  int32_t *csr_c, *csc_v, *cvar0, *cvar1, *cvar2, *ccol1, *ccol2;
  double *csr_w, *csc_w, *pen, *vb, *cb;
  uint8_t* cf;
  const int64_t nblk = (nV + kCompactRows - 1) / kCompactRows + 1;
  int rc = 0;
  rc |= dalloc(c, &vp, nV + 1);
  rc |= dalloc(c, &csr_c, nnz);
  rc |= dalloc(c, &csr_w, nnz);
  rc |= dalloc(c, &cp, nC + 1);
  rc |= dalloc(c, &csc_v, nnz);
  rc |= dalloc(c, &csc_w, nnz);
  rc |= dalloc(c, &d.csc_u, nnz);
  rc |= dalloc(c, &d.csc_p, nnz);
  rc |= dalloc(c, &d.csc_row, nnz);
  rc |= dalloc(c, &pen, nV);
  rc |= dalloc(c, &vb, nV);
  rc |= dalloc(c, &cb, nC);
  rc |= dalloc(c, &cf, nC);
  rc |= dalloc(c, &d.x, nV);
  rc |= dalloc(c, &f.fixr, nV);
  rc |= dalloc(c, &f.vtmp, nV);
  rc |= dalloc(c, &f.vst, int64_t(nV) + 32);  // (+32: read 32 flags at a time by fb_pack_vst)
  rc |= dalloc(c, &f.vstb, (int64_t(nV) + 31) / 32 + 1);
  rc |= dalloc(c, &d.ratio, nC);
  rc |= dalloc(c, &d.key, nC);
  rc |= dalloc(c, &d.rem, nC);
  rc |= dalloc(c, &d.use, nC);
  rc |= dalloc(c, &d.cst, nC);
  rc |= dalloc(c, &d.cexp, nC);
  rc |= dalloc(c, &d.nvote, nC);
  rc |= dalloc(c, &cvar0, nV);
  rc |= dalloc(c, &cvar1, nV);
  rc |= dalloc(c, &cvar2, nV);
  rc |= dalloc(c, &crow1, nV + 1);
  rc |= dalloc(c, &crow2, nV + 1);
  rc |= dalloc(c, &ccol1, nnz);
  rc |= dalloc(c, &ccol2, nnz);
  rc |= dalloc(c, &d.vstate, nV);
  for (int b = 0; b < 3; b++) {
    rc |= dalloc(c, &d.rtgt[b], nV);
    rc |= dalloc(c, &d.skey[b], nV);
  }
  rc |= dalloc(c, &d.chg, nC);
  rc |= dalloc(c, &d.chgbits, (nC + 127) / 128 * 2 + 2);
  rc |= dalloc(c, &d.flagbits, (nC + 127) / 128 * 2 + 2);
  rc |= dalloc(c, &d.ready, nC + kMaxBlocks);
  rc |= dalloc(c, &d.bready, kMaxBlocks);
  rc |= dalloc(c, &d.ctouch, nC);
  rc |= dalloc(c, &d.cdup, nC);
  rc |= dalloc(c, &d.balive, kMaxBlocks);
  rc |= dalloc(c, &d.clist[0], nC);
  rc |= dalloc(c, &d.clist[1], nC);
  rc |= dalloc(c, &d.bsum, 2 * nblk);
  rc |= dalloc(c, &d.ctl, CTL_ALLOC);
  int32_t *chc, *cch;
  uint32_t* chb;
  rc |= dalloc(c, &chc, nch);
  rc |= dalloc(c, &chb, nch);
  rc |= dalloc(c, &cch, nC + 1);
  rc |= dalloc(c, &f.pcnt, nch);
  rc |= dalloc(c, &f.pacc, nch);
  rc |= dalloc(c, &f.erased, nC);
  rc |= dalloc(c, &f.xnb, nC + 1);  // the context's own exchange buffers (a sharded solve brings its xnb)
  rc |= dalloc(c, &f.xmin, nC);
  if (rc) {
    free_all(c);
    return LMMHIP_E_HIP;
  }
  f.nch = int32_t(nch);
  f.ch_cnst = chc;
  f.ch_beg = chb;
  f.c_ch = cch;
  d.var_ptr = vp;
  d.csr_c = csr_c;
  d.csr_w = csr_w;
  d.cnst_ptr = cp;
  d.csc_v = csc_v;
  d.csc_w = csc_w;
  d.pen = pen;
  d.vbound = vb;
  d.cbound = cb;
  d.cflags = cf;
  d.cvar[0] = cvar0;
  d.crow[0] = vp;
  d.ccol[0] = csr_c;
  d.cvar[1] = cvar1;
  d.crow[1] = crow1;
  d.ccol[1] = ccol1;
  d.cvar[2] = cvar2;
  d.crow[2] = crow2;
  d.ccol[2] = ccol2;
  *o = FlatBufs{vp, cp, chb, csr_c, csc_v, cvar0, chc, cch, csr_w, csc_w, pen, vb, cb, cf};
  return 0;
}

// Buffers for a system of this shape, reusing the current ones when they are large enough (a
// simulation re-solves systems of similar size every step: no hipMalloc / hipFree on that path);
// otherwise reallocated with 25 % headroom over the previous capacity.
int alloc_flat(lmmhip_ctx* c, int64_t nV, int64_t nC, int64_t nnz, int64_t nch, FlatBufs* o) {
  c->sys_gen++;  // the dense numbering is about to change (bound action tables rebind)
  const bool have = !c->allocs.v.empty();
  const bool fits = have && nV <= c->fcap[0] && nC <= c->fcap[1] && nnz <= c->fcap[2] && nch <= c->fcap[3];
  if (!fits) {
    int64_t a[4] = {nV, nC, nnz, nch};
    // headroom: a simulation's next system is usually a little larger (flows arriving, a link's bound
    // leaving 0); growing the flat buffers costs ~10 ms of frees and allocations at C2's size
    for (int i = 0; i < 4; i++)
      a[i] = have ? std::max(a[i], c->fcap[i] + c->fcap[i] / 4) : a[i] + a[i] / 16;
    if (a[2] > INT32_MAX)
      a[2] = std::max(nnz, int64_t(INT32_MAX));
    if (int rc = alloc_flat_exact(c, a[0], a[1], a[2], a[3], &c->fb_last))
      return rc;
    for (int i = 0; i < 4; i++)
      c->fcap[i] = a[i];
  } else {
    c->uploaded = false;
    c->res_flat = false;
    c->fair.shard_xnb = nullptr;
    free_owner(c);  // owned constraints refer to the previous system
  }
  c->d.nV = int32_t(nV);
  c->d.nC = int32_t(nC);
  c->d.nnz = nnz;
  c->fair.f.nch = int32_t(nch);
  *o = c->fb_last;
  return 0;
}

// Solver launch parameters from the system's shape + per-element usage; the system is then solvable.
int finish_flat(lmmhip_ctx* c, int64_t nV, int64_t nC, int64_t nnz, bool elem_done) {
  Dev& d = c->d;
  c->fair.perm_ok = false;
  c->frontier.map_ok = false;
  c->res_c2c_ok = false;  // (a resident flatten sets it again once finish_flat returns)
  const double mean = nV > 0 ? double(nnz) / double(nV) : 1.0;
  c->group = mean <= 4 ? 4 : mean <= 8 ? 8 : mean <= 16 ? 16 : mean <= 32 ? 32 : 64;
  const double cmean = nC > 0 ? double(nnz) / double(nC) : 1.0;  // mean constraint degree
  c->sat_waves = cmean <= 64 ? 1 : cmean <= 160 ? 2 : 4;
  if (nC > 0)  // constraints with a duplicate (variable, constraint) pair (structure only)
    HIPCHK(hipMemsetAsync(d.cdup, 0, size_t(nC), c->stream));
  if (nnz > 0) {  // per-element usage w / penalty, kept in step with pen (lmmhip_update_vars)
    if (!elem_done)
      if (int rc = launch_elem_usage(c, 1))
        return rc;
    hipLaunchKernelGGL(mm_dup_check, dim3(grid_for(nV, kBlock)), dim3(kBlock), 0, c->stream, d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
  }
  c->uploaded = true;
  c->sys_gen++;
  c->solved = false;
  c->bt_n = 0;  // a new system: no batch declared
  c->stats = lmmhip_stats{};
  c->stats.n_var = nV;
  c->stats.n_cnst = nC;
  c->stats.nnz = nnz;
  return 0;
}

int lmmhip_upload(lmmhip_ctx* c, int64_t nV, int64_t nC, int64_t nnz, const int64_t* var_ptr,
                  const int32_t* cnst_idx, const double* weight, const double* penalty, const double* var_bound,
                  const double* cnst_bound, const uint8_t* cnst_flags) {
  return lmmhip_upload2(c, nV, nC, nnz, var_ptr, cnst_idx, weight, penalty, var_bound, cnst_bound, cnst_flags,
                        nullptr);
}

int lmmhip_upload2(lmmhip_ctx* c, int64_t nV, int64_t nC, int64_t nnz, const int64_t* var_ptr,
                   const int32_t* cnst_idx, const double* weight, const double* penalty, const double* var_bound,
                   const double* cnst_bound, const uint8_t* cnst_flags, const int64_t* csc_order) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (nV < 0 || nC < 0 || nnz < 0 || nV >= (1 << 30) || nC >= (1 << 30) || nnz > INT32_MAX)
    return fail(LMMHIP_E_ARG, "sizes out of range");
  if (nV > 0 && (!var_ptr || !penalty || !var_bound))
    return fail(LMMHIP_E_ARG, "null variable arrays");
  if (nC > 0 && (!cnst_bound || !cnst_flags))
    return fail(LMMHIP_E_ARG, "null constraint arrays");
  if (nnz > 0 && (!cnst_idx || !weight))
    return fail(LMMHIP_E_ARG, "null element arrays");
  if (nV > 0 && (var_ptr[0] != 0 || var_ptr[nV] != nnz))
    return fail(LMMHIP_E_ARG, "var_ptr must start at 0 and end at nnz");
  // host-side validation + 32-bit offsets + CSC (constraint-major) mirror by a stable counting sort
  std::vector<uint32_t> vp32(static_cast<size_t>(nV) + 1, 0);
  for (int64_t v = 0; v < nV; v++) {
    if (var_ptr[v + 1] < var_ptr[v])
      return fail(LMMHIP_E_ARG, "var_ptr not monotone");
    vp32[size_t(v) + 1] = uint32_t(var_ptr[v + 1]);
  }
  std::vector<uint32_t> cptr(static_cast<size_t>(nC) + 1, 0);
  for (int64_t j = 0; j < nnz; j++) {
    int32_t k = cnst_idx[j];
    if (k < 0 || k >= nC)
      return fail(LMMHIP_E_ARG, "cnst_idx out of range");
    if (!(weight[j] > 0))
      return fail(LMMHIP_E_ARG, "element weights must be > 0 (only active elements are flattened)");
    cptr[size_t(k) + 1]++;
  }
  for (int64_t v = 0; v < nV; v++)
    if (!(penalty[v] > 0))
      return fail(LMMHIP_E_ARG, "penalties must be > 0 (only enabled variables are flattened)");
  for (int64_t k = 0; k < nC; k++)
    cptr[size_t(k) + 1] += cptr[size_t(k)];
  std::vector<int32_t> cv(static_cast<size_t>(nnz));
  std::vector<double> cw(static_cast<size_t>(nnz));
  if (!csc_order) {
    std::vector<uint32_t> cur(cptr.begin(), cptr.end() - 1);
    for (int64_t v = 0; v < nV; v++)
      for (int64_t j = var_ptr[v]; j < var_ptr[v + 1]; j++) {
        uint32_t pos = cur[size_t(cnst_idx[j])]++;
        cv[pos] = int32_t(v);
        cw[pos] = weight[j];
      }
  } else {  // the caller's order within each constraint: a permutation of its CSR elements
    std::vector<int32_t> row(static_cast<size_t>(nnz));
    for (int64_t v = 0; v < nV; v++)
      for (int64_t j = var_ptr[v]; j < var_ptr[v + 1]; j++)
        row[size_t(j)] = int32_t(v);
    std::vector<uint8_t> seen(static_cast<size_t>(nnz), 0);
    int64_t k = 0;
    for (int64_t pos = 0; pos < nnz; pos++) {
      while (k < nC && cptr[size_t(k) + 1] <= uint32_t(pos))
        k++;
      const int64_t j = csc_order[pos];
      if (j < 0 || j >= nnz || seen[size_t(j)] || cnst_idx[j] != k)
        return fail(LMMHIP_E_ARG, "csc_order is not a constraint-major permutation of the CSR elements");
      seen[size_t(j)] = 1;
      cv[size_t(pos)] = row[size_t(j)];
      cw[size_t(pos)] = weight[j];
    }
  }
  // fair bottleneck CSC chunks (lmm_fb_kernels.hpp)
  std::vector<int32_t> c_ch(static_cast<size_t>(nC) + 1, 0), ch_cnst;
  std::vector<uint32_t> ch_beg;
  for (int64_t k = 0; k < nC; k++) {
    c_ch[size_t(k)] = int32_t(ch_cnst.size());
    for (uint32_t b = cptr[size_t(k)]; b < cptr[size_t(k) + 1]; b += kFbChunk) {
      ch_cnst.push_back(int32_t(k));
      ch_beg.push_back(b);
    }
  }
  const int64_t nch = int64_t(ch_cnst.size());
  c_ch[size_t(nC)] = int32_t(nch);
  std::vector<int32_t> iota(static_cast<size_t>(nV));
  for (int64_t v = 0; v < nV; v++)
    iota[size_t(v)] = int32_t(v);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  FlatBufs fb;
  if (int rc = alloc_flat(c, nV, nC, nnz, nch, &fb))
    return rc;
  uint32_t *vp = fb.vp, *cp = fb.cp, *chb = fb.chb;
  int32_t *csr_c = fb.csr_c, *csc_v = fb.csc_v, *cvar0 = fb.cvar0, *chc = fb.chc, *cch = fb.cch;
  double *csr_w = fb.csr_w, *csc_w = fb.csc_w, *pen = fb.pen, *vb = fb.vb, *cb = fb.cb;
  uint8_t* cf = fb.cf;
  HIPCHK(hipMemcpyAsync(vp, vp32.data(), sizeof(uint32_t) * (nV + 1), hipMemcpyHostToDevice, c->stream));
  if (nnz > 0) {
    HIPCHK(hipMemcpyAsync(csr_c, cnst_idx, sizeof(int32_t) * nnz, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(csr_w, weight, sizeof(double) * nnz, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(csc_v, cv.data(), sizeof(int32_t) * nnz, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(csc_w, cw.data(), sizeof(double) * nnz, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipMemcpyAsync(cp, cptr.data(), sizeof(uint32_t) * (nC + 1), hipMemcpyHostToDevice, c->stream));
  if (nV > 0) {
    HIPCHK(hipMemcpyAsync(pen, penalty, sizeof(double) * nV, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(vb, var_bound, sizeof(double) * nV, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(cvar0, iota.data(), sizeof(int32_t) * nV, hipMemcpyHostToDevice, c->stream));
  }
  if (nC > 0) {
    HIPCHK(hipMemcpyAsync(cb, cnst_bound, sizeof(double) * nC, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(cf, cnst_flags, sizeof(uint8_t) * nC, hipMemcpyHostToDevice, c->stream));
  }
  if (nch > 0) {
    HIPCHK(hipMemcpyAsync(chc, ch_cnst.data(), sizeof(int32_t) * nch, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(chb, ch_beg.data(), sizeof(uint32_t) * nch, hipMemcpyHostToDevice, c->stream));
  }
  HIPCHK(hipMemcpyAsync(cch, c_ch.data(), sizeof(int32_t) * (nC + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));  // host staging vectors die at return
  return finish_flat(c, nV, nC, nnz);
}

int lmmhip_update_vars(lmmhip_ctx* c, const double* penalty, const double* var_bound) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  HIPCHK(hipSetDevice(c->device));
  if (penalty && c->d.nV)
    HIPCHK(hipMemcpyAsync((void*)c->d.pen, penalty, sizeof(double) * c->d.nV, hipMemcpyHostToDevice, c->stream));
  if (penalty && c->d.nnz)
    if (int rc = launch_elem_usage(c, 0))
      return rc;
  if (var_bound && c->d.nV)
    HIPCHK(
        hipMemcpyAsync((void*)c->d.vbound, var_bound, sizeof(double) * c->d.nV, hipMemcpyHostToDevice, c->stream));
  // the dense penalties / bounds (and csc_u / csc_p) no longer match the resident records for variables the delta
  // list does not name: the next resident refresh must rewrite every member
  if (penalty || var_bound)
    c->res_vl_n = -1;
  if (penalty)
    c->res_pen_dirty = true;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_update_cnsts(lmmhip_ctx* c, const double* cnst_bound) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  HIPCHK(hipSetDevice(c->device));
  if (cnst_bound && c->d.nC)
    HIPCHK(
        hipMemcpyAsync((void*)c->d.cbound, cnst_bound, sizeof(double) * c->d.nC, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int launch_elem_usage(lmmhip_ctx* c, int rows) {
  hipLaunchKernelGGL(mm_elem_usage, dim3(grid_for(c->d.nnz, kBlock)), dim3(kBlock), 0, c->stream, c->d, rows);
  HIPCHK(hipGetLastError());
  return 0;
}

int dev_scan(lmmhip_ctx* c, const int64_t* in, int64_t* out, int64_t n) {
  size_t tb = 0;
  HIPCHK(scan_i64(nullptr, tb, in, out, n, c->stream));
  uint8_t* t = nullptr;
  if (int rc = scratch(c, c->rs_tmp, int64_t(tb), &t))
    return rc;
  HIPCHK(scan_i64(t, tb, in, out, n, c->stream));
  return 0;
}

int64_t read_i64(lmmhip_ctx* c, const int64_t* dptr, int* rc) {
  int64_t h = 0;
  if (hipMemcpyAsync(&h, dptr, sizeof(h), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
      hipStreamSynchronize(c->stream) != hipSuccess)
    *rc = fail(LMMHIP_E_HIP, "resident flatten: reading a count back failed");
  return h;
}

int lmmhip_flat_download(lmmhip_ctx* c, int64_t* counts3, uint32_t* var_ptr, int32_t* csr_c, double* csr_w,
                         uint32_t* cnst_ptr, int32_t* csc_v, double* csc_w, double* penalty, double* var_bound,
                         double* cnst_bound, uint8_t* cnst_flags) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  if (!counts3)
    return fail(LMMHIP_E_ARG, "null counts");
  const Dev& d = c->d;
  counts3[0] = d.nV;
  counts3[1] = d.nC;
  counts3[2] = d.nnz;
  HIPCHK(hipSetDevice(c->device));
  auto get = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst && bytes)
      HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    return 0;
  };
  int rc = get(var_ptr, d.var_ptr, sizeof(uint32_t) * (size_t(d.nV) + 1)) |
           get(csr_c, d.csr_c, sizeof(int32_t) * size_t(d.nnz)) | get(csr_w, d.csr_w, sizeof(double) * size_t(d.nnz)) |
           get(cnst_ptr, d.cnst_ptr, sizeof(uint32_t) * (size_t(d.nC) + 1)) |
           get(csc_v, d.csc_v, sizeof(int32_t) * size_t(d.nnz)) | get(csc_w, d.csc_w, sizeof(double) * size_t(d.nnz)) |
           get(penalty, d.pen, sizeof(double) * size_t(d.nV)) | get(var_bound, d.vbound, sizeof(double) * size_t(d.nV)) |
           get(cnst_bound, d.cbound, sizeof(double) * size_t(d.nC)) | get(cnst_flags, d.cflags, size_t(d.nC));
  if (rc)
    return rc;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_set_profiling(lmmhip_ctx* c, int on) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  c->profiling = on != 0;
  return 0;
}

int lmmhip_solve(lmmhip_ctx* c, int kind, double precision) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "solve before upload");
  if (kind != LMMHIP_KIND_MAXMIN && kind != LMMHIP_KIND_FAIR_BOTTLENECK)
    return fail(LMMHIP_E_ARG, "unknown solver kind");
  if (c->res_flat && kind != c->res_flat_kind)
    return fail(LMMHIP_E_STATE, "the resident flatten was built for the other solver kind");
  HIPCHK(hipSetDevice(c->device));
  for (int i = 0; i < 8; i++) {
    c->stats.kernel_ms[i] = 0;
    c->stats.kernel_launches[i] = 0;
  }
  c->pool_used = 0;
  c->launch_slot.clear();
  c->launch_round.clear();
  c->launch_ms.clear();
  HIPCHK(hipMemsetAsync(c->d.ctl, 0, CTL_ALLOC * sizeof(int32_t), c->stream));
  const size_t stat_bytes = sizeof(int32_t) * 2 * size_t(kStatRounds) * kMaxBlocks;
  if (c->profiling && !c->vstat.p)
    HIPCHK(hipMalloc(&c->vstat.p, stat_bytes));
  c->d.vstat = c->profiling ? c->vstat.p : nullptr;
  if (c->profiling)
    HIPCHK(hipMemsetAsync(c->vstat.p, 0, stat_bytes, c->stream));
  // round anatomy (diagnostic builds only): the round engine's waves stamp the rounds LMMHIP_ANAT_ROUNDS names
  c->d.anat = nullptr;
  for (int k = 0; k < kAnatSlots; k++)
    c->d.anat_r[k] = -1000;
  if (LMM_ANAT && std::getenv("LMMHIP_ANAT_ROUNDS")) {
    const size_t bytes = sizeof(unsigned long long) * size_t(kAnatSlots) * kAnatKernels * kAnatWaves * kAnatFields;
    if (!c->anat.p)
      HIPCHK(hipMalloc(&c->anat.p, bytes));
    HIPCHK(hipMemsetAsync(c->anat.p, 0, bytes, c->stream));
    const char* e = std::getenv("LMMHIP_ANAT_ROUNDS");
    for (int k = 0; k < kAnatSlots; k++) {
      char* end = nullptr;
      const long v = std::strtol(e, &end, 10);
      if (end == e)
        break;
      c->d.anat_r[k] = int(v);
      if (*end != ',')
        break;
      e = end + 1;
    }
    c->d.anat = c->anat.p;
  }
  HIPCHK(hipEventRecord(c->ev0.p, c->stream));
  c->last_kind = kind;
  c->last_prec = precision;
  c->solved = false;
  c->ev1_done = false;
  int rc = kind == LMMHIP_KIND_FAIR_BOTTLENECK
               ? (fb_batch_fits(c) ? solve_fair_batch(c, precision) : solve_fair(c, precision))
           : batch_fits(c)                             ? solve_maxmin_batch(c, precision)
           : engine_of(c) == LMMHIP_ENGINE_PERSISTENT ? solve_maxmin_persist(c, precision)
           : engine_of(c) == LMMHIP_ENGINE_FRONTIER   ? solve_maxmin_frontier(c, precision)
                                                     : solve_maxmin(c, precision);
  if (rc)
    return rc;
  if (!c->ev1_done)
    HIPCHK(hipEventRecord(c->ev1.p, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0.p, c->ev1.p));
  c->stats.device_ms = ms;
  c->solved = true;
  c->last_engine = c->ran_engine;
  c->stats.rounds = c->h_ctl.p[CTL_ROUNDS];
  if (kind == LMMHIP_KIND_MAXMIN && c->stats.rounds > 0)  // launched rounds include empty tail rounds
    c->stats.rounds = c->h_ctl.p[CTL_LASTR] + 1;
  if (c->profiling)
    return resolve_profile(c);
  return 0;
}

int lmmhip_last_engine(lmmhip_ctx* c, int* engine) {
  if (!c || !engine)
    return fail(LMMHIP_E_ARG, "null argument");
  if (c->last_engine < 0)
    return fail(LMMHIP_E_STATE, "no solve has succeeded on this context yet");
  *engine = c->last_engine;
  return 0;
}

int prof_event(lmmhip_ctx* c, hipEvent_t* out) {
  if (c->pool_used == c->pool.size()) {
    Event ev;
    HIPCHK(hipEventCreate(&ev.p));
    c->pool.push_back(std::move(ev));
  }
  *out = c->pool[c->pool_used++].p;
  return 0;
}

int resolve_profile(lmmhip_ctx* c) {
  c->launch_ms.assign(c->launch_slot.size(), 0.f);
  for (size_t i = 0; i < c->launch_slot.size(); i++) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->pool[2 * i].p, c->pool[2 * i + 1].p));
    c->launch_ms[i] = ms;
    c->stats.kernel_ms[c->launch_slot[i]] += ms;
  }
  return 0;
}

int poll_ctl(lmmhip_ctx* c) {
  HIPCHK(hipMemcpyAsync(c->h_ctl.p, c->d.ctl, CTL_WORDS * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int CtlPoll::init(lmmhip_ctx* ctx) {
  c = ctx;
  for (int k = 0; k < 2; k++) {
    hc[k] = c->h_ctl.p + (k + 1) * CTL_WORDS;
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&hcd[k]), hc[k], 0));
  }
  return 0;
}

int CtlPoll::step(const Dev& d, int64_t round, bool stop, const int32_t** words) {
  *words = nullptr;
  LAUNCH(6, round, mm_ctl_out, 1, kWave, d, hcd[slot]);
  HIPCHK(hipEventRecord(c->ev_poll[slot].p, c->stream));
  if (pending) {  // the previous chunk's words (this chunk is queued behind them)
    HIPCHK(hipEventSynchronize(c->ev_poll[slot ^ 1].p));
    *words = hc[slot ^ 1];
  }
  pending = !stop;
  if (stop && !(*words && (*words)[CTL_DONE])) {
    HIPCHK(hipEventSynchronize(c->ev_poll[slot].p));
    *words = hc[slot];
  }
  slot ^= 1;
  return 0;
}

int lmmhip_ctx_set_stream(lmmhip_ctx* c, void* stream) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stream = static_cast<hipStream_t>(stream);  // 0 = the legacy null stream, like any other handle
  return 0;
}

int lmmhip_ctx_use_own_stream(lmmhip_ctx* c) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->stream = c->own_stream.p;
  return 0;
}

int lmmhip_persist_profile(lmmhip_ctx* c, int on, int64_t* t, int64_t cap, int64_t* n) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  c->persist_prof = on != 0;
  if (n)
    *n = 0;
  if (!t || !c->ptime.p)
    return 0;
  HIPCHK(hipSetDevice(c->device));
  std::vector<long long> h(2 * size_t(kPersistProfCap));
  HIPCHK(hipMemcpyAsync(h.data(), c->ptime.p, h.size() * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  int64_t m = 0;
  while (m < int64_t(kPersistProfCap) && h[2 * size_t(m) + 1] != 0)
    m++;
  for (int64_t i = 0; i < m && 2 * i + 1 < cap; i++) {
    t[2 * i] = h[2 * size_t(i)];
    t[2 * i + 1] = h[2 * size_t(i) + 1];
  }
  if (n)
    *n = m;
  return 0;
}

int lmmhip_persist_profile_blocks(lmmhip_ctx* c, int64_t* t, int64_t cap, int64_t* nbar, int64_t* nblk) {
  if (!c || !c->ptime.p || !c->persist_grid)
    return fail(LMMHIP_E_STATE, "no profiled persistent solve");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = 2 * size_t(kPBlkCap) * size_t(c->persist_grid);
  std::vector<long long> h(n);
  HIPCHK(hipMemcpyAsync(h.data(), c->ptime.p + 2 * size_t(kPersistProfCap), n * sizeof(long long),
                        hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < n && int64_t(i) < cap; i++)
    t[i] = h[i];
  *nbar = kPBlkCap;
  *nblk = c->persist_grid;
  return 0;
}

int lmmhip_anatomy(lmmhip_ctx* c, unsigned long long* out, int64_t cap, int64_t* n, int32_t* rounds4) {
  if (!c || !n)
    return fail(LMMHIP_E_ARG, "null argument");
  const int64_t words = int64_t(kAnatSlots) * kAnatKernels * kAnatWaves * kAnatFields;
  *n = 0;
  if (!LMM_ANAT)
    return fail(LMMHIP_E_STATE, "not an anatomy build (make EXTRA_HIPFLAGS=-DLMM_ANAT=1)");
  if (!c->anat.p || !c->solved)
    return fail(LMMHIP_E_STATE, "no solve recorded an anatomy (set LMMHIP_ANAT_ROUNDS)");
  *n = words;
  if (rounds4)
    for (int k = 0; k < kAnatSlots; k++)
      rounds4[k] = c->d.anat_r[k];
  if (out) {
    if (cap < words)
      return fail(LMMHIP_E_ARG, "anatomy: cap too small");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(out, c->anat.p, size_t(words) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  }
  return 0;
}

int lmmhip_engine_fallbacks(lmmhip_ctx* c, int64_t* n) {
  if (!c || !n)
    return fail(LMMHIP_E_ARG, "null argument");
  *n = c->persist_fallbacks;
  return 0;
}

int lmmhip_key_window(lmmhip_ctx* c, int64_t* out) {
  if (!c || !out)
    return fail(LMMHIP_E_ARG, "null argument");
  if (!c->solved || c->last_engine != LMMHIP_RAN_ROUNDS)
    return fail(LMMHIP_E_STATE, "the last solve of this context did not run the round engine");
  out[0] = int64_t(uint32_t(c->h_ctl.p[CTL_KW_BASE]));
  out[1] = c->h_ctl.p[CTL_KW_SHIFT];
  out[2] = c->h_ctl.p[CTL_KW_STORES];
  out[3] = c->h_ctl.p[CTL_KW_CLAMP];
  return 0;
}

int lmmhip_ctx_set_engine(lmmhip_ctx* c, int engine) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (engine != LMMHIP_ENGINE_PERSISTENT && engine != LMMHIP_ENGINE_ROUNDS && engine != LMMHIP_ENGINE_AUTO &&
      engine != LMMHIP_ENGINE_FRONTIER)
    return fail(LMMHIP_E_ARG, "unknown maxmin engine");
  c->engine = engine;
  return 0;
}

int lmmhip_launch_profile(lmmhip_ctx* c, int* slot, int* round, float* ms, int cap) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  int n = int(c->launch_ms.size());
  for (int i = 0; i < n && i < cap; i++) {
    slot[i] = c->launch_slot[size_t(i)];
    round[i] = c->launch_round[size_t(i)];
    ms[i] = c->launch_ms[size_t(i)];
  }
  return n;
}

int lmmhip_round_profile(lmmhip_ctx* c, int64_t* alive_vars, int64_t* alive_elems, int cap) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  const int64_t nV = c->d.nV;
  std::vector<int32_t> fr(size_t(nV > 0 ? nV : 1));
  std::vector<uint32_t> vp(size_t(nV) + 1);
  HIPCHK(hipSetDevice(c->device));
  if (nV) {
    // maxmin: vstate = exit round + 1 (0 = never fixed); fair bottleneck: fixr = last listed round
    const int32_t* src = c->last_kind == LMMHIP_KIND_MAXMIN ? c->d.vstate : c->fair.f.fixr;
    HIPCHK(hipMemcpyAsync(fr.data(), src, sizeof(int32_t) * nV, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(vp.data(), c->d.var_ptr, sizeof(uint32_t) * (nV + 1), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (c->last_kind == LMMHIP_KIND_MAXMIN)
    for (auto& f : fr)
      f -= 1;
  const int R = int(c->stats.rounds);
  // a variable is alive in rounds 0..fixr (inclusive); -1 = never processed
  std::vector<int64_t> dv(size_t(R) + 2, 0), de(size_t(R) + 2, 0);
  for (int64_t v = 0; v < nV; v++) {
    int f = fr[size_t(v)];
    if (f < 0)
      continue;
    if (f > R)
      f = R;
    dv[size_t(f)] += 1;
    de[size_t(f)] += vp[size_t(v) + 1] - vp[size_t(v)];
  }
  int64_t av = 0, ae = 0;
  for (int r = R; r >= 0; r--) {  // suffix sums
    av += dv[size_t(r)];
    ae += de[size_t(r)];
    if (r < cap) {
      alive_vars[r] = av;
      alive_elems[r] = ae;
    }
  }
  return R;
}

int lmmhip_vote_profile(lmmhip_ctx* c, int64_t* rows, int64_t* elems, int cap) {
  if (!c || !c->vstat.p)
    return fail(LMMHIP_E_STATE, "no profiled maxmin solve");
  const int R = int(std::min<int64_t>(c->stats.rounds, kStatRounds));
  std::vector<int32_t> h(size_t(2) * kStatRounds * kMaxBlocks);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpy(h.data(), c->vstat.p, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
  for (int r = 0; r < R && r < cap; r++) {
    int64_t a = 0, b = 0;
    for (int k = 0; k < kDiagSlot; k++) {
      a += h[2 * (size_t(r) * kMaxBlocks + k)];
      b += h[2 * (size_t(r) * kMaxBlocks + k) + 1];
    }
    rows[r] = a;
    elems[r] = b;
  }
  return R;
}

int lmmhip_vote_diag_profile(lmmhip_ctx* c, int64_t* out8, int cap) {
  if (!c || !c->vstat.p)
    return fail(LMMHIP_E_STATE, "no profiled maxmin solve");
  const int R = int(std::min<int64_t>(c->stats.rounds, kStatRounds));
  std::vector<int32_t> h(size_t(2) * kStatRounds * kMaxBlocks);
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemcpy(h.data(), c->vstat.p, sizeof(int32_t) * h.size(), hipMemcpyDeviceToHost));
  for (int r = 0; r < R && r < cap; r++)
    for (int k = 0; k < 8; k++)
      out8[8 * r + k] = h[2 * (size_t(r) * kMaxBlocks + kDiagSlot) + k];
  return R;
}

int lmmhip_get_values(lmmhip_ctx* c, double* out) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  if (!out && c->d.nV)
    return fail(LMMHIP_E_ARG, "null output");
  HIPCHK(hipSetDevice(c->device));
  if (c->d.nV)
    HIPCHK(hipMemcpyAsync(out, c->d.x, sizeof(double) * c->d.nV, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_get_var_rounds(lmmhip_ctx* c, int32_t* out) {
  if (!c || !c->solved || c->last_kind != LMMHIP_KIND_MAXMIN)
    return fail(LMMHIP_E_STATE, "no max-min solve to read rounds from");
  if (c->last_engine == LMMHIP_RAN_BATCH)  // mm_batch_lds keeps its rounds in LDS: vstate is not written
    return fail(LMMHIP_E_STATE, "the batch engine ran the last max-min solve: it records no per-variable rounds");
  if (!out && c->d.nV)
    return fail(LMMHIP_E_ARG, "null output");
  HIPCHK(hipSetDevice(c->device));
  if (c->d.nV)
    HIPCHK(hipMemcpyAsync(out, c->d.vstate, sizeof(int32_t) * c->d.nV, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_get_saturated(lmmhip_ctx* c, uint8_t* sat) {
  if (!c || !c->uploaded || !c->solved)
    return fail(LMMHIP_E_STATE, "no solved system");
  if (!sat && c->d.nC)
    return fail(LMMHIP_E_ARG, "null output");
  HIPCHK(hipSetDevice(c->device));
  if (c->d.nC) {
    uint8_t* o = nullptr;
    if (int rc = scratch(c, c->sat_out, c->d.nC, &o))
      return rc;
    hipLaunchKernelGGL(mm_saturated, dim3(grid_for(c->d.nC, kBlock / kWave)), dim3(kBlock), 0, c->stream, c->d,
                       c->last_prec, int(c->last_kind == LMMHIP_KIND_FAIR_BOTTLENECK), o);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sat, o, size_t(c->d.nC), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// mm_usage over the solved system into the context's usage scratch, on the context's stream (not synchronised)
static int launch_usage(lmmhip_ctx* c, double** out) {
  if (!c || !c->uploaded || !c->solved)
    return fail(LMMHIP_E_STATE, "no solved system");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = scratch(c, c->usage_out, c->d.nC, out))
    return rc;
  if (c->d.nC) {
    hipLaunchKernelGGL(mm_usage, dim3(grid_for(c->d.nC, kBlock / kWave)), dim3(kBlock), 0, c->stream, c->d, *out);
    HIPCHK(hipGetLastError());
  }
  return 0;
}

int lmmhip_get_usage(lmmhip_ctx* c, double* usage) {
  if (!c || !c->uploaded || !c->solved)
    return fail(LMMHIP_E_STATE, "no solved system");
  if (!usage && c->d.nC)
    return fail(LMMHIP_E_ARG, "null output");
  double* o = nullptr;
  if (int rc = launch_usage(c, &o))
    return rc;
  if (c->d.nC)
    HIPCHK(hipMemcpyAsync(usage, o, sizeof(double) * size_t(c->d.nC), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_usage_device_ptr(lmmhip_ctx* c, const double** dptr) {
  if (!dptr)
    return fail(LMMHIP_E_ARG, "null output");
  double* o = nullptr;
  if (int rc = launch_usage(c, &o))
    return rc;
  *dptr = o;
  return 0;
}

int lmmhip_certificate(lmmhip_ctx* c, double precision, lmmhip_cert* out, int32_t* witness) {
  if (!c || !c->uploaded || !c->solved)
    return fail(LMMHIP_E_STATE, "no solved system");
  if (!out)
    return fail(LMMHIP_E_ARG, "null output");
  HIPCHK(hipSetDevice(c->device));
  const Dev& d = c->d;
  const bool fair = c->last_kind == LMMHIP_KIND_FAIR_BOTTLENECK;
  const int gc = grid_for(d.nC, kBlock / kWave), gv = fair ? 0 : grid_for(d.nV, kBlock);
  double* top = nullptr;
  int32_t* wit = nullptr;
  lmmhip_cert* part = nullptr;  // [gc + gv] the workgroups' parts, then the result
  if (int rc = scratch(c, c->cert_top, d.nC, &top))
    return rc;
  if (int rc = scratch(c, c->cert_part, int64_t(gc) + gv + 1, &part))
    return rc;
  if (witness && !fair)
    if (int rc = scratch(c, c->cert_wit, d.nV, &wit))
      return rc;
  hipLaunchKernelGGL(cert_cnst, dim3(gc), dim3(kBlock), 0, c->stream, d, precision, top, part);
  HIPCHK(hipGetLastError());
  if (!fair) {
    hipLaunchKernelGGL(cert_var, dim3(gv), dim3(kBlock), 0, c->stream, d, precision, static_cast<const double*>(top),
                       wit, part + gc);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(cert_fold, dim3(1), dim3(kBlock), 0, c->stream, static_cast<const lmmhip_cert*>(part), gc, gv,
                     part + gc + gv);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, part + gc + gv, sizeof(lmmhip_cert), hipMemcpyDeviceToHost, c->stream));
  if (wit && d.nV)
    HIPCHK(hipMemcpyAsync(witness, wit, sizeof(int32_t) * size_t(d.nV), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (witness && fair)
    std::fill(witness, witness + d.nV, int32_t(LMMHIP_WIT_NOT_JUDGED));
  return 0;
}

int lmmhip_components(lmmhip_ctx* c, int32_t* var_label, int32_t* cnst_label, int64_t* ncomp) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  if (!ncomp || (c->d.nV && !var_label) || (c->d.nC && !cnst_label))
    return fail(LMMHIP_E_ARG, "null output");
  HIPCHK(hipSetDevice(c->device));
  const int64_t nv = c->d.nV, n = int64_t(c->d.nV) + int64_t(c->d.nC);
  *ncomp = 0;
  if (n == 0)
    return 0;
  if (n > INT32_MAX)  // union-find node ids are int32 (lmm_cc_kernels.hpp)
    return fail(LMMHIP_E_ARG, "components: variables + constraints exceed 2^31 - 1");
  int32_t *par = nullptr, *out = nullptr;
  int64_t *flag = nullptr, *rank = nullptr;
  if (int rc = scratch(c, c->cc_par, n, &par))
    return rc;
  if (int rc = scratch(c, c->cc_flag, n, &flag))
    return rc;
  if (int rc = scratch(c, c->cc_rank, n, &rank))
    return rc;
  if (int rc = scratch(c, c->cc_out, n, &out))
    return rc;
  hipLaunchKernelGGL(cc_init, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, c->stream, par, n);
  HIPCHK(hipGetLastError());
  if (nv > 0) {
    hipLaunchKernelGGL(cc_hook, dim3(grid_for(nv, kBlock)), dim3(kBlock), 0, c->stream, c->d, par);
    HIPCHK(hipGetLastError());
  }
  hipLaunchKernelGGL(cc_root, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, c->stream, par, n, flag);
  HIPCHK(hipGetLastError());
  if (int rc = dev_scan(c, flag, rank, n))
    return rc;
  hipLaunchKernelGGL(cc_label, dim3(grid_for(n, kBlock)), dim3(kBlock), 0, c->stream, par, rank, nv, n, out,
                     out + nv);
  HIPCHK(hipGetLastError());
  int rc = 0;
  const int64_t last = read_i64(c, rank + n - 1, &rc) + read_i64(c, flag + n - 1, &rc);
  if (rc)
    return rc;
  if (nv)
    HIPCHK(hipMemcpyAsync(var_label, out, size_t(nv) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (n > nv)
    HIPCHK(hipMemcpyAsync(cnst_label, out + nv, size_t(n - nv) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *ncomp = last;
  return 0;
}

int lmmhip_get_touched_vars(lmmhip_ctx* c, int32_t* ids, int64_t cap, int64_t* n) {
  if (!c || !c->uploaded || !n)
    return fail(LMMHIP_E_STATE, "no system uploaded / null count");
  const int64_t nv = c->d.nV;
  *n = nv;
  if (!ids)
    return 0;  // size query
  if (cap < nv)
    return fail(LMMHIP_E_ARG, "touched vars: output capacity below the system's variable count");
  HIPCHK(hipSetDevice(c->device));
  if (!c->res_flat) {  // lmmhip_upload: the caller's ids are the dense CSR indices
    for (int64_t v = 0; v < nv; v++)
      ids[v] = int32_t(v);
    return 0;
  }
  int32_t* o = nullptr;
  if (int rc = scratch(c, c->tv_out, nv, &o))
    return rc;
  const int64_t ns = c->res_flat_nv;
  if (ns) {
    hipLaunchKernelGGL(rs_touched, dim3(grid_for(ns, kBlock)), dim3(kBlock), 0, c->stream, ns,
                       static_cast<const int64_t*>(c->rs_vm.p), static_cast<const int64_t*>(c->rs_dv.p), o);
    HIPCHK(hipGetLastError());
  }
  if (nv)
    HIPCHK(hipMemcpyAsync(ids, o, size_t(nv) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_get_touched_cnsts(lmmhip_ctx* c, int32_t* ids, int64_t cap, int64_t* n) {
  if (!c || !c->uploaded || !n)
    return fail(LMMHIP_E_STATE, "no system uploaded / null count");
  const int64_t nc = c->d.nC;
  *n = nc;
  if (!ids)
    return 0;  // size query
  if (cap < nc)
    return fail(LMMHIP_E_ARG, "touched constraints: output capacity below the system's constraint count");
  HIPCHK(hipSetDevice(c->device));
  if (!c->res_flat) {  // lmmhip_upload: the caller's ids are the dense indices
    for (int64_t k = 0; k < nc; k++)
      ids[k] = int32_t(k);
    return 0;
  }
  // resident flatten: the list, its member mask and the mask's scan are kept with the flattened structure (the
  // refresh path reads them too)
  int32_t* o = nullptr;
  if (int rc = scratch(c, c->tc_out, nc, &o))
    return rc;
  const int64_t nl = int64_t(c->res_last_list.size());
  if (nl) {
    hipLaunchKernelGGL(rs_touched_cnsts, dim3(grid_for(nl, kBlock)), dim3(kBlock), 0, c->stream, nl,
                       static_cast<const int32_t*>(c->rs_list.p), static_cast<const int64_t*>(c->rs_lany.p),
                       static_cast<const int64_t*>(c->rs_dcl.p), o);
    HIPCHK(hipGetLastError());
  }
  if (nc)
    HIPCHK(hipMemcpyAsync(ids, o, size_t(nc) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_values_device_ptr(lmmhip_ctx* c, const double** dptr) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  *dptr = c->d.x;
  return 0;
}

int lmmhip_get_stats(lmmhip_ctx* c, lmmhip_stats* out) {
  if (!c || !out)
    return fail(LMMHIP_E_ARG, "null argument");
  *out = c->stats;
  return 0;
}

