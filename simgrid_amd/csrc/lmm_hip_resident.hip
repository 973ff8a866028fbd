// lmm_hip_resident.hip — the resident System mirror and its delta log (lmmhip_res_apply), the device flatten with
// its refresh path (lmmhip_res_flatten*), and the value fetches (lmm_resident_kernels.hpp).
#include <cstring>

#include "lmm_ctx.hpp"
#include "lmm_resident_kernels.hpp"
#include "lmm_scan.hpp"

// Flags and crossing list of the delta batches (lmmhip_ctx::res_dirty), zeroed on first use.
static int res_dirty_alloc(lmmhip_ctx* c) {
  if (c->res_dirty.p)
    return 0;
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->res_dirty.p), (4 + kResCrossCap) * sizeof(int32_t)));
  HIPCHK(hipMemsetAsync(c->res_dirty.p, 0, 4 * sizeof(int32_t), c->stream));
  return 0;
}

#define RS_LAUNCH(kern, n, ...)                                                                     \
  do {                                                                                              \
    hipLaunchKernelGGL(kern, dim3(grid_for((n) + 1, kBlock)), dim3(kBlock), 0, c->stream, __VA_ARGS__); \
    HIPCHK(hipGetLastError());                                                                      \
  } while (0)

int lmmhip_res_apply(lmmhip_ctx* c, int64_t n_elem_total, int64_t n_var_total, int64_t n_cnst_total, int64_t ne,
                     const int64_t* e_id, const int32_t* e_cnst, const double* e_weight, const uint8_t* e_flags,
                     int64_t nv, const int32_t* v_id, const int64_t* v_ebase, const int32_t* v_nelem,
                     const double* v_penalty, const double* v_bound, int64_t nc, const int32_t* c_id,
                     const double* c_bound, const uint8_t* c_flags) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (n_elem_total < 0 || n_var_total < 0 || n_cnst_total < 0 || ne < 0 || nv < 0 || nc < 0 ||
      n_var_total >= (1 << 30) || n_cnst_total >= (1 << 30) || n_elem_total > INT32_MAX)
    return fail(LMMHIP_E_ARG, "resident sizes out of range");
  if ((ne && (!e_id || !e_cnst || !e_weight || !e_flags)) ||
      (nv && (!v_id || !v_ebase || !v_nelem || !v_penalty || !v_bound)) || (nc && (!c_id || !c_bound || !c_flags)))
    return fail(LMMHIP_E_ARG, "null delta arrays");
  // host-side validation: every record lands inside the tables, every slab inside the element table
  for (int64_t i = 0; i < ne; i++)
    if (e_id[i] < 0 || e_id[i] >= n_elem_total || e_cnst[i] < -1 || e_cnst[i] >= n_cnst_total)
      return fail(LMMHIP_E_ARG, "element delta out of range");
  for (int64_t i = 0; i < nv; i++)
    if (v_id[i] < 0 || v_id[i] >= n_var_total || v_nelem[i] < -1 || v_ebase[i] < 0 ||
        v_ebase[i] + std::max(v_nelem[i], 0) > n_elem_total)
      return fail(LMMHIP_E_ARG, "variable delta out of range");
  for (int64_t i = 0; i < nc; i++)
    if (c_id[i] < 0 || c_id[i] >= n_cnst_total)
      return fail(LMMHIP_E_ARG, "constraint delta out of range");
  HIPCHK(hipSetDevice(c->device));
  ResDev& r = c->res;
  if (n_elem_total > c->res_capE) {
    const int64_t cap = std::max(n_elem_total, c->res_capE + c->res_capE / 2);
    int rc = res_grow(c, c->res_own[0], &r.e_cnst, c->res_nE, cap) | res_grow(c, c->res_own[1], &r.e_w, c->res_nE, cap) |
             res_grow(c, c->res_own[2], &r.e_fl, c->res_nE, cap);
    if (rc)
      return rc;
    c->res_capE = cap;
  }
  if (n_var_total > c->res_capV) {
    const int64_t cap = std::max(n_var_total, c->res_capV + c->res_capV / 2);
    int rc = res_grow(c, c->res_own[3], &r.v_ebase, c->res_nV, cap) | res_grow(c, c->res_own[4], &r.v_n, c->res_nV, cap) |
             res_grow(c, c->res_own[5], &r.v_pen, c->res_nV, cap) | res_grow(c, c->res_own[6], &r.v_bound, c->res_nV, cap);
    if (rc)
      return rc;
    c->res_capV = cap;
  }
  if (n_cnst_total > c->res_capC) {
    const int64_t cap = std::max(n_cnst_total, c->res_capC + c->res_capC / 2);
    int rc = res_grow(c, c->res_own[7], &r.c_bound, c->res_nC, cap) | res_grow(c, c->res_own[8], &r.c_fl, c->res_nC, cap);
    if (rc)
      return rc;
    c->res_capC = cap;
  }
  if (int rc = res_dirty_alloc(c))
    return rc;
  if (ne || n_var_total > c->res_nV || n_cnst_total > c->res_nC)
    c->res_struct_host = true;
  c->res_nE = std::max(c->res_nE, n_elem_total);
  c->res_nV = std::max(c->res_nV, n_var_total);
  c->res_nC = std::max(c->res_nC, n_cnst_total);
  if (ne) {
    const int64_t* did;
    const int32_t* dcn;
    const double* dw;
    const uint8_t* dfl;
    int rc = stage(c, 0, e_id, ne, &did) | stage(c, 1, e_cnst, ne, &dcn) | stage(c, 2, e_weight, ne, &dw) |
             stage(c, 3, e_flags, ne, &dfl);
    if (rc)
      return rc;
    RS_LAUNCH(rs_apply_e, ne, ne, did, dcn, dw, dfl, r);
  }
  if (nv) {
    const int32_t* did;
    const int64_t* deb;
    const int32_t* dn;
    const double *dp, *db;
    int rc = stage(c, 4, v_id, nv, &did) | stage(c, 5, v_ebase, nv, &deb) | stage(c, 6, v_nelem, nv, &dn) |
             stage(c, 7, v_penalty, nv, &dp) | stage(c, 8, v_bound, nv, &db);
    if (rc)
      return rc;
    RS_LAUNCH(rs_apply_v, nv, nv, did, deb, dn, dp, db, r, c->res_dirty.p);
    // the touched variables, for the refresh path (up to 1/8 of the slots: beyond that a full pass is as cheap)
    if (c->res_vl_n >= 0 && c->res_vl_n + nv <= std::max<int64_t>(4096, n_var_total / 8)) {
      int32_t* vl = nullptr;
      if (c->rs_vlist.bytes < size_t(c->res_vl_n + nv) * sizeof(int32_t)) {  // grow, keeping the list
        Scr old = std::move(c->rs_vlist);
        if (int rc = scratch(c, c->rs_vlist, std::max<int64_t>(4096, 2 * (c->res_vl_n + nv)), &vl))
          return rc;
        if (old.p && c->res_vl_n > 0)
          HIPCHK(hipMemcpyAsync(vl, old.p, size_t(c->res_vl_n) * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        HIPCHK(old.reset());
      }
      vl = static_cast<int32_t*>(c->rs_vlist.p);
      HIPCHK(hipMemcpyAsync(vl + c->res_vl_n, did, size_t(nv) * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
      c->res_vl_n += nv;
    } else {
      c->res_vl_n = -1;  // too many: the refresh path rewrites every member
    }
  }
  if (nc) {
    const int32_t* did;
    const double* db;
    const uint8_t* dfl;
    int rc = stage(c, 9, c_id, nc, &did) | stage(c, 10, c_bound, nc, &db) | stage(c, 11, c_flags, nc, &dfl);
    if (rc)
      return rc;
    RS_LAUNCH(rs_apply_c, nc, nc, did, db, dfl, r, c->res_last_prec < 0 ? 1e-5 : c->res_last_prec, c->res_dirty.p,
              c->res_dirty.p + 3, c->res_dirty.p + 4);
  }
  HIPCHK(hipStreamSynchronize(c->stream));  // host delta arrays are borrowed for the call only
  return 0;
}

static int res_flatten(lmmhip_ctx* c, bool fair, int64_t n_list, const int32_t* cnst_list, double precision,
                       int64_t* counts3) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (n_list < 0 || (n_list && !cnst_list))
    return fail(LMMHIP_E_ARG, "bad constraint list");
  for (int64_t i = 0; i < n_list; i++)
    if (cnst_list[i] < 0 || cnst_list[i] >= c->res_nC)
      return fail(LMMHIP_E_ARG, "listed constraint is not in the resident mirror");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  const ResDev& r = c->res;
  const int64_t nl = n_list, nvs = c->res_nV;
  // Refresh path: same list, same precision, no element record and no slab change since the last
  // flatten, and no constraint-bound crossing of the part test that changes the member set (rs_cross_check)
  // -> the structure (CSR/CSC, dense maps, reset mask) stands; only penalties, variable bounds and
  // constraint bounds / policies are rewritten in dense order.
  if (!fair && c->res_flat && c->res_flat_kind == LMMHIP_KIND_MAXMIN && c->uploaded && !c->res_struct_host &&
      c->res_dirty.p && precision == c->res_last_prec &&
      nvs == c->res_flat_nv && size_t(nl) == c->res_last_list.size() &&
      (nl == 0 || std::memcmp(c->res_last_list.data(), cnst_list, size_t(nl) * sizeof(int32_t)) == 0)) {
    int32_t fl4[4] = {0, 0, 0, 0};  // flags, (fair error), mixed, crossings
    HIPCHK(hipMemcpyAsync(fl4, c->res_dirty.p, sizeof(fl4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    int32_t flags = fl4[0];
    const int32_t nx = fl4[3];
    if (nx < 0 || (nx > 0 && (fl4[2] || nx > kResCrossCap || env_int("LMMHIP_RES_CROSS", 1) == 0)))
      flags |= kResStruct;
    if (!(flags & kResStruct)) {
      Dev& d = c->d;
      const int32_t* list = static_cast<const int32_t*>(c->rs_list.p);
      const int64_t* lany = static_cast<const int64_t*>(c->rs_lany.p);
      const int64_t* dcl = static_cast<const int64_t*>(c->rs_dcl.p);
      RS_LAUNCH(rs_cmeta, nl, nl, list, r, lany, dcl, nullptr, const_cast<double*>(d.cbound),
                const_cast<uint8_t*>(d.cflags));
      if (nx > 0) {  // part-test crossings: structural only if the member set changes
        const int grid = int(std::min<int64_t>(nx, 2048));
        hipLaunchKernelGGL(rs_cross_check, dim3(grid), dim3(kBlock), 0, c->stream, nx, c->res_dirty.p + 4, r,
                           precision, static_cast<const uint8_t*>(c->rs_cls.p),
                           static_cast<const uint8_t*>(c->rs_outc.p), static_cast<const int32_t*>(c->rs_posd.p),
                           d.cnst_ptr, d.csc_v, d.var_ptr, d.csr_c, d.cbound, c->res_dirty.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&flags, c->res_dirty.p, sizeof(flags), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
      }
    }
    if (!(flags & kResStruct)) {
      Dev& d = c->d;
      const int64_t* vm = static_cast<const int64_t*>(c->rs_vm.p);
      const int64_t* dv = static_cast<const int64_t*>(c->rs_dv.p);
      if (c->res_vl_n >= 0 && c->res_c2c_ok && env_int("LMMHIP_RES_VLIST", 1)) {  // the touched variables only
        const int64_t n = c->res_vl_n;
        if (n > 0)
          RS_LAUNCH(rs_refresh_vl, n, n, static_cast<const int32_t*>(c->rs_vlist.p), r, vm, dv,
                    const_cast<double*>(d.pen), const_cast<double*>(d.vbound), d.var_ptr,
                    static_cast<const int32_t*>(c->rs_c2c.p), d.csc_w, d.csc_u, d.csc_p, int(flags & kResPenalty));
      } else {
        RS_LAUNCH(rs_refresh_v, nvs, nvs, r, vm, dv, const_cast<double*>(d.pen), const_cast<double*>(d.vbound));
        if (((flags & kResPenalty) || c->res_pen_dirty) && d.nnz > 0)
          if (int rc = launch_elem_usage(c, 0))
            return rc;
      }
      c->res_vl_n = 0;
      c->res_pen_dirty = false;
      HIPCHK(hipMemsetAsync(c->res_dirty.p, 0, sizeof(int32_t), c->stream));
      HIPCHK(hipMemsetAsync(c->res_dirty.p + 3, 0, sizeof(int32_t), c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      c->res_refreshes++;
      c->sys_gen++;  // (the dense maps stand; every flatten counts, so that a rebind never depends on which path ran)
      c->res_cross_refreshes += nx > 0;
      if (counts3) {
        counts3[0] = d.nV;
        counts3[1] = d.nC;
        counts3[2] = d.nnz;
      }
      return 0;
    }
  }
  int32_t *pos, *list, *posd;
  uint8_t *lpart, *vrst, *lzero, *cls = nullptr, *lanyc = nullptr, *outc = nullptr;
  int64_t *lany, *dcl, *cdeg, *cptr, *vm, *dv, *rl, *ro;
  int rc = scratch(c, c->rs_pos, c->res_nC, &pos) | scratch(c, c->rs_list, nl, &list) |
           scratch(c, c->rs_lzero, nl, &lzero) |
           scratch(c, c->rs_lpart, nl, &lpart) | scratch(c, c->rs_lany, nl + 1, &lany) |
           scratch(c, c->rs_dcl, nl + 1, &dcl) | scratch(c, c->rs_cdeg, nl + 1, &cdeg) |
           scratch(c, c->rs_cptr, nl + 1, &cptr) | scratch(c, c->rs_vrst, nvs, &vrst) |
           scratch(c, c->rs_vm, nvs + 1, &vm) | scratch(c, c->rs_dv, nvs + 1, &dv) |
           scratch(c, c->rs_rl, nvs + 1, &rl) | scratch(c, c->rs_ro, nvs + 1, &ro) |
           scratch(c, c->rs_posd, std::max<int64_t>(c->res_nC, 1), &posd);
  if (!fair)
    rc |= scratch(c, c->rs_cls, c->res_nC, &cls) | scratch(c, c->rs_lanyc, c->res_nC, &lanyc) |
          scratch(c, c->rs_outc, c->res_nC, &outc);
  if (rc)
    return rc;
  if (nl)
    HIPCHK(hipMemcpyAsync(list, cnst_list, size_t(nl) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  if (c->res_nC)
    HIPCHK(hipMemsetAsync(pos, 0xFF, size_t(c->res_nC) * sizeof(int32_t), c->stream));
  HIPCHK(hipMemsetAsync(cdeg, 0, size_t(nl + 1) * sizeof(int64_t), c->stream));
  if (int rc = res_dirty_alloc(c))
    return rc;
  if (!fair && c->res_nC) {
    HIPCHK(hipMemsetAsync(cls, 0, size_t(c->res_nC), c->stream));
    HIPCHK(hipMemsetAsync(lanyc, 0, size_t(c->res_nC), c->stream));
    HIPCHK(hipMemsetAsync(outc, 0, size_t(c->res_nC), c->stream));
  }
  RS_LAUNCH(rs_pos, nl, nl, list, r, precision, int(fair), pos, lpart, lany, lzero, cls);
  if (fair) {
    HIPCHK(hipMemsetAsync(c->res_dirty.p + 1, 0, sizeof(int32_t), c->stream));
    RS_LAUNCH(rs_mark_fair, nvs, nvs, r, pos, lany, lzero, vrst, vm, c->res_dirty.p + 1);
  } else {
    HIPCHK(hipMemsetAsync(c->res_dirty.p + 2, 0, sizeof(int32_t), c->stream));
    RS_LAUNCH(rs_mark, nvs, nvs, r, cls, lanyc, outc, vrst, vm, rl, c->res_dirty.p + 2);
    RS_LAUNCH(rs_lany_list, nl, nl, list, lanyc, lany);
  }
  if ((rc = dev_scan(c, lany, dcl, nl + 1)))
    return rc;
  // posd[c] = dense id of constraint c, or -1: one gather per element in rs_rowlen / rs_write instead of the
  // dependent pos -> lany -> dcl chain
  if (c->res_nC)
    HIPCHK(hipMemsetAsync(posd, 0xFF, size_t(c->res_nC) * sizeof(int32_t), c->stream));
  RS_LAUNCH(rs_posd, nl, nl, list, lany, dcl, posd);
  if (fair)
    RS_LAUNCH(rs_rowlen_fair, nvs, nvs, r, pos, lany, dcl, vm, rl, cdeg);
  else  // (max-min: rs_mark counted the rows unless a member has a disabled element; CSC offsets from the sort)
    RS_LAUNCH(rs_rowlen, nvs, nvs, r, posd, vm, rl, c->res_dirty.p + 2);
  if ((rc = dev_scan(c, vm, dv, nvs + 1)) || (rc = dev_scan(c, rl, ro, nvs + 1)) ||
      (fair && (rc = dev_scan(c, cdeg, cptr, nl + 1))))
    return rc;
  const int64_t nC = read_i64(c, dcl + nl, &rc);
  const int64_t nV = read_i64(c, dv + nvs, &rc);
  const int64_t nnz = read_i64(c, ro + nvs, &rc);
  if (rc)
    return rc;
  if (nnz > INT32_MAX)
    return fail(LMMHIP_E_ARG, "resident flatten: more than 2^31 active elements");
  int64_t nch = 0;
  int64_t *nck = nullptr, *cch = nullptr;
  if (fair) {  // chunk counts before the allocation (lmm_fb_kernels.hpp)
    int32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, c->res_dirty.p + 1, sizeof(err), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (err)
      return fail(LMMHIP_E_ARG, "FairBottleneck: negative consumption weights are not supported");
    if ((rc = scratch(c, c->rs_nck, nC + 1, &nck) | scratch(c, c->rs_cch, nC + 1, &cch)))
      return rc;
    RS_LAUNCH(rs_nchunks, nC, nC, cdeg, kFbChunk, nck);
    if ((rc = dev_scan(c, nck, cch, nC + 1)))
      return rc;
    nch = read_i64(c, cch + nC, &rc);
    if (rc)
      return rc;
  }
  FlatBufs fb;
  if ((rc = alloc_flat(c, nV, nC, nnz, nch, &fb)))
    return rc;
  c->res_flat = true;
  c->res_flat_kind = fair ? LMMHIP_KIND_FAIR_BOTTLENECK : LMMHIP_KIND_MAXMIN;
  c->res_flat_nv = nvs;
  int32_t *kidx, *skey, *sval;
  WRow* wrow;
  RowPen* rowpen;
  rc = scratch(c, c->rs_rowid, nnz, &wrow) | scratch(c, c->rs_kidx, nnz, &kidx) |
       scratch(c, c->rs_skey, nnz, &skey) | scratch(c, c->rs_sval, nnz, &sval) |
       scratch(c, c->rs_rowpen, std::max<int64_t>(nV, 1), &rowpen);
  if (rc)
    return rc;
  RS_LAUNCH(rs_cmeta, nl, nl, list, r, lany, dcl, fair ? lzero : nullptr, fb.cb, fb.cf);
  RS_LAUNCH(rs_write, nvs, nvs, r, posd, vm, dv, ro, fb.vp, fb.csr_c, fb.csr_w, fb.pen, fb.vb, fb.cvar0,
            wrow, kidx, rowpen);
  const uint32_t nnz32 = uint32_t(nnz);
  HIPCHK(hipMemcpyAsync(fb.vp + nV, &nnz32, sizeof(nnz32), hipMemcpyHostToDevice, c->stream));
  if (fair)
    RS_LAUNCH(rs_ptr32, nC, nC, cptr, fb.cp);
  else if (!nnz)
    HIPCHK(hipMemsetAsync(fb.cp, 0, size_t(nC + 1) * sizeof(uint32_t), c->stream));
  if (fair)
    RS_LAUNCH(rs_chunks, nC, nC, cptr, nck, cch, kFbChunk, fb.cch, fb.chc, fb.chb);
  else
    HIPCHK(hipMemsetAsync(fb.cch, 0, size_t(nC + 1) * sizeof(int32_t), c->stream));  // no FB chunks
  if (nnz) {
    int bits = 1;
    while (bits < 31 && (int64_t(1) << bits) < nC)
      bits++;
    size_t tb = 0;
    HIPCHK(sort_pairs_i32(nullptr, tb, fb.csr_c, skey, kidx, sval, nnz, bits, c->stream));
    uint8_t* t = nullptr;
    if ((rc = scratch(c, c->rs_tmp, int64_t(tb), &t)))
      return rc;
    HIPCHK(sort_pairs_i32(t, tb, fb.csr_c, skey, kidx, sval, nnz, bits, c->stream));
    int32_t* c2c = nullptr;
    if (!fair && (rc = scratch(c, c->rs_c2c, nnz, &c2c)))
      return rc;
    RS_LAUNCH(rs_csc, nnz, nnz, sval, wrow, rowpen, fb.csc_v, fb.csc_w, c->d.csc_u, c->d.csc_p,
              c->d.csc_row, c2c);
    if (!fair)
      RS_LAUNCH(rs_cptr_sorted, nnz, nnz, nC, skey, fb.cp);
  }
  HIPCHK(hipStreamSynchronize(c->stream));  // before the host's list buffer is released
  if ((rc = finish_flat(c, nV, nC, nnz, true)))  // (rs_csc wrote the per-element usage, penalty and row)
    return rc;
  c->res_last_list.assign(cnst_list, cnst_list + nl);
  c->res_last_prec = precision;
  c->res_struct_host = false;
  c->res_c2c_ok = !fair;
  c->res_vl_n = 0;
  c->res_pen_dirty = false;
  if (c->res_dirty.p) {
    HIPCHK(hipMemsetAsync(c->res_dirty.p, 0, sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(c->res_dirty.p + 3, 0, sizeof(int32_t), c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  if (counts3) {
    counts3[0] = nV;
    counts3[1] = nC;
    counts3[2] = nnz;
  }
  return 0;
}

int lmmhip_res_flatten(lmmhip_ctx* c, int64_t n_list, const int32_t* cnst_list, double precision, int64_t* counts3) {
  return res_flatten(c, false, n_list, cnst_list, precision, counts3);
}

int lmmhip_res_flatten_fair(lmmhip_ctx* c, int64_t n_list, const int32_t* cnst_list, int64_t* counts3) {
  return res_flatten(c, true, n_list, cnst_list, 0.0, counts3);
}

int lmmhip_res_refreshes(lmmhip_ctx* c, int64_t* n) {
  if (!c || !n)
    return fail(LMMHIP_E_ARG, "null argument");
  *n = c->res_refreshes;
  return 0;
}

int lmmhip_res_cross_refreshes(lmmhip_ctx* c, int64_t* n) {
  if (!c || !n)
    return fail(LMMHIP_E_ARG, "null argument");
  *n = c->res_cross_refreshes;
  return 0;
}

// Pinned host staging of the value fetch, grown with 1/4 headroom (the headroom was computed after the
// capacity had been reset); the reset flags only for lmmhip_res_values_pinned.
static int pin_grow(lmmhip_ctx* c, int64_t n, bool with_rst) {
  if (n > c->pin_cap) {
    const int64_t cap = std::max(n, c->pin_cap + c->pin_cap / 4);
    c->pin_cap = 0;
    HIPCHK(c->pin_vals.reset());
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->pin_vals.p), size_t(cap) * sizeof(double), hipHostMallocDefault));
    c->pin_cap = cap;
  }
  if (with_rst && n > c->pin_rst_cap) {
    const int64_t cap = std::max(n, c->pin_rst_cap + c->pin_rst_cap / 4);
    c->pin_rst_cap = 0;
    HIPCHK(c->pin_rst.reset());
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&c->pin_rst.p), size_t(cap), hipHostMallocDefault));
    c->pin_rst_cap = cap;
  }
  return 0;
}

int lmmhip_res_values_pinned(lmmhip_ctx* c, int64_t n, const double** values, const uint8_t** reset) {
  if (!c || !c->uploaded || !c->res_flat)
    return fail(LMMHIP_E_STATE, "no resident flatten to read values from");
  if (n != c->res_flat_nv || !values || !reset)
    return fail(LMMHIP_E_ARG, "values: n must be the variable slot count of the last resident flatten");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = pin_grow(c, n, true))
    return rc;
  double* vout = nullptr;
  if (int rc = scratch(c, c->rs_vout, n, &vout))
    return rc;
  if (n) {  // (kernel stores straight into the mapped pinned buffers measured 1.0-1.4 ms slower in bench.py)
    const int64_t* vm = static_cast<const int64_t*>(c->rs_vm.p);
    const int64_t* dv = static_cast<const int64_t*>(c->rs_dv.p);
    RS_LAUNCH(rs_values, n, n, vm, dv, static_cast<const uint8_t*>(c->rs_vrst.p), c->d.x, vout,
              static_cast<uint8_t*>(nullptr));
    HIPCHK(hipMemcpyAsync(c->pin_vals.p, vout, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->pin_rst.p, c->rs_vrst.p, size_t(n), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  *values = c->pin_vals.p;
  *reset = c->pin_rst.p;
  return 0;
}

int lmmhip_res_values_sliced(lmmhip_ctx* c, int64_t n, int nslices, const double** values) {
  if (!c || !c->uploaded || !c->res_flat)
    return fail(LMMHIP_E_STATE, "no resident flatten to read values from");
  if (n != c->res_flat_nv || !values || nslices < 1 || nslices > 256)
    return fail(LMMHIP_E_ARG, "values: n must be the last resident flatten's slot count, 1 <= nslices <= 256");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = pin_grow(c, n, false))
    return rc;
  while (int(c->ev_slice.size()) < nslices) {
    Event ev;
    HIPCHK(hipEventCreateWithFlags(&ev.p, hipEventDisableTiming));
    c->ev_slice.push_back(std::move(ev));
  }
  double* vout = nullptr;
  if (int rc = scratch(c, c->rs_vout, n, &vout))
    return rc;
  if (n) {
    const int64_t* vm = static_cast<const int64_t*>(c->rs_vm.p);
    const int64_t* dv = static_cast<const int64_t*>(c->rs_dv.p);
    RS_LAUNCH(rs_values_mark, n, n, vm, dv, static_cast<const uint8_t*>(c->rs_vrst.p), c->d.x,
              reinterpret_cast<unsigned long long*>(vout));
  }
  const int64_t per = (n + nslices - 1) / nslices;
  for (int i = 0; i < nslices; i++) {
    const int64_t lo = std::min(n, i * per), hi = std::min(n, lo + per);
    if (hi > lo)
      HIPCHK(hipMemcpyAsync(c->pin_vals.p + lo, vout + lo, size_t(hi - lo) * sizeof(double), hipMemcpyDeviceToHost,
                            c->stream));
    HIPCHK(hipEventRecord(c->ev_slice[size_t(i)].p, c->stream));
  }
  *values = c->pin_vals.p;
  return 0;
}

int lmmhip_res_values_wait(lmmhip_ctx* c, int slice) {
  if (!c || slice < 0 || slice >= int(c->ev_slice.size()))
    return fail(LMMHIP_E_ARG, "no such slice");
  HIPCHK(hipEventSynchronize(c->ev_slice[size_t(slice)].p));
  return 0;
}

int lmmhip_res_values(lmmhip_ctx* c, int64_t n, double* values, uint8_t* reset) {
  if (!c || !c->uploaded || !c->res_flat)
    return fail(LMMHIP_E_STATE, "no resident flatten to read values from");
  if (n != c->res_flat_nv || (n && (!values || !reset)))
    return fail(LMMHIP_E_ARG, "values: n must be the variable slot count of the last resident flatten");
  HIPCHK(hipSetDevice(c->device));
  double* vout = nullptr;
  if (int rc = scratch(c, c->rs_vout, n, &vout))
    return rc;
  const int64_t* vm = static_cast<const int64_t*>(c->rs_vm.p);
  const int64_t* dv = static_cast<const int64_t*>(c->rs_dv.p);
  if (n) {
    RS_LAUNCH(rs_values, n, n, vm, dv, static_cast<const uint8_t*>(c->rs_vrst.p), c->d.x, vout,
              static_cast<uint8_t*>(nullptr));
    HIPCHK(hipMemcpyAsync(values, vout, size_t(n) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(reset, c->rs_vrst.p, size_t(n), hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
