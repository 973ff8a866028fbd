// lmm_hip_fair.hip — FairBottleneck (lmmhip_solve's LMMHIP_KIND_FAIR_BOTTLENECK, lmm_ctx.hpp): the chunked engine
// and its sharded protocol lmmhip_fb_shard_* (lmm_fb_kernels.hpp), and the batch engine of a declared
// block-diagonal system (lmm_fb_batch_kernels.hpp).
#include <chrono>

#include "lmm_ctx.hpp"
#include "lmm_fb_batch_kernels.hpp"
#include "lmm_fb_kernels.hpp"
#include "lmm_scan.hpp"

// The launches below take the view of the solve they belong to: solve_fair's (its long-constraint list, the locality
// order and, paced, the progress words) or a sharded call's (shard_view).
static int fb_begin(lmmhip_ctx* c, const FbDev& d, double prec) {
  c->fair.round = 0;
  c->fair.prec = prec;
  LAUNCH(0, -1, fb_init, grid_for(std::max(d.nV, d.nC), kBlock), kBlock, d);
  return 0;
}

// One phase of a fair-bottleneck round (lmm_fb_kernels.hpp); phase 2 ends the round.
static int fb_phase(lmmhip_ctx* c, const FbDev& d, int phase) {
  FairEngine& e = c->fair;
  const int64_t r = e.round;
  const int par = int(r & 1);
  const int gQ = grid_for(d.nch, kBlock / kWave);
  const int gC = grid_for(d.nC, kBlock);
  const int gV = grid_for(d.nV, kBlock);
  switch (phase) {
  case 0:  // round 0 lists every flattened variable (fair_bottleneck.cpp:29-41): counts without gathers
    if (r > 0)
      LAUNCH(2, r, fb_pack_vst, grid_for((int64_t(d.nV) + 31) / 32, kBlock), kBlock, d);
    LAUNCH(2, r, fbk_count, gQ, kBlock, d, int(r == 0));
    LAUNCH(2, r, fbk_nb, gC, kBlock, d, par);
    break;
  case 1:
    LAUNCH(3, r, fbk_share, gC, kBlock, d, par);
    LAUNCH(3, r, fb_var_inc, gV, kBlock, d, par, int(r));
    if (e.shard_xnb) {  // shards: this shard's mu into the gathered vector, then the caller's all-gather
      LAUNCH(3, r, fbo_put_mu, gV, kBlock, d, e.owner);
      break;
    }
    LAUNCH(4, r, fbk_acc, gQ, kBlock, d, int(r == 0), e.longmin);
    LAUNCH(4, r, fbk_accc, gC, kBlock, d);
    break;
  case 2:
    if (e.shard_xnb) {  // the owned constraints' chains from the gathered mu -> xrem (all-gathered)
      LAUNCH(4, r, fbo_acc, grid_for(e.owner.nch, kBlock / kWave), kBlock, d, e.owner);
      LAUNCH(5, r, fbo_chain, grid_for(e.owner.nc, kBlock / kWave), kBlock, d, e.owner, e.prec);
      break;
    }
    // one context: element by element in the CSC order, bit-identical to the reference
    LAUNCH(5, r, fbk_update_seq, e.nlb + grid_for(d.nC, kBlock / kWave), kBlock, d, e.prec, e.longmin, e.nlb);
    LAUNCH(5, r, fbk_unlist, gQ, kBlock, d, int(r > 0));  // (vstb is packed in rounds > 0)
    e.round++;
    break;
  case 3:
    if (!e.shard_xnb)
      return fail(LMMHIP_E_ARG, "phase 3 exists only in a sharded solve");
    LAUNCH(5, r, fbo_apply, gC, kBlock, d, e.owner);
    LAUNCH(5, r, fbk_unlist, gQ, kBlock, d, int(r > 0));  // (vstb is packed in rounds > 0)
    e.round++;
    break;
  default:
    return fail(LMMHIP_E_ARG, "fair-bottleneck phase must be 0..2 (one context) or 0..3 (shard)");
  }
  return 0;
}

// The locality order of the one-context FairBottleneck's mu gathers (lmm_fb_kernels.hpp fbp_*): once per
// uploaded system, outside the solve.  LMMHIP_FB_PERM=0 gathers mu by variable id instead (measurement knob): the
// view's mu_p stays null.
static int fb_perm(lmmhip_ctx* c, FbDev& d) {
  if (!env_int("LMMHIP_FB_PERM", 1) || d.nV == 0)
    return 0;
  int32_t *v0, *v1;
  unsigned long long *k0, *k1;
  int rc = scratch(c, c->fair.k0, d.nV, &k0);
  rc = rc ? rc : scratch(c, c->fair.k1, d.nV, &k1);
  rc = rc ? rc : scratch(c, c->fair.v0, d.nV, &v0);
  rc = rc ? rc : scratch(c, c->fair.v1, d.nV, &v1);
  rc = rc ? rc : scratch(c, c->fair.perm, d.nV, &d.vperm);
  rc = rc ? rc : scratch(c, c->fair.cscvp, std::max<int64_t>(d.nnz, 1), &d.csc_vp);
  rc = rc ? rc : scratch(c, c->fair.mu, d.nV, &d.mu_p);
  if (rc)
    return rc;
  if (!c->fair.perm_ok) {
    const unsigned long long span = (unsigned long long)d.nC * (unsigned long long)d.nC + 1;
    const int bits = std::min(64, 64 - __builtin_clzll(span));
    hipLaunchKernelGGL(fbp_keys, dim3(grid_for(d.nV, kBlock)), dim3(kBlock), 0, c->stream, d, k0, v0);
    HIPCHK(hipGetLastError());
    size_t tb = 0;
    HIPCHK(sort_pairs_u64_i32(nullptr, tb, k0, k1, v0, v1, d.nV, 64, c->stream));
    uint8_t* t = nullptr;
    if ((rc = scratch(c, c->fair.tmp, int64_t(tb), &t)))
      return rc;
    // (keys of empty rows are all ones: sorted with the 64-bit width when the span needs it)
    HIPCHK(sort_pairs_u64_i32(t, tb, k0, k1, v0, v1, d.nV, bits < 64 ? 64 : bits, c->stream));
    hipLaunchKernelGGL(fbp_inv, dim3(grid_for(d.nV, kBlock)), dim3(kBlock), 0, c->stream, d, v1);
    HIPCHK(hipGetLastError());
    if (d.nnz > 0) {
      hipLaunchKernelGGL(fbp_csc, dim3(grid_for(d.nnz, kBlock)), dim3(kBlock), 0, c->stream, d);
      HIPCHK(hipGetLastError());
    }
    c->fair.perm_ok = true;
  }
  return 0;
}

static int solve_fair_rounds(lmmhip_ctx* c, FbDev& d, double prec) {
  if (int rc = fb_begin(c, d, prec))
    return rc;
  // The reference's rounds are not bounded by the system size (FATPIPE remaining can shrink
  // geometrically: millions of rounds on 60-variable systems); give up past this budget.
  const int64_t max_rounds = 64 * (int64_t(d.nV) + int64_t(d.nC)) + 4096;
  // (LMMHIP_FB_PACE=0) One round queued ahead of the termination poll: after round r the control words go to a pinned
  // slot (mm_ctl_out), round r + 1 is queued, then the host waits for round r's words.  A FairBottleneck round is
  // long (C5: 0.2-3 ms), so the GPU never waits on the host and at most one empty round (its launches return
  // at once) runs after the last one; chunks of 4, 8, ... rounds left up to 7 empty rounds (63 launches,
  // ~0.2 ms on C5) plus a host round trip between chunks.
  // Pacing by progress words (default; LMMHIP_FB_PACE=0: the polls below): fbk_share stores the number of rounds
  // it has started into a pinned host word, or "done" beside it when nothing is listed (lmm_fb_kernels.hpp), and the
  // host queues round r + 1 once round r's fbk_share has started — the rest of round r (its chains: 0.1-1 ms on C5)
  // covers the queueing, no copy kernel or event per round, and no returning round after the one that finds the
  // solve over.  Round 6, C5: 7.94-7.96 ms against 7.99-8.00 with LMMHIP_FB_PACE=0 (one box, scripts/gpu_r06_o.sh),
  // 7.82-7.93 against 7.92-7.93 for the previous build (scripts/gpu_r06_p.sh).
  if (env_int("LMMHIP_FB_PACE", 1)) {
    volatile int32_t* hp = c->h_ctl.p + 3 * CTL_WORDS;
    hp[0] = 0;
    hp[1] = 0;
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void**>(&d.hprog), c->h_ctl.p + 3 * CTL_WORDS, 0));
    // rounds shorter than the host's queueing of the next one (small systems: a round is its ~9 launches) would
    // leave the GPU idle under this pacing, so when the rounds come faster than every 150 us one round stays queued
    // ahead (lag 1), as with the polls below
    int lag = 0;
    auto t_last = std::chrono::steady_clock::now();
    for (;;) {
      for (int ph = 0; ph < 3; ph++)
        if (int rc = fb_phase(c, d, ph))
          return rc;
      const int32_t want = int32_t(c->fair.round) - lag;  // rounds started, counting the one just queued
      for (unsigned spin = 0;; spin++) {
        if (hp[1] || hp[0] >= want) {
          const auto t = std::chrono::steady_clock::now();
          lag = t - t_last < std::chrono::microseconds(150) ? 1 : 0;
          t_last = t;
          break;
        }
        if ((spin & 1023) == 1023) {  // everything queued has run (a guard: the words should have said so)
          const hipError_t q = hipStreamQuery(c->stream);
          if (q == hipSuccess)
            break;
          if (q != hipErrorNotReady)
            return fail(LMMHIP_E_HIP, std::string("fair-bottleneck pacing: ") + hipGetErrorString(q));
        }
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
      }
      if (hp[1])
        break;
      if (c->fair.round > max_rounds)
        return fail(LMMHIP_E_NOCONVERGE, "fair-bottleneck round guard tripped");
    }
    return poll_ctl(c);
  }
  CtlPoll poll;
  if (int rc = poll.init(c))
    return rc;
  for (;;) {
    for (int ph = 0; ph < 3; ph++)
      if (int rc = fb_phase(c, d, ph))
        return rc;
    const int32_t* h = nullptr;
    if (int rc = poll.step(d, c->fair.round, false, &h))
      return rc;
    if (h && h[CTL_DONE])
      break;
    if (c->fair.round > max_rounds)
      return fail(LMMHIP_E_NOCONVERGE, "fair-bottleneck round guard tripped");
  }
  return poll_ctl(c);  // (the queued round has run: final words for the stats)
}

int solve_fair(lmmhip_ctx* c, double prec) {
  c->ran_engine = LMMHIP_RAN_FB_ROUNDS;
  FairEngine& e = c->fair;
  e.shard_xnb = nullptr;
  // shared constraints of at least this many elements get their increments precomputed element-parallel
  // (fbk_acc) and streamed into their chains (fb_chain); shorter ones compute them inside the chain
  // (fb_chain_pull).  Pulling in round 0 and streaming fbk_acc's listed-variable rewrites afterwards measured
  // 3 % slower on C5 (9.68 vs 9.42 ms, same box): the increments' gathers move, they do not go away.
  e.longmin = uint32_t(std::max(0, env_int("LMMHIP_FB_LONG", 16384)));
  if (e.fbd_cap < c->d.nnz) {  // increments in CSC order (fbk_acc -> fbk_update_seq)
    if (int rc = dalloc(c, &e.f.fbd, c->d.nnz))
      return rc;
    e.fbd_cap = c->d.nnz;
  }
  FbDev d{c->d, e.f};  // (the context's own exchange buffers; what follows is this solve's alone)
  if (int rc = scratch(c, e.longl, int64_t(d.nC) + 1, &d.fb_long))  // the long shared constraints
    return rc;
  HIPCHK(hipMemsetAsync(d.fb_long, 0, sizeof(int32_t), c->stream));
  hipLaunchKernelGGL(fb_long_list, dim3(grid_for(d.nC, kBlock)), dim3(kBlock), 0, c->stream, d, e.longmin);
  HIPCHK(hipGetLastError());
  // the long chains by LMMHIP_FB_LONGWG workgroups
  e.nlb = std::max(1, env_int("LMMHIP_FB_LONGWG", kLongBlocks));
  if (int rc = fb_perm(c, d))
    return rc;
  return solve_fair_rounds(c, d, prec);
}

// ---- block-diagonal batches: one workgroup per system, the system in LDS (lmm_fb_batch_kernels.hpp) ----
// The conditions of batch_fits (lmm_hip_maxmin.hip), with this kernel's LDS layout.
bool fb_batch_fits(const lmmhip_ctx* c) {
  if (c->bt_n <= 0 || c->profiling)
    return false;
  if (const char* e = std::getenv("LMMHIP_BATCH"); e && *e == '0')
    return false;
  return c->bt_max_nv < 65535 && c->bt_max_nc < 65535 && c->bt_max_nnz < 65535 &&
         fb_batch_lds_bytes(c->bt_max_nv, c->bt_max_nc, c->bt_max_nnz) <= kBatchLdsMax;
}

int solve_fair_batch(lmmhip_ctx* c, double prec) {
  c->ran_engine = LMMHIP_RAN_FB_BATCH;
  c->fair.shard_xnb = nullptr;
  size_t lds = fb_batch_lds_bytes(c->bt_max_nv, c->bt_max_nc, c->bt_max_nnz);
  // both copies of the weights in LDS too when the budget allows (LMMHIP_FB_BATCH_WLDS=0: never; measurement)
  const bool wl = lds + fb_batch_lds_weights(c->bt_max_nnz) <= kBatchLdsMax && env_int("LMMHIP_FB_BATCH_WLDS", 1);
  if (wl)
    lds += fb_batch_lds_weights(c->bt_max_nnz);
  const void* kern = wl ? reinterpret_cast<const void*>(&fbk_batch_lds<true>)
                        : reinterpret_cast<const void*>(&fbk_batch_lds<false>);
  int per_cu = 0;
  HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(kBatchLdsMax)));
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kFBB, lds));
  int64_t grid = std::max<int64_t>(1, std::min<int64_t>(c->bt_n, int64_t(c->n_cu) * std::max(per_cu, 1)));
  // LMMHIP_FB_BATCH_GRID=n: at most n workgroups (tests, measurement: several systems per workgroup's LDS)
  if (const int cap = env_int("LMMHIP_FB_BATCH_GRID", 0); cap > 0)
    grid = std::min<int64_t>(grid, cap);
  if (grid > c->bt_cap) {
    HIPCHK(c->bt_rounds.reset());
    c->bt_cap = 0;
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->bt_rounds.p), sizeof(int32_t) * size_t(grid)));
    c->bt_cap = grid;
  }
  // the chunked engine's budget for this input (solve_fair_rounds): the union's sizes
  const int64_t budget = 64 * (int64_t(c->d.nV) + int64_t(c->d.nC)) + 4096;
  const int max_rounds = int(std::min<int64_t>(budget, INT32_MAX - 1));
  const FbDev d{c->d, c->fair.f};
  if (wl)
    hipLaunchKernelGGL(fbk_batch_lds<true>, dim3(unsigned(grid)), dim3(kFBB), lds, c->stream, d, c->bt_voff.p,
                       c->bt_coff.p, c->bt_n, prec, c->bt_max_nv, c->bt_max_nc, c->bt_max_nnz, max_rounds,
                       c->bt_rounds.p);
  else
    hipLaunchKernelGGL(fbk_batch_lds<false>, dim3(unsigned(grid)), dim3(kFBB), lds, c->stream, d, c->bt_voff.p,
                       c->bt_coff.p, c->bt_n, prec, c->bt_max_nv, c->bt_max_nc, c->bt_max_nnz, max_rounds,
                       c->bt_rounds.p);
  HIPCHK(hipGetLastError());
  c->stats.kernel_launches[2] += 1;
  HIPCHK(hipEventRecord(c->ev1.p, c->stream));
  c->ev1_done = true;
  if (int rc = batch_rounds_to_ctl(c, int(grid)))  // CTL_ROUNDS = the maximum over the systems, CTL_ERR
    return rc;
  if (int rc = poll_ctl(c))
    return rc;
  if (c->h_ctl.p[CTL_ERR] == 2)
    return fail(LMMHIP_E_NOCONVERGE, "batch fair-bottleneck round guard tripped");
  return 0;
}

int lmmhip_fb_shard_owner(lmmhip_ctx* c, int64_t n_own, const int32_t* own_cnst, const int64_t* optr,
                          const int32_t* ovar, const double* oweight, const int32_t* cpos, int64_t n_mu,
                          int64_t n_rem) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  const Dev& d = c->d;
  if (n_own < 0 || n_own > d.nC || n_mu < 0 || n_rem < 0 || (n_own > 0 && (!own_cnst || !optr)) ||
      (d.nC > 0 && !cpos))
    return fail(LMMHIP_E_ARG, "bad owner arguments");
  const int64_t onnz = n_own > 0 ? optr[n_own] : 0;
  if (n_own > 0 && optr[0] != 0)
    return fail(LMMHIP_E_ARG, "optr must start at 0");
  if (onnz > INT32_MAX || (onnz > 0 && (!ovar || !oweight)))
    return fail(LMMHIP_E_ARG, "bad owned elements");
  std::vector<uint32_t> op(size_t(n_own) + 1, 0);
  std::vector<int32_t> och_o;
  std::vector<uint32_t> och_b;
  for (int64_t i = 0; i < n_own; i++) {
    if (own_cnst[i] < 0 || own_cnst[i] >= d.nC || optr[i + 1] < optr[i])
      return fail(LMMHIP_E_ARG, "owned constraint id / offsets out of range");
    op[size_t(i) + 1] = uint32_t(optr[i + 1]);
    for (int64_t b = optr[i]; b < optr[i + 1]; b += kFbChunk) {
      och_o.push_back(int32_t(i));
      och_b.push_back(uint32_t(b));
    }
  }
  for (int64_t j = 0; j < onnz; j++)
    if (ovar[j] < 0 || ovar[j] >= n_mu || !(oweight[j] > 0))
      return fail(LMMHIP_E_ARG, "owned element: variable position outside the gathered mu, or weight <= 0");
  for (int64_t k = 0; k < d.nC; k++)
    if (cpos[k] < 0 || cpos[k] >= n_rem)
      return fail(LMMHIP_E_ARG, "cpos outside the gathered remaining");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  free_owner(c);
  FbOwner& o = c->fair.owner;
  auto get = [&](auto** p, int64_t n, const auto* src) { return c->fair.owner_allocs.alloc(p, n, src, c->stream); };
  int32_t *oc, *ov, *cho, *cp;
  uint32_t *opp, *chb;
  double* ow;
  int rc = 0;
  rc |= get(&oc, n_own, own_cnst);
  rc |= get(&opp, n_own + 1, op.data());
  rc |= get(&ov, onnz, ovar);
  rc |= get(&ow, onnz, oweight);
  rc |= get(&cho, int64_t(och_o.size()), och_o.data());
  rc |= get(&chb, int64_t(och_b.size()), och_b.data());
  rc |= get(&cp, d.nC, cpos);
  rc |= get(&o.fbd, onnz, static_cast<const double*>(nullptr));
  if (rc) {
    free_owner(c);
    return rc;
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  o.nc = int32_t(n_own);
  o.nch = int32_t(och_o.size());
  o.oc = oc;
  o.optr = opp;
  o.ovar = ov;
  o.ow = ow;
  o.och_o = cho;
  o.och_b = chb;
  o.cpos = cp;
  c->fair.owner_ready = true;
  c->fair.owner_nmu = n_mu;
  return 0;
}

// The view a sharded call launches with: the caller's all-reduced counts for the context's own, and what only
// solve_fair sets (the locality order, the long-constraint list, the progress words) null — the shard kernels gather
// mu by variable id.
static FbDev shard_view(const lmmhip_ctx* c) {
  FbDev d{c->d, c->fair.f};
  d.xnb = c->fair.shard_xnb;
  return d;
}

int lmmhip_fb_shard_begin(lmmhip_ctx* c, double precision, int32_t* xnb, double* xmu, int64_t mu_off, double* xrem) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  if (!c->fair.owner_ready)
    return fail(LMMHIP_E_STATE, "lmmhip_fb_shard_owner first");
  if (!xnb || !xmu || !xrem)
    return fail(LMMHIP_E_ARG, "null exchange buffer");
  if (mu_off < 0 || mu_off + c->d.nV > c->fair.owner_nmu)
    return fail(LMMHIP_E_ARG, "this shard's mu block lies outside the gathered mu");
  HIPCHK(hipSetDevice(c->device));
  c->pool_used = 0;
  c->launch_slot.clear();
  c->launch_round.clear();
  c->launch_ms.clear();
  HIPCHK(hipMemsetAsync(c->d.ctl, 0, CTL_ALLOC * sizeof(int32_t), c->stream));
  c->fair.shard_xnb = xnb;
  c->fair.owner.xmu = xmu;
  c->fair.owner.xrem = xrem;
  c->fair.owner.mu_off = mu_off;
  c->last_kind = LMMHIP_KIND_FAIR_BOTTLENECK;
  return fb_begin(c, shard_view(c), precision);
}

int lmmhip_fb_shard_step(lmmhip_ctx* c, int phase) {
  if (!c || !c->fair.shard_xnb)
    return fail(LMMHIP_E_STATE, "lmmhip_fb_shard_begin first");
  HIPCHK(hipSetDevice(c->device));
  return fb_phase(c, shard_view(c), phase);
}

int lmmhip_fb_shard_pack_mu(lmmhip_ctx* c, int32_t* pos, double* mu, int32_t* count) {
  if (!c || !c->fair.shard_xnb)
    return fail(LMMHIP_E_STATE, "lmmhip_fb_shard_begin first");
  if (!pos || !mu || !count)
    return fail(LMMHIP_E_ARG, "null buffer");
  HIPCHK(hipSetDevice(c->device));
  const FbDev d = shard_view(c);
  LAUNCH(3, c->fair.round, fbo_pack_mu, grid_for(d.nV, kBlock), kBlock, d, c->fair.owner, int(c->fair.round == 0), pos,
         mu, count);
  return 0;
}

int lmmhip_fb_work(lmmhip_ctx* c, int64_t* out3) {
  if (!c || !out3)
    return fail(LMMHIP_E_ARG, "null argument");
  if (c->last_kind != LMMHIP_KIND_FAIR_BOTTLENECK)
    return fail(LMMHIP_E_STATE, "the last solve was not a FairBottleneck solve");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = poll_ctl(c))
    return rc;
  uint64_t sl[3 * kFbwSlots];
  HIPCHK(hipMemcpy(sl, c->d.ctl + CTL_FBW_AT, sizeof sl, hipMemcpyDeviceToHost));
  for (int k = 0; k < 3; k++) {
    uint64_t v = 0;
    for (int i = 0; i < kFbwSlots; i++)
      v += sl[k * kFbwSlots + i];
    out3[k] = int64_t(v);
  }
  return 0;
}

int lmmhip_fb_shard_poll(lmmhip_ctx* c, int* done, int64_t* rounds) {
  if (!c || !c->fair.shard_xnb)
    return fail(LMMHIP_E_STATE, "lmmhip_fb_shard_begin first");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = poll_ctl(c))
    return rc;
  if (done)
    *done = c->h_ctl.p[CTL_DONE];
  if (rounds)
    *rounds = c->h_ctl.p[CTL_ROUNDS];
  c->stats.rounds = c->h_ctl.p[CTL_ROUNDS];
  return 0;
}
