// lmm_ctx.hpp — the device context and what the driver's translation units share (private: not installed).
//
//   lmm_hip.hip           context, flat allocation and upload, lmmhip_solve, setters, getters, profile exports;
//                         owns lmm_common_kernels.hpp and lmm_cc_kernels.hpp
//   lmm_hip_maxmin.hip    the round, frontier, persistent and batch max-min engines; the first two are chains of
//                         launches: a plan per solve (RoundPlan / FrontierPlan below) and one chunk driver (run_chunks)
//   lmm_hip_fair.hip      FairBottleneck: the chunked engine, its sharded protocol, and the batch engine
//   lmm_hip_resident.hip  the resident mirror, the device flatten and the value fetches
//   lmm_hip_step.hip      the model-side action state
//
// Every __global__ kernel is compiled in exactly one of them (each kernel header is included by one unit); a
// kernel another unit needs is reached through a host function declared here.
//
// Three types carry the system to the device (lmm_dev.hpp).  Dev, the context's `d`: the flattened system and the
// max-min state the round, persistent and batch engines and the getters share; their kernels take it (the round
// engine a copy with its mode's buffers).  FrDev = Dev + FrFields: the frontier engine's kernels alone; built per
// solve by solve_maxmin_frontier from the FrontierEngine's buffers.  FbDev = Dev + FbFields: the FairBottleneck
// kernels alone; built per solve, and per call of the sharded protocol, from the FairEngine's `f`.  An engine cannot
// name another's fields, and none of them is ever written into the context's Dev.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "../../include/lmm/lmm_hip.h"
#include "lmm_dev.hpp"
#include "lmm_chunk.hpp"
#include "lmm_round_mode.hpp"

using namespace lmmdev;

inline thread_local std::string g_err;  // lmmhip_last_error

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPCHK(expr)                                                                                    \
  do {                                                                                                  \
    hipError_t e_ = (expr);                                                                             \
    if (e_ != hipSuccess)                                                                               \
      return fail(LMMHIP_E_HIP, std::string(#expr " -> ") + hipGetErrorString(e_) + " @" + __FILE__ + \
                                    ":" + std::to_string(__LINE__));                                    \
  } while (0)

// Integer knob from the environment (A/B switches, documented where read).
inline int env_int(const char* name, int dflt) {
  const char* v = std::getenv(name);
  return v && *v ? std::atoi(v) : dflt;
}

// ---- owners: every allocation, event and stream has one, which releases it in its destructor ----
struct DevFree {
  hipError_t operator()(void* p) const { return hipFree(p); }
};
struct PinFree {
  hipError_t operator()(void* p) const { return hipHostFree(p); }
};
struct EventFree {
  hipError_t operator()(hipEvent_t e) const { return hipEventDestroy(e); }
};
struct StreamFree {
  hipError_t operator()(hipStream_t s) const { return hipStreamDestroy(s); }
};
template <class H, class Free> struct Owned {  // move-only handle; p is filled by the creating HIP call (&x.p)
  H p{};
  Owned() = default;
  Owned(Owned&& o) noexcept : p(std::exchange(o.p, H{})) {}
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) {
      (void)reset();
      p = std::exchange(o.p, H{});
    }
    return *this;
  }
  ~Owned() { (void)reset(); }
  hipError_t reset() { return p ? Free{}(std::exchange(p, H{})) : hipSuccess; }
};
template <class T> using DevPtr = Owned<T*, DevFree>;  // hipMalloc
template <class T> using PinPtr = Owned<T*, PinFree>;  // hipHostMalloc
using Event = Owned<hipEvent_t, EventFree>;
using Stream = Owned<hipStream_t, StreamFree>;

// Scratch buffer: grown on demand (scratch()), contents not kept.
struct Scr : DevPtr<void> {
  size_t bytes = 0;
  Scr() = default;
  Scr(Scr&& o) noexcept : DevPtr<void>(std::move(o)), bytes(std::exchange(o.bytes, 0)) {}
  Scr& operator=(Scr&& o) noexcept {
    DevPtr<void>::operator=(std::move(o));
    bytes = std::exchange(o.bytes, 0);
    return *this;
  }
};

// Device allocations released together: mid-life by clear(), else with the context.
struct Arena {
  std::vector<void*> v;
  Arena() = default;
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;
  ~Arena() { clear(); }
  void clear() {
    for (void* p : v)
      (void)hipFree(p);
    v.clear();
  }
  // n (at least one) elements of T, filled from `src` on `stream` when given
  template <class T> int alloc(T** out, int64_t n, const T* src = nullptr, hipStream_t stream = nullptr) {
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, size_t(n > 0 ? n : 1) * sizeof(T)));
    v.push_back(p);
    *out = static_cast<T*>(p);
    if (src && n > 0)
      HIPCHK(hipMemcpyAsync(p, src, size_t(n) * sizeof(T), hipMemcpyHostToDevice, stream));
    return 0;
  }
};

// Device buffers of one flattened system: allocated by alloc_flat, filled by the host upload
// (lmmhip_upload) or on the device by the resident flatten (lmmhip_res_flatten).
struct FlatBufs {
  uint32_t *vp, *cp, *chb;
  int32_t *csr_c, *csc_v, *cvar0, *chc, *cch;
  double *csr_w, *csc_w, *pen, *vb, *cb;
  uint8_t* cf;
};

// ---- the engines' entry points (lmmhip_solve dispatches to them) and their private state ----
// round engine (lmm_hip_maxmin.hip solve_maxmin), the buffers of its mode (lmm_round_mode.hpp): the packed row records
// of RowForm Rec8 / Rec16, the vote mode's ready queue and the update's segments
struct RoundEngine {
  Scr crec[3], rdq[2], rqst, useg, ucnt;
  Scr cmpbits;  // RowForm::Rec16: the compaction count's alive bits, one per row
  Scr kwmm;     // the init's per-workgroup extremes of the alive ratios (mm_key_window)
};
// What one round-engine solve launches (round_plan: the context, the system's sizes and the environment, read once per
// solve — tests change the environment between solves); const from there on, handed to everything that launches.
using VoteKernel = void (*)(Dev, int);          // (s, round)
using SatKernel = void (*)(Dev, int, int);      // (s, round, segments)
using UpdKernel = void (*)(Dev, int, double);   // (s, round, prec)
struct RoundPlan {
  // the vote mode (lmm_round_mode.hpp): the RowForm the re-votes read (short rows: LMMHIP_CREC, LMMHIP_CMP_ROWS); on
  // the record forms the ready queue in place of the mm_ready pass (LMMHIP_RDQ) and the filter retiring the rows of
  // saturated targets (LMMHIP_SATKEY)
  VoteMode mode;
  // the vote: the LDS-bitmap form (null: never; one 1024-thread workgroup per CU) while the alive rows (host view) are
  // at least vote_bits_rows, else the scan form (one lane per row of the work queue / mm_vote<G>)
  VoteKernel vote_bitmap = nullptr, vote_scan = nullptr;
  int64_t vote_bits_rows = 0;
  SatKernel saturate = nullptr;  // mm_saturate<K> / mm_saturate_q<K>
  int sat_waves = 4;             // its K: waves per ready constraint
  bool upd_quad = false;         // the update's touched records as one 64-B request per quad (LMMHIP_UPD_QUAD)
  UpdKernel update = nullptr;    // mm_update<UpdMode{mode.queue, upd_quad}>
  // grids and caps
  int g_init_c = 1, g_c = 1;  // mm_init_cnsts (a wave per constraint), thread per constraint
  int g_upd = 1;              // mm_update and mm_done's argument: capped identity grid, or the ready-queue segments'
  int cap_sat = 0, sat_max = 0;  // saturation: grid cap (0: none), block cap of the uncapped grid
  // cadences: compaction of the alive rows (every cmp_every rounds, rewritten under cmp_pct % alive), constraint list
  int cmp_every = 48, cmp_pct = 75, cl_every = 8;
  // the 16-bit keys as codes of a window chosen on the device from this solve's initial ratios (LMMHIP_KEY_WINDOW;
  // false: the legacy window), distinct up to key_headroom times the initial maximum (lmm_keywin.hpp)
  bool key_window = true;
  double key_headroom = 4.0;  // (kKeyHeadroom, lmm_hip_maxmin.hip)
  ChunkPolicy chunk;
  int64_t tail_rows = 0, tail_cnst = 0;  // the solve is in its tail at this many alive rows / listed constraints
};
int solve_maxmin(lmmhip_ctx* c, double prec);

// frontier engine (lmm_hip_maxmin.hip, lmm_frontier_kernels.hpp): CSR -> CSC map of the uploaded structure, vote
// slots, floors, re-vote queue; the map and the largest CSC degree are rebuilt after every structural change
struct FrontierEngine {
  Scr c2s, slot, minfl, qa, qb, qn, md, pvb, key;
  bool map_ok = false;
  int maxdeg = 0;
};
// What one frontier solve launches (frontier_plan, like RoundPlan; built once the CSR -> CSC map has its largest degree)
struct FrontierPlan {
  int nblk = 1, nblk_sat = 1;  // fr_update / fr_vote (/ fr_sat<256>) workgroups, fr_sat<kFS> workgroups
  int bigch = 1, bigw = 1;     // fr_sat_big: constraints of more CSC chunks than bigch, bigw waves each
  bool big = false;            // ... and whether the system has one
  int g_big = 1;
  bool long_rows = false;      // fr_vote<16> instead of <8>
  int spb = 1;                 // fr_vote: segments per workgroup
  int sat_b = 256;             // fr_sat workgroup: 256 threads or kFS
  int upd_spec = 0;            // fr_update: state loaded with the key
  ChunkPolicy chunk;
};
int solve_maxmin_frontier(lmmhip_ctx* c, double prec);

// persistent engine (lmm_hip_maxmin.hip): its launches are serialised per device, process-wide, so every context
// counts itself in and out
int solve_maxmin_persist(lmmhip_ctx* c, double prec);
void persist_ctx_ref(int device, int delta);
constexpr unsigned kPersistProfCap = 1 << 16;  // barriers covered by lmmhip_persist_profile

// block-diagonal batch (lmm_hip_maxmin.hip, lmmhip_set_batch)
constexpr size_t kBatchLdsMax = 64 * 1024;  // LDS per workgroup; larger systems take the global engines
bool batch_fits(const lmmhip_ctx* c);
int solve_maxmin_batch(lmmhip_ctx* c, double prec);
int batch_rounds_to_ctl(lmmhip_ctx* c, int grid);  // mm_batch_rounds: bt_rounds[0..grid) -> CTL_ROUNDS / CTL_ERR
int engine_of(const lmmhip_ctx* c);

// FairBottleneck (lmm_hip_fair.hip): the one-context solve (solve_fair) and the sharded protocol (lmmhip_fb_shard_*).
// `f` holds the fields of the engine's view (FbFields, lmm_dev.hpp) that live with the flat system's buffers: the
// chunk arrays, the per-variable and per-chunk state, the context's own exchange buffers (xnb, xmin) and fbd.  A solve,
// and each call of the sharded protocol, launches with an FbDev built from the context's Dev and `f`; what only
// solve_fair uses (fb_long, the locality order, hprog) is null in `f` and set in that solve's view alone.
struct FairEngine {
  FbFields f{};
  int64_t fbd_cap = 0;  // elements of f.fbd (allocated by the first one-context solve, with the flat system's buffers)
  // the long shared constraints (fb_long_list) and the locality order of the mu gathers (fb_perm), which matches the
  // uploaded system while perm_ok
  Scr longl, k0, k1, v0, v1, tmp, perm, cscvp, mu;
  bool perm_ok = false;
  // round state of the solve in flight (solve_fair and the sharded protocol)
  int64_t round = 0;
  double prec = 0;
  uint32_t longmin = 0;  // solve_fair: shared constraints with >= this many elements use fbk_acc's increments
  int nlb = 128;         // solve_fair: fbk_update_seq workgroups for the long chains
  // sharded solve: the caller's all-reduced listed counts (in place of f.xnb; non-null while the solve is in
  // flight: begin sets it, an upload or a one-context solve clears it), the owned constraints
  // (lmmhip_fb_shard_owner) and the length of the gathered mu vector their elements index
  int32_t* shard_xnb = nullptr;
  FbOwner owner{};
  bool owner_ready = false;
  int64_t owner_nmu = 0;
  Arena owner_allocs;
};
int solve_fair(lmmhip_ctx* c, double prec);
// FairBottleneck of a declared batch (lmm_hip_fair.hip, lmm_fb_batch_kernels.hpp): one workgroup per system
bool fb_batch_fits(const lmmhip_ctx* c);
int solve_fair_batch(lmmhip_ctx* c, double prec);

struct lmmhip_ctx {
  int device = 0;
  // streams first: members are destroyed in reverse order, the buffers before the streams their work ran on
  Stream own_stream;                   // the context's own stream (back to it: lmmhip_ctx_use_own_stream)
  std::vector<Stream> retired_streams;  // (persistent engine, below)
  hipStream_t stream = nullptr;        // the stream every launch and copy goes to (own_stream or the caller's)
  Dev d{};
  Arena allocs;            // the flat system's buffers (alloc_flat_exact)
  PinPtr<int32_t> h_ctl;   // pinned mirror of the control words (+ 2 slots: the pipelined polls, CtlPoll;
                           // + 1: the words the device writes itself, FbFields::hprog)
  Event ev_poll[2];        // completion of the pipelined control-word copies
  std::vector<Event> ev_slice;  // lmmhip_res_values_sliced: completion of each slice's copy
  bool uploaded = false;
  bool profiling = false;
  int group = 8;  // lanes per row in mm_vote (power of two >= mean row length, <= 64)
  int n_cu = 256;  // compute units (grid of the one-block-per-CU kernels)
  Event ev0, ev1;
  // per-launch event pairs (profiling mode): recorded without synchronising, resolved after the
  // solve, so the timed launch sequence is not serialised by the measurement.
  std::vector<Event> pool;
  size_t pool_used = 0;
  std::vector<int> launch_slot, launch_round;
  std::vector<float> launch_ms;
  lmmhip_stats stats{};
  int last_kind = LMMHIP_KIND_MAXMIN;
  int ran_engine = -1;   // LMMHIP_RAN_* of the solve in flight (set by the engine that runs it)
  int last_engine = -1;  // ... of the last successful solve (lmmhip_last_engine); -1 = none yet
  double last_prec = 1e-5;  // precision of the last solve (lmmhip_get_saturated)
  bool solved = false;      // a solve completed since the last upload / flatten
  DevPtr<int32_t> vstat;    // profiling counters of mm_vote ([round][block] x 2)
  DevPtr<unsigned long long> anat;  // round anatomy records (LMM_ANAT builds, LMMHIP_ANAT_ROUNDS)
  // maxmin engine (lmmhip_ctx_set_engine): one persistent launch per solve (default) or the
  // multi-launch round chain; grid-barrier words of the persistent launch
  int engine = LMMHIP_ENGINE_AUTO;
  int sat_waves = 1;  // waves per ready constraint in mm_saturate (mean 64-element CSC chunks, 1/2/4)
  bool vote_diag = std::getenv("LMMHIP_VOTE_DIAG") != nullptr;  // profiling: diagnostic vote launches
  DevPtr<unsigned> pbar;
  bool persist_prof = false;    // record barrier timestamps in the persistent launch
  DevPtr<long long> ptime;      // [2 * kPersistProfCap] last arrival / exit per barrier
  int persist_grid = 0;  // workgroups of the persistent launch (one per CU, checked at first use)
  int64_t persist_fallbacks = 0;  // persistent solves re-run by the multi-launch engine (barrier timeout)
  // co-residency fallback (lmm_persist_kernels.hpp bar_rdv): mapped host word the closed-and-drained launch
  // rendezvous raises (d_rdv: the same word as the device sees it), the streams left behind holding such a launch
  // (retired_streams: its late workgroups still to run), and the solves left before the persistent engine is tried
  // again on this context
  PinPtr<int32_t> h_rdv;
  int32_t* d_rdv = nullptr;
  int64_t persist_cool = 0;
  bool ev1_done = false;  // the solve recorded ev1 itself (right behind its last kernel)
  // block-diagonal batch (lmmhip_set_batch): system offsets on the device, largest system
  int64_t bt_n = 0;
  DevPtr<int64_t> bt_voff, bt_coff;
  DevPtr<int32_t> bt_rounds;  // [grid] rounds of each workgroup's systems
  int bt_max_nv = 0, bt_max_nc = 0, bt_max_nnz = 0;
  size_t bt_lds = 0;  // mm_batch_lds' LDS bytes: the largest batch_lds_bytes over the systems, each by its own sizes
  int64_t bt_cap = 0;
  // rounds the previous solve of this context had to queue before its termination test could fire (round engine:
  // LASTR + 1, mm_done at the end of the chunk; frontier: ROUNDS + 1, the vote after the last update): a hint for
  // where to end a chunk and wait for it (round_hint_chunk); 0 = none
  int64_t hint_rounds_mm = 0, hint_rounds_fr = 0;
  ActDev act{};                        // model-side action state (lmm_step_kernels.hpp)
  Arena act_allocs;
  // bound action table (lmmhip_actions_bind): the caller's variable id of every action (in act_allocs); sys_gen
  // counts the uploads and flattens (alloc_flat, finish_flat, the resident refresh path), act_gen is the sys_gen
  // act.vidx was last rebound at (act_rebind, queued by the step entry points when the two differ)
  int32_t* act_slot = nullptr;
  uint64_t sys_gen = 1, act_gen = 0;
  Scr act_stage, act_mask, act_evout;  // lmmhip_actions_patch staging, the `extra` byte mask, lmmhip_actions_events
  // resident System mirror (lmmhip_res_*, lmm_resident_kernels.hpp): outlives uploads, freed with the
  // context.  Mirror arrays (res_own: the nine arrays of `res`, in its order) keep their contents when they grow;
  // scratch buffers do not.
  ResDev res{};
  DevPtr<void> res_own[9];
  int64_t res_capE = 0, res_capV = 0, res_capC = 0;
  int64_t res_nE = 0, res_nV = 0, res_nC = 0;  // host table sizes of the last delta batch
  bool res_flat = false;                        // the uploaded system came from lmmhip_res_flatten
  FlatBufs fb_last{};
  PinPtr<double> pin_vals;  // pinned host staging of lmmhip_res_values_pinned
  PinPtr<uint8_t> pin_rst;  // (lmmhip_res_values_pinned only: the sliced fetch marks kept slots in the values)
  int64_t pin_cap = 0, pin_rst_cap = 0;  // capacities of pin_vals / pin_rst (elements)
  int64_t fcap[4] = {0, 0, 0, 0};               // capacities of the flat-system buffers (nV, nC, nnz, nch)
  int64_t res_flat_nv = 0;                      // variable slots covered by that flatten
  // refresh path of lmmhip_res_flatten: the last flatten's list and precision, host-side structural
  // flag (element records shipped since), device flags of rs_apply_v / rs_apply_c (kResStruct / kResPenalty)
  // res_dirty: [0] flags, [1] fair error, [2] "mixed" member (rs_mark), [3] part-test crossings since the
  // last flatten, [4 ..) their constraint ids (kResCrossCap, rs_apply_c)
  std::vector<int32_t> res_last_list;
  double res_last_prec = -1.0;
  bool res_struct_host = true;
  DevPtr<int32_t> res_dirty;
  int64_t res_refreshes = 0, res_cross_refreshes = 0;
  // refresh path: the variables the delta batches touched since the last flatten (-1: too many), and whether rs_c2c
  // (CSR -> CSC position map, written by the device flatten's transpose) matches the uploaded structure
  Scr rs_vlist, rs_c2c;
  int64_t res_vl_n = 0;
  bool res_pen_dirty = false;  // lmmhip_update_vars wrote penalties behind the mirror's back: recompute csc_u / csc_p
  bool res_c2c_ok = false;
  int res_flat_kind = LMMHIP_KIND_MAXMIN;  // solver the last resident flatten built for
  Scr sat_out, tv_out;  // lmmhip_get_saturated / lmmhip_get_touched_vars staging
  Scr usage_out, tc_out;  // lmmhip_get_usage and lmmhip_usage_device_ptr / lmmhip_get_touched_cnsts
  Scr cert_top, cert_wit, cert_part;      // lmmhip_certificate: sattop, witness, the workgroups' parts + the result
  Scr cc_par, cc_flag, cc_rank, cc_out;  // lmmhip_components
  RoundEngine rounds;
  FrontierEngine frontier;
  FairEngine fair;
  Scr rs_stage[12], rs_pos, rs_list, rs_lpart, rs_lany, rs_dcl, rs_cdeg, rs_cptr, rs_vrst, rs_vm, rs_dv, rs_rl,
      rs_ro, rs_rowid, rs_kidx, rs_skey, rs_sval, rs_vout, rs_tmp, rs_lzero, rs_nck, rs_cch, rs_rowpen, rs_posd, rs_cls, rs_lanyc,
      rs_outc;
};

// ---- allocation ----
template <class T> int dalloc(lmmhip_ctx* c, T** out, int64_t n) { return c->allocs.alloc(out, n); }

template <class T> int scratch(lmmhip_ctx* c, Scr& b, int64_t n, T** out) {
  const size_t need = size_t(n > 0 ? n : 1) * sizeof(T);
  if (b.bytes < need) {
    HIPCHK(hipStreamSynchronize(c->stream));  // the old buffer may still be read by queued work
    const size_t bytes = b.bytes ? std::max(need, b.bytes + b.bytes / 2) : need + need / 16;  // (alloc_flat)
    b.bytes = 0;
    HIPCHK(b.reset());
    HIPCHK(hipMalloc(&b.p, bytes));
    b.bytes = bytes;
  }
  *out = static_cast<T*>(b.p);
  return 0;
}

// Grow a mirror array to `cap` elements, keeping the first `used` ones.
template <class T> int res_grow(lmmhip_ctx* c, DevPtr<void>& own, T** p, int64_t used, int64_t cap) {
  DevPtr<void> q;
  HIPCHK(hipMalloc(&q.p, size_t(cap > 0 ? cap : 1) * sizeof(T)));
  HIPCHK(hipMemsetAsync(q.p, 0, size_t(cap > 0 ? cap : 1) * sizeof(T), c->stream));
  if (*p && used > 0)
    HIPCHK(hipMemcpyAsync(q.p, *p, size_t(used) * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *p = static_cast<T*>(q.p);
  std::swap(own.p, q.p);
  HIPCHK(q.reset());
  return 0;
}

template <class T> int stage(lmmhip_ctx* c, int slot, const T* host, int64_t n, const T** out) {
  T* d = nullptr;
  if (int rc = scratch(c, c->rs_stage[slot], n, &d))
    return rc;
  if (n > 0)
    HIPCHK(hipMemcpyAsync(d, host, size_t(n) * sizeof(T), hipMemcpyHostToDevice, c->stream));
  *out = d;
  return 0;
}

// ---- lmm_hip.hip: flat system, helpers over its kernels ----
void free_owner(lmmhip_ctx* c);  // drops the sharded solve's owned constraints
int alloc_flat(lmmhip_ctx* c, int64_t nV, int64_t nC, int64_t nnz, int64_t nch, FlatBufs* o);
int finish_flat(lmmhip_ctx* c, int64_t nV, int64_t nC, int64_t nnz, bool elem_done = false);
int launch_elem_usage(lmmhip_ctx* c, int rows);  // mm_elem_usage over the uploaded system
int dev_scan(lmmhip_ctx* c, const int64_t* in, int64_t* out, int64_t n);
int64_t read_i64(lmmhip_ctx* c, const int64_t* dptr, int* rc);
int poll_ctl(lmmhip_ctx* c);  // the control words into h_ctl, synchronously

// ---- launch helper ----
// In profiling mode every launch is bracketed by two events from a pool (no host synchronisation); their
// elapsed times are resolved once the solve has finished.
int prof_event(lmmhip_ctx* c, hipEvent_t* out);
int resolve_profile(lmmhip_ctx* c);

#define LAUNCH(slot, round, kern, grid, block, ...)                                 \
  do {                                                                              \
    hipEvent_t e0_ = nullptr, e1_ = nullptr;                                        \
    if (c->profiling) {                                                             \
      if (int rc_ = prof_event(c, &e0_))                                            \
        return rc_;                                                                 \
      HIPCHK(hipEventRecord(e0_, c->stream));                                       \
    }                                                                               \
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), 0, c->stream, __VA_ARGS__);  \
    HIPCHK(hipGetLastError());                                                      \
    if (c->profiling) {                                                             \
      if (int rc_ = prof_event(c, &e1_))                                            \
        return rc_;                                                                 \
      HIPCHK(hipEventRecord(e1_, c->stream));                                       \
      c->launch_slot.push_back(slot);                                               \
      c->launch_round.push_back(int(round));                                        \
    }                                                                               \
    c->stats.kernel_launches[slot] += 1;                                            \
  } while (0)

// Pipelined termination polls of the multi-launch engines: the control words after chunk k are written into a
// pinned slot by a one-wave kernel (mm_ctl_out, profile slot 6) behind an event, chunk k + 1 is queued, then the
// host waits for chunk k's words — the GPU never idles on the host, and the host learns of termination one chunk
// late: what is queued after the last round is a run of launches that return at once (CTL_DONE).
struct CtlPoll {
  lmmhip_ctx* c;
  int slot = 0;
  bool pending = false;  // the other slot's words are queued and not yet waited for
  int32_t* hc[2];        // the two pinned slots, and as the device sees them
  int32_t* hcd[2];
  int init(lmmhip_ctx* ctx);
  // Queues the words (of `d`, after everything queued so far) into the current slot, then waits for the previous
  // chunk's words if they are pending and, unless those say CTL_DONE, with `stop` for this chunk's too (the hinted
  // end: its words before anything more is queued).  *words: the newest words waited for, null if none yet.
  int step(const Dev& d, int64_t round, bool stop, const int32_t** words);
};
