// lmm_hip_maxmin.hip — the max-min engines of lmmhip_solve (lmm_ctx.hpp): the multi-launch round engine, the
// frontier engine, the persistent engine with its fallback, and the block-diagonal batch engine.
//
// The round engine and the frontier engine are chains of launches and share their host side: round_plan / frontier_plan
// build what a solve will launch (mode, kernels, grids, cadences, chunk policy: RoundPlan / FrontierPlan in lmm_ctx.hpp)
// once per solve and read every environment knob of the two engines; run_chunks owns the chunk / poll / guard loop
// (policy arithmetic: lmm_chunk.hpp).  Each engine works on its own copy of the context's Dev (the frontier: an FrDev).
#include <cstring>

#include <array>
#include <map>
#include <mutex>
#include <thread>
#include <utility>

#include "lmm_ctx.hpp"
#include "lmm_maxmin_kernels.hpp"
#include "lmm_persist_kernels.hpp"
#include "lmm_frontier_kernels.hpp"
#include "lmm_batch_kernels.hpp"

// The round engine's key window stays distinct up to this factor above the solve's initial maximum ratio
// (RoundPlan::key_headroom; DESIGN.md "Key window" has the clamped shares it was chosen from).
constexpr double kKeyHeadroom = 4.0;
constexpr int64_t kAutoPersistVars = 1 << 18;   // LMMHIP_ENGINE_AUTO: one of the single-GPU small-system engines up to
constexpr int64_t kAutoPersistMaxVars = 1 << 14;  // this many variables: persistent up to 2^14, frontier above

// Persistent launches are serialised per device, process-wide (solve_maxmin_persist_once): the completion event
// of each device's last persistent launch, and the number of live contexts on the device (the event is destroyed
// with the last one, so a device reset between two sets of contexts never leaves a stale event behind).
namespace {
std::mutex g_persist_mu;
// device -> completion event of its last persistent launch (never destroyed at process exit: the runtime may be gone)
std::map<int, Event>& g_persist_last = *new std::map<int, Event>;
std::map<int, int> g_persist_users;        // device -> live contexts
}  // namespace

void persist_ctx_ref(int device, int delta) {
  std::lock_guard<std::mutex> lk(g_persist_mu);
  int& n = g_persist_users[device];
  n += delta;
  if (n <= 0) {
    g_persist_users.erase(device);
    g_persist_last.erase(device);
  }
}

// ---- the round-chain engines: the round engine and the frontier engine --------------------------------------------
// Both run as a chain of launches, a chunk of rounds per pipelined termination poll.  A solve is: allocate, build its
// plan (every environment knob of the engine is read there, once per solve, and nowhere else), drive the chunks.

// The chunk / poll / guard loop of both engines.  Per chunk: the chunk's length (ChunkPolicy, cut at the hinted end:
// round_hint_chunk), round_launches(r) for each of its rounds, chunk_end(r) behind them (r: the rounds queued so far),
// the poll's mm_ctl_out (CtlPoll::step), then — on the newest control words the host has, one chunk behind, null before
// the first have arrived — the done test, in_tail(words) (the engine refreshes its view of the sizes there and says
// whether the solve is in its tail), the round guard and the next chunk's length.  Termination polls are pipelined
// (CtlPoll): a chunk queued after the last round is a run of launches that return at once (CTL_DONE).  Ends with the
// final words in c->h_ctl (the queued tail has run: final words for the stats and the caller's hint).
template <class Rounds, class ChunkEnd, class InTail>
static int run_chunks(lmmhip_ctx* c, const Dev& d, const ChunkPolicy& p, Rounds&& round_launches, ChunkEnd&& chunk_end,
                      InTail&& in_tail) {
  // Every round fixes at least one variable (progress), so nV + 2 rounds bound it.
  const int64_t max_rounds = int64_t(d.nV) + 2;
  CtlPoll poll;
  if (int rc = poll.init(c))
    return rc;
  int chunk = p.first;
  for (int64_t r = 0;;) {
    bool stop = false;
    const int n = round_hint_chunk(r, chunk, p.hint, &stop);
    for (int k = 0; k < n; k++, r++)
      if (int rc = round_launches(r))
        return rc;
    if (int rc = chunk_end(r))
      return rc;
    const int32_t* h = nullptr;
    if (int rc = poll.step(d, r, stop, &h))
      return rc;
    if (h && h[CTL_DONE])
      break;
    const bool tail = in_tail(h);
    // the guard counts the rounds the device has RUN without finishing (CTL_ROUNDS of the newest words), not the rounds
    // queued: the polls are one chunk behind, so a system of 3 variables and 3 rounds has 6 rounds queued when the
    // words of its first two arrive, and counting those failed it
    if (h && h[CTL_ROUNDS] > max_rounds)
      return fail(LMMHIP_E_NOCONVERGE, "maxmin round guard tripped");
    chunk = chunk_grow(chunk, p, tail);
  }
  return poll_ctl(c);
}

// The round engine's kernels by mode (lmm_round_mode.hpp).  The short-row lane vote (groups of 4 and 8: one lane per
// row, more gathers in flight per wave): entry i is the vote mode of index i, in its LDS-bitmap form and its scan form —
// built by enumerating the indices, so a mode cannot reach a kernel built for another.  The long-row votes
// mm_vote<16|32|64> have the Arrays mode and the scan form only.
struct VoteKernels {
  VoteKernel bitmap, scan;
};
template <int... I> constexpr std::array<VoteKernels, sizeof...(I)> lane_votes(std::integer_sequence<int, I...>) {
  return {{{mm_vote_lane<VoteForm::Bitmap, I>, mm_vote_lane<VoteForm::Scan, I>}...}};
}
constexpr auto kVoteTable = lane_votes(std::make_integer_sequence<int, kVoteModes>{});
constexpr VoteKernel kVoteLong[3] = {mm_vote<16>, mm_vote<32>, mm_vote<64>};
// Saturation: [mm_ready's list, the ready queue][1, 2, 4 waves per ready constraint]
constexpr SatKernel kSatTable[2][3] = {{mm_saturate<1>, mm_saturate<2>, mm_saturate<4>},
                                       {mm_saturate_q<1>, mm_saturate_q<2>, mm_saturate_q<4>}};
// Update: entry i is the update mode of index i (queue, quad)
template <int... I> constexpr std::array<UpdKernel, sizeof...(I)> updates(std::integer_sequence<int, I...>) {
  return {{mm_update<I>...}};
}
constexpr auto kUpdTable = updates(std::make_integer_sequence<int, kUpdModes>{});

static RoundPlan round_plan(const lmmhip_ctx* c, const Dev& d) {
  RoundPlan P;
  // The mode (resolve_round_mode, lmm_round_mode.hpp), from the knobs' values:
  // LMMHIP_CREC=0: no packed row records for the re-votes (vote_row: with them the row's variable and CSR range from
  // one record instead of the cvar / crow arrays, one line per re-vote less): C2 25.94-26.00 vs 26.10-26.17 ms, stress
  // 28.83 vs 29.13 (same box).
  // LMMHIP_CMP_ROWS=0: the 8-B records and the compaction that copies the alive rows' elements, instead of the 16-B
  // records {cvar, begin, end, 0}: a re-vote loads one record and reads its elements from the original CSR, and a
  // compaction moves the per-row words only (cmp_count_rows / cmp_write_rows).
  // LMMHIP_RDQ=0: the mm_ready pass.  Without it the update's workgroups (at most kMaxBlocks, each updating at most
  // kUSeg constraints) list the ready constraints for the next round, the vote queues the ones it makes ready (C2
  // 25.07-25.22 vs 25.34-25.39 ms, stress 28.29 vs 28.46, same box).
  // LMMHIP_UPDQ_BLOCKS: those update workgroups, 4 per CU, each with a longer segment, so that the saturation's prefix
  // over the segment counts is shorter — but enough of them to keep every segment within kUSeg.  Round 5, same box: C2
  // 24.52-24.54 ms against 24.84-24.85 with one per 256 constraints (2,048 at C2), stress 27.86-27.94 vs 28.14; with
  // the saturation cap at 5 per CU below, 24.41-24.45 (stress 27.75-27.77).
  // LMMHIP_SATKEY=0: the state-read path.  Else the filter retires the rows of saturated targets on the key it gathered
  // (kSatKey, vote_waves) and the re-votes read no variable state (the record forms of the short-row vote).
  // LMMHIP_UPD_QUAD=0: mm_update moves a touched constraint's record lane by lane, in eight pieces, instead of one 64-B
  // request per quad of lanes, both ways (update_groups, kQuad).
  // LMMHIP_UPD_BLOCKS (launch-width cap, tuning knob; 0 = uncapped): fewer blocks cut the fixed per-round cost of the
  // grid-stride update once the alive set is small.
  RoundKnobs k;
  k.crec = env_int("LMMHIP_CREC", 1);
  k.rdq = env_int("LMMHIP_RDQ", 1);
  k.satkey = env_int("LMMHIP_SATKEY", 1);
  k.cmp_rows = env_int("LMMHIP_CMP_ROWS", 1);
  k.upd_quad = env_int("LMMHIP_UPD_QUAD", 1);
  k.upd_blocks = env_int("LMMHIP_UPD_BLOCKS", 0);
  k.updq_blocks = env_int("LMMHIP_UPDQ_BLOCKS", updq_blocks_default(c->n_cu));
  const RoundMode m = resolve_round_mode(c->group, d.nC, k, RoundLimits{kBlock, kUSeg, kMaxBlocks});
  P.mode = m.vote;
  P.upd_quad = m.upd_quad;
  P.g_upd = m.g_upd;
  // the saturation's grid capped at 4 workgroups per CU (round 5, same box: C2 24.73-24.90 ms against 25.04-25.16
  // uncapped, i.e. up to kMaxBlocks = 2048; 768: 24.79-25.03, 1280: 24.76-24.81, 1536: 24.83-25.00, 512: 25.42-25.73;
  // stress 27.99-28.05 vs 28.29-28.36): every workgroup first rebuilds the prefix of the update's segment counts,
  // and half as many of them still give each ready constraint its waves
  // (with 4 update workgroups per CU: 5 per CU, 24.41-24.45 ms against 24.52-24.54 at 4 and 24.52-24.60 at 6 / 8)
  P.cap_sat = env_int("LMMHIP_SAT_BLOCKS", 5 * c->n_cu);
  const bool short_rows = c->group == 4 || c->group == 8;
  const VoteKernels vk = short_rows ? kVoteTable[P.mode.index()]
                                    : VoteKernels{nullptr, kVoteLong[c->group == 16 ? 0 : c->group == 32 ? 1 : 2]};
  // the LDS bitmap of changed constraints (one 1024-thread workgroup per CU); below LMMHIP_VOTE_BITS_ROWS alive rows
  // (host view, A/B knob; 0 = always) the change stamps gathered per row instead: no ~125-KB copy per CU
  // (LMMHIP_VOTE_BITS=0: always the stamps' path)
  const bool bits = int64_t(d.nC) <= int64_t(kBitWords) * 64 && env_int("LMMHIP_VOTE_BITS", 1) != 0;
  P.vote_bitmap = bits ? vk.bitmap : nullptr;
  P.vote_scan = vk.scan;
  P.vote_bits_rows = env_int("LMMHIP_VOTE_BITS_ROWS", 0);
  // mm_saturate: waves per ready constraint and the grid's block cap (measurement knobs)
  const int sat_k = env_int("LMMHIP_SAT_WAVES", c->sat_waves);
  P.sat_waves = sat_k == 1 || sat_k == 2 ? sat_k : 4;
  P.saturate = kSatTable[P.mode.rdq()][P.sat_waves == 4 ? 2 : P.sat_waves - 1];
  P.sat_max = env_int("LMMHIP_SAT_GRID_MAX", kMaxBlocks);
  P.update = kUpdTable[m.upd().index()];
  P.g_init_c = grid_for(d.nC, kBlock / kWave);
  P.g_c = grid_for(d.nC, kBlock);
  // LMMHIP_KEY_WINDOW=0: the legacy key window {0, 16} (the f32's upper 16 bits) instead of the one mm_key_window
  // chooses from the solve's initial ratios; results are the same under every window (lmm_keywin.hpp).
  // LMMHIP_KEY_HEADROOM (measurement knob): the window keeps the codes distinct up to this factor above the initial
  // maximum ratio (DESIGN.md "Key window": the choice and the clamped share it was read from).
  P.key_window = env_int("LMMHIP_KEY_WINDOW", 1) != 0;
  const char* kh = std::getenv("LMMHIP_KEY_HEADROOM");
  const double khv = kh ? std::atof(kh) : 0.0;
  P.key_headroom = khv >= 1.0 ? khv : kKeyHeadroom;
  // Compaction cadence (knobs): alive rows are re-counted every cmp_every rounds and rewritten when
  // fewer than cmp_pct % of the scanned rows are alive; the alive-constraint list every cl_every rounds.
  // Both decide and switch buffers on the device (ctl CTL_BUF / CTL_CB): no host round trip.
  // (round 5, re-swept on the final code, same box: every 48 rounds 24.94-25.08 ms against 25.10-25.21 at 32, 25.49-25.56
  // at 16, 25.11-25.21 at 64, 25.30-25.34 at 96; stress 28.29-28.37 vs 28.42-28.44)
  P.cmp_every = env_int("LMMHIP_COMPACT_EVERY", 48);
  P.cmp_pct = env_int("LMMHIP_COMPACT_PCT", 75);
  P.cl_every = env_int("LMMHIP_CLIST_EVERY", 8);
  // rounds queued per poll: the host learns of termination one chunk late, so up to 2 x chunk_max no-op
  // rounds run after the last one (LMMHIP_CHUNK_MAX, A/B knob): C2 25.96-25.99 ms at 16, 26.01 at 8,
  // 26.15-26.20 at 4; round 5, with compactions every 48 rounds: 25.03-25.06 at 32 against 25.07-25.08 at 16
  P.chunk.hint = env_int("LMMHIP_ROUND_HINT", 1) ? c->hint_rounds_mm : 0;  // (round_hint_chunk)
  // under a hint no returning rounds follow the last one, and 64-round chunks (fewer polls, a sparser list / compaction
  // cadence) measured 23.13-23.36 ms against 23.21-23.47 at 32 over five same-box pairs, stress 26.85 vs 26.88
  // (scripts/gpu_r06_v.sh, _w.sh)
  P.chunk.first = 2;
  P.chunk.max = std::max(2, env_int("LMMHIP_CHUNK_MAX", P.chunk.hint > 0 ? 64 : 32));
  // Near the end of the solve, short chunks: the rounds queued after the last one are no-op launches of the full
  // grids (~32 of them after C2's last round with 32-round chunks, rocprofv3 trace of round 5), so once the alive rows
  // (host view: refreshed at each compaction) fall to LMMHIP_CHUNK_TAIL_PCT % of the variables (default 5), or below
  // LMMHIP_CHUNK_TAIL_ROWS / the alive-constraint list below LMMHIP_CHUNK_TAIL_CNST (A/B knobs), a chunk is at most
  // LMMHIP_CHUNK_TAIL rounds (default 4).  Round 5, same box, two passes (scripts/gpu_r05_ctail.sh,
  // profiles/r05_ab_c2_ctail.json): C2 23.90-23.95 ms at 5e5 rows (5 %) / 4 rounds against 24.10-24.12 without;
  // 1e6 / 8 and 2e6 / 8 23.92-23.94, 1e6 / 4 23.95-24.07; the constraint-list thresholds (2e4, 1e5) 24.06-24.11.
  // (the short tail chunks stay under a hint too: dropping them measured 23.10 against 23.05-23.08 ms,
  // scripts/gpu_r06_t.sh)
  P.tail_rows = env_int("LMMHIP_CHUNK_TAIL_ROWS",
                        int(int64_t(d.nV) * std::max(0, env_int("LMMHIP_CHUNK_TAIL_PCT", 5)) / 100));
  P.tail_cnst = env_int("LMMHIP_CHUNK_TAIL_CNST", 0);
  P.chunk.tail = std::max(1, env_int("LMMHIP_CHUNK_TAIL", 4));
  return P;
}

// The plan's buffers, into the solve's own Dev: the context's never carries them (lmm_dev.hpp), so no other engine —
// whose compactions do not maintain the row records — ever sees them.
// (cmpbits: the compaction's alive bits, RowForm::Rec16 only — an argument of its two kernels, not part of the Dev)
static int round_buffers(lmmhip_ctx* c, Dev& d, const RoundPlan& P, uint8_t** cmpbits, double** kwmm) {
  if (P.key_window)
    if (int rc = scratch(c, c->rounds.kwmm, 2 * int64_t(P.g_init_c), kwmm))
      return rc;
  for (int k = 0; k < 3 && P.mode.rec(); k++)  // (the member of RowRecs the RowForm selects)
    if (int rc = P.mode.rec16() ? scratch(c, c->rounds.crec[k], int64_t(d.nV) + 1, &d.crec[k].r16)
                                : scratch(c, c->rounds.crec[k], int64_t(d.nV) + 1, &d.crec[k].r8))
      return rc;
  if (P.mode.rec16())
    if (int rc = scratch(c, c->rounds.cmpbits, (int64_t(d.nV) + kCompactRows - 1) / kCompactRows * kBlock, cmpbits))
      return rc;
  if (P.mode.rdq()) {
    const int64_t n = std::max<int64_t>(d.nC, 1);
    if (int rc = scratch(c, c->rounds.rdq[0], n, &d.rdq[0]) | scratch(c, c->rounds.rdq[1], n, &d.rdq[1]) |
                 scratch(c, c->rounds.rqst, n, &d.rqst) | scratch(c, c->rounds.useg, int64_t(P.g_upd) * kUSeg, &d.useg) |
                 scratch(c, c->rounds.ucnt, kMaxBlocks, &d.ucnt))
      return rc;
    HIPCHK(hipMemsetAsync(d.rqst, 0xFF, size_t(n) * sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(d.ucnt, 0, size_t(kMaxBlocks) * sizeof(int32_t), c->stream));
  }
  return 0;
}

// The alive-row buffer in use is read by the vote on the device (ctl CTL_BUF); nrows (an upper bound of its
// rows, refreshed at every poll) only sizes the scan forms' grids (one lane per row in the work-queue scan).
static int launch_vote(lmmhip_ctx* c, const Dev& d, const RoundPlan& P, int64_t r, int64_t nrows) {
  const bool bitmap = P.vote_bitmap && nrows >= P.vote_bits_rows;
  if (bitmap && c->profiling && c->vote_diag) {  // measurement: bitmap load alone, filter alone (slot 7)
    LAUNCH(7, r + 1000000, (mm_vote_lane<VoteForm::Bitmap, kVoteArrays, 2>), c->n_cu, kVBlock, d, int(r));
    LAUNCH(7, r, (mm_vote_lane<VoteForm::Bitmap, kVoteArrays, 1>), c->n_cu, kVBlock, d, int(r));
    LAUNCH(7, r, mm_vote_diagcount, grid_for((int64_t(d.nC) + 63) / 64, kBlock), kBlock, d, int(r));
  }
  LAUNCH(2, r, bitmap ? P.vote_bitmap : P.vote_scan, bitmap ? c->n_cu : grid_for(nrows, kBlock), bitmap ? kVBlock : kBlock,
         d, int(r));
  return 0;
}

// Slots: 0 mm_init_cnsts, 1 mm_init_vars, 2 mm_vote, 3 mm_ready, 4 mm_saturate, 5 mm_update,
// 6 compaction.
int solve_maxmin(lmmhip_ctx* c, double prec) {
  c->ran_engine = LMMHIP_RAN_ROUNDS;
  Dev d = c->d;  // (a copy, as in the other engines: the mode's buffers go into it alone)
  const RoundPlan P = round_plan(c, d);
  uint8_t* cmpbits = nullptr;
  double* kwmm = nullptr;  // (null: the legacy key window)
  if (int rc = round_buffers(c, d, P, &cmpbits, &kwmm))
    return rc;
  LAUNCH(0, -1, mm_init_cnsts, P.g_init_c, kBlock, d, static_cast<uint32_t*>(nullptr), prec, kwmm);
  // (with the key window's choice and the alive constraints' keys in it: key_window_pass)
  LAUNCH(1, -1, mm_init_vars, grid_for(d.nV, kBlock), kBlock, d, int(P.mode.rec16()), static_cast<const double*>(kwmm),
         P.g_init_c, P.key_headroom);
  LAUNCH(1, -1, mm_clist, std::min(P.g_c, 2 * c->n_cu), kBlock, d, 1);
  HIPCHK(hipMemsetAsync(d.chgbits, 0, sizeof(uint64_t) * ((d.nC + 127) / 128 * 2 + 2), c->stream));
  // Host view of the sizes (upper bounds: rows and constraints only leave), refreshed at every poll; they
  // size grids only, the kernels read the exact counts from the control words.
  int64_t last_compact = 0, last_clist = 0, nrows = d.nV, ncl = d.nC;
  auto round_launches = [&](int64_t r) -> int {
    if (int rc = launch_vote(c, d, P, r, nrows))
      return rc;
    const int gL = grid_for(ncl, kBlock);
    if (!P.mode.rdq())  // (ready-queue mode: no mm_ready pass, the update's segments — g_upd of them — and the vote's queue)
      LAUNCH(3, r, mm_ready, gL, kBlock, d);
    const int64_t gS = std::max<int64_t>(1, std::min<int64_t>((P.sat_waves * ncl + kBlock - 1) / kBlock, P.sat_max));
    LAUNCH(4, r, P.saturate, int(P.cap_sat > 0 && gS > P.cap_sat ? P.cap_sat : gS), kBlock, d, int(r),
           P.mode.rdq() ? P.g_upd : gL);
    LAUNCH(5, r, P.update, P.g_upd, kBlock, d, int(r), prec);
    if (c->profiling && c->vote_diag)  // measurement: the keys this update stored, and those at the window's top
      LAUNCH(7, r, mm_key_diag, P.g_c, kBlock, d, int(r));
    return 0;
  };
  // the termination test, then the alive-constraint list and the alive-row compaction, at the end of a chunk (their
  // cadence is the chunks')
  auto chunk_end = [&](int64_t r) -> int {
    LAUNCH(6, r, mm_done, 1, kBlock, d, P.g_upd);
    const int gL = grid_for(ncl, kBlock);
    bool cl = false, cm = false;
    if (r - last_clist >= P.cl_every && ncl > 4096) {  // alive-constraint list (order not preserved)
      LAUNCH(6, r, mm_clist, std::min(gL, 2 * c->n_cu), kBlock, d, 0);
      last_clist = r;
      cl = true;
    }
    if (r - last_compact >= P.cmp_every && nrows > 4096) {  // order-preserving compaction of the alive rows
      const int nblk = int((nrows + kCompactRows - 1) / kCompactRows);
      switch (P.mode.form) {
        case RowForm::Rec16:  // the per-row words only
          LAUNCH(6, r, cmp_count_rows, nblk, kBlock, d, cmpbits);
          LAUNCH(6, r, cmp_scan<true>, 1, 1024, d, nblk, P.cmp_pct);
          LAUNCH(6, r, cmp_write_rows, nblk, kBlock, d, cmpbits);
          break;
        case RowForm::Arrays:
        case RowForm::Rec8:  // rows and elements (and the 8-B records where the solve has them)
          LAUNCH(6, r, cmp_count, nblk, kBlock, d);
          LAUNCH(6, r, cmp_scan<false>, 1, 1024, d, nblk, P.cmp_pct);
          LAUNCH(6, r, cmp_write, nblk, kBlock, d);
          break;
      }
      last_compact = r;
      cm = true;
    }
    if (cl || cm)
      LAUNCH(6, r, mm_flip, 1, 1, d, int(cl), int(cm));
    return 0;
  };
  auto in_tail = [&](const int32_t* h) {
    if (h) {
      ncl = h[CTL_NCL0 + h[CTL_CB]];
      nrows = h[CTL_NROWS + h[CTL_BUF]];
    }
    return nrows <= P.tail_rows || ncl <= P.tail_cnst;
  };
  if (int rc = run_chunks(c, d, P.chunk, round_launches, chunk_end, in_tail))
    return rc;
  c->hint_rounds_mm = int64_t(c->h_ctl.p[CTL_LASTR]) + 1;
  return 0;
}

static FrontierPlan frontier_plan(const lmmhip_ctx* c, const Dev& d) {
  FrontierPlan P;
  // fr_update / fr_vote (/ fr_sat<256>) workgroups; one for a system without constraints (every variable disabled
  // or on zero-bound constraints only: nothing flattened), whose first round then finds nothing alive — a grid of
  // zero workgroups is a launch error
  P.nblk = int(std::max<int64_t>(1, (int64_t(d.nC) + kFB - 1) / kFB));
  P.nblk_sat = int(std::max<int64_t>(1, (int64_t(d.nC) + kFS - 1) / kFS));  // fr_sat workgroups
  // constraints of more CSC chunks than this saturate in fr_sat_big, kFrBigWaves waves each over the whole grid
  // (LMMHIP_FR_BIGCH, A/B knob: fat-tree core links' chunk chains in C4)
  P.bigch = std::max(1, env_int("LMMHIP_FR_BIGCH", kFrBigCh));
  P.big = c->frontier.maxdeg > P.bigch * kWave;
  P.bigw = std::max(1, env_int("LMMHIP_FR_BIGW", kFrBigWaves));  // waves per big constraint (A/B knob)
  P.g_big = std::min(kMaxBlocks, 4 * c->n_cu);
  // (round 6, removed after their A/Bs: the re-vote reading the floors with the keys, LMMHIP_FR_MFEARLY, and the round
  // engine's chunk body in fr_sat, LMMHIP_FR_SATOLD — both slower on C2 and C4, scripts/gpu_fr_ab.sh)
  // re-votes keep 16 row elements in registers when the mean row is longer than 8 (LMMHIP_FR_R16=0: 8)
  P.long_rows = c->group > 8 && env_int("LMMHIP_FR_R16", 1) != 0;
  // fr_vote: segments per workgroup, so that the grid still covers the chip twice (C2: 4, small systems: 1)
  P.spb = int(std::max<int64_t>(1, std::min<int64_t>(kFVS, int64_t(P.nblk) / (2 * int64_t(c->n_cu)))));
  // fr_sat workgroup: kFS threads (the round-4 choice on C2-size systems) unless that leaves the chip mostly
  // idle — C4 (25 workgroups of kFS): 3.37-3.40 ms with 256-thread workgroups against 3.49
  const int sat_b0 = int64_t(P.nblk_sat) >= 2 * int64_t(c->n_cu) ? kFS : 256;
  P.sat_b = env_int("LMMHIP_FR_SATB", sat_b0) == 256 ? 256 : kFS;
  // fr_update: every constraint's state loaded with its key (one dependent level less) on the small systems, where the
  // 256-thread saturation workgroups run (LMMHIP_FR_UPDSPEC, A/B knob)
  P.upd_spec = env_int("LMMHIP_FR_UPDSPEC", P.sat_b == 256 ? 1 : 0);
  // rounds queued per poll: the host learns of termination one chunk late, so up to 2 x chunk_max no-op
  // rounds run after the last one (LMMHIP_CHUNK_MAX, A/B knob): C4 3.48 ms at 8, 3.51-3.53 at 4, 3.55 at 16
  // (short rounds: the no-op tail is a larger share)
  const int chunk_max = std::max(2, env_int("LMMHIP_CHUNK_MAX", 8));
  P.chunk.hint = env_int("LMMHIP_ROUND_HINT", 1) ? c->hint_rounds_fr : 0;
  // with a hint the returning rounds after the last one are gone, and what longer chunks cost is with them: fewer
  // polls (mm_ctl_out, 3.6 us of kernel each) up to the hinted end (LMMHIP_HINT_CHUNK_MAX, A/B knob)
  P.chunk.max = P.chunk.hint > 0 ? std::max(chunk_max, env_int("LMMHIP_HINT_CHUNK_MAX", 32)) : chunk_max;
  // and the first chunk need not be short either (its point is an early poll for systems of few rounds)
  P.chunk.first = 2;
  if (P.chunk.hint > 0)
    P.chunk.first = std::max(2, std::min(P.chunk.max, env_int("LMMHIP_HINT_CHUNK0", P.chunk.max)));
  return P;
}

// Frontier engine (lmm_frontier_kernels.hpp): three launches per round, work proportional to the touched
// constraints and the moving votes.  Slots: 2 fr_vote, 4 fr_sat (+ fr_sat_big), 5 fr_update, 6 the per-chunk
// control-word copy; 0 / 1 init.
int solve_maxmin_frontier(lmmhip_ctx* c, double prec) {
  c->ran_engine = LMMHIP_RAN_FRONTIER;
  FrDev d{c->d, FrFields{}};  // (the engine's view of the system: its buffers are in no other engine's)
  if (!c->vote_diag)  // per-round diagnostic counters only on request (LMMHIP_VOTE_DIAG): they cost atomics
    d.vstat = nullptr;
  const int64_t nnz = std::max<int64_t>(d.nnz, 1);
  const int64_t nblk = std::max<int64_t>(1, (int64_t(d.nC) + kFB - 1) / kFB);  // (FrontierPlan::nblk)
  int2* cs = nullptr;
  int32_t* md = nullptr;
  int rc = scratch(c, c->frontier.c2s, nnz, &cs);
  rc = rc ? rc : scratch(c, c->frontier.pvb, std::max<int64_t>(d.nV, 1), &d.pvb);
  rc = rc ? rc : scratch(c, c->frontier.slot, nnz, &d.vslot);
  rc = rc ? rc : scratch(c, c->frontier.minfl, std::max<int64_t>(d.nC, 1), &d.minfl);
  rc = rc ? rc : scratch(c, c->frontier.key, std::max<int64_t>(d.nC, 1), &d.key32);
  rc = rc ? rc : scratch(c, c->frontier.qa, nnz, &d.fq_a);
  rc = rc ? rc : scratch(c, c->frontier.qb, nnz, &d.fq_b);
  rc = rc ? rc : scratch(c, c->frontier.qn, nblk + 1, &d.fq_n);
  rc = rc ? rc : scratch(c, c->frontier.md, 1, &md);
  if (rc)
    return rc;
  d.csr_cs = cs;
  if (!c->frontier.map_ok) {  // once per uploaded structure
    HIPCHK(hipMemsetAsync(md, 0, sizeof(int32_t), c->stream));
    if (d.nnz > 0) {
      hipLaunchKernelGGL(fr_c2s, dim3(grid_for(d.nC, kBlock / kWave)), dim3(kBlock), 0, c->stream, d, cs, md);
      HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(&c->frontier.maxdeg, md, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->frontier.map_ok = true;
  }
  const FrontierPlan P = frontier_plan(c, d);
  LAUNCH(0, -1, mm_init_cnsts, grid_for(d.nC, kBlock / kWave), kBlock, d, d.key32, prec, static_cast<double*>(nullptr));
  LAUNCH(1, -1, fr_init_vars, grid_for(std::max<int64_t>(std::max<int64_t>(d.nV, d.nC), d.nnz / 4), kBlock), kBlock, d);
  auto round_launches = [&](int64_t r) -> int {
    if (r == 0) {
      LAUNCH(2, r, fr_vote_all, grid_for(d.nV, kBlock), kBlock, d);
      LAUNCH(2, r, fr_minfl_all, grid_for(d.nC, kBlock / 16), kBlock, d);
    } else if (P.long_rows) {  // (LV08 routes: ~12 elements per row)
      LAUNCH(2, r, fr_vote<16>, (P.nblk + P.spb - 1) / P.spb, kFB, d, int(r), P.spb);
    } else {
      LAUNCH(2, r, fr_vote<8>, (P.nblk + P.spb - 1) / P.spb, kFB, d, int(r), P.spb);
    }
    if (P.sat_b == 256)
      LAUNCH(4, r, fr_sat<256>, P.nblk, 256, d, int(r), P.bigch);
    else
      LAUNCH(4, r, fr_sat<kFS>, P.nblk_sat, kFS, d, int(r), P.bigch);
    if (P.big)
      LAUNCH(4, r, fr_sat_big, P.g_big, kBlock, d, int(r), P.bigw);
    LAUNCH(5, r, fr_update, P.nblk, kFB, d, int(r), prec, P.upd_spec);
    return 0;
  };
  // pipelined termination polls (run_chunks); rounds queued after the last one return at once.  (Round 6,
  // measured and not kept: fr_vote storing "done" into a pinned host word itself, so that a poll is the event
  // alone without mm_ctl_out — C4 3.083-3.091 ms against 3.060-3.069, scripts/gpu_r06_p.sh; and the launches paced
  // by a per-round progress word, 2-5 rounds queued ahead — 3.17-3.28 against 3.12, scripts/gpu_r06_o.sh.)
  // Nothing at the end of a chunk but the poll, and no tail rule.
  if (int rc = run_chunks(c, d, P.chunk, round_launches, [](int64_t) { return 0; }, [](const int32_t*) { return false; }))
    return rc;
  c->hint_rounds_fr = int64_t(c->h_ctl.p[CTL_ROUNDS]) + 1;
  return 0;
}

int engine_of(const lmmhip_ctx* c) {
  // LMMHIP_ENGINE=rounds|persistent|frontier overrides the context's engine; "auto" (or any other value,
  // which is ignored) leaves the context's choice in place
  const char* e = std::getenv("LMMHIP_ENGINE");
  int eng = c->engine;
  if (e && std::strcmp(e, "rounds") == 0)
    eng = LMMHIP_ENGINE_ROUNDS;
  if (e && std::strcmp(e, "persistent") == 0)
    eng = LMMHIP_ENGINE_PERSISTENT;
  if (e && std::strcmp(e, "frontier") == 0)
    eng = LMMHIP_ENGINE_FRONTIER;
  // the profiling mode times every phase launch: a multi-launch engine
  if (c->profiling)
    return eng == LMMHIP_ENGINE_FRONTIER ? LMMHIP_ENGINE_FRONTIER : LMMHIP_ENGINE_ROUNDS;
  if (eng != LMMHIP_ENGINE_AUTO)
    return eng;
  // AUTO (measured): one launch per solve where the host round-trips and launches of the
  // round chain dominate (small systems: a tie at C4, 1e5 variables, and ahead below); the round chain
  // above, where the kernel boundaries (~1.5 us) are cheaper than grid barriers (~4 us) and per-launch
  // grids keep 32 waves per CU in flight instead of 16
  // round 4: the frontier engine between the two (C4, 1e5 LV08 flows: 3.54 ms against 4.34 persistent and
  // 4.48 rounds), the round engine above (C2: 25.8 against 28.2 frontier)
  if (int64_t(c->d.nV) <= kAutoPersistMaxVars)
    return LMMHIP_ENGINE_PERSISTENT;
  return int64_t(c->d.nV) <= kAutoPersistVars ? LMMHIP_ENGINE_FRONTIER : LMMHIP_ENGINE_ROUNDS;
}

// One persistent launch per solve (lmm_persist_kernels.hpp): one 1024-thread workgroup per CU, all
// resident (the occupancy query admits exactly one per CU); every barrier wait is bounded, so a fault in
// the protocol ends the launch with CTL_ERR instead of hanging the GPU.
// Persistent launches are serialised per device, process-wide: a persistent grid needs every CU for one
// workgroup at once (its barriers rely on co-residency), so two of them running side by side — two Systems
// on two streams, or two threads — could each hold part of the chip and wait on the other.  Each persistent
// launch waits (on its own stream, no host blocking) for the previous one's completion event
// (g_persist_last, above).

static int solve_maxmin_persist_once(lmmhip_ctx* c, double prec, bool* closed) {
  Dev d = c->d;
  d.vstat = nullptr;
  const bool bits = int64_t(d.nC) <= int64_t(kPBitWords) * 64;
  // 8 row elements in registers in the re-vote, longer rows loop over the rest.  (A 10-register variant for
  // long mean rows — C4's LV08 routes, 11.7 elements, when C4 still ran here — sat at the 128-VGPR budget of a
  // 1024-thread workgroup and spilled once the launch rendezvous moved ahead of the init; C4 runs on the
  // frontier engine since round 4, and AUTO keeps this engine for systems of at most 2^14 variables.)
  const void* kern = bits ? reinterpret_cast<const void*>(&mm_persist<true, 8>)
                          : reinterpret_cast<const void*>(&mm_persist<false, 8>);
  if (!c->pbar.p)
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->pbar.p), BAR_WORDS * sizeof(unsigned)));
  int per_cu = 0;
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kPB, 0));
  if (per_cu < 1)
    return fail(LMMHIP_E_HIP, "persistent maxmin kernel: not one workgroup per CU (occupancy query)");
  const int grid = c->n_cu;
  c->persist_grid = grid;
  const int max_rounds = int(std::min<int64_t>(int64_t(d.nV) + 2, INT32_MAX - 1));
  const int cmp_every = env_int("LMMHIP_COMPACT_EVERY", 16);
  unsigned* barw = c->pbar.p;
  long long* pt = nullptr;
  unsigned pt_cap = 0;
  if (c->persist_prof) {  // barrier timestamps (lmmhip_persist_profile)
    pt_cap = kPersistProfCap;
    const size_t bytes = sizeof(long long) * (2 * size_t(pt_cap) + 2 * size_t(kPBlkCap) * size_t(grid));
    if (!c->ptime.p)
      HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->ptime.p), bytes));
    HIPCHK(hipMemsetAsync(c->ptime.p, 0, bytes, c->stream));
    pt = c->ptime.p;
  }
  int sysf = env_int("LMMHIP_PERSIST_SYSFENCE", 0);
  // launch rendezvous deadline (bar_rdv): the grid's workgroups are dispatched within microseconds when the CUs
  // are free, so 20 ms of waiting means part of the chip is held by someone else
  long long rdv_ticks = 100000LL * env_int("LMMHIP_PERSIST_RDV_MS", 20);  // 100 MHz wall clock
  int32_t* hflag = c->d_rdv;
  void* args[] = {&d, &barw, &prec, const_cast<int*>(&max_rounds), const_cast<int*>(&cmp_every), &pt, &pt_cap, &sysf,
                  &rdv_ticks, &hflag};
  // A plain launch on the context's stream: the occupancy query above guarantees one workgroup per CU, so the
  // n_cu workgroups are co-resident once the stream's earlier work has drained and nothing else holds CUs; the
  // rendezvous deadline and the bounded barrier waits cover the case where something does.
  // (Not hipLaunchCooperativeKernel: it runs the same kernel through the runtime's device-wide cooperative queue,
  // whose teardown at process exit crashed inside the HSA runtime under rocprofv3 — SIGSEGV in libamdhip64's exit
  // handler)
  {
    std::lock_guard<std::mutex> lk(g_persist_mu);
    Event& last = g_persist_last[c->device];
    if (last.p && hipStreamWaitEvent(c->stream, last.p, 0) != hipSuccess) {  // (a stale event: make a new one)
      (void)hipGetLastError();
      (void)last.reset();
    }
    if (!last.p)
      HIPCHK(hipEventCreateWithFlags(&last.p, hipEventDisableTiming));
    // the barrier words are reset behind the previous persistent launch (whose late workgroups, after a closed
    // rendezvous, still read them)
    HIPCHK(hipMemsetAsync(c->pbar.p, 0, BAR_WORDS * sizeof(unsigned), c->stream));
    HIPCHK(hipMemsetAsync(d.chgbits, 0, sizeof(uint64_t) * ((d.nC + 127) / 128 * 2 + 2), c->stream));
    __atomic_store_n(c->h_rdv.p, 0, __ATOMIC_RELEASE);
    HIPCHK(hipLaunchKernel(kern, dim3(grid), dim3(kPB), args, 0, c->stream));
    HIPCHK(hipEventRecord(last.p, c->stream));
  }
  c->stats.kernel_launches[2] += 1;
  HIPCHK(hipEventRecord(c->ev1.p, c->stream));
  c->ev1_done = true;
  // wait for the launch, or for its rendezvous to close (the mapped word), whichever comes first
  for (;;) {
    const hipError_t q = hipEventQuery(c->ev1.p);
    if (q == hipSuccess)
      break;
    if (q != hipErrorNotReady)
      HIPCHK(q);
    if (__atomic_load_n(c->h_rdv.p, __ATOMIC_ACQUIRE)) {  // closed: no workgroup of it has written anything
      // The launch is left behind with its late workgroups (they return at once when they get CUs).  A context
      // on its own stream moves to a new one, so the fallback and everything after it run on the free CUs now;
      // a caller-provided stream keeps its order (the fallback then waits for the late workgroups).
      *closed = true;
      if (c->stream == c->own_stream.p) {
        Stream ns;
        HIPCHK(hipStreamCreateWithFlags(&ns.p, hipStreamNonBlocking));
        std::swap(ns.p, c->own_stream.p);
        c->stream = c->own_stream.p;
        c->retired_streams.push_back(std::move(ns));
      }
      return fail(LMMHIP_E_HIP, "persistent maxmin kernel: the launch rendezvous closed (grid not co-resident)");
    }
    std::this_thread::yield();
  }
  if (int rc = poll_ctl(c))
    return rc;
  if (c->h_ctl.p[CTL_ERR] == 1)
    return fail(LMMHIP_E_HIP, "persistent maxmin kernel: a grid-barrier wait timed out");
  if (c->h_ctl.p[CTL_ERR] == 2)
    return fail(LMMHIP_E_NOCONVERGE, "maxmin round guard tripped");
  return 0;
}

// A persistent solve that cannot run — its launch rendezvous closed because part of the grid could not become
// resident within LMMHIP_PERSIST_RDV_MS (another kernel or process holding CUs: bar_rdv), or, later, a
// grid-barrier wait timed out (CTL_ERR 1) — is not an error of the system: the solve is re-run by the
// multi-launch engine, whose results are bit-identical (tests/test_gpu_engines.py).  The next
// LMMHIP_PERSIST_COOLDOWN solves of the context then take the multi-launch engine directly (a
// fallback that did not stick made every later solve under sustained contention pay the wait again).

// Streams left behind by closed persistent launches (their late workgroups may still run): each one whose work has
// drained is destroyed; past kRetiredCap of them the oldest is waited for (under sustained contention
// the list grew by one stream per close without bound).
constexpr size_t kRetiredCap = 8;
static int reap_retired_streams(lmmhip_ctx* c) {
  auto& v = c->retired_streams;
  for (size_t i = 0; i < v.size();) {
    const hipError_t q = hipStreamQuery(v[i].p);
    if (q == hipErrorNotReady) {
      i++;
      continue;
    }
    v.erase(v.begin() + long(i));  // (destroys it)
  }
  while (v.size() > kRetiredCap) {
    HIPCHK(hipStreamSynchronize(v.front().p));
    v.erase(v.begin());
  }
  return 0;
}

int solve_maxmin_persist(lmmhip_ctx* c, double prec) {
  c->ran_engine = LMMHIP_RAN_PERSISTENT;  // (solve_maxmin overwrites it when the solve falls back)
  if (int rc = reap_retired_streams(c))
    return rc;
  if (c->persist_cool > 0) {
    c->persist_cool -= 1;
    return solve_maxmin(c, prec);
  }
  c->h_ctl.p[CTL_ERR] = 0;
  bool closed = false;
  const int rc = solve_maxmin_persist_once(c, prec, &closed);
  if (!closed && (rc != LMMHIP_E_HIP || c->h_ctl.p[CTL_ERR] != 1))
    return rc;
  c->persist_fallbacks += 1;
  c->persist_cool = env_int("LMMHIP_PERSIST_COOLDOWN", 64);
  HIPCHK(hipMemsetAsync(c->d.ctl, 0, CTL_ALLOC * sizeof(int32_t), c->stream));
  c->ev1_done = false;
  return solve_maxmin(c, prec);
}

// ---- block-diagonal batches: one workgroup per system, the system in LDS (lmm_batch_kernels.hpp) ----
bool batch_fits(const lmmhip_ctx* c) {
  if (c->bt_n <= 0 || c->profiling)
    return false;
  if (const char* e = std::getenv("LMMHIP_BATCH"); e && *e == '0')
    return false;
  // (every member has to fit alone: solve_maxmin_batch lays the LDS out for each system by its own sizes if need be)
  return c->bt_max_nv < 65535 && c->bt_max_nc < 65535 && c->bt_max_nnz < 65535 && c->bt_lds <= kBatchLdsMax;
}

int batch_rounds_to_ctl(lmmhip_ctx* c, int grid) {
  hipLaunchKernelGGL(mm_batch_rounds, dim3(1), dim3(kBlock), 0, c->stream, c->bt_rounds.p, grid, c->d.ctl);
  HIPCHK(hipGetLastError());
  return 0;
}

int solve_maxmin_batch(lmmhip_ctx* c, double prec) {
  c->ran_engine = LMMHIP_RAN_BATCH;
  // one layout for the launch when the batch's largest counts fit together, else every system by its own sizes
  const size_t lds_max = batch_lds_bytes(c->bt_max_nv, c->bt_max_nc, c->bt_max_nnz);
  const bool own = lds_max > kBatchLdsMax;
  const size_t lds = own ? c->bt_lds : lds_max;
  const void* kern = own ? reinterpret_cast<const void*>(&mm_batch_lds<true>)
                         : reinterpret_cast<const void*>(&mm_batch_lds<false>);
  int per_cu = 0;
  HIPCHK(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(kBatchLdsMax)));
  HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, kBB, lds));
  int64_t grid = std::max<int64_t>(1, std::min<int64_t>(c->bt_n, int64_t(c->n_cu) * std::max(per_cu, 1)));
  // LMMHIP_BATCH_GRID=n: at most n workgroups (tests, measurement: several systems per workgroup's LDS)
  if (const int cap = env_int("LMMHIP_BATCH_GRID", 0); cap > 0)
    grid = std::min<int64_t>(grid, cap);
  if (grid > c->bt_cap) {
    HIPCHK(c->bt_rounds.reset());
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->bt_rounds.p), sizeof(int32_t) * size_t(grid)));
    c->bt_cap = grid;
  }
  Dev d = c->d;
  if (own)
    hipLaunchKernelGGL(mm_batch_lds<true>, dim3(unsigned(grid)), dim3(kBB), lds, c->stream, d, c->bt_voff.p,
                       c->bt_coff.p, c->bt_n, prec, c->bt_max_nv, c->bt_max_nc, c->bt_max_nnz, c->bt_rounds.p);
  else
    hipLaunchKernelGGL(mm_batch_lds<false>, dim3(unsigned(grid)), dim3(kBB), lds, c->stream, d, c->bt_voff.p,
                       c->bt_coff.p, c->bt_n, prec, c->bt_max_nv, c->bt_max_nc, c->bt_max_nnz, c->bt_rounds.p);
  HIPCHK(hipGetLastError());
  c->stats.kernel_launches[2] += 1;
  HIPCHK(hipEventRecord(c->ev1.p, c->stream));
  c->ev1_done = true;
  if (int rc = batch_rounds_to_ctl(c, int(grid)))
    return rc;
  if (int rc = poll_ctl(c))
    return rc;
  if (c->h_ctl.p[CTL_ERR] == 2)
    return fail(LMMHIP_E_NOCONVERGE, "batch maxmin round guard tripped");
  return 0;
}

int lmmhip_set_batch(lmmhip_ctx* c, int64_t nsys, const int64_t* var_off, const int64_t* cnst_off) {
  if (!c || !c->uploaded)
    return fail(LMMHIP_E_STATE, "no system uploaded");
  c->bt_n = 0;
  if (nsys == 0)
    return 0;
  if (nsys < 0 || !var_off || !cnst_off)
    return fail(LMMHIP_E_ARG, "bad batch arguments");
  const Dev& d = c->d;
  if (var_off[0] != 0 || var_off[nsys] != d.nV || cnst_off[0] != 0 || cnst_off[nsys] != d.nC)
    return fail(LMMHIP_E_ARG, "batch offsets must cover the uploaded system");
  for (int64_t i = 0; i < nsys; i++)
    if (var_off[i + 1] < var_off[i] || cnst_off[i + 1] < cnst_off[i])
      return fail(LMMHIP_E_ARG, "batch offsets not monotone");
  HIPCHK(hipSetDevice(c->device));
  std::vector<uint32_t> vp(size_t(d.nV) + 1);
  HIPCHK(hipMemcpyAsync(vp.data(), d.var_ptr, vp.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  int64_t mv = 0, mc = 0, me = 0;
  size_t lds = 0;  // the max-min batch kernel's need: the largest over the systems, each by its own sizes
  for (int64_t i = 0; i < nsys; i++) {
    const int64_t nv = var_off[i + 1] - var_off[i], nc = cnst_off[i + 1] - cnst_off[i];
    const int64_t ne = int64_t(vp[size_t(var_off[i + 1])]) - int64_t(vp[size_t(var_off[i])]);
    mv = std::max(mv, nv);
    mc = std::max(mc, nc);
    me = std::max(me, ne);
    if (nv < 65535 && nc < 65535 && ne < 65535)  // (larger ones: no batch engine, batch_fits)
      lds = std::max(lds, batch_lds_bytes(int(nv), int(nc), int(ne)));
  }
  HIPCHK(c->bt_voff.reset());
  HIPCHK(c->bt_coff.reset());
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->bt_voff.p), sizeof(int64_t) * size_t(nsys + 1)));
  HIPCHK(hipMalloc(reinterpret_cast<void**>(&c->bt_coff.p), sizeof(int64_t) * size_t(nsys + 1)));
  HIPCHK(hipMemcpyAsync(c->bt_voff.p, var_off, sizeof(int64_t) * size_t(nsys + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemcpyAsync(c->bt_coff.p, cnst_off, sizeof(int64_t) * size_t(nsys + 1), hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipMemsetAsync(d.ctl + CTL_ERR, 0, sizeof(int32_t), c->stream));
  hipLaunchKernelGGL(mm_batch_check, dim3(unsigned(std::min<int64_t>(nsys, 4096))), dim3(kBlock), 0, c->stream, d,
                     c->bt_voff.p, c->bt_coff.p, nsys, d.ctl + CTL_ERR);
  HIPCHK(hipGetLastError());
  int32_t bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, d.ctl + CTL_ERR, sizeof(bad), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (bad)
    return fail(LMMHIP_E_ARG, "batch: an element links two declared systems (not block-diagonal)");
  c->bt_n = nsys;
  c->bt_max_nv = int(mv);
  c->bt_max_nc = int(mc);
  c->bt_max_nnz = int(me);
  c->bt_lds = lds;
  return 0;
}
