// lmm_round_mode.hpp — the round engine's modes by name: what a re-vote reads its row from, whether the vote queues the
// constraints it makes ready, whether its filter retires the rows of saturated targets, and how the update moves its
// records.  Plain host / device code (constexpr only, no HIP): the kernels of lmm_maxmin_kernels.hpp take a mode's index
// as their template argument and read its properties, round_plan (lmm_hip_maxmin.hip) resolves the solve's mode from
// the knobs' values and indexes the kernel tables with the same index; tests/c/round_mode_check.cpp replays the
// resolution.
#pragma once
#include <algorithm>
#include <cstdint>

// What a re-vote reads the row from (vote_row): the cvar / crow arrays, or one packed record per alive row —
// 8 B {cvar, begin} (the end is the next record's begin; a compaction copies the alive rows' elements), or 16 B
// {cvar, begin, end, 0} (offsets into the original CSR; a compaction moves the per-row words only).  Selects the member
// of RowRecs (lmm_dev.hpp) too.
enum class RowForm { Arrays, Rec8, Rec16 };

// The form of the short-row lane vote: the changed-constraint bitmap in LDS, one 1024-thread workgroup per CU, or the
// change stamps gathered per row by 256-thread workgroups over the rows.
enum class VoteForm { Bitmap, Scan };
constexpr int vote_block(VoteForm f) { return f == VoteForm::Bitmap ? 1024 : 256; }
constexpr bool vote_bits(VoteForm f) { return f == VoteForm::Bitmap; }

// A vote mode.  The queue (LMMHIP_RDQ) and the filter (LMMHIP_SATKEY) exist on the record forms only: nine modes,
// index 0 = Arrays, 1 + 4 * (Rec16) + 2 * queue + filter the others.
constexpr int kVoteModes = 9;
struct VoteMode {
  RowForm form = RowForm::Arrays;
  bool queue = false;   // a constraint a re-vote makes ready is queued for the saturation (no mm_ready pass)
  bool filter = false;  // the filter retires a row whose target's key is kSatKey; the re-votes read no variable state
  constexpr bool rec() const { return form != RowForm::Arrays; }
  constexpr bool rec16() const { return form == RowForm::Rec16; }
  constexpr bool rdq() const { return queue; }
  constexpr bool sat_retire() const { return filter; }
  // the tied constraints' exact ratios loaded together (vote_row): the record forms, which only the round engine's
  // short-row vote runs.  Arrays — the round engine without records, the persistent kernel — keeps its registers.
  constexpr bool tie_loads() const { return rec(); }
  // a bounded variable's level bound * penalty compared by its key first, the exact ratios read only where the keys tie
  // (vote_row): the record forms again — in the persistent kernel the key's register spilled 39 VGPRs
  constexpr bool bound_keys() const { return rec(); }
  constexpr bool valid() const { return rec() || (!queue && !filter); }
  constexpr int index() const { return !rec() ? 0 : 1 + 4 * int(rec16()) + 2 * int(queue) + int(filter); }
};
constexpr VoteMode vote_mode(int i) {
  return i == 0 ? VoteMode{} : VoteMode{(i - 1) & 4 ? RowForm::Rec16 : RowForm::Rec8, ((i - 1) & 2) != 0, ((i - 1) & 1) != 0};
}
// (what a kernel asserts of its template argument: a mode of the valid set, in its one encoding)
constexpr bool vote_mode_ok(int i) {
  return i >= 0 && i < kVoteModes && vote_mode(i).valid() && vote_mode(i).index() == i;
}
constexpr int kVoteArrays = 0;  // the mode of everything that is not the round engine's record vote

// The update's mode: the ready queue's segments (as the vote's queue) and the touched records as one 64-B request per
// quad of lanes (LMMHIP_UPD_QUAD).  Index 2 * queue + quad.
constexpr int kUpdModes = 4;
struct UpdMode {
  bool queue = false, quad4 = false;
  constexpr bool rdq() const { return queue; }
  constexpr bool quad() const { return quad4; }
  constexpr int index() const { return 2 * int(queue) + int(quad4); }
};
constexpr UpdMode upd_mode(int i) { return UpdMode{(i & 2) != 0, (i & 1) != 0}; }
constexpr bool upd_mode_ok(int i) { return i >= 0 && i < kUpdModes; }
constexpr int kUpdPlain = 0;  // no queue, lane by lane: the persistent kernel's

// ---- resolution: the solve's mode from the knobs' values ----
struct RoundKnobs {  // LMMHIP_CREC, _RDQ, _SATKEY, _CMP_ROWS, _UPD_QUAD (0 = off), _UPD_BLOCKS (0 = uncapped), _UPDQ_BLOCKS
  int crec = 1, rdq = 1, satkey = 1, cmp_rows = 1, upd_quad = 1, upd_blocks = 0, updq_blocks = 0;
};
constexpr int updq_blocks_default(int n_cu) { return 4 * n_cu; }  // four update workgroups per CU
struct RoundLimits {  // kBlock, kUSeg, kMaxBlocks
  int block, useg, max_blocks;
};
struct RoundMode {
  VoteMode vote;
  bool upd_quad = false;
  bool rdq_fits = false;  // the ready queue's precondition: every update workgroup's constraints fit its segment
  int g_upd = 1;          // mm_update's grid: the ready queue's segments, or the (capped) thread-per-constraint grid
  constexpr UpdMode upd() const { return UpdMode{vote.queue, upd_quad}; }
};

constexpr int64_t round_grid_for(int64_t n, int per_block, int max_blocks) {
  return std::max<int64_t>(1, std::min<int64_t>((n + per_block - 1) / per_block, max_blocks));
}

// Row records on short rows (groups of 4 and 8) only; with them the 16-B form, the ready queue — when at most
// L.max_blocks update workgroups, four per CU unless more are needed, keep every segment within L.useg and the update's
// grid is uncapped — and the filter.
constexpr RoundMode resolve_round_mode(int group, int64_t nC, const RoundKnobs& k, const RoundLimits& L) {
  RoundMode m;
  const bool rec = (group == 4 || group == 8) && k.crec != 0;
  const int64_t g_c = round_grid_for(nC, L.block, L.max_blocks);
  const int64_t g_need = (nC + L.useg - 1) / L.useg;
  const int64_t g_rdq = std::max<int64_t>(1, std::min<int64_t>(g_c, std::max<int64_t>(g_need, k.updq_blocks)));
  const int64_t per_blk = int64_t(L.block) * ((nC + g_rdq * L.block - 1) / (g_rdq * L.block));
  m.rdq_fits = per_blk <= L.useg && k.upd_blocks == 0;
  m.vote.form = !rec ? RowForm::Arrays : k.cmp_rows != 0 ? RowForm::Rec16 : RowForm::Rec8;
  m.vote.queue = rec && k.rdq != 0 && m.rdq_fits;
  m.vote.filter = rec && k.satkey != 0;
  m.upd_quad = k.upd_quad != 0;
  m.g_upd = int(m.vote.queue ? g_rdq : k.upd_blocks > 0 && g_c > k.upd_blocks ? k.upd_blocks : g_c);
  return m;
}
