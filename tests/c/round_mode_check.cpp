// CPU check of the round engine's mode resolution (simgrid_amd/csrc/lmm_round_mode.hpp: resolve_round_mode, VoteMode,
// UpdMode; called by round_plan in lmm_hip_maxmin.hip).  round_plan used to compute the mode as loose bools and to pick
// the vote kernels from two hand-written tables; those lines are kept here literally (old_plan, the environment's values
// as arguments) and replayed next to the header's functions over group sizes, knob values, CU counts and constraint
// counts on both sides of every boundary of kUSeg, kBlock and kMaxBlocks.  Same mode, same update grid, same table
// position (under the map of the old tables' positions to mode indices); every resolved mode is one of the nine valid
// ones and every one of the nine is reached.  Prints the number of cases; exit 1 on a mismatch.  (Built and run by
// tests/test_round_mode.py.)
#include <cstdio>
#include <set>
#include <vector>

#include "../../simgrid_amd/csrc/lmm_round_mode.hpp"

constexpr int kBlock = 256, kUSeg = 1024, kMaxBlocks = 2048;  // (lmm_dev.hpp, lmm_maxmin_kernels.hpp)

// every index decodes to a valid mode and encodes back to itself; nothing else is a mode
template <int I> constexpr bool all_ok() { return vote_mode_ok(I) && all_ok<I - 1>(); }
template <> constexpr bool all_ok<-1>() { return true; }
static_assert(all_ok<kVoteModes - 1>() && !vote_mode_ok(-1) && !vote_mode_ok(kVoteModes), "nine modes, 0..8");
static_assert(!VoteMode{RowForm::Arrays, true, false}.valid() && !VoteMode{RowForm::Arrays, false, true}.valid(),
              "the queue and the filter exist on the record forms only");
static_assert(vote_block(VoteForm::Bitmap) == 1024 && vote_bits(VoteForm::Bitmap) && vote_block(VoteForm::Scan) == 256 &&
                  !vote_bits(VoteForm::Scan),
              "the two lane-vote forms");

static int grid_for(int64_t n, int per_block) {  // (lmm_dev.hpp)
  int64_t g = (n + per_block - 1) / per_block;
  if (g < 1)
    g = 1;
  if (g > kMaxBlocks)
    g = kMaxBlocks;
  return int(g);
}

struct Env {  // env_int's results: a knob's value, or its default
  int crec, rdq, satkey, cmp_rows, upd_quad, upd_blocks, updq_blocks;
};
struct Old {
  bool crec, rdq, satkey, rows, upd_quad;
  int g_upd;
  int table, row, col;  // 0: kVoteTable[row][col], 1: kVoteRowsTable[row][col]
  int upd_row, upd_col;  // kUpdTable[rdq][upd_quad]
};

// round_plan's lines as they were
static Old old_plan(int group, int64_t nC, const Env& e) {
  Old P;
  const bool short_rows = group == 4 || group == 8;
  P.crec = short_rows && e.crec;
  const int cap_upd = e.upd_blocks;
  const int64_t gU_need = (int64_t(nC) + kUSeg - 1) / kUSeg;
  const int64_t gU_rdq = std::max<int64_t>(
      1, std::min<int64_t>(grid_for(nC, kBlock), std::max<int64_t>(gU_need, e.updq_blocks)));
  const int64_t per_blk = int64_t(kBlock) * ((int64_t(nC) + gU_rdq * kBlock - 1) / (gU_rdq * kBlock));
  P.rdq = P.crec && e.rdq && per_blk <= kUSeg && cap_upd == 0;
  P.satkey = e.satkey != 0;
  P.rows = P.crec && e.cmp_rows != 0;
  const int row = short_rows ? (P.rdq ? 2 : P.crec ? 1 : 0) : group == 16 ? 3 : group == 32 ? 4 : 5;
  P.table = P.rows ? 1 : 0;
  P.row = P.rows ? int(P.rdq) : row;
  P.col = int(P.satkey);
  P.upd_quad = e.upd_quad != 0;
  P.upd_row = int(P.rdq);
  P.upd_col = int(P.upd_quad);
  const int g_c = grid_for(nC, kBlock);
  P.g_upd = P.rdq ? int(gU_rdq) : cap_upd > 0 && g_c > cap_upd ? cap_upd : g_c;
  return P;
}

// The old tables' positions as mode indices: kVoteTable rows 0-2 were no records / 8-B records / 8-B records + ready
// queue, each [without, with] the filter (row 0: the same kernels in both columns), rows 3-5 mm_vote<16|32|64> (no
// records: the Arrays mode); kVoteRowsTable[queue][filter] the 16-B records.
static int old_index(const Old& P) {
  if (P.table == 1)
    return 5 + 2 * P.row + P.col;
  return P.row == 0 || P.row >= 3 ? 0 : P.row == 1 ? 1 + P.col : 3 + P.col;
}

int main() {
  std::set<int64_t> ncs = {0, 1};
  const int n_cus[] = {1, 8, 256};
  std::vector<int64_t> bounds = {kBlock, 2 * kBlock, 7 * kBlock, kUSeg, 2 * kUSeg, int64_t(kMaxBlocks) * kBlock,
                                 int64_t(kMaxBlocks) * kUSeg};
  for (int n_cu : n_cus) {  // the segments of the default update grid full / the default grid's whole blocks
    bounds.push_back(int64_t(updq_blocks_default(n_cu)) * kUSeg);
    bounds.push_back(int64_t(updq_blocks_default(n_cu)) * kBlock);
  }
  for (int64_t b : bounds)
    for (int64_t x = b - 1; x <= b + 1; x++)
      ncs.insert(x);
  long cases = 0;
  std::set<int> reached;
  const int groups[] = {4, 8, 16, 32, 64};
  for (int group : groups)
    for (int bits = 0; bits < 32; bits++)
      for (int upd_blocks : {0, 7})
        for (int n_cu : n_cus)
          for (int updq : {1, updq_blocks_default(n_cu)})
            for (int64_t nC : ncs) {
              const Env e = {bits & 1, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1, (bits >> 4) & 1, upd_blocks, updq};
              const Old o = old_plan(group, nC, e);
              RoundKnobs k;
              k.crec = e.crec, k.rdq = e.rdq, k.satkey = e.satkey, k.cmp_rows = e.cmp_rows, k.upd_quad = e.upd_quad;
              k.upd_blocks = e.upd_blocks, k.updq_blocks = e.updq_blocks;
              const RoundMode m = resolve_round_mode(group, nC, k, RoundLimits{kBlock, kUSeg, kMaxBlocks});
              const VoteMode v = m.vote;
              const RowForm form = !o.crec ? RowForm::Arrays : o.rows ? RowForm::Rec16 : RowForm::Rec8;
              // (the old satkey flag was set without records too, where both columns of the table held the same kernels)
              const bool same = v.form == form && v.rec() == o.crec && v.rec16() == o.rows && v.rdq() == o.rdq &&
                                v.sat_retire() == (o.crec && o.satkey) && m.upd_quad == o.upd_quad && m.g_upd == o.g_upd;
              const bool pos = v.index() == old_index(o) && m.upd().index() == 2 * o.upd_row + o.upd_col &&
                               m.upd().rdq() == o.rdq && m.upd().quad() == o.upd_quad;
              const bool valid = v.valid() && vote_mode_ok(v.index()) && vote_mode(v.index()).form == v.form &&
                                 vote_mode(v.index()).queue == v.queue && vote_mode(v.index()).filter == v.filter &&
                                 (!v.rdq() || m.rdq_fits) && (group == 4 || group == 8 || v.index() == kVoteArrays);
              if (!same || !pos || !valid) {
                std::printf("mismatch: group %d nC %lld n_cu %d knobs %d upd_blocks %d updq %d: index %d old %d g_upd %d old %d\n",
                            group, (long long)nC, n_cu, bits, upd_blocks, updq, v.index(), old_index(o), m.g_upd, o.g_upd);
                return 1;
              }
              reached.insert(v.index());
              cases++;
            }
  if (int(reached.size()) != kVoteModes) {
    std::printf("only %zu of the %d modes reached\n", reached.size(), kVoteModes);
    return 1;
  }
  std::printf("ok %ld\n", cases);
  return 0;
}
