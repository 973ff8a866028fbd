// CPU check of the chunk policy of the round-chain engines (simgrid_amd/csrc/lmm_chunk.hpp: ChunkPolicy,
// round_hint_chunk, chunk_grow; driven by run_chunks in lmm_hip_maxmin.hip).  The two engines each had their own copy
// of the loop; those two copies' arithmetic is kept here literally (old_rounds, old_frontier) and replayed next to the
// shared one on a model of the pipelined polls: a solve of R rounds whose words after r queued rounds say "done" when
// r >= R, arrive one chunk late unless the chunk ended at the hint, and — round engine — show the tail from round T
// on.  The sequences of chunk lengths must be equal.  Prints the number of cases; exit 1 on a mismatch.  (Built and
// run by tests/test_chunk_policy.py.)
#include <cstdio>
#include <vector>

#include "../../simgrid_amd/csrc/lmm_chunk.hpp"

struct Polls {  // CtlPoll::step on the model: the newest round count the host has seen, -1 = none yet
  int64_t prev = -1;
  bool pending = false;
  int64_t step(int64_t r, bool stop, int64_t R) {
    int64_t seen = pending ? prev : -1;
    pending = !stop;
    if (stop && !(seen >= 0 && seen >= R))
      seen = r;
    prev = r;
    return seen;
  }
};

// solve_maxmin's loop as it was: chunk 2, doubling to chunk_max, the tail rule on the host's view of the sizes
static std::vector<int> old_rounds(int64_t hint, int64_t R, int chunk_max, int ctail, int64_t T) {
  std::vector<int> seq;
  Polls poll;
  int64_t r = 0;
  bool tail_seen = T <= 0;  // (nrows <= ctail_rows || ncl <= ctail_cnst) on the words the host has
  int chunk = 2;
  for (;;) {
    bool stop = false;
    int n = chunk;
    if (hint > r && r + chunk >= hint) {
      stop = true;
      n = int(hint - r);
    }
    r += n;
    seq.push_back(n);
    const int64_t h = poll.step(r, stop, R);
    if (h >= 0) {
      if (h >= R)
        break;
      tail_seen = h >= T;
    }
    if (chunk < chunk_max)
      chunk = std::min(2 * chunk, chunk_max);
    if (tail_seen && chunk > ctail)
      chunk = ctail;
  }
  return seq;
}

// solve_maxmin_frontier's loop as it was: the first chunk and the cap depend on the hint (chunk0 / chunk_cap)
static std::vector<int> old_frontier(int64_t hint, int64_t R, int chunk0, int chunk_cap) {
  std::vector<int> seq;
  Polls poll;
  int64_t r = 0;
  int chunk = chunk0;
  for (;;) {
    bool stop = false;
    int n = chunk;
    if (hint > r && r + chunk >= hint) {
      stop = true;
      n = int(hint - r);
    }
    r += n;
    seq.push_back(n);
    const int64_t h = poll.step(r, stop, R);
    if (h >= 0 && h >= R)
      break;
    if (chunk < chunk_cap)
      chunk = std::min(2 * chunk, chunk_cap);
  }
  return seq;
}

// run_chunks' loop on the same model
static std::vector<int> shared(const ChunkPolicy& p, int64_t R, int64_t T) {
  std::vector<int> seq;
  Polls poll;
  int64_t r = 0;
  bool tail_seen = T <= 0;
  int chunk = p.first;
  for (;;) {
    bool stop = false;
    const int n = round_hint_chunk(r, chunk, p.hint, &stop);
    r += n;
    seq.push_back(n);
    const int64_t h = poll.step(r, stop, R);
    if (h >= 0 && h >= R)
      break;
    if (h >= 0)
      tail_seen = h >= T;
    chunk = chunk_grow(chunk, p, tail_seen);
  }
  return seq;
}

int main() {
  long cases = 0;
  const int64_t Rs[] = {1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 100, 257, 1000};
  for (int64_t R : Rs)
    for (int64_t dh : {-1000000, -40, -3, -1, 0, 1, 2, 7, 64}) {  // hint = R + dh; <= 0: none
      const int64_t hint = std::max<int64_t>(0, R + dh);
      for (int chunk_max : {2, 3, 4, 8, 16, 32, 64})
        for (int ctail : {1, 3, 4, 8, 100})
          for (int64_t T : {int64_t(0), R / 2, R - 3, R + 10}) {
            ChunkPolicy p;
            p.first = 2;
            p.max = chunk_max;
            p.hint = hint;
            p.tail = ctail;
            if (old_rounds(hint, R, chunk_max, ctail, T) != shared(p, R, T)) {
              std::printf("round engine: mismatch at R=%lld hint=%lld max=%d tail=%d T=%lld\n", (long long)R,
                          (long long)hint, chunk_max, ctail, (long long)T);
              return 1;
            }
            cases++;
          }
      for (int chunk_cap : {2, 4, 8, 32})
        for (int chunk0 : {2, 4, 8, 32}) {
          if (chunk0 > chunk_cap)
            continue;
          ChunkPolicy p;  // (no tail rule: tail = 0)
          p.first = chunk0;
          p.max = chunk_cap;
          p.hint = hint;
          if (old_frontier(hint, R, chunk0, chunk_cap) != shared(p, R, R + 1)) {
            std::printf("frontier: mismatch at R=%lld hint=%lld cap=%d first=%d\n", (long long)R, (long long)hint,
                        chunk_cap, chunk0);
            return 1;
          }
          cases++;
        }
    }
  std::printf("ok %ld cases\n", cases);
  return 0;
}
