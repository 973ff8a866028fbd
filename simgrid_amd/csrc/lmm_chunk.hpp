// lmm_chunk.hpp — how many rounds the round-chain engines (round, frontier) queue per termination poll: the policy and
// its arithmetic, plain host code (run_chunks in lmm_hip_maxmin.hip drives it; tests/c/chunk_policy_check.cpp replays it).
#pragma once
#include <algorithm>
#include <cstdint>

struct ChunkPolicy {
  int first = 2;     // rounds of the first chunk: an early poll for systems of few rounds
  int max = 2;       // a chunk doubles after every poll up to this many rounds
  int64_t hint = 0;  // rounds the context's previous solve had to queue (round_hint_chunk); 0 = none
  int tail = 0;      // once the engine says the solve is in its tail, a chunk is at most this long (0 = no tail rule)
};

// Chunk length under a round-count hint: a chunk that would cross the hinted end E is cut to end at it, and the
// caller waits for that chunk before queueing more (*stop), so a solve as long as the previous one runs no returning
// rounds after its last one; a longer one pays one host round trip there, a shorter one is caught by the usual polls.
// Consecutive solves of a simulation change little, so their round counts do too.  LMMHIP_ROUND_HINT=0: off.
inline int round_hint_chunk(int64_t r, int chunk, int64_t hint, bool* stop) {
  *stop = false;
  if (hint > r && r + chunk >= hint) {
    *stop = true;
    return int(hint - r);
  }
  return chunk;
}

// The next chunk after a poll: twice the last one up to the maximum, cut to the tail length in the solve's tail.
inline int chunk_grow(int chunk, const ChunkPolicy& p, bool in_tail) {
  if (chunk < p.max)
    chunk = std::min(2 * chunk, p.max);
  if (in_tail && p.tail > 0 && chunk > p.tail)
    chunk = p.tail;
  return chunk;
}
