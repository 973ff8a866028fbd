// lmm_common_kernels.hpp — the small kernels that more than one part of the driver needs (upload, resident
// refresh, the termination polls of the max-min and FairBottleneck engines, the getters).
//
// Every __global__ kernel is compiled in exactly one translation unit: this header is included by lmm_hip.hip
// only, and the other units reach these kernels through its host functions (lmm_ctx.hpp: launch_elem_usage,
// CtlPoll).
#pragma once
#include "../../include/lmm/lmm_hip.h"
#include "lmm_cert.hpp"
#include "lmm_dev.hpp"

namespace lmmdev {

// Per-element usage w / penalty of every CSC element (maxmin.cpp:531-533's summand), computed at upload
// and whenever the penalties change, so the per-solve init streams it instead of gathering pen[v].
// Per CSC element: usage w / penalty and the penalty (with every penalty change), and — rows = 1, with every
// structure change — its variable's CSR row.
__global__ void __launch_bounds__(kBlock) mm_elem_usage(Dev s, int rows) {
  for (int64_t j = int64_t(blockIdx.x) * kBlock + threadIdx.x; j < s.nnz; j += int64_t(gridDim.x) * kBlock) {
    const int32_t v = s.csc_v[j];
    const double p = s.pen[v];
    s.csc_u[j] = s.csc_w[j] / p;
    s.csc_p[j] = p;
    if (rows)
      s.csc_row[j] = (unsigned long long)s.var_ptr[v] | ((unsigned long long)s.var_ptr[v + 1] << 32);
  }
}

// cdup (zeroed before): constraints holding two elements of one variable; every constraint of a row longer
// than 64 elements is flagged without the pairwise test.
__global__ void __launch_bounds__(kBlock) mm_dup_check(Dev s) {
  for (int64_t v = int64_t(blockIdx.x) * kBlock + threadIdx.x; v < s.nV; v += int64_t(gridDim.x) * kBlock) {
    const uint32_t b = s.var_ptr[v], e = s.var_ptr[v + 1];
    if (e - b > 64) {
      for (uint32_t i = b; i < e; i++)
        s.cdup[s.csr_c[i]] = 1;
      continue;
    }
    if (e - b <= 16) {  // the row in registers, its loads in flight together
      int32_t cc[16];
#pragma unroll
      for (int i = 0; i < 16; i++)
        cc[i] = b + i < e ? s.csr_c[b + i] : -1 - i;
#pragma unroll
      for (int i = 0; i < 16; i++)
#pragma unroll
        for (int j = i + 1; j < 16; j++)
          if (cc[i] >= 0 && cc[i] == cc[j])
            s.cdup[cc[i]] = 1;
      continue;
    }
    for (uint32_t i = b; i < e; i++)
      for (uint32_t j = i + 1; j < e; j++)
        if (s.csr_c[i] == s.csr_c[j])
          s.cdup[s.csr_c[i]] = 1;
  }
}

// The control words into a pinned host slot, written by the GPU itself (mapped memory, system-scope release):
// a copy-engine transfer on the stream cost a 20-40 us gap before the next kernel at every poll (~1 ms per C2
// solve in the rocprofv3 trace).
__global__ void mm_ctl_out(Dev s, int32_t* dst) {
  const int i = threadIdx.x;
  if (i < CTL_WORDS)
    __hip_atomic_store(dst + i, s.ctl[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
}

// U_c = Constraint::get_usage() of constraint c from the solved values (maxmin.cpp:948-961: sum, or max for
// FATPIPE, of w * x over the enabled elements of weight > 0 — exactly the flattened CSC of c), by one whole wave
// (every lane calls it with the same c): lane l takes the elements l, l + 64, ... of the segment in order, then the
// butterfly of wave_sum / wave_max, so every lane returns the same U_c.  A fixed function of the segment and x: no
// atomics, nothing of the grid.  Reads x, csc_w, csc_v, cnst_ptr and cflags only, which every engine of either
// solver leaves valid.  Both the saturated set and the usage the caller reads come from here.
__device__ __forceinline__ double cnst_usage_wave(const Dev& s, int64_t c, int lane) {
  const bool fat = s.cflags[c] & 1;
  double u = 0.0;
  for (uint32_t j = s.cnst_ptr[c] + lane; j < s.cnst_ptr[c + 1]; j += kWave) {
    const double t = s.csc_w[j] * s.x[s.csc_v[j]];
    u = fat ? fmax(u, t) : u + t;
  }
  return fat ? wave_max(u) : wave_sum(u);
}

// Saturated set of the solved system: sat(c) = NOT double_positive(bound - U_c,
// bound * prec) with U_c = cnst_usage_wave.  One wave per constraint.  FairBottleneck: sat(c) = c was erased
// (fair_bottleneck.cpp:129-140, ratio = +inf).
__global__ void __launch_bounds__(kBlock) mm_saturated(Dev s, double prec, int fair, uint8_t* out) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t c = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave; c < s.nC;
       c += int64_t(gridDim.x) * (kBlock / kWave)) {
    if (fair) {
      if (lane == 0)
        out[c] = s.ratio[c] != 0.0;
      continue;
    }
    const double u = cnst_usage_wave(s, c, lane);
    if (lane == 0) {
      const double b = s.cbound[c];
      out[c] = !((b - u) > b * prec);
    }
  }
}

// Usage of every constraint of the solved system, dense order: out[c] = U_c (cnst_usage_wave), 0 for a constraint
// without an element.  One wave per constraint; either solver kind.
__global__ void __launch_bounds__(kBlock) mm_usage(Dev s, double* out) {
  const int lane = threadIdx.x & (kWave - 1);
  for (int64_t c = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave; c < s.nC;
       c += int64_t(gridDim.x) * (kBlock / kWave)) {
    const double u = cnst_usage_wave(s, c, lane);
    if (lane == 0)
      out[c] = u;
  }
}

// ---- max-min certificate of the solved system (lmmhip_certificate; the rules: lmm_cert.hpp) ----
// Both passes read the flattened system as HBM holds it now — x, pen, vbound, cbound, cflags, the CSR and the CSC —
// and nothing an engine keeps per solve.  Penalties are gathered from pen, not streamed from csc_p: pen is what
// lmmhip_flat_download shows and what every writer of penalties writes first.
//
// Counts and the worst excess leave each workgroup as one CertPart (slot blockIdx.x of `part`); cert_fold adds them
// up in slot order.  Integer sums and a maximum: the result does not depend on the scheduling, and no atomic is used.
using CertPart = lmmhip_cert;  // (the ABI's struct: the worst excess and five counts)
static_assert(lmmcert::kWitAtBound == LMMHIP_WIT_AT_BOUND && lmmcert::kWitNone == LMMHIP_WIT_NONE &&
                  lmmcert::kWitNotJudged == LMMHIP_WIT_NOT_JUDGED,
              "the witness codes of lmm_cert.hpp are the ABI's");

// excess may be NaN (a value of +inf): std::max(worst, NaN) keeps worst on the host, as fmax does here
__device__ __forceinline__ void cert_part_add(CertPart& a, const CertPart& b) {
  a.max_excess = fmax(a.max_excess, b.max_excess);
  a.n_infeasible += b.n_infeasible;
  a.n_unbottlenecked += b.n_unbottlenecked;
  a.n_judged_cnst += b.n_judged_cnst;
  a.n_judged_var += b.n_judged_var;
  a.n_at_bound += b.n_at_bound;
}
__device__ __forceinline__ CertPart cert_part_zero() { return CertPart{lmmcert::kNoExcess, 0, 0, 0, 0, 0}; }

// One lane per wave holds the wave's sums (`mine` says which; the other lanes pass zeros): the workgroup's CertPart.
__device__ __forceinline__ void cert_part_out(const CertPart& p, bool mine, CertPart* part) {
  __shared__ CertPart wp[kBlock / kWave];
  if (mine)
    wp[threadIdx.x / kWave] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    CertPart t = wp[0];
    for (int w = 1; w < kBlock / kWave; w++)
      cert_part_add(t, wp[w]);
    part[blockIdx.x] = t;
  }
}

// Constraint half, one wave per constraint c: U_c = cnst_usage_wave (the bytes of lmmhip_get_usage), top_c = the
// largest level x * pen over the segment (0 for an empty one).  sattop[c] = top_c when c is judged and saturated,
// else +inf, which no level carries: cert_var then asks one array whether an element's constraint can be a witness.
__global__ void __launch_bounds__(kBlock) cert_cnst(Dev s, double prec, double* sattop, CertPart* part) {
  const int lane = threadIdx.x & (kWave - 1);
  CertPart p = cert_part_zero();
  for (int64_t c = (int64_t(blockIdx.x) * kBlock + threadIdx.x) / kWave; c < s.nC;
       c += int64_t(gridDim.x) * (kBlock / kWave)) {
    const double u = cnst_usage_wave(s, c, lane);
    double top = 0.0;
    for (uint32_t j = s.cnst_ptr[c] + lane; j < s.cnst_ptr[c + 1]; j += kWave) {
      const int32_t v = s.csc_v[j];
      top = fmax(top, s.x[v] * s.pen[v]);
    }
    top = wave_max(top);
    if (lane == 0) {
      const double b = s.cbound[c];
      const bool jd = lmmcert::judged(b, prec);
      sattop[c] = jd && lmmcert::saturated(u, b, prec) ? top : dinf();
      if (jd) {
        p.n_judged_cnst++;
        p.n_infeasible += lmmcert::infeasible(u, b, prec);
        p.max_excess = fmax(p.max_excess, lmmcert::excess(u, b));
      }
    }
  }
  cert_part_out(p, lane == 0, part);
}

// Variable half, over the CSR rows: the witness of variable v is, in this order, kWitNotJudged (penalty or value not
// positive), kWitAtBound, the constraint of the first element in row order that carries v's level (sattop), or
// kWitNone.  A lane takes a row; one of at most kCertLaneRow elements it scans itself, from the last element to the
// first with every load in flight, so the first carrier wins.  The wave then takes the longer rows of its lanes one at
// a time, 64 elements per step, and stops at the first step with a carrier: the lowest such lane is the first in row
// order.  witness may be null (counts only).
constexpr uint32_t kCertLaneRow = 8;
__global__ void __launch_bounds__(kBlock) cert_var(Dev s, double prec, const double* __restrict__ sattop,
                                                   int32_t* witness, CertPart* part) {
  const int lane = threadIdx.x & (kWave - 1);
  int64_t njudged = 0, nbound = 0, nnone = 0;
  // (the trip count is the workgroup's: every lane of a wave reaches the ballots)
  for (int64_t v0 = int64_t(blockIdx.x) * kBlock; v0 < s.nV; v0 += int64_t(gridDim.x) * kBlock) {
    const int64_t v = v0 + threadIdx.x;
    const bool in = v < s.nV;
    int32_t wit = lmmcert::kWitNotJudged;
    uint32_t b = 0, e = 0;
    double level = 0.0;
    bool search = false;
    if (in) {
      const double x = s.x[v], pen = s.pen[v];
      if (pen > 0 && x > 0) {
        if (lmmcert::at_bound(x, s.vbound[v], prec)) {
          wit = lmmcert::kWitAtBound;
        } else {
          wit = lmmcert::kWitNone;
          search = true;
          level = x * pen;
          b = s.var_ptr[v];
          e = s.var_ptr[v + 1];
        }
      }
    }
    if (search && e - b <= kCertLaneRow) {
      int32_t cc[kCertLaneRow];
      double tt[kCertLaneRow];
#pragma unroll
      for (uint32_t i = 0; i < kCertLaneRow; i++)
        cc[i] = b + i < e ? s.csr_c[b + i] : -1;
#pragma unroll
      for (uint32_t i = 0; i < kCertLaneRow; i++)
        tt[i] = cc[i] >= 0 ? sattop[cc[i]] : dinf();
#pragma unroll
      for (int i = int(kCertLaneRow) - 1; i >= 0; i--)
        if (cc[i] >= 0 && lmmcert::carries(level, tt[i]))
          wit = cc[i];
      search = false;
    }
    for (unsigned long long todo = __ballot(search); todo; todo &= todo - 1) {
      const int l = __ffsll((long long)todo) - 1;
      const uint32_t rb = __shfl(b, l, kWave), re = __shfl(e, l, kWave);
      const double lv = __shfl(level, l, kWave);
      int32_t w = lmmcert::kWitNone;
      for (uint32_t i0 = rb; i0 < re; i0 += kWave) {
        const uint32_t i = i0 + lane;
        const int32_t c = i < re ? s.csr_c[i] : -1;
        const unsigned long long hit = __ballot(c >= 0 && lmmcert::carries(lv, sattop[c >= 0 ? c : 0]));
        if (hit) {
          w = __shfl(c, __ffsll((long long)hit) - 1, kWave);
          break;
        }
      }
      if (lane == l)
        wit = w;
    }
    if (in) {
      if (witness)
        witness[v] = wit;
      njudged += wit != lmmcert::kWitNotJudged;
      nbound += wit == lmmcert::kWitAtBound;
      nnone += wit == lmmcert::kWitNone;
    }
  }
  // the lanes' counts into lane 0 of each wave (integer sums: any order)
  CertPart p = cert_part_zero();
  p.n_judged_var = njudged;
  p.n_at_bound = nbound;
  p.n_unbottlenecked = nnone;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    p.n_judged_var += __shfl_xor(p.n_judged_var, o, kWave);
    p.n_at_bound += __shfl_xor(p.n_at_bound, o, kWave);
    p.n_unbottlenecked += __shfl_xor(p.n_unbottlenecked, o, kWave);
  }
  cert_part_out(p, lane == 0, part);
}

// The workgroups' parts (nc of cert_cnst, then nv of cert_var; nv = 0: the feasibility half alone) into the ABI's
// struct, by one workgroup: thread t folds the slots t, t + kBlock, ..., then the threads' sums are folded in thread
// order.
__global__ void __launch_bounds__(kBlock) cert_fold(const CertPart* part, int nc, int nv, CertPart* out) {
  __shared__ CertPart tp[kBlock];
  CertPart p = cert_part_zero();
  for (int i = threadIdx.x; i < nc + nv; i += kBlock)
    cert_part_add(p, part[i]);
  tp[threadIdx.x] = p;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int t = 1; t < kBlock; t++)
      cert_part_add(p, tp[t]);
    if (nv == 0)
      p.n_unbottlenecked = -1;
    *out = p;
  }
}

// Constraints of the solved system in the caller's id space (resident flatten): listed constraint i with a member
// element (lany) has the dense index dcl[i] (exclusive scan of lany) and the host slot list[i].
__global__ void __launch_bounds__(kBlock) rs_touched_cnsts(int64_t nl, const int32_t* __restrict__ list,
                                                           const int64_t* __restrict__ lany,
                                                           const int64_t* __restrict__ dcl, int32_t* out) {
  for (int64_t i = int64_t(blockIdx.x) * kBlock + threadIdx.x; i < nl; i += int64_t(gridDim.x) * kBlock)
    if (lany[i])
      out[dcl[i]] = list[i];
}

// Variables of the solved system in the caller's id space: dense index d -> host slot (resident
// flatten: dv = exclusive scan of the membership mask vm), written at out[d] (ascending slots).
__global__ void __launch_bounds__(kBlock) rs_touched(int64_t nslots, const int64_t* vm, const int64_t* dv,
                                                     int32_t* out) {
  for (int64_t v = int64_t(blockIdx.x) * kBlock + threadIdx.x; v < nslots; v += int64_t(gridDim.x) * kBlock)
    if (vm[v])
      out[dv[v]] = int32_t(v);
}

}  // namespace lmmdev
