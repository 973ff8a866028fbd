// lmm_common_kernels.hpp — the small kernels that more than one part of the driver needs (upload, resident
// refresh, the termination polls of the max-min and FairBottleneck engines, the getters).
//
// Every __global__ kernel is compiled in exactly one translation unit: this header is included by lmm_hip.hip
// only, and the other units reach these kernels through its host functions (lmm_ctx.hpp: launch_elem_usage,
// CtlPoll).
#pragma once
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
