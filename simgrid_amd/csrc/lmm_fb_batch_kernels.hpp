// lmm_fb_batch_kernels.hpp — many small independent FairBottleneck systems, one workgroup per system, the whole
// system in LDS: the FairBottleneck twin of mm_batch_lds (lmm_batch_kernels.hpp), included by lmm_hip_fair.hip.
//
// The uploaded system is a disjoint union declared block-diagonal by lmmhip_set_batch.  A workgroup stages one
// system's structure in LDS (16-bit local indices) and runs the three Jacobi phases of a reference round
// (fair_bottleneck.cpp:59-145) exactly as the chunked engine does (lmm_fb_kernels.hpp), with every round inside
// the workgroup — no launch per phase, no host pacing, and every system stops after its own rounds:
//   S  thread per listed constraint: nb = its listed variables (FATPIPE: 1); nb == 0 erases it, else
//      usage = remaining / nb                                                  (fbk_count / fbk_nb / fbk_share)
//   I  thread per listed variable: mu = min over its row of usage / w, capped by bound - value; value += mu;
//      exact value == bound delists it; a delisted variable keeps its last mu  (fb_var_inc)
//   U  thread per listed constraint: shared — remaining -= w * mu one element at a time in the CSC order of the
//      upload, clamped below the precision after every step (the reference's own chain, two roundings per
//      element); FATPIPE — fb_fat_update's minimum; remaining <= 0 erases the constraint and delists its
//      variables                                                               (fbk_update_seq / fbk_unlist)
// Termination is the chunked engine's: a round runs while the previous round's phase I left a variable listed
// (round 0: while the system has a variable), so a system whose last variables were delisted by an erasure runs
// one more round, in which its remaining listed constraints find nb == 0.  Values, rounds, remaining, usage, the
// saturated set and the work counters of every system are therefore those of that system solved ALONE by the
// chunked engine.  The chunked engine on the union gives the same values and the same round count (the maximum
// over the systems), but it erases the left-over constraints of a finished system only when a later round of
// the union counts them (nb == 0), and counts them once more in its work counters: an artefact of sharing
// rounds that this engine does not reproduce.
// No workgroup waits for another, and every loop is bounded: a system still listed after max_rounds rounds
// stops its workgroup and reports the round guard (block_rounds = -1 -> mm_batch_rounds -> CTL_ERR = 2).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define LMM_FBB_HD __host__ __device__
#else
#define LMM_FBB_HD
#endif

namespace lmmdev {

// LDS bytes of a workgroup for systems of at most nv variables, nc constraints and nnz elements, the weights
// left in HBM (csr_w / csc_w); fb_batch_lds_weights more keep both copies of the weights in LDS too.
LMM_FBB_HD inline size_t fb_batch_lds_bytes(int nv, int nc, int nnz) {
  size_t b = sizeof(double) * (2 * size_t(nc) + 3 * size_t(nv)) +  // rem, use; x, mu, vbound
             sizeof(int32_t) * size_t(nv) +                        // last listed round
             sizeof(uint16_t) * (size_t(nv) + 1 + size_t(nc) + 1 + 2 * size_t(nnz)) +
             2 * size_t(nc) + size_t(nv);  // constraint state, flags; listed
  return (b + 15) / 16 * 16;
}
LMM_FBB_HD inline size_t fb_batch_lds_weights(int nnz) { return 2 * sizeof(double) * size_t(nnz); }

}  // namespace lmmdev

#if defined(__HIPCC__)
#include "lmm_dev.hpp"

namespace lmmdev {

constexpr int kFBB = 256;  // threads per workgroup

// WL: the weights staged in LDS (behind the per-variable doubles), else read from csr_w / csc_w.
template <bool WL>
__global__ void __launch_bounds__(kFBB, 6)
    fbk_batch_lds(FbDev s, const int64_t* __restrict__ var_off, const int64_t* __restrict__ cnst_off, int64_t nsys,
                  double prec, int max_nv, int max_nc, int max_nnz, int max_rounds, int32_t* block_rounds) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  double* c_rem = reinterpret_cast<double*>(lds);
  double* c_use = c_rem + max_nc;
  double* v_x = c_use + max_nc;
  double* v_mu = v_x + max_nv;
  double* v_vb = v_mu + max_nv;
  double* w_csr = v_vb + max_nv;                   // [max_nnz] (WL)
  double* w_csc = w_csr + (WL ? max_nnz : 0);      // [max_nnz] (WL)
  int32_t* v_fixr = reinterpret_cast<int32_t*>(w_csc + (WL ? max_nnz : 0));
  uint16_t* l_vp = reinterpret_cast<uint16_t*>(v_fixr + max_nv);  // [max_nv + 1] CSR offsets
  uint16_t* l_cp = l_vp + (max_nv + 1);                            // [max_nc + 1] CSC offsets
  uint16_t* l_cc = l_cp + (max_nc + 1);                            // [max_nnz] CSR local constraint
  uint16_t* l_cv = l_cc + max_nnz;                                 // [max_nnz] CSC local variable
  uint8_t* c_st = reinterpret_cast<uint8_t*>(l_cv + max_nnz);      // 0 listed, 1 erased
  uint8_t* c_fl = c_st + max_nc;                                   // cflags: bit0 FATPIPE, bit1 zero-weight element
  uint8_t* v_ls = c_fl + max_nc;                                   // 1 listed
  __shared__ unsigned long long wsum[3][kFBB / kWave];
  unsigned long long w_ne = 0, w_nv = 0, w_nc = 0;  // lmmhip_fb_work's counters, this thread's share
  int rounds_max = 0;
  for (int64_t sy = blockIdx.x; sy < nsys; sy += gridDim.x) {
    const int64_t vb = var_off[sy], cb = cnst_off[sy];
    const int nv = int(var_off[sy + 1] - vb), nc = int(cnst_off[sy + 1] - cb);
    const uint32_t eb = s.var_ptr[vb], kb = s.cnst_ptr[cb];
    const int ne = int(s.var_ptr[vb + nv] - eb);
    // ---- stage the system; init (fb_init) ----
    for (int i = threadIdx.x; i <= nv; i += kFBB)
      l_vp[i] = uint16_t(s.var_ptr[vb + i] - eb);
    for (int i = threadIdx.x; i <= nc; i += kFBB)
      l_cp[i] = uint16_t(s.cnst_ptr[cb + i] - kb);
    for (int j = threadIdx.x; j < ne; j += kFBB) {
      l_cc[j] = uint16_t(s.csr_c[eb + j] - cb);
      l_cv[j] = uint16_t(s.csc_v[kb + j] - vb);
      if (WL) {
        w_csr[j] = s.csr_w[eb + j];
        w_csc[j] = s.csc_w[kb + j];
      }
    }
    for (int v = threadIdx.x; v < nv; v += kFBB) {
      v_x[v] = 0.0;
      v_mu[v] = 0.0;
      v_vb[v] = s.vbound[vb + v];
      v_fixr[v] = -1;
      v_ls[v] = 1;
    }
    for (int c = threadIdx.x; c < nc; c += kFBB) {
      c_rem[c] = s.cbound[cb + c];
      c_use[c] = 0.0;
      c_st[c] = 0;
      c_fl[c] = s.cflags[cb + c];
    }
    __syncthreads();
    const double* __restrict__ wr = WL ? w_csr : s.csr_w + eb;
    const double* __restrict__ wc = WL ? w_csc : s.csc_w + kb;
    int round = 0;
    int any = nv > 0;
    while (any) {  // workgroup-uniform
      if (round >= max_rounds) {  // guard: report it and stop this workgroup
        if (threadIdx.x == 0)
          block_rounds[blockIdx.x] = -1;
        return;
      }
      // ---- S: shares (fair_bottleneck.cpp:65-87) ----
      for (int c = threadIdx.x; c < nc; c += kFBB) {
        if (c_st[c])
          continue;
        const int b = l_cp[c], e = l_cp[c + 1];
        w_ne += unsigned(e - b);
        w_nc += 1;
        int nb = 0;
        for (int k = b; k < e; k++)
          nb += v_ls[l_cv[k]];
        if (nb > 0 && (c_fl[c] & 1))
          nb = 1;
        if (nb == 0) {
          c_rem[c] = 0.0;
          c_use[c] = 0.0;
          c_st[c] = 1;
        } else {
          c_use[c] = c_rem[c] / nb;
        }
      }
      __syncthreads();
      // ---- I: increments (:89-105) ----
      int left = 0;
      for (int v = threadIdx.x; v < nv; v += kFBB) {
        if (!v_ls[v])
          continue;
        w_nv += 1;
        double inc = DBL_MAX;
        for (int j = l_vp[v], je = l_vp[v + 1]; j < je; j++)
          inc = fmin(inc, c_use[l_cc[j]] / wr[j] + 0.0);
        const double bd = v_vb[v];
        double x = v_x[v];
        if (bd > 0)
          inc = fmin(inc, bd - x);
        v_mu[v] = inc;
        x += inc;
        v_x[v] = x;
        v_fixr[v] = round;
        if (x == bd)
          v_ls[v] = 0;
        else
          left = 1;
      }
      any = __syncthreads_or(left);
      // ---- U: remaining, erasure, delisting (:107-140) ----
      for (int c = threadIdx.x; c < nc; c += kFBB) {
        if (c_st[c])
          continue;
        const int b = l_cp[c], e = l_cp[c + 1];
        double rem = c_rem[c];
        if (c_fl[c] & 1) {  // fb_fat_update
          double mn = dinf();
          for (int k = b; k < e; k++)
            mn = fmin(mn, wc[k] * v_mu[l_cv[k]]);
          double u = c_use[c];
          if (c_fl[c] & 2)
            u = fmin(u, 0.0);
          u = fmin(u, mn);
          c_use[c] = u;
          rem -= u;
          if (rem < prec)
            rem = 0.0;
        } else {
          for (int k = b; k < e; k++) {
            const double d = wc[k] * v_mu[l_cv[k]];
            rem -= d;
            if (rem < prec)
              rem = 0.0;
          }
        }
        c_rem[c] = rem;
        if (rem <= 0.0) {
          c_st[c] = 1;
          for (int k = b; k < e; k++)
            v_ls[l_cv[k]] = 0;
        }
      }
      __syncthreads();
      round++;
    }
    rounds_max = round > rounds_max ? round : rounds_max;
    // ---- results ----
    for (int v = threadIdx.x; v < nv; v += kFBB) {
      s.x[vb + v] = v_x[v];
      s.fixr[vb + v] = v_fixr[v];
    }
    for (int c = threadIdx.x; c < nc; c += kFBB) {
      s.rem[cb + c] = c_rem[c];
      s.use[cb + c] = c_use[c];
      s.ratio[cb + c] = c_st[c] ? dinf() : 0.0;  // 0 = still listed, +inf = erased (mm_saturated)
    }
    __syncthreads();  // the next system restages the LDS
  }
  // work counters: one sum and one atomic each per workgroup, spread over the slots (lmmhip_fb_work sums them)
  unsigned long long w3[3] = {w_ne, w_nv, w_nc};
#pragma unroll
  for (int k = 0; k < 3; k++) {
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1)
      w3[k] += __shfl_xor(w3[k], o, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0)
      wsum[k][threadIdx.x / kWave] = w3[k];
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    unsigned long long t = 0;
    for (int i = 0; i < kFBB / kWave; i++)
      t += wsum[threadIdx.x][i];
    if (t)
      atomicAdd(reinterpret_cast<unsigned long long*>(s.ctl + CTL_FBW_AT) + threadIdx.x * kFbwSlots +
                    (blockIdx.x & (kFbwSlots - 1)),
                t);
  }
  if (threadIdx.x == 0)
    block_rounds[blockIdx.x] = rounds_max;
}

}  // namespace lmmdev
#endif  // __HIPCC__
