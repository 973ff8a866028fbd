// lmm_hip_step.hip — the model side of a simulation step: lmmhip_actions_*, lmmhip_next_event_*,
// lmmhip_update_actions_full (lmm_step_kernels.hpp).
#include <cmath>
#include <cstring>

#include "lmm_ctx.hpp"
#include "lmm_step_kernels.hpp"

template <class T> static int act_alloc(lmmhip_ctx* c, T** out, int64_t n, const T* src) {
  return c->act_allocs.alloc(out, n, src, c->stream);
}

int lmmhip_actions_upload(lmmhip_ctx* c, int64_t n, const int32_t* var_index, const double* remains,
                          const double* max_duration, const double* latency, const double* penalty,
                          const double* sharing_penalty, const uint8_t* flags) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (n < 0 || (n > 0 && (!var_index || !remains || !max_duration || !latency || !penalty || !sharing_penalty ||
                          !flags)))
    return fail(LMMHIP_E_ARG, "null action arrays");
  const int64_t nV = c->uploaded ? c->d.nV : 0;
  for (int64_t i = 0; i < n; i++)
    if (var_index[i] < -1 || var_index[i] >= nV)
      return fail(LMMHIP_E_ARG, "action var_index out of range of the uploaded system");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamSynchronize(c->stream));
  c->act_allocs.clear();
  c->act_slot = nullptr;  // a new table is unbound
  ActDev& a = c->act;
  a = ActDev{};
  a.n = n;
  int rc = 0;
  rc |= act_alloc(c, &a.vidx, n, var_index);
  rc |= act_alloc(c, &a.remains, n, remains);
  rc |= act_alloc(c, &a.max_duration, n, max_duration);
  rc |= act_alloc(c, &a.latency, n, latency);
  rc |= act_alloc(c, &a.penalty, n, penalty);
  rc |= act_alloc(c, &a.share_pen, n, sharing_penalty);
  rc |= act_alloc(c, &a.flags, n, flags);
  rc |= act_alloc<uint8_t>(c, &a.events, n, nullptr);
  rc |= act_alloc<unsigned long long>(c, &a.umin, 1, nullptr);
  rc |= act_alloc<int32_t>(c, &a.nev, 1, nullptr);
  if (rc)
    return rc;
  HIPCHK(hipMemsetAsync(a.events, 0, size_t(n > 0 ? n : 1), c->stream));  // no event before the first update
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

// ---- bound table ----
static ActBind bind_of(const lmmhip_ctx* c) {
  if (!c->uploaded)
    return ActBind{BIND_NONE, 0, nullptr, nullptr};
  if (!c->res_flat)
    return ActBind{BIND_DENSE, c->d.nV, nullptr, nullptr};
  return ActBind{BIND_RESIDENT, c->res_flat_nv, static_cast<const int64_t*>(c->rs_vm.p),
                 static_cast<const int64_t*>(c->rs_dv.p)};
}

// Queues act_rebind when an upload or a flatten happened since the bound table's vidx was written.
static int act_sync_bind(lmmhip_ctx* c) {
  if (!c->act_slot || c->act_gen == c->sys_gen)
    return 0;
  if (c->act.n > 0)
    LAUNCH(7, -1, act_rebind, grid_for(c->act.n, kBlock), kBlock, c->act.n, c->act_slot, bind_of(c), c->act.vidx);
  c->act_gen = c->sys_gen;
  return 0;
}

int lmmhip_actions_bind(lmmhip_ctx* c, int64_t n, const int32_t* var_slot) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (!c->act.nev)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_upload first");
  if (n != c->act.n || (n > 0 && !var_slot))
    return fail(LMMHIP_E_ARG, "bind: one variable id per action of the uploaded table");
  for (int64_t i = 0; i < n; i++)
    if (var_slot[i] < -1)
      return fail(LMMHIP_E_ARG, "bind: variable id below -1");
  HIPCHK(hipSetDevice(c->device));
  if (!c->act_slot)
    if (int rc = act_alloc<int32_t>(c, &c->act_slot, n, nullptr))
      return rc;
  if (n > 0)
    HIPCHK(hipMemcpyAsync(c->act_slot, var_slot, size_t(n) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
  c->act_gen = 0;  // (sys_gen starts at 1: the next entry point rebinds)
  if (int rc = act_sync_bind(c))
    return rc;
  HIPCHK(hipStreamSynchronize(c->stream));  // var_slot is borrowed for the call only
  return 0;
}

int lmmhip_actions_var_index(lmmhip_ctx* c, int32_t* out) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (!c->act.nev)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_upload first");
  if (c->act.n > 0 && !out)
    return fail(LMMHIP_E_ARG, "null output");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = act_sync_bind(c))
    return rc;
  if (c->act.n > 0)
    HIPCHK(hipMemcpyAsync(out, c->act.vidx, size_t(c->act.n) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_actions_patch(lmmhip_ctx* c, int64_t k, const int32_t* idx, int fields, const int32_t* var_slot,
                         const double* remains, const double* max_duration, const double* latency,
                         const double* penalty, const double* sharing_penalty, const uint8_t* flags,
                         const double* last_update, const double* last_value, const double* start_time,
                         const double* date, const uint8_t* heap_type) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (!c->act.nev)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_upload first");
  const int64_t n = c->act.n;
  if (k < 0 || (k > 0 && !idx) || (fields & ~PF_ALL))
    return fail(LMMHIP_E_ARG, "patch: bad index list or unknown field bit");
  if ((fields & PF_LAZY) && !c->act.htype)
    return fail(LMMHIP_E_ARG, "patch: a lazy field before lmmhip_actions_lazy_upload");
  if ((fields & PF_VAR_SLOT) && !c->act_slot)
    return fail(LMMHIP_E_STATE, "patch: a variable id on an unbound table (lmmhip_actions_bind first)");
  const double* dsrc[9] = {remains, max_duration, latency,    penalty, sharing_penalty,
                           last_update, last_value, start_time, date};
  static const int dbit[9] = {PF_REMAINS,     PF_MAX_DURATION, PF_LATENCY,    PF_PENALTY, PF_SHARE_PEN,
                              PF_LAST_UPDATE, PF_LAST_VALUE,   PF_START_TIME, PF_DATE};
  if (k > 0) {
    bool null_field = ((fields & PF_VAR_SLOT) && !var_slot) || ((fields & PF_FLAGS) && !flags) ||
                      ((fields & PF_HEAP_TYPE) && !heap_type);
    for (int f = 0; f < 9; f++)
      null_field |= (fields & dbit[f]) && !dsrc[f];
    if (null_field)
      return fail(LMMHIP_E_ARG, "patch: null array of a named field");
  }
  // the patch in ascending action order (act_patch), each action once
  std::vector<int64_t> ord(static_cast<size_t>(k));
  for (int64_t j = 0; j < k; j++) {
    if (idx[j] < 0 || idx[j] >= n)
      return fail(LMMHIP_E_ARG, "patch: action index out of range");
    if ((fields & PF_VAR_SLOT) && var_slot[j] < -1)
      return fail(LMMHIP_E_ARG, "patch: variable id below -1");
    if ((fields & PF_HEAP_TYPE) && heap_type[j] > HEAP_NORMAL)
      return fail(LMMHIP_E_ARG, "unknown heap type");
    ord[size_t(j)] = j;
  }
  std::sort(ord.begin(), ord.end(), [&](int64_t x, int64_t y) { return idx[x] < idx[y]; });
  for (int64_t j = 1; j < k; j++)
    if (idx[ord[size_t(j)]] == idx[ord[size_t(j - 1)]])
      return fail(LMMHIP_E_ARG, "patch: duplicate action index");
  if (k == 0 || fields == 0)
    return 0;
  HIPCHK(hipSetDevice(c->device));
  if (int rc = act_sync_bind(c))  // (before the patch: a rebind after it would be the same, this keeps one order)
    return rc;
  // one staging buffer, SoA: 9 double arrays, 2 int32 arrays, 2 byte arrays of K = k rounded up to 8 entries
  const size_t K = (size_t(k) + 7) & ~size_t(7), bytes = K * (9 * 8 + 2 * 4 + 2);
  std::vector<unsigned char> h(bytes);
  double* hd = reinterpret_cast<double*>(h.data());
  int32_t* hi = reinterpret_cast<int32_t*>(h.data() + K * 72);
  uint8_t* hb = h.data() + K * 80;
  for (int64_t j = 0; j < k; j++) {
    const size_t s = size_t(ord[size_t(j)]);
    for (int f = 0; f < 9; f++)
      hd[size_t(f) * K + size_t(j)] = (fields & dbit[f]) ? dsrc[f][s] : 0.0;
    hi[j] = idx[s];
    hi[K + size_t(j)] = (fields & PF_VAR_SLOT) ? var_slot[s] : -1;
    hb[j] = (fields & PF_FLAGS) ? flags[s] : 0;
    hb[K + size_t(j)] = (fields & PF_HEAP_TYPE) ? heap_type[s] : 0;
  }
  unsigned char* dbuf = nullptr;
  if (int rc = scratch(c, c->act_stage, int64_t(bytes), &dbuf))
    return rc;
  HIPCHK(hipMemcpyAsync(dbuf, h.data(), bytes, hipMemcpyHostToDevice, c->stream));
  const double* dd = reinterpret_cast<const double*>(dbuf);
  const int32_t* di = reinterpret_cast<const int32_t*>(dbuf + K * 72);
  const uint8_t* db = dbuf + K * 80;
  const PatchSrc src{di,         di + K,     dd,         dd + K,     dd + 2 * K, dd + 3 * K, dd + 4 * K,
                     dd + 5 * K, dd + 6 * K, dd + 7 * K, dd + 8 * K, db,         db + K};
  LAUNCH(7, -1, act_patch, grid_for(k, kBlock), kBlock, c->act, c->act_slot, bind_of(c), k, fields, src);
  HIPCHK(hipStreamSynchronize(c->stream));  // the staging vector dies at return
  return 0;
}

int lmmhip_actions_events(lmmhip_ctx* c, int32_t* ids, uint8_t* events, int64_t cap, int64_t* n_out) {
  if (!c || !n_out)
    return fail(LMMHIP_E_ARG, "null argument");
  if (!c->act.nev)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_upload first");
  HIPCHK(hipSetDevice(c->device));
  const int64_t n = c->act.n;
  unsigned long long* out = nullptr;
  if (int rc = scratch(c, c->act_evout, n + 1, &out))  // word n: the count
    return rc;
  int32_t* cnt = reinterpret_cast<int32_t*>(out + n);
  int32_t h = 0;
  HIPCHK(hipMemsetAsync(cnt, 0, sizeof(int32_t), c->stream));
  if (n > 0)
    LAUNCH(7, -1, act_events, grid_for(n, kBlock), kBlock, c->act, out, cnt);
  HIPCHK(hipMemcpyAsync(&h, cnt, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *n_out = h;
  if (!ids && !events)
    return 0;  // size query
  if (h > cap || (h && (!ids || !events)))
    return fail(LMMHIP_E_ARG, "events: output capacity below the number of actions with an event");
  if (h) {
    std::vector<unsigned long long> v(static_cast<size_t>(h));
    HIPCHK(hipMemcpyAsync(v.data(), out, size_t(h) * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::sort(v.begin(), v.end());  // ascending action index (as lmmhip_actions_lazy_due orders `due`)
    for (int32_t j = 0; j < h; j++) {
      ids[j] = int32_t(v[size_t(j)] >> 8);
      events[j] = uint8_t(v[size_t(j)] & 0xFF);
    }
  }
  return 0;
}

int lmmhip_next_event_full(lmmhip_ctx* c, int with_latency, double* out) {
  if (!c || !out)
    return fail(LMMHIP_E_ARG, "null argument");
  if (!c->act.umin)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_upload first");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = act_sync_bind(c))
    return rc;
  unsigned long long h = ~0ull;
  HIPCHK(hipMemsetAsync(c->act.umin, 0xFF, sizeof(unsigned long long), c->stream));
  if (c->act.n > 0)
    LAUNCH(7, -1, act_next_event, grid_for(c->act.n, kBlock), kBlock, c->act, c->d.x, with_latency);
  HIPCHK(hipMemcpyAsync(&h, c->act.umin, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (h == ~0ull) {
    *out = -1.0;
  } else {
    double m;
    std::memcpy(&m, &h, sizeof(m));
    *out = m;
  }
  return 0;
}

int lmmhip_update_actions_full(lmmhip_ctx* c, int model, double delta, double maxmin_precision,
                               double surf_precision, int64_t* n_events) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (!c->act.nev)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_upload first");
  if (model != MODEL_CPU && model != MODEL_CM02 && model != MODEL_L07)
    return fail(LMMHIP_E_ARG, "unknown model");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = act_sync_bind(c))
    return rc;
  int32_t h = 0;
  HIPCHK(hipMemsetAsync(c->act.nev, 0, sizeof(int32_t), c->stream));
  if (c->act.n > 0)
    LAUNCH(7, -1, act_update, grid_for(c->act.n, kBlock), kBlock, c->act, c->d.x, model, delta, maxmin_precision,
           surf_precision);
  HIPCHK(hipMemcpyAsync(&h, c->act.nev, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (n_events)
    *n_events = h;
  return 0;
}

int lmmhip_actions_download(lmmhip_ctx* c, double* remains, double* max_duration, double* latency, double* penalty,
                            uint8_t* events) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = size_t(c->act.n);
  if (n) {
    if (remains)
      HIPCHK(hipMemcpyAsync(remains, c->act.remains, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (max_duration)
      HIPCHK(hipMemcpyAsync(max_duration, c->act.max_duration, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (latency)
      HIPCHK(hipMemcpyAsync(latency, c->act.latency, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (penalty)
      HIPCHK(hipMemcpyAsync(penalty, c->act.penalty, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (events)
      HIPCHK(hipMemcpyAsync(events, c->act.events, n, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_actions_lazy_upload(lmmhip_ctx* c, const double* last_update, const double* last_value,
                               const double* start_time, const double* date, const uint8_t* heap_type) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (!c->act.nev)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_upload first");
  const int64_t n = c->act.n;
  if (n > 0 && (!last_update || !last_value || !start_time || !date || !heap_type))
    return fail(LMMHIP_E_ARG, "null lazy action arrays");
  if (n >= (int64_t(1) << 30))
    return fail(LMMHIP_E_ARG, "too many actions for the lazy heap (< 2^30)");
  for (int64_t i = 0; i < n; i++)
    if (heap_type[i] > HEAP_NORMAL)
      return fail(LMMHIP_E_ARG, "unknown heap type");
  HIPCHK(hipSetDevice(c->device));
  ActDev& a = c->act;
  double* st;
  std::vector<double> d(date, date + n);
  for (int64_t i = 0; i < n; i++)
    if (heap_type[i] == HEAP_UNSET)
      d[size_t(i)] = __builtin_huge_val();
  int rc = act_alloc(c, &a.last_update, n, last_update) | act_alloc(c, &a.last_value, n, last_value) |
           act_alloc(c, &st, n, start_time) | act_alloc(c, &a.date, n, d.data()) |
           act_alloc(c, &a.htype, n, heap_type) | act_alloc<int32_t>(c, &a.due, n, nullptr) |
           act_alloc<int32_t>(c, &a.ndue, 1, nullptr) | act_alloc<int32_t>(c, &a.err, 1, nullptr);
  if (rc)
    return rc;
  a.start_time = st;
  HIPCHK(hipMemsetAsync(a.err, 0, sizeof(int32_t), c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_actions_lazy_update(lmmhip_ctx* c, int model, double now, double maxmin_precision, double surf_precision,
                               int64_t n_modified, const int32_t* modified, int64_t* n_finished) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (!c->act.htype)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_lazy_upload first");
  if (model != MODEL_CPU && model != MODEL_CM02)
    return fail(LMMHIP_E_ARG, "lazy update: CPU or CM02 model");
  if (n_modified < 0 || (n_modified && !modified))
    return fail(LMMHIP_E_ARG, "bad modified-action list");
  {  // the modified set holds each action once (its hook): a duplicate would race on the action
    std::vector<uint8_t> seen(size_t(c->act.n), 0);
    for (int64_t j = 0; j < n_modified; j++) {
      if (modified[j] < 0 || modified[j] >= c->act.n)
        return fail(LMMHIP_E_ARG, "modified action out of range");
      if (seen[size_t(modified[j])]++)
        return fail(LMMHIP_E_ARG, "duplicate action in the modified list");
    }
  }
  HIPCHK(hipSetDevice(c->device));
  if (int rc = act_sync_bind(c))
    return rc;
  int32_t h[2] = {0, 0};
  HIPCHK(hipMemsetAsync(c->act.nev, 0, sizeof(int32_t), c->stream));
  if (n_modified) {
    int32_t* dmod = nullptr;
    if (int rc = scratch(c, c->rs_stage[0], n_modified, &dmod))
      return rc;
    HIPCHK(hipMemcpyAsync(dmod, modified, size_t(n_modified) * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    LAUNCH(7, -1, act_lazy_update, grid_for(n_modified, kBlock), kBlock, c->act, c->d.x, model, now,
           maxmin_precision * surf_precision, surf_precision, n_modified, dmod);
  }
  HIPCHK(hipMemcpyAsync(&h[0], c->act.nev, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&h[1], c->act.err, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (h[1])
    return fail(LMMHIP_E_STATE, "next_occuring_event_lazy: an action got no date (DIE_IMPOSSIBLE, Model.cpp:96)");
  if (n_finished)
    *n_finished = h[0];
  return 0;
}

int lmmhip_actions_lazy_update_solved(lmmhip_ctx* c, int model, double now, double maxmin_precision,
                                      double surf_precision, int64_t n_extra, const int32_t* extra,
                                      int64_t* n_modified, int64_t* n_finished) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (!c->act.htype)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_lazy_upload first");
  if (!c->act_slot)
    return fail(LMMHIP_E_STATE, "lazy update of the solved set: lmmhip_actions_bind first");
  if (model != MODEL_CPU && model != MODEL_CM02)
    return fail(LMMHIP_E_ARG, "lazy update: CPU or CM02 model");
  if (n_extra < 0 || (n_extra && !extra))
    return fail(LMMHIP_E_ARG, "bad extra-action list");
  const int64_t n = c->act.n;
  const size_t nb = (size_t(n) + 7) & ~size_t(7);  // the mask's bytes; the modified count sits behind them
  std::vector<uint8_t> mask;
  if (n_extra) {
    mask.assign(nb, 0);
    for (int64_t j = 0; j < n_extra; j++) {
      if (extra[j] < 0 || extra[j] >= n)
        return fail(LMMHIP_E_ARG, "extra action out of range");
      mask[size_t(extra[j])] = 1;  // (listed twice, or in the system too: processed once)
    }
  }
  HIPCHK(hipSetDevice(c->device));
  if (int rc = act_sync_bind(c))
    return rc;
  uint8_t* dmask = nullptr;
  if (int rc = scratch(c, c->act_mask, int64_t(nb) + 8, &dmask))
    return rc;
  int32_t* dnmod = reinterpret_cast<int32_t*>(dmask + nb);
  int32_t h[3] = {0, 0, 0};
  HIPCHK(hipMemsetAsync(c->act.nev, 0, sizeof(int32_t), c->stream));
  HIPCHK(hipMemsetAsync(dnmod, 0, sizeof(int32_t), c->stream));
  if (n_extra)
    HIPCHK(hipMemcpyAsync(dmask, mask.data(), nb, hipMemcpyHostToDevice, c->stream));
  if (n > 0)
    LAUNCH(7, -1, act_lazy_update_solved, grid_for(n, kBlock), kBlock, c->act, c->d.x, model, now,
           maxmin_precision * surf_precision, surf_precision, n_extra ? dmask : nullptr, dnmod);
  HIPCHK(hipMemcpyAsync(&h[0], c->act.nev, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&h[1], c->act.err, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(&h[2], dnmod, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (h[1])
    return fail(LMMHIP_E_STATE, "next_occuring_event_lazy: an action got no date (DIE_IMPOSSIBLE, Model.cpp:96)");
  if (n_modified)
    *n_modified = h[2];
  if (n_finished)
    *n_finished = h[0];
  return 0;
}

static int lazy_top(lmmhip_ctx* c, bool* any, double* top) {
  unsigned long long h = ~0ull;
  HIPCHK(hipMemsetAsync(c->act.umin, 0xFF, sizeof(unsigned long long), c->stream));
  if (c->act.n > 0)
    LAUNCH(7, -1, act_lazy_min, grid_for(c->act.n, kBlock), kBlock, c->act);
  HIPCHK(hipMemcpyAsync(&h, c->act.umin, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *any = h != ~0ull;
  if (*any) {
    const unsigned long long b = (h >> 63) ? (h & 0x7FFFFFFFFFFFFFFFull) : ~h;
    std::memcpy(top, &b, sizeof(*top));
  }
  return 0;
}

int lmmhip_next_event_lazy(lmmhip_ctx* c, double now, double* out) {
  if (!c || !out)
    return fail(LMMHIP_E_ARG, "null argument");
  if (!c->act.htype)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_lazy_upload first");
  HIPCHK(hipSetDevice(c->device));
  bool any = false;
  double top = 0;
  if (int rc = lazy_top(c, &any, &top))
    return rc;
  *out = any ? top - now : -1.0;  // Model.cpp:95-100
  return 0;
}

int lmmhip_actions_lazy_due(lmmhip_ctx* c, int model, double now, double surf_precision, int32_t* ids,
                            uint8_t* events, int64_t cap, int64_t* n_due) {
  if (!c || !n_due)
    return fail(LMMHIP_E_ARG, "null argument");
  if (!c->act.htype)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_lazy_upload first");
  if (model != MODEL_CPU && model != MODEL_CM02)
    return fail(LMMHIP_E_ARG, "lazy update: CPU or CM02 model");
  HIPCHK(hipSetDevice(c->device));
  *n_due = 0;
  bool any = false;
  double top = 0;
  if (int rc = lazy_top(c, &any, &top))
    return rc;
  if (!any || !(std::fabs(top - now) < surf_precision))  // the heap loop's first test
    return 0;
  int32_t h = 0;
  HIPCHK(hipMemsetAsync(c->act.ndue, 0, sizeof(int32_t), c->stream));
  LAUNCH(7, -1, act_lazy_due, grid_for(c->act.n, kBlock), kBlock, c->act, model, now, surf_precision);
  HIPCHK(hipMemcpyAsync(&h, c->act.ndue, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (h > cap || (h && (!ids || !events)))
    return fail(LMMHIP_E_ARG, "lazy due: output capacity too small (the heap entries are already popped)");
  if (h) {
    std::vector<int32_t> v(static_cast<size_t>(h));
    std::vector<uint8_t> e(static_cast<size_t>(c->act.n));
    HIPCHK(hipMemcpyAsync(v.data(), c->act.due, size_t(h) * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(e.data(), c->act.events, size_t(c->act.n), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::sort(v.begin(), v.end());  // deterministic order (the reference pops by (date, Action*))
    for (int32_t k = 0; k < h; k++) {
      ids[k] = v[size_t(k)];
      events[k] = e[size_t(v[size_t(k)])];
    }
  }
  *n_due = h;
  return 0;
}

int lmmhip_actions_lazy_download(lmmhip_ctx* c, double* last_update, double* last_value, double* date,
                                 uint8_t* heap_type) {
  if (!c)
    return fail(LMMHIP_E_ARG, "null context");
  if (!c->act.htype)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_lazy_upload first");
  HIPCHK(hipSetDevice(c->device));
  const size_t n = size_t(c->act.n);
  if (n) {
    if (last_update)
      HIPCHK(hipMemcpyAsync(last_update, c->act.last_update, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (last_value)
      HIPCHK(hipMemcpyAsync(last_value, c->act.last_value, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (date)
      HIPCHK(hipMemcpyAsync(date, c->act.date, n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (heap_type)
      HIPCHK(hipMemcpyAsync(heap_type, c->act.htype, n, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}
