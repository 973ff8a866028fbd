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
  ActDev& a = c->act;
  a = ActDev{};
  a.n = n;
  int32_t* vidx;
  double *sp;
  uint8_t* fl;
  int rc = 0;
  rc |= act_alloc(c, &vidx, n, var_index);
  rc |= act_alloc(c, &a.remains, n, remains);
  rc |= act_alloc(c, &a.max_duration, n, max_duration);
  rc |= act_alloc(c, &a.latency, n, latency);
  rc |= act_alloc(c, &a.penalty, n, penalty);
  rc |= act_alloc(c, &sp, n, sharing_penalty);
  rc |= act_alloc(c, &fl, n, flags);
  rc |= act_alloc<uint8_t>(c, &a.events, n, nullptr);
  rc |= act_alloc<unsigned long long>(c, &a.umin, 1, nullptr);
  rc |= act_alloc<int32_t>(c, &a.nev, 1, nullptr);
  if (rc)
    return rc;
  a.vidx = vidx;
  a.share_pen = sp;
  a.flags = fl;
  HIPCHK(hipStreamSynchronize(c->stream));
  return 0;
}

int lmmhip_next_event_full(lmmhip_ctx* c, int with_latency, double* out) {
  if (!c || !out)
    return fail(LMMHIP_E_ARG, "null argument");
  if (!c->act.umin)
    return fail(LMMHIP_E_STATE, "lmmhip_actions_upload first");
  HIPCHK(hipSetDevice(c->device));
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
