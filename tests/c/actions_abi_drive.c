/* A C99 client of the resident action table's ABI (include/lmm/lmm_hip.h): every new entry point is declared,
 * links, and refuses a missing context with LMMHIP_E_ARG and a message — on a machine without a HIP device too,
 * where lmmhip_ctx_create leaves no context to pass.  Prints "ok" and returns 0, or names the call that misbehaved. */
#include <stdio.h>
#include <string.h>

#include "lmm/lmm_hip.h"

static int refused(const char* what, int rc) {
  const char* msg = lmmhip_last_error();
  if (rc != LMMHIP_E_ARG || !msg || !strlen(msg)) {
    fprintf(stderr, "%s: rc %d, message '%s'\n", what, rc, msg ? msg : "(null)");
    return 1;
  }
  return 0;
}

int main(void) {
  int32_t idx[2] = {0, 1}, slot[2] = {-1, 3}, ids[2];
  double remains[2] = {1.0, 2.0};
  uint8_t ev[2];
  int64_t n = 0, nm = 0, nf = 0;
  int bad = 0;
  lmmhip_ctx* none = NULL;
  bad += refused("bind", lmmhip_actions_bind(none, 2, slot));
  bad += refused("patch", lmmhip_actions_patch(none, 2, idx, LMMHIP_ACT_F_VAR_SLOT | LMMHIP_ACT_F_REMAINS, slot,
                                               remains, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL));
  bad += refused("lazy_update_solved", lmmhip_actions_lazy_update_solved(none, LMMHIP_MODEL_CM02, 0.0, 1e-5, 1e-5, 2,
                                                                         idx, &nm, &nf));
  bad += refused("events", lmmhip_actions_events(none, ids, ev, 2, &n));
  bad += refused("var_index", lmmhip_actions_var_index(none, ids));
  if (LMMHIP_ACT_F_HEAP_TYPE != 2048 || LMMHIP_ACT_F_DATE != 1024)
    bad++;
  if (!bad)
    puts("ok");
  return bad;
}
