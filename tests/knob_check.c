/*
 * knob_check.c -- the switch table (omp_amg_amd/csrc/amgd_knob.c) on its own, for a sanitizer
 * build on the host: gcc -std=c11 -fsanitize=address,undefined knob_check.c amgd_knob.c.
 * Set, clear and re-read over the whole table, long and malformed values, unknown names.
 * Prints "ok <entries>" and returns 0, else names the first failure.
 */
#define _POSIX_C_SOURCE 200809L
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "amgd_knob.h"

#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); return 1; } \
  } while (0)

int main(void) {
  const char *name, *env;
  int64_t dflt;
  /* nothing set: every entry is its default, from source 0 */
  for (int id = 0; id < AMGD_K_N; id++) {
    CHECK(amgd_knob_info(id, &name, &env, &dflt) == 0);
    if (env) unsetenv(env);
  }
  amgd_knobs_read_env();
  for (int id = 0; id < AMGD_K_N; id++) {
    amgd_knob_info(id, &name, &env, &dflt);
    CHECK(amgd_knob_find(name) == id);
    CHECK(amgd_knob(id) == dflt && amgd_knob_source(id) == 0);
  }
  CHECK(amgd_knob_info(-1, &name, &env, &dflt) == -1 && amgd_knob_info(AMGD_K_N, &name, &env, &dflt) == -1);
  CHECK(amgd_knob_find("no_such_switch") == -1 && amgd_knob_find("") == -1 && amgd_knob_find(NULL) == -1);
  /* override, clear, environment, empty value, re-read: every entry */
  for (int id = 0; id < AMGD_K_N; id++) {
    amgd_knob_info(id, &name, &env, &dflt);
    amgd_knob_set(id, dflt + 7);
    CHECK(amgd_knob(id) == dflt + 7 && amgd_knob_source(id) == 2);
    if (env) {
      setenv(env, "3", 1);
      amgd_knobs_read_env();
      CHECK(amgd_knob(id) == dflt + 7 && amgd_knob_source(id) == 2);   /* the override stays */
      amgd_knob_clear(id);
      CHECK(amgd_knob_source(id) == 1 && amgd_knob(id) != dflt + 7);
      setenv(env, "", 1);
      amgd_knobs_read_env();
      CHECK(amgd_knob(id) == dflt && amgd_knob_source(id) == 0);
      unsetenv(env);
    }
    amgd_knob_clear(id);
    amgd_knobs_read_env();
    CHECK(amgd_knob(id) == dflt && amgd_knob_source(id) == 0);
  }
  /* long and malformed text through every parser: no crash, a defined value */
  char *big = malloc(70000);
  memset(big, '9', 69999);
  big[69999] = 0;
  const char *bad[] = {"abc", "-", " 12", "12abc", "1e400", "-1e400", "nan", "inf", ",,,", "8,,4", "2;4;8;16",
                       "99999999999999999999999999", "-99999999999999999999999999", "wave", "general", "0x10", big};
  for (unsigned b = 0; b < sizeof bad / sizeof *bad; b++) {
    for (int id = 0; id < AMGD_K_N; id++) {
      amgd_knob_info(id, &name, &env, &dflt);
      if (env) setenv(env, bad[b], 1);
    }
    amgd_knobs_read_env();
    for (int id = 0; id < AMGD_K_N; id++) {
      amgd_knob_info(id, &name, &env, &dflt);
      CHECK(amgd_knob_source(id) == (env ? 1 : 0));
      (void)amgd_knob(id);
    }
  }
  free(big);
  /* the text forms */
  setenv("AMGD_RESOLVE", "wave", 1);
  setenv("AMGD_LMOP", "general", 1);
  setenv("AMGD_VC_MRHS_K", "4,2", 1);
  setenv("AMGD_HBM_CAP_GB", "0.5", 1);
  setenv("AMGD_QQ_BUDGET_MB", "3", 1);
  setenv("AMGD_SHARD_MIN", "0.25", 1);
  setenv("AMGD_QF_CHAIN", "12abc", 1);
  setenv("AMGD_SGLOG", "0", 1);
  amgd_knobs_read_env();
  CHECK(amgd_knob(AMGD_K_RESOLVE_WAVE) == 1 && amgd_knob(AMGD_K_LMOP_MODE) == 1);
  CHECK(amgd_knob(AMGD_K_VC_MRHS_K) == 6);
  CHECK(amgd_knob(AMGD_K_HBM_CAP) == 536870912 && amgd_knob(AMGD_K_LMOP_QQ_BUDGET) == 3145728);
  CHECK(amgd_knob(AMGD_K_SHARD_MIN) == 250000);
  CHECK(amgd_knob(AMGD_K_QF_CHAIN) == 12);
  CHECK(amgd_knob(AMGD_K_SGLOG) == 0 && amgd_knob_source(AMGD_K_SGLOG) == 1);
  setenv("AMGD_RESOLVE", "block", 1);
  setenv("AMGD_VC_MRHS_K", "0", 1);
  amgd_knobs_read_env();
  CHECK(amgd_knob(AMGD_K_RESOLVE_WAVE) == 0 && amgd_knob(AMGD_K_VC_MRHS_K) == 0);
  printf("ok %d\n", AMGD_K_N);
  return 0;
}
