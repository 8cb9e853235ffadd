/*
 * amgd_knob.c -- the switch table's state: defaults, environment values, overrides
 * (amgd_knob.h).  Plain arrays, no locking, like the globals they replace.
 */
#include <stdlib.h>
#include <string.h>

#include "amgd_knob.h"

typedef int64_t (*knob_parse)(const char *text);

/* AMGD_RESOLVE=wave, AMGD_LMOP=general: the first letter decides */
static int64_t amgd_knob_parse_resolve(const char *e) { return e[0] == 'w'; }
static int64_t amgd_knob_parse_lmop(const char *e) { return e[0] == 'g'; }
/* GB with fractions -> bytes (nothing positive: 0); whole MB -> bytes */
static int64_t amgd_knob_parse_gb(const char *e) {
  const double gb = strtod(e, NULL);
  return gb > 0 && gb < 8e9 ? (int64_t)(gb * 1073741824.0) : 0;
}
static int64_t amgd_knob_parse_mb(const char *e) { return (int64_t)((uint64_t)strtoll(e, NULL, 10) << 20); }
/* a decimal factor -> millionths */
static int64_t amgd_knob_parse_micro(const char *e) {
  const double v = strtod(e, NULL) * 1e6;
  return v > -9e18 && v < 9e18 ? (int64_t)(v < 0 ? v - 0.5 : v + 0.5) : 0;
}
/* a list out of 2, 4, 8 (any one-character separator) -> their mask; other numbers drop out */
static int64_t amgd_knob_parse_ksizes(const char *e) {
  int64_t mask = 0;
  while (*e) {
    char *end;
    const long v = strtol(e, &end, 10);
    if (end == e) break;
    if (v == 2 || v == 4 || v == 8) mask |= v;
    e = *end ? end + 1 : end;
  }
  return mask;
}

static const struct { const char *name, *env; int64_t dflt; knob_parse parse; const char *doc; } g_tab[AMGD_K_N] = {
#define AMGD_KNOB_ROW(id, name, env, dflt, parse, doc) {name, env, dflt, parse, doc},
  AMGD_KNOBS(AMGD_KNOB_ROW)
#undef AMGD_KNOB_ROW
};

int64_t amgd_knob_val[AMGD_K_N];
int amgd_knob_ready;
static int64_t g_envv[AMGD_K_N];                  /* the environment's value where g_src & 1 */
static unsigned char g_src[AMGD_K_N];             /* bit 0: the variable is set, bit 1: an override is */

static void settle(int id) {
  if (!(g_src[id] & 2)) amgd_knob_val[id] = g_src[id] & 1 ? g_envv[id] : g_tab[id].dflt;
}
void amgd_knobs_read_env(void) {
  amgd_knob_ready = 1;
  for (int id = 0; id < AMGD_K_N; id++) {
    const char *e = g_tab[id].env ? getenv(g_tab[id].env) : NULL;
    g_src[id] = (unsigned char)((g_src[id] & 2) | (e && *e ? 1 : 0));
    if (e && *e) g_envv[id] = g_tab[id].parse ? g_tab[id].parse(e) : strtoll(e, NULL, 10);
    settle(id);
  }
}
int amgd_knob_source(int id) {
  if (!amgd_knob_ready) amgd_knobs_read_env();
  return g_src[id] & 2 ? 2 : g_src[id] & 1;
}
void amgd_knob_set(int id, int64_t v) {
  if (!amgd_knob_ready) amgd_knobs_read_env();
  g_src[id] |= 2;
  amgd_knob_val[id] = v;
}
void amgd_knob_clear(int id) {
  if (!amgd_knob_ready) amgd_knobs_read_env();
  g_src[id] &= 1;
  settle(id);
}
int amgd_knob_find(const char *name) {
  for (int id = 0; name && id < AMGD_K_N; id++)
    if (!strcmp(g_tab[id].name, name)) return id;
  return -1;
}
int amgd_knob_info(int id, const char **name, const char **env, int64_t *dflt) {
  if (id < 0 || id >= AMGD_K_N) return -1;
  *name = g_tab[id].name; *env = g_tab[id].env; *dflt = g_tab[id].dflt;
  return 0;
}
