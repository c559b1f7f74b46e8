// The process-wide dispatch knobs behind ctd_tuning_set / ctd_tuning_get: one plain variable per row of tuning.def (defined
// in tuning.cpp), read directly by the launchers, plan() and the tail.  Plain C++, no HIP.
#pragma once

#define TUNE(key, type, var, def, lowest, flags) extern type var;
#include "tuning.def"
#undef TUNE

// 0, or -1 for an unknown key (or a null pointer).  `set` stores the value as its row says (clamped, truncated to the
// variable's type) and reports in *replan (may be null) whether cached plans are stale; `get` returns what is stored.
int tuning_set(const char* key, long long value, bool* replan);
int tuning_get(const char* key, long long* value);
