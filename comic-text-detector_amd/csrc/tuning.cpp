// The variables of tuning.def and their lookup by key.
#include "tuning.h"

#include <climits>
#include <cstring>

#define TUNE(key, type, var, def, lowest, flags) type var = def;
#include "tuning.def"
#undef TUNE

namespace {

enum { NONE = 0, REPLAN = 1, BOOL = 2 };
constexpr long long NO_MIN = LLONG_MIN;

struct Row {
  const char* key;
  int* i;            // the variable: exactly one of the two
  long long* ll;
  long long lowest;
  int flags;
};
constexpr Row row(const char* key, int* p, long long lowest, int flags) { return {key, p, nullptr, lowest, flags}; }
constexpr Row row(const char* key, long long* p, long long lowest, int flags) { return {key, nullptr, p, lowest, flags}; }

const Row kRows[] = {
#define TUNE(key, type, var, def, lowest, flags) row(key, &var, lowest, flags),
#include "tuning.def"
#undef TUNE
};

const Row* find(const char* key) {
  if (key)
    for (const Row& r : kRows)
      if (!std::strcmp(r.key, key)) return &r;
  return nullptr;
}

}  // namespace

int tuning_set(const char* key, long long value, bool* replan) {
  const Row* r = find(key);
  if (!r) return -1;
  if (r->flags & BOOL) value = value != 0;
  if (value < r->lowest) value = r->lowest;
  if (r->i) *r->i = (int)value;
  else *r->ll = value;
  if (replan) *replan = (r->flags & REPLAN) != 0;
  return 0;
}

int tuning_get(const char* key, long long* value) {
  const Row* r = find(key);
  if (!r || !value) return -1;
  *value = r->i ? *r->i : *r->ll;
  return 0;
}
