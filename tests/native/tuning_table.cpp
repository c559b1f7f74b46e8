// The tuning table (csrc/tuning.def, tuning.cpp) on its own: what every row holds and does, through tuning_get / tuning_set
// alone.  Built by `make san` from tuning.cpp and this file (no HIP, no Python) with and without the sanitizers, run by
// tests/test_host_sanitizers.py, which compares the lines below with the one table of defaults the tests keep.
//   <key> <type> <default> <replan> <stored after set(-7)> <stored after set(1 << 40)>
#include <cstdio>
#include <vector>

#include "tuning.h"

int main() {
  struct Row { const char* key; const char* type; };
  const std::vector<Row> rows = {
#define TUNE(key, type, var, def, lowest, flags) {key, #type},
#include "tuning.def"
#undef TUNE
  };
  std::vector<long long> held;
  for (const Row& r : rows) {
    long long was = 0, low = 0, big = 0;
    bool replan = false, again = true;
    int bad = tuning_get(r.key, &was);
    bad |= tuning_set(r.key, -7, &replan) | tuning_get(r.key, &low);
    bad |= tuning_set(r.key, 1LL << 40, &again) | tuning_get(r.key, &big);
    bad |= tuning_set(r.key, 3, nullptr);                  // the replan flag is optional
    if (bad || again != replan) return std::printf("%s: a call failed\n", r.key), 1;
    std::printf("%s %s %lld %d %lld %lld\n", r.key, r.type, was, (int)replan, low, big);
    held.push_back(was);
  }
  long long v = 12345;
  bool replan = false;
  std::printf("unknown key: set %d get %d, null key: set %d get %d, null value: get %d, untouched %lld %d\n",
              tuning_set("tail_", 1, &replan), tuning_get("fuse ", &v), tuning_set(nullptr, 1, &replan), tuning_get(nullptr, &v),
              tuning_get("fuse", nullptr), v, (int)replan);
  for (size_t i = rows.size(); i-- > 0;) {
    if (tuning_set(rows[i].key, held[i], nullptr) || tuning_get(rows[i].key, &v) || v != held[i])
      return std::printf("%s: not restored\n", rows[i].key), 1;
  }
  std::printf("restored %zu keys\n", rows.size());
  return 0;
}
