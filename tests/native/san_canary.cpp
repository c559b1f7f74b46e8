// Canary of tests/test_host_sanitizers.py: three small, deliberate defects in host-only CPU code, built by the same `san` rule of
// csrc/Makefile as the replay harness.  The asan flavour must REPORT `heap` and `overflow`, the tsan flavour `race`, the plain
// flavour runs all three silently -- so a -fsanitize flag dropped from the Makefile cannot turn the sanitizer tests green.
// Test-only: never linked into the product, never near a GPU.
//   san_canary heap | overflow | race
#include <climits>
#include <cstdio>
#include <cstring>
#include <thread>

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  if (!std::strcmp(argv[1], "heap")) {              // a read one element past a heap array
    volatile int n = 4;
    int* a = new int[n];
    for (int i = 0; i < n; ++i) a[i] = i;
    volatile int idx = n;
    const int v = a[idx];
    delete[] a;
    std::printf("heap %d\n", v);
  } else if (!std::strcmp(argv[1], "overflow")) {   // a signed overflow
    volatile int big = INT_MAX;
    const int v = big + argc;
    std::printf("overflow %d\n", v);
  } else if (!std::strcmp(argv[1], "race")) {       // an unlocked counter bumped by two threads
    static long counter = 0;
    auto bump = [] {
      for (int i = 0; i < 100000; ++i) counter = counter + 1;
    };
    std::thread a(bump), b(bump);
    a.join(), b.join();
    std::printf("race %ld\n", counter);
  } else {
    return 2;
  }
  return 0;
}
