// Host thread-sanitizer check of the kernel-option table (mlic_amd/csrc/options.cpp): writer threads set every
// option over and over while reader threads open an OptionScope and read every switch many times.  Build and run
// from the repository root:
//
//   g++ -std=c++17 -O1 -g -fsanitize=thread -pthread -Imlic_amd/csrc \
//       tools/options_check.cpp mlic_amd/csrc/options.cpp -o /tmp/options_check && /tmp/options_check
//
// Exit status 0 and a final "options_check ok" line mean: within a scope no read of any switch ever differed
// from the scope's first read, a nested scope read the outer snapshot, a child thread that adopted the snapshot
// (as Model::over_lanes' lane threads do) read the same values and left nothing installed behind, the readers
// did see the writers' sets from one scope to the next, and the sanitizer reported nothing.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "options.h"

using namespace mlic;

static const char* kNames[OPT_SETTABLE] = {"x4_halo", "x4_splitk", "linatt_fused", "dw_strip",     "ep_half",
                                           "chain_nj", "dwpw2",    "pw3",          "narrow_limit", "image_io_path",
                                           "lrp_half", "intra_half",   "gdn_skip",     "x4_epi"};

#define REQUIRE(cond)                                                      \
  do {                                                                     \
    if (!(cond)) {                                                         \
      std::fprintf(stderr, "options_check: %s (line %d)\n", #cond, __LINE__); \
      std::abort();                                                        \
    }                                                                      \
  } while (0)

static void read_all(int* v) {
  for (int o = 0; o < OPT_COUNT; ++o) v[o] = opt((Opt)o);
}
static void same_as(const int* first) {
  for (int o = 0; o < OPT_COUNT; ++o) REQUIRE(opt((Opt)o) == first[o]);
}

int main() {
  std::atomic<bool> stop{false};
  std::atomic<long> changes{0};
  std::vector<std::thread> writers, readers;
  for (int w = 0; w < 3; ++w)
    writers.emplace_back([&stop, w] {
      const int vals[6] = {-1, 0, 1, 2, 3, 40};
      for (unsigned k = w; !stop.load(); ++k)
        for (int o = 0; o < OPT_SETTABLE; ++o)
          opt_set(kNames[o], o == OPT_IMAGE_IO_PATH ? (int)(k % 4) - 1 : vals[(k + o) % 6]);
    });
  for (int r = 0; r < 4; ++r)
    readers.emplace_back([&changes] {
      int prev[OPT_COUNT] = {};
      for (int it = 0; it < 3000; ++it) {
        REQUIRE(OptionScope::current() == nullptr);
        {
          OptionScope scope;
          const int* snap = OptionScope::current();
          REQUIRE(snap != nullptr);
          int first[OPT_COUNT];
          read_all(first);
          for (int k = 0; k < 100; ++k) same_as(first);
          {
            OptionScope nested;  // reuses the outer snapshot
            REQUIRE(OptionScope::current() == snap);
            same_as(first);
          }
          REQUIRE(OptionScope::current() == snap);  // the nested scope's end leaves the outer one installed
          if (it % 16 == 0) {
            std::thread child([snap, &first] {
              {
                OptionScope adopted(snap);
                REQUIRE(OptionScope::current() == snap);
                for (int k = 0; k < 100; ++k) same_as(first);
              }
              REQUIRE(OptionScope::current() == nullptr);
            });
            child.join();
          }
          for (int o = 0; o < OPT_SETTABLE; ++o)
            if (it > 0 && first[o] != prev[o]) ++changes;
          for (int o = 0; o < OPT_COUNT; ++o) prev[o] = first[o];
        }
      }
    });
  for (auto& t : readers) t.join();
  stop = true;
  for (auto& t : writers) t.join();
  REQUIRE(changes.load() > 0);
  for (int o = 0; o < OPT_SETTABLE; ++o) opt_set(kNames[o], o == OPT_NARROW_LIMIT ? 0 : -1);
  const int dflt[OPT_SETTABLE] = {1, 0, 1, 1, 1, 1, 2, 1, 32767, -1, 0, 0, 1, 1};  // with no MLIC_* variable set
  bool env = false;
  for (int o = 0; o < OPT_COUNT; ++o) env = env || opt_str((Opt)o) != nullptr;
  for (int o = 0; o < OPT_SETTABLE && !env; ++o) REQUIRE(opt_get(kNames[o]) == dflt[o]);
  std::printf("options_check ok: %ld changes seen between scopes\n", changes.load());
  return 0;
}
