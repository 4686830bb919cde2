// The switch table (options.h).  The only file of the library that reads the environment.
#include "options.h"

#include <atomic>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>

namespace mlic {
namespace {

// A row's rule gives the effective value from v (the value last set; -1 = never set, and always -1 for a
// frozen switch), the environment string e (nullptr = unset) and the row's default d.
int env_int(const char* e, int d) { return e ? std::atoi(e) : d; }
int raw(int v, const char* e, int d) { return v >= 0 ? v : env_int(e, d); }
int flag(int v, const char* e, int d) { return v >= 0 ? v != 0 : env_int(e, d) != 0; }
int lead0(int, const char* e, int) { return !(e && e[0] == '0'); }
int is1(int, const char* e, int d) { return env_int(e, d) == 1; }
int str(int, const char* e, int) { return e != nullptr; }  // a string switch: opt_str, parsed beside its user
// internal 0 = off, 1 = the default forms (5 x 5 and, since round 10, 3 x 3: conv_x4.hip x4_halo), 2 = every
// K x K that fits (the option's 1), 5 = 5 x 5 only ($MLIC_X4_HALO=5, an A/B arm)
int halo(int v, const char* e, int d) { return v >= 0 ? (v == 0 ? 0 : 2) : env_int(e, d); }
int nj(int v, const char* e, int d) { return (v > 0 ? v : env_int(e, d)) == 2 ? 2 : 1; }  // 0 reverts too
int narrow(int v, const char*, int d) { return v <= 0 || v > d ? d : v; }

struct Row {
  const char* name;  // mlic_set_kernel_option's name; nullptr = frozen
  const char* env;
  int dflt;
  int (*rule)(int v, const char* e, int d);
};
const Row kRows[] = {
    {"x4_halo", "MLIC_X4_HALO", 1, halo},
    {"x4_splitk", "MLIC_X4_SPLITK", 0, flag},
    {"linatt_fused", "MLIC_LINATT_FUSED", 1, flag},
    {"dw_strip", "MLIC_DW_STRIP", 1, flag},
    {"ep_half", "MLIC_EP_HALF", 1, flag},
    {"chain_nj", "MLIC_CHAIN_NJ", 1, nj},
    {"dwpw2", "MLIC_DWPW2", 2, raw},
    {"pw3", "MLIC_PW3", 1, raw},
    {"narrow_limit", nullptr, 32767, narrow},
    {"image_io_path", nullptr, -1, raw},  // -1 = by layout; opt_set refuses values outside [-1, 2]
    // round 7; the two half forms are off by default: they did not move the main line beyond its spread
    {"lrp_half", "MLIC_LRP_HALF", 0, flag},
    {"intra_half", "MLIC_INTRA_HALF", 0, raw},  // 2 = on, and the module-level test entry takes the half form too
    {"gdn_skip", "MLIC_GDN_SKIP", 1, flag},
    // conv_x4's lean epilogue: 0 = off, 1 = the tile classes that measured faster, 2 = every class (launch_x4)
    {"x4_epi", "MLIC_X4_EPI", 1, raw},
    // frozen, in the enum's order.  MLIC_HOIST: -1 = auto (Model::hoist_on); MLIC_HOST_THREADS and mlic_create's
    // MLIC_LANES, MLIC_PRECISION, MLIC_SYNTH_FP16, MLIC_POISON apply only when set (opt_str)
    {nullptr, "MLIC_X4", 1, flag},           {nullptr, "MLIC_X4_K", 0, str},
    {nullptr, "MLIC_X4_BM_FOR", 0, str},     {nullptr, "MLIC_X4_BM96", 1, lead0},
    {nullptr, "MLIC_X4_BM224", 1, lead0},    {nullptr, "MLIC_X4_RS", 1, flag},
    {nullptr, "MLIC_X4_DIRECT", 1, flag},    {nullptr, "MLIC_X4_ABL", 0, raw},
    {nullptr, "MLIC_V2_WIDE", 1, flag},      {nullptr, "MLIC_LOCAL_ATTN_VALU", 0, flag},
    {nullptr, "MLIC_TAPS", 1, flag},         {nullptr, "MLIC_HOIST", -1, raw},
    {nullptr, "MLIC_DWPW", 1, flag},         {nullptr, "MLIC_CHAIN", 1, flag},
    {nullptr, "MLIC_LA_PACKED", 1, flag},    {nullptr, "MLIC_LANE_PRIORITY", 1, flag},
    {nullptr, "MLIC_PHASE_D2H", 0, raw},     {nullptr, "MLIC_HOST_THREADS", 0, raw},
    {nullptr, "MLIC_POOL_PRIO", 2, raw},     {nullptr, "MLIC_LANES", 0, raw},
    {nullptr, "MLIC_PRECISION", 0, raw},     {nullptr, "MLIC_SYNTH_FP16", 0, is1},
    {nullptr, "MLIC_POISON", 0, flag},
};
static_assert(sizeof(kRows) / sizeof(kRows[0]) == OPT_COUNT, "one row per Opt");

struct {
  std::atomic<int> v{-1};
} g_set[OPT_SETTABLE];

struct Env {  // the environment as first read, and the frozen switches' values
  bool has[OPT_COUNT];
  std::string text[OPT_COUNT];
  int frozen[OPT_COUNT];
  Env() {
    for (int i = 0; i < OPT_COUNT; ++i) {
      const char* e = kRows[i].env ? std::getenv(kRows[i].env) : nullptr;
      has[i] = e != nullptr;
      if (e) text[i] = e;
      frozen[i] = kRows[i].rule(-1, e, kRows[i].dflt);
    }
  }
  const char* get(int i) const { return has[i] ? text[i].c_str() : nullptr; }
};
const Env& env() {
  static const Env e;
  return e;
}

Opt find(const char* name) {
  for (int i = 0; i < OPT_SETTABLE; ++i)
    if (std::strcmp(name, kRows[i].name) == 0) return (Opt)i;
  throw std::runtime_error(std::string("mlic: unknown kernel option ") + name);
}

}  // namespace

int opt_live(Opt o) {
  const Env& e = env();
  if (o >= OPT_SETTABLE) return e.frozen[o];
  return kRows[o].rule(g_set[o].v.load(std::memory_order_relaxed), e.get(o), kRows[o].dflt);
}

const char* opt_str(Opt o) { return env().get(o); }

void opt_set(const char* name, int value) {
  const Opt o = find(name);
  if (o == OPT_IMAGE_IO_PATH && (value < -1 || value > 2))
    throw std::runtime_error("mlic: image_io_path must be -1 (by layout), 0, 1 or 2");
  g_set[o].v.store(value, std::memory_order_relaxed);
}

int opt_get(const char* name) { return opt_live(find(name)); }

OptionScope::OptionScope() : owner_(tl_opt_snap == nullptr) {
  if (!owner_) return;
  for (int i = 0; i < OPT_COUNT; ++i) vals_[i] = opt_live((Opt)i);
  tl_opt_snap = vals_;
}

OptionScope::OptionScope(const int* snap) : owner_(tl_opt_snap == nullptr && snap != nullptr) {
  if (owner_) tl_opt_snap = snap;
}

}  // namespace mlic
