// Every runtime switch of the library: one table (options.cpp), one snapshot per call.  Host-only C++17.
//
// Frozen switches come from the environment alone and are read once per process (they shape what model
// creation builds: packed weight layouts, streams, pools).  Settable options are the names
// mlic_set_kernel_option accepts, each with its environment fallback; their live values are atomics.
// A call never reads a live value: every C-ABI entry opens an OptionScope, which copies the effective values
// into a plain array that opt() reads for the rest of the call -- so the dry and the real pass of
// Model::planned, a workspace's sizing and its launch, and every lane thread of the call (which adopts the
// caller's snapshot) see one value of every switch, and a set from another thread lands at the next call.
// Host-pool workers run under no scope: what they need is read by the submitter and passed down.
#pragma once

namespace mlic {

enum Opt : int {
  // settable (mlic_set_kernel_option), in the table's order
  OPT_X4_HALO, OPT_X4_SPLITK, OPT_LINATT_FUSED, OPT_DW_STRIP, OPT_EP_HALF, OPT_CHAIN_NJ, OPT_DWPW2, OPT_PW3,
  OPT_NARROW_LIMIT, OPT_IMAGE_IO_PATH, OPT_LRP_HALF, OPT_INTRA_HALF, OPT_GDN_SKIP, OPT_X4_EPI,
  OPT_SETTABLE,
  // frozen
  OPT_X4 = OPT_SETTABLE, OPT_X4_K, OPT_X4_BM_FOR, OPT_X4_BM96, OPT_X4_BM224, OPT_X4_RS, OPT_X4_DIRECT, OPT_X4_ABL,
  OPT_V2_WIDE, OPT_LOCAL_ATTN_VALU, OPT_TAPS, OPT_HOIST, OPT_DWPW, OPT_CHAIN, OPT_LA_PACKED, OPT_LANE_PRIORITY,
  OPT_PHASE_D2H, OPT_HOST_THREADS, OPT_POOL_PRIO, OPT_LANES, OPT_PRECISION, OPT_SYNTH_FP16, OPT_POISON,
  OPT_COUNT
};

int opt_live(Opt o);                        // the effective value the next call would see
const char* opt_str(Opt o);                 // the switch's environment string as first read, or nullptr when unset
void opt_set(const char* name, int value);  // throws on an unknown name or a refused value
int opt_get(const char* name);              // opt_live by name; throws on an unknown name

inline thread_local const int* tl_opt_snap = nullptr;  // the active snapshot of this thread

// The one read site: the call's snapshot, or the live value where no scope is active.
inline int opt(Opt o) {
  const int* s = tl_opt_snap;
  return s ? s[o] : opt_live(o);
}

class OptionScope {
 public:
  OptionScope();                          // snapshots now; nested in an active scope, reuses that one
  explicit OptionScope(const int* snap);  // a thread the call fans out to adopts the caller's current()
  ~OptionScope() { if (owner_) tl_opt_snap = nullptr; }
  OptionScope(const OptionScope&) = delete;
  OptionScope& operator=(const OptionScope&) = delete;
  static const int* current() { return tl_opt_snap; }

 private:
  int vals_[OPT_COUNT];
  bool owner_;
};

}  // namespace mlic
