// knobs.hpp -- the environment knobs of the kernel library, in ONE table (knobs.hip), as host/plugin_switches.c keeps the plugin's.
// A launcher asks knob(K_...): the variable is read on the first call for that knob (never when the library is loaded), checked against
// the values the row accepts, and cached; a value that is not accepted costs one line on stderr and gives the default.  Two knobs also
// have a setter in the C ABI (hpgmg_hip_set_27pt_tile32, hpgmg_hip_set_27pt_rb_box_maxdim): knob_set() overwrites the cached value, so
// a site never keeps a copy of its own.  The launchers are called from one thread, as the "next launch" requests they take assume.
// The one variable of the library the table does not hold is HPGMG_IPC_TIMEOUT (comm_ipc.hip): a real number of seconds.
#pragma once

namespace hpgmg {

enum Knob {
  K_PAIR_PACKED, K_PAIR_KC, K_PAIR_NW,
  K_TY, K_KCHUNK, K_MIN_KCHUNK, K_WANT_BLOCKS,
  K_27PT_TILE32, K_27PT_DIRECT, K_27PT_KCHUNK,
  K_FV4_TILE32, K_FV4_KCHUNK_MIN, K_FV4_KCHUNK, K_FV4_TJ, K_FV4_DIRECT,
  K_NO_WIDE, K_WIDE_WJ, K_7PT_NO_TILE, K_7PT_TILE_KCHUNK, K_SMALL_RR,
  K_27PT_NO_RB, K_27PT_RB_KCHUNK, K_27PT_NO_RB_BOX, K_27PT_RB_BOX_MAXDIM,
  K_FV4_NO_RB, K_FV4_RB_ORDER, K_FV4_RB_KCHUNK, K_EXP_TIMELINE_WG,
  K_SMALL_NO_LDS, K_BOTTOM_THREADS,
  K_COPY_NT, K_INTERP_NT,
  K_TEST_BRICK_CAPACITY, K_TEST_BRICK_ABSENT,
  K_RCCL_SUBCOMM, K_IPC_DEBUG, K_ROCTX, K_GRAPH_DEBUG,
  KNOB_COUNT
};

long long knob(Knob k);                       // the value in force
void knob_set(Knob k, long long value);       // overwrite it (the setters of the C ABI)

}  // namespace hpgmg
