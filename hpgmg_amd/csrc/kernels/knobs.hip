// knobs.hip -- the environment knobs of the kernel library: the table, its parse, and the part of the C ABI that lists it (knobs.hpp).
// Host code only: no HIP header and no HIP call, so a process without a GPU can load the library and read the table.
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include "hpgmg_hip.h"
#include "knobs.hpp"

namespace hpgmg {

// What a row accepts: n == 0, the closed range [v[0], v[1]]; n > 0, the list v[0 .. n - 1].
struct Accept { int n; long long v[4]; };
static constexpr Accept kFlag = {2, {0, 1}};
// ">= lo": the sites add a level's side to a chunk length in int arithmetic, so the range ends well below INT_MAX
static constexpr long long kMany = 1 << 30;
static constexpr Accept at_least(long long lo) { return Accept{0, {lo, kMany}}; }

struct Row { Knob id; const char *env; long long dflt; Accept ok; const char *what; };
static constexpr Row table[] = {
  // pair.hip
  { K_PAIR_PACKED, "HPGMG_TUNE_PAIR_PACKED", 1, kFlag, "7-pt sweep pairs: the pre-pass reads its coefficient values packed once per operator rebuild; 0: in place" },
  { K_PAIR_KC, "HPGMG_TUNE_PAIR_KC", 0, at_least(0), "7-pt sweep pairs: output planes per k chunk; 0: the launcher's choice (8 .. 64).  Any length is a valid launch: the kernel ends a chunk at the level's last plane" },
  { K_PAIR_NW, "HPGMG_TUNE_PAIR_NW", 0, {4, {0, 10, 12, 16}}, "7-pt sweep pairs: waves per workgroup (the kernel's instances); 0: the cost model's choice per launch" },
  // stencil.hip
  { K_TY, "HPGMG_TUNE_TY", 0, {4, {0, 1, 2, 4}}, "register kernels on boxes of side > 32: rows per workgroup of 64-lane rows (the kernels are bound to 256 lanes); 0: 4.  Experiments only" },
  { K_KCHUNK, "HPGMG_TUNE_KCHUNK", 0, at_least(0), "register and wide 7-pt kernels: planes per k chunk; 0: the launcher's rule (wide kernel: 16).  Experiments only" },
  { K_MIN_KCHUNK, "HPGMG_TUNE_MIN_KCHUNK", 1, at_least(1), "register kernels: the shortest k chunk the halving rule goes down to" },
  { K_WANT_BLOCKS, "HPGMG_TUNE_WANT_BLOCKS", 4096, at_least(1), "register kernels: k chunks are halved until a launch has this many workgroups (~16 per CU)" },
  { K_27PT_TILE32, "HPGMG_TUNE_27PT_TILE32", 0, kFlag, "27-pt: the LDS-tiled kernel also takes boxes of 32^3, as 32 x 16 tiles (covered by the tests; measured 0.35 ms per `7 64` F-cycle SLOWER than the register kernel on that level: the 128^3 level is cache resident)" },
  { K_27PT_DIRECT, "HPGMG_TUNE_27PT_DIRECT", 0, kFlag, "27-pt: the register kernel everywhere (no LDS-tiled kernel)" },
  { K_27PT_KCHUNK, "HPGMG_TUNE_27PT_KCHUNK", 0, at_least(0), "27-pt tiled kernel: planes per k chunk where it divides the box side; 0: the launcher's rule" },
  { K_FV4_TILE32, "HPGMG_TUNE_FV4_TILE32", 1, kFlag, "fv4: the LDS-tiled kernel takes boxes whose side is a multiple of 32; 0: of 64" },
  { K_FV4_KCHUNK_MIN, "HPGMG_TUNE_FV4_KCHUNK_MIN", 8, at_least(1), "fv4 tiled kernel: the shortest k chunk the halving rule goes down to (a chunk costs four extra planes of loads: chunks of 4 planes -- what filling 1024 slots asked for on the 128^3 level of `7 64` -- fetch every plane twice; 8: 29 vs 34 us per half sweep there, tools/ab_fv4_kcmin.sh)" },
  { K_FV4_KCHUNK, "HPGMG_TUNE_FV4_KCHUNK", 0, at_least(0), "fv4 tiled kernel: planes per k chunk where it divides the box side; 0: the launcher's rule" },
  { K_FV4_TJ, "HPGMG_TUNE_FV4_TJ", 8, {2, {8, 16}}, "fv4 tiled kernel on boxes of side 64 m: rows per tile (8: two workgroups per CU; 16: one of 16 waves; measured at launch_fv4_tile, stencil.hip)" },
  { K_FV4_DIRECT, "HPGMG_TUNE_FV4_DIRECT", 0, kFlag, "fv4: the register kernel everywhere (no LDS-tiled kernel)" },
  { K_NO_WIDE, "HPGMG_TUNE_NO_WIDE", 0, kFlag, "7-pt: no wide kernel on boxes of side 128 m" },
  { K_WIDE_WJ, "HPGMG_TUNE_WIDE_WJ", 8, {2, {4, 8}}, "7-pt wide kernel: wave rows per workgroup (the kernel's instances)" },
  { K_7PT_NO_TILE, "HPGMG_TUNE_7PT_NO_TILE", 0, kFlag, "7-pt: no LDS-staged tile kernel on boxes of side 64 m" },
  { K_7PT_TILE_KCHUNK, "HPGMG_TUNE_7PT_TILE_KCHUNK", 8, at_least(0), "7-pt tile kernel: planes per k chunk where it divides the box side; else 8" },
  { K_SMALL_RR, "HPGMG_TUNE_SMALL_RR", 1, kFlag, "7-pt: residual + restriction + zero_vector as one launch on the launch-bound levels; 0: the two launches (experiments)" },
  { K_27PT_NO_RB, "HPGMG_TUNE_27PT_NO_RB", 0, kFlag, "27-pt GSRB: no one-pass red + black kernel on boxes of side 64 m" },
  { K_27PT_RB_KCHUNK, "HPGMG_TUNE_27PT_RB_KCHUNK", 0, at_least(0), "27-pt red + black kernel: planes per k chunk where it divides the box side; 0: the launcher's rule" },
  { K_27PT_NO_RB_BOX, "HPGMG_TUNE_27PT_NO_RB_BOX", 0, kFlag, "27-pt GSRB: no one-workgroup-per-box red + black kernel on small boxes" },
  { K_27PT_RB_BOX_MAXDIM, "HPGMG_TUNE_27PT_RB_BOX_MAXDIM", 8, at_least(0), "27-pt GSRB: largest box side that kernel takes.  Boxes of 16^3 and 32^3 are handled as cubes of 8^3 (bit-identical, tested) but measure no faster (16^3) or slower (32^3: 14.3 vs 14.2 ms per `7 64` F-cycle) than the launches they replace -- every cube re-reads a two-cell rim, 3.4 values per cell" },
  // fv4_rb.hip
  { K_FV4_NO_RB, "HPGMG_TUNE_FV4_NO_RB", 0, kFlag, "fv4 GSRB: no one-pass red + black kernel (the tiled kernel, one half sweep per launch)" },
  { K_FV4_RB_ORDER, "HPGMG_TUNE_FV4_RB_ORDER", 1, kFlag, "fv4 red + black kernel: every XCD starts with its tiles at a domain wall (they take a quarter longer); 0: in order" },
  { K_FV4_RB_KCHUNK, "HPGMG_TUNE_FV4_RB_KCHUNK", 0, at_least(0), "fv4 red + black kernel: planes per k chunk where it divides the box side; 0: the launcher's rule" },
  { K_EXP_TIMELINE_WG, "HPGMG_EXP_TIMELINE_WG", -1, at_least(-1), "experiment build (-DHPGMG_EXP_TIMELINE) only: the workgroup of the fv4 red + black kernel that records its timeline; -1: none" },
  // small_levels.hip
  { K_SMALL_NO_LDS, "HPGMG_TUNE_SMALL_NO_LDS", 0, kFlag, "one-box small levels: no LDS image (the launcher then refuses the level)" },
  { K_BOTTOM_THREADS, "HPGMG_TUNE_BOTTOM_THREADS", 512, at_least(0), "device BiCGStab bottom solve: lanes of its one workgroup are 512 from this value up, 256 from 256 up, else sized by the cells (eight waves whatever the level: the 26 boundary entries are a wave's work each)" },
  // blas1.hip, blocks.hip
  { K_COPY_NT, "HPGMG_TUNE_COPY_NT", 1, kFlag, "norm + copy + restriction: non-temporal stores of a fine vector beyond the infinity cache (256 MB)" },
  { K_INTERP_NT, "HPGMG_TUNE_INTERP_NT", 1, kFlag, "interpolation onto a zeroed vector: the same (nothing of it would still be cached when the next kernel reads it)" },
  // brick_visit.hip
  { K_TEST_BRICK_CAPACITY, "HPGMG_TEST_BRICK_CAPACITY", -1, at_least(-1), "tests: the workgroups of a brick launch the device is said to hold at once; -1: ask the device" },
  { K_TEST_BRICK_ABSENT, "HPGMG_TEST_BRICK_ABSENT", -1, at_least(-1), "tests: this workgroup of every brick launch leaves at once, as if it had never become resident; -1: none" },
  // comm_rccl.hip, comm_ipc.hip, runtime.hip, graph.hip
  { K_RCCL_SUBCOMM, "HPGMG_RCCL_SUBCOMM", 1, kFlag, "RCCL: reductions over a subset of the ranks on a communicator split for it; 0: keep the all-to-all (every rank must say the same)" },
  { K_IPC_DEBUG, "HPGMG_IPC_DEBUG", 0, kFlag, "IPC transport: report every HIP call it makes on stderr" },
  { K_ROCTX, "HPGMG_ROCTX", 0, kFlag, "roctx range \"<dim>^3 <operator>\" around every operator (the marker library is resolved with dlopen)" },
  { K_GRAPH_DEBUG, "HPGMG_GRAPH_DEBUG", 0, kFlag, "graph capture: report the first hipStreamBeginCapture that fails" },
};
static_assert(sizeof table / sizeof table[0] == KNOB_COUNT, "one row per Knob");
static constexpr bool rows_in_enum_order() { for (int k = 0; k < KNOB_COUNT; k++) if (table[k].id != k) return false; return true; }
static_assert(rows_in_enum_order(), "row k describes Knob k");

static long long g_value[KNOB_COUNT];
static bool g_known[KNOB_COUNT];

static bool accepted(const Accept &ok, long long v) {
  if (ok.n == 0) return v >= ok.v[0] && v <= ok.v[1];
  for (int q = 0; q < ok.n; q++) if (v == ok.v[q]) return true;
  return false;
}
static const char *accept_text(const Accept &ok, char *buf, size_t len) {
  if (ok.n == 0) { snprintf(buf, len, "[%lld, %lld]", ok.v[0], ok.v[1]); return buf; }
  int at = snprintf(buf, len, "{");
  for (int q = 0; q < ok.n; q++) at += snprintf(buf + at, len - (size_t)at, q ? ",%lld" : "%lld", ok.v[q]);
  snprintf(buf + at, len - (size_t)at, "}");
  return buf;
}

long long knob(Knob k) {
  if (!g_known[k]) {
    const Row &r = table[k];
    long long v = r.dflt;
    const char *e = getenv(r.env);
    if (e && *e) {
      char *end = nullptr;
      errno = 0;
      const long long got = strtoll(e, &end, 10);
      if (errno == 0 && *end == '\0' && accepted(r.ok, got)) v = got;
      else { char set[64]; fprintf(stderr, "hpgmg_hip: %s=%s is not accepted (%s); using %lld\n", r.env, e, accept_text(r.ok, set, sizeof set), r.dflt); }
    }
    g_value[k] = v; g_known[k] = true;
  }
  return g_value[k];
}
void knob_set(Knob k, long long value) { g_value[k] = value; g_known[k] = true; }

}  // namespace hpgmg
using namespace hpgmg;

extern "C" {

int hpgmg_hip_knob_count(void) { return KNOB_COUNT; }
const char *hpgmg_hip_knob_name(int k) { return (k >= 0 && k < KNOB_COUNT) ? table[k].env : nullptr; }
long long hpgmg_hip_knob_value(int k) { return (k >= 0 && k < KNOB_COUNT) ? knob((Knob)k) : 0; }
long long hpgmg_hip_knob_default(int k) { return (k >= 0 && k < KNOB_COUNT) ? table[k].dflt : 0; }
void hpgmg_hip_print_knobs(void) {      // (the line format of hpgmg_print_switches, the accepted values in front of the description)
  char set[64];
  for (int k = 0; k < KNOB_COUNT; k++)
    fprintf(stderr, "  %-28s = %-8lld (default %lld)  %s  %s\n", table[k].env, knob((Knob)k), table[k].dflt, accept_text(table[k].ok, set, sizeof set), table[k].what);
}

}  // extern "C"
