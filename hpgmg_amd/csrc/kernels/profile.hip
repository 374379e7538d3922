// profile.hip -- smoother-kernel profiling: a hipEvent pair around every smoother launch (bench.py's roofline).  The launchers of stencil.hip,
// pair.hip and fv4_rb.hip bracket their launches with profile_begin / profile_end (declared in stencil_direct.hpp).
#include "stencil_direct.hpp"

extern "C" int hpgmg_hip_graph_is_open(void);

namespace hpgmg {

static bool g_profile = false;
static long long g_profile_min_cells = 0;   // only launches covering at least this many cells are timed
static const int kMaxPairs = 8192;
static hipEvent_t g_ev[2 * kMaxPairs];
static int g_pairs_alloc = 0, g_pairs_used = 0;
static long long g_prof_cells = 0, g_prof_launches = 0;
static double g_prof_ms_flushed = 0.0;
static bool g_profile_skipped_part1 = false;

static void profile_flush() {
  for (int p = 0; p < g_pairs_used; p++) {
    float ms = 0.f;
    hipEventSynchronize(g_ev[2 * p + 1]);
    if (hipEventElapsedTime(&ms, g_ev[2 * p], g_ev[2 * p + 1]) == hipSuccess) g_prof_ms_flushed += ms;
  }
  g_pairs_used = 0;
}
// An event is a marker packet, and the GPU idles ~5 us around each (measured: 8 per config-2 solve = 1.2 % of it; events attached to the dispatches
// themselves, hipExtLaunchKernelGGL, idle it longer).  So only every g_profile_stride-th eligible launch is timed: a stride coprime with the launches
// per solve (4 sweep pairs, 6 red + black passes, 8 sweeps) visits every position of the cycle in turn.
static int g_profile_stride = 1, g_profile_seen = 0;
int profile_begin(long long cells) {
  if (!g_profile || cells < g_profile_min_cells || hpgmg_hip_graph_is_open()) return -1;
  if (g_tile_part != 2 && (g_profile_seen++ % g_profile_stride) != 0) { g_profile_skipped_part1 = (g_tile_part == 1); return -1; }
  if (g_tile_part == 2 && g_profile_skipped_part1) return -1;          // the second part of a launch whose first part was not timed
  if (g_pairs_used == kMaxPairs) profile_flush();
  if (g_pairs_used == g_pairs_alloc) { hipEventCreate(&g_ev[2 * g_pairs_alloc]); hipEventCreate(&g_ev[2 * g_pairs_alloc + 1]); g_pairs_alloc++; }
  int p = g_pairs_used++;
  hipEventRecord(g_ev[2 * p], g_stream);
  return p;
}
// first_part: part 1 of a two-part launch (hpgmg_hip_set_tile_part): its time and cells are added to the launch that part 2 completes
void profile_end(int p, long long cells, bool first_part) {
  if (p < 0) return;
  hipEventRecord(g_ev[2 * p + 1], g_stream);
  g_prof_cells += cells;
  if (!first_part) g_prof_launches++;
}

}  // namespace hpgmg
using namespace hpgmg;

extern "C" {

void hpgmg_hip_profile_smoother(int enable) {
  if (enable) { profile_flush(); g_prof_ms_flushed = 0.0; g_prof_cells = 0; g_prof_launches = 0; }
  g_profile = enable != 0;
}
void hpgmg_hip_profile_smoother_min_cells(long long min_cells) { g_profile_min_cells = min_cells; }
void hpgmg_hip_profile_smoother_stride(int stride) { g_profile_stride = stride > 0 ? stride : 1; g_profile_seen = 0; }
int hpgmg_hip_profile_smoother_read(double *total_ms, long long *launches, long long *cells) {
  profile_flush();
  if (total_ms) *total_ms = g_prof_ms_flushed;
  if (launches) *launches = g_prof_launches;
  if (cells) *cells = g_prof_cells;
  return 0;
}

}  // extern "C"
