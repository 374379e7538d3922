// stencil.hip -- the hot path: Chebyshev / GSRB / Jacobi smoother sweeps and the
// residual / apply_op stencil of the 7-point operator, written for gfx950.
//
// Reference semantics (paths relative to finite-volume/source/):
//   apply_op_ijk      operators.7pt.c:49-89 (VC Helmholtz :51-62, VC Poisson :64-74, CC :77-88)
//   Chebyshev update  operators/chebyshev.c:86-95      GSRB update operators/gsrb.c:90-105
//   Jacobi update     operators/jacobi.c:53-60         residual    operators/residual.c:42-48
// Every floating-point expression keeps the reference's association and the
// file is compiled with -ffp-contract=off, so results are bit-identical to the
// reference's gcc -O2 build (no FMA, no reassociation): see DESIGN.md "parity".
//
// Bound: HBM bandwidth (about 25 flop per 64-72 B per cell).  This file holds the request state, the launch planner, every single-sweep
// launcher, the fused residual forms and the 27-point red/black launchers; the kernels it instantiates live in headers only it includes:
//   * stencil7.hpp: stencil7_kernel (any box size; the mid-size, cache-resident levels) and stencil7_shell_kernel (the cells next to
//     faces owned by another rank, after the overlapped exchange);
//   * stencil7_wide.hpp: stencil7_wide_kernel (boxes of side 128 m; the bandwidth-bound fine level);
//   * stencil7_tile.hpp, stencil27_tile.hpp, fv4_tile.hpp, stencil27_rb.hpp, stencil27_rb_box.hpp: the LDS-staged kernels;
//   * stencil_untiled.hpp: stencil27_kernel (27-point) and stencil_direct_kernel (4th-order fv4, black-box probes);
//   * (cheby_pair_kernel, two sweeps per pass on the fine level: cheby_pair.hpp, launched from pair.hip; the single-workgroup kernels of
//     the small levels: small_levels.hip; the smoother profiler: profile.hip; shared declarations: stencil_direct.hpp)
//   * logical tiles are ordered box, k, j, i and dealt to XCDs in contiguous ranges (common.hpp) so halo
//     planes shared by adjacent tiles hit the same L2.
// A run-time variant becomes a template argument through with_variant (launch_dispatch.hpp): each site names the list of variants it has
// instances for, and refuses any other.
#include "reduce.hpp"
#include "knobs.hpp"
#include "launch_dispatch.hpp"
#include "stencil_direct.hpp"
#include "stencil7.hpp"
#include "stencil7_wide.hpp"
#include "stencil_untiled.hpp"
#include "stencil27_rb.hpp"
#include "stencil27_rb_box.hpp"
#include "stencil7_tile.hpp"

extern "C" int hpgmg_hip_graph_flush(void);

namespace hpgmg {

static InterpFold g_fold = {};            // set by hpgmg_hip_stencil_fold_interpolation for the NEXT hpgmg_hip_smooth_cheby call, which moves it to g_fold_now whatever path it takes
static InterpFold g_fold_now = {};        // the fold of the hpgmg_hip_smooth_cheby call in progress
static int g_ghost_free = 0;
static int g_tile_ghost_free = 0;
static TileFused g_tile_fused = {};      // consumed by the next tiled residual launch (27-point / fv4): what becomes of the residual
static int g_tile_last_blocks = 0;       // workgroups of that launch (= partial maxima written)   // the LDS-tiled fv4 / 27-point kernels read x outside a box from the neighbouring box (all boxes local)
static int g_defer_mode = 0;   // 0: whole boxes; 1: skip the cells next to remote faces; 2: only those cells (stencil7_shell_kernel)

// A fused residual form was requested (g_tile_fused) but the launch is about to take a kernel that cannot honour it -- it would STORE the
// residual over the vector the caller passed as a dummy output.  Refuse loudly; never leave the request pending for a later launch.
static int refuse_unfused(const char *kernel) {
  if (!g_tile_fused.kind) return 0;
  g_tile_fused = TileFused{};
  return record_error(hipErrorInvalidValue, kernel);
}
// A variant outside the list of the launcher it reached: refused, nothing launched.
static int refuse_variant() { return record_error(hipErrorInvalidValue, "stencil variant not implemented"); }

static void plan(const hpgmg_hip_level *L, StencilArgs &P, dim3 &block, int &grid) {
  const int tune_ty = (int)knob(K_TY), tune_kchunk = (int)knob(K_KCHUNK);
  P.ghost_free = (g_ghost_free && L->box_nbr) ? 1 : 0;
  int tx = 64;
  while (tx > 1 && tx / 2 >= L->dim) tx /= 2;           // smallest power of two >= dim, capped at one wave
  int ty = 256 / tx;
  if (tune_ty > 0 && tx == 64) ty = tune_ty;
  while (ty > 1 && ty / 2 >= L->dim) ty /= 2;
  block = dim3(tx, ty, 1);
  P.tiles_i = (L->dim + tx - 1) / tx;
  P.tiles_j = (L->dim + ty - 1) / ty;
  // k chunk: as long as possible (plane reuse in registers) while still exposing ~16 workgroups per CU; on the
  // mid-size levels (<= 128^3) parallelism wins over reuse -- their planes are L2 resident anyway (measured:
  // 7.07 -> 5.70 ms per 256^3 F-cycle going from a 16-plane minimum to this rule)
  int kchunk = L->dim;
  const int min_kchunk = (int)knob(K_MIN_KCHUNK), want_blocks = (int)knob(K_WANT_BLOCKS);
  while (kchunk > min_kchunk && (long long)L->num_boxes * P.tiles_i * P.tiles_j * ((L->dim + kchunk - 1) / kchunk) < want_blocks) kchunk /= 2;
  if (tune_kchunk > 0 && L->dim >= tune_kchunk) kchunk = tune_kchunk;
  P.kchunk = kchunk;
  P.chunks_k = (L->dim + kchunk - 1) / kchunk;
  P.total_blocks = L->num_boxes * P.chunks_k * P.tiles_j * P.tiles_i;
  grid = grid_for(P.total_blocks, &P.per_xcd);
}

static int s27_tile_granule() { return knob(K_27PT_TILE32) ? 32 : 64; }      // smallest box side the tiled 27-point kernel takes
template <int MODE>
static int launch27(const hpgmg_hip_level *L, StencilArgs P, bool is_smoother) {
  HPGMG_SKIP_IF_REPLAY();
  if (L->num_boxes <= 0) return 0;
  if (MODE != MODE_BLACKBOX && !knob(K_27PT_DIRECT) && L->dim % s27_tile_granule() == 0 && P.xn_id != P.xout_id) {       // LDS-staged kernel (stencil27_tile.hpp)
    constexpr int TM = (MODE == MODE_BLACKBOX) ? MODE_APPLY : MODE;
    const bool narrow = (L->dim % 64 != 0);               // boxes of 32^3: 32 x 16 tiles
    const int TI = narrow ? 32 : 64, TJ = narrow ? 16 : 8;
    S27TileArgs A = {};
    A.xn_id = P.xn_id; A.xout_id = P.xout_id; A.rhs_id = P.rhs_id; A.mode = TM; A.a = P.a; A.b = P.b; A.h2inv = P.h2inv; A.c1 = P.c1; A.c2 = P.c2; A.sweep = P.sweep;
    A.ghost_free = (g_tile_ghost_free && L->box_nbr) ? 1 : 0;
    A.fused = g_tile_fused; g_tile_fused = TileFused{};
    A.tiles_i = L->dim / TI; A.tiles_j = L->dim / TJ;
    int kchunk = L->dim;
    while (kchunk > 32 && (long long)L->num_boxes * A.tiles_i * A.tiles_j * (L->dim / kchunk) < 8192) kchunk /= 2;   // measured at 512^3: 32-plane chunks 929 us, whole boxes 952
    const int tune_kc = (int)knob(K_27PT_KCHUNK);
    if (tune_kc > 0 && L->dim % tune_kc == 0) kchunk = tune_kc;
    A.kchunk = kchunk; A.chunks_k = (L->dim + kchunk - 1) / kchunk;
    A.total_blocks = L->num_boxes * A.chunks_k * A.tiles_j * A.tiles_i;
    g_tile_last_blocks = A.total_blocks;
    int tgrid = grid_for(A.total_blocks, &A.per_xcd);
    long long tcells = (long long)L->num_boxes * L->dim * L->dim * L->dim;
    const long long whole_cells = tcells;
    const bool first_part = g_tile_part == 1 && A.fused.kind == 0;
    if (g_tile_part && A.fused.kind == 0) {      // one part of the launch (hpgmg_hip_set_tile_part): part 1 = the tiles that read nothing of an image of another rank's box
      int count = 0;
      A.order = tile_part_order(L, A.tiles_i, A.tiles_j, A.chunks_k, g_tile_part, false, &tgrid, &A.per_xcd, &count);
      if (tgrid == 0) return 0;
      if (!A.order) return record_error(hipErrorOutOfMemory, "stencil27_tile: dispatch list of a partial launch");
      tcells = tcells * count / A.total_blocks;
    }
    const int tprof = is_smoother ? profile_begin(whole_cells) : -1;
    if (narrow) hipLaunchKernelGGL((stencil27_tile_kernel<TM, 16, 32>), dim3(tgrid), dim3(32, 16), 0, g_stream, *L, A);
    else        hipLaunchKernelGGL((stencil27_tile_kernel<TM, 8, 64>), dim3(tgrid), dim3(64, 8), 0, g_stream, *L, A);
    profile_end(tprof, tcells, first_part);
    HPGMG_LAUNCH_CHECK("stencil27_tile_kernel");
    return 0;
  }
  if (int e = refuse_unfused("fused residual form requested, but this level runs stencil27_kernel")) return e;
  dim3 block; int grid;
  plan(L, P, block, grid);
  const long long cells = (long long)L->num_boxes * L->dim * L->dim * L->dim;
  int prof = is_smoother ? profile_begin(cells) : -1;
  hipLaunchKernelGGL((stencil27_kernel<MODE>), dim3(grid), block, 0, g_stream, *L, P);
  profile_end(prof, cells);
  HPGMG_LAUNCH_CHECK("stencil27_kernel");
  return 0;
}

static int fv4_tile_granule() { return knob(K_FV4_TILE32) ? 32 : 64; }   // smallest box side the tiled fv4 kernel takes
// the LDS-tiled 4th-order kernel (fv4_tile.hpp): boxes whose side is a multiple of 32, out of place
template <int MODE, int TJ, int TI>
static int launch_fv4_tile_tj(const hpgmg_hip_level *L, int variant, const StencilArgs &S, bool is_smoother) {
  Fv4TileArgs P = {};
  P.xn_id = S.xn_id; P.xout_id = S.xout_id; P.rhs_id = S.rhs_id; P.a = S.a; P.b = S.b; P.h2inv = S.h2inv; P.c1 = S.c1; P.c2 = S.c2;
  P.sweep = S.sweep; P.copy_other_colour = S.copy_other_colour; P.ghost_free = (g_tile_ghost_free && L->box_nbr) ? 1 : 0;
  P.fused = g_tile_fused; g_tile_fused = TileFused{};
  P.tiles_i = L->dim / TI; P.tiles_j = L->dim / TJ;
  int kchunk = L->dim;                                   // enough workgroups to fill the chip, as few chunk prologues as possible
  const int want = (TJ * TI >= 1024) ? 512 : 1024;
  const int kc_min = (int)knob(K_FV4_KCHUNK_MIN);
  while (kchunk > kc_min && (long long)L->num_boxes * P.tiles_i * P.tiles_j * (L->dim / kchunk) < want) kchunk /= 2;
  const int tune_kc = (int)knob(K_FV4_KCHUNK);
  if (tune_kc > 0 && L->dim % tune_kc == 0) kchunk = tune_kc;
  P.kchunk = kchunk; P.chunks_k = (L->dim + kchunk - 1) / kchunk;
  P.total_blocks = L->num_boxes * P.chunks_k * P.tiles_j * P.tiles_i;
  g_tile_last_blocks = P.total_blocks;
  int grid = grid_for(P.total_blocks, &P.per_xcd);
  const size_t lds = (size_t)11 * (TI + 4) * (TJ + 4) * sizeof(double);
  long long cells = (long long)L->num_boxes * L->dim * L->dim * L->dim;
  const long long whole_cells = cells;
  const bool first_part = g_tile_part == 1 && P.fused.kind == 0;
  if (g_tile_part && P.fused.kind == 0) {        // one part of the launch (hpgmg_hip_set_tile_part): part 1 = the tiles that read nothing of an image of another rank's box
    int count = 0;
    P.order = tile_part_order(L, P.tiles_i, P.tiles_j, P.chunks_k, g_tile_part, false, &grid, &P.per_xcd, &count);
    if (grid == 0) return 0;
    if (!P.order) return record_error(hipErrorOutOfMemory, "fv4_tile: dispatch list of a partial launch");
    cells = cells * count / P.total_blocks;
  }
  const int prof = is_smoother ? profile_begin(whole_cells) : -1;
  int e = 0;
  if (!with_variant(kFv4Variants, variant, &e, [&](auto v) { return launch_lds<fv4_tile_kernel<v, MODE, TJ, TI>>(lds, dim3(grid), dim3(TI, TJ), lds, *L, P); })) return refuse_variant();
  if (e) return e;
  profile_end(prof, cells, first_part);
  HPGMG_LAUNCH_CHECK("fv4_tile_kernel");
  return 0;
}
// Tile height 8 (two workgroups per CU; 1.59 values loaded per cell and array) measured 1.85 ms per half sweep at 512^3, height 16 (one
// workgroup of 16 waves and 120 KB of LDS per CU; 1.33 values) 1.92 ms: the second resident workgroup hides more latency than the smaller
// halo saves.  Boxes of 32^3 (the 128^3 level of `7 64`): 32 x 16 tiles (a wave = two rows of 32 cells, still conflict free in LDS).
template <int MODE>
static int launch_fv4_tile(const hpgmg_hip_level *L, int variant, const StencilArgs &S, bool is_smoother) {
  if (L->dim % 64 != 0) return launch_fv4_tile_tj<MODE, 16, 32>(L, variant, S, is_smoother);
  if (knob(K_FV4_TJ) == 8) return launch_fv4_tile_tj<MODE, 8, 64>(L, variant, S, is_smoother);
  return launch_fv4_tile_tj<MODE, 16, 64>(L, variant, S, is_smoother);
}

template <int MODE>
static int launch_direct(const hpgmg_hip_level *L, int variant, StencilArgs P, bool is_smoother) {
  HPGMG_SKIP_IF_REPLAY();
  if (L->num_boxes <= 0) return 0;
  if (MODE != MODE_BLACKBOX && (variant == HPGMG_HIP_FV4_VC_HELMHOLTZ || variant == HPGMG_HIP_FV4_VC_POISSON)) {
    if (!knob(K_FV4_DIRECT) && L->dim % fv4_tile_granule() == 0 && L->ghosts >= 2 && P.xn_id != P.xout_id) return launch_fv4_tile<(MODE == MODE_BLACKBOX) ? MODE_APPLY : MODE>(L, variant, P, is_smoother);
  }
  if (int e = refuse_unfused("fused residual form requested, but this level runs stencil_direct_kernel")) return e;
  dim3 block; int grid;
  plan(L, P, block, grid);
  P.ghost_free = 0;
  if (MODE == MODE_GSRB) {                       // a lane owns two cells along i (see the kernel)
    P.tiles_i = ((L->dim + 1) / 2 + (int)block.x - 1) / (int)block.x;
    P.total_blocks = L->num_boxes * P.chunks_k * P.tiles_j * P.tiles_i;
    grid = grid_for(P.total_blocks, &P.per_xcd);
  }
  const long long cells = (long long)L->num_boxes * L->dim * L->dim * L->dim;
  int prof = is_smoother ? profile_begin(cells) : -1;
  int e = 0;
  if (!with_variant(kDirectVariants, variant, &e, [&](auto v) { hipLaunchKernelGGL((stencil_direct_kernel<v, MODE>), dim3(grid), block, 0, g_stream, *L, P); return 0; })) return refuse_variant();
  profile_end(prof, cells);
  HPGMG_LAUNCH_CHECK("stencil_direct_kernel");
  return 0;
}

template <int MODE>
static int launch(const hpgmg_hip_level *L, int variant, StencilArgs P, bool is_smoother) {
  HPGMG_SKIP_IF_REPLAY();
  if (L->num_boxes <= 0) return 0;
  if (variant == HPGMG_HIP_27PT_CC) return launch27<MODE>(L, P, is_smoother);
  if (variant == HPGMG_HIP_FV4_VC_HELMHOLTZ || variant == HPGMG_HIP_FV4_VC_POISSON) return launch_direct<MODE>(L, variant, P, is_smoother);
  if (int e = refuse_unfused("fused residual form requested for a variant without tiled kernels")) return e;
  dim3 block; int grid, e = 0;
  plan(L, P, block, grid);
  if (g_defer_mode) {
    if (!P.ghost_free || P.copy_other_colour || MODE == MODE_BLACKBOX) return record_error(hipErrorInvalidValue, "deferred stencil launch needs the ghost-free 7-point path");
    if (g_defer_mode == 2) {
      if (L->dim < 2) return record_error(hipErrorInvalidValue, "deferred stencil launch needs boxes of at least 2^3");
      dim3 sgrid((L->dim * L->dim + 255) / 256, L->num_boxes * 6);
      if (!with_variant(k7ptVariants, variant, &e, [&](auto v) { hipLaunchKernelGGL((stencil7_shell_kernel<v, MODE>), sgrid, dim3(256), 0, g_stream, *L, P); return 0; })) return refuse_variant();
      HPGMG_LAUNCH_CHECK("stencil7_shell_kernel");
      return 0;
    }
    P.defer = 1;
  }
  const long long cells = (long long)L->num_boxes * L->dim * L->dim * L->dim;
  int prof = is_smoother ? profile_begin(cells) : -1;
  // wide kernel: side a multiple of 128, 16-byte aligned interior rows (even strides; the box bases are checked by the host)
  if (g_fold_now.which && L->dim % 128 == 0) { return record_error(hipErrorInvalidValue, "folded interpolation: not in the wide kernel (hpgmg_hip_smooth_cheby_fold_supported)"); }
  if (!knob(K_NO_WIDE) && L->dim % 128 == 0 && L->jStride % 2 == 0 && L->kStride % 2 == 0 && L->volume % 2 == 0 && (L->flags & 1)) {
    const int wj = (int)knob(K_WIDE_WJ), tune_kc = (int)knob(K_KCHUNK);
    block = dim3(64, wj, 1);
    P.tiles_i = L->dim / 128; P.tiles_j = L->dim / (2 * wj);
    const int kchunk = tune_kc > 0 ? tune_kc : 16;
    P.kchunk = kchunk; P.chunks_k = (L->dim + kchunk - 1) / kchunk;
    P.total_blocks = L->num_boxes * P.chunks_k * P.tiles_j * P.tiles_i;
    grid = grid_for(P.total_blocks, &P.per_xcd);
    if (!with_variant(k7ptVariants, variant, &e, [&](auto v) {
          if (wj == 8) hipLaunchKernelGGL((stencil7_wide_kernel<v, MODE, 8>), dim3(grid), block, 0, g_stream, *L, P, FusedArgs{});
          else         hipLaunchKernelGGL((stencil7_wide_kernel<v, MODE, 4>), dim3(grid), block, 0, g_stream, *L, P, FusedArgs{});
          return 0; })) return refuse_variant();
    profile_end(prof, cells);
    HPGMG_LAUNCH_CHECK("stencil7_wide_kernel");
    return 0;
  }
  // boxes of side 64 m (the 128^3 level of config 2): LDS-staged tile kernel (stencil7_tile.hpp)
  const int tile7_kc = (int)knob(K_7PT_TILE_KCHUNK);
  if (!knob(K_7PT_NO_TILE) && !g_defer_mode && MODE != MODE_BLACKBOX && L->dim % 64 == 0) {
    constexpr int TJ = 8, TM = (MODE == MODE_BLACKBOX) ? MODE_APPLY : MODE;
    S7TileArgs A = {};
    A.xn_id = P.xn_id; A.xout_id = P.xout_id; A.rhs_id = P.rhs_id; A.a = P.a; A.b = P.b; A.h2inv = P.h2inv; A.c1 = P.c1; A.c2 = P.c2; A.sweep = P.sweep;
    A.ghost_free = P.ghost_free;
    A.tiles_i = L->dim / 64; A.tiles_j = L->dim / TJ;
    A.kchunk = (tile7_kc > 0 && L->dim % tile7_kc == 0) ? tile7_kc : 8; A.chunks_k = L->dim / A.kchunk;
    A.total_blocks = L->num_boxes * A.chunks_k * A.tiles_j * A.tiles_i;
    const int tgrid = grid_for(A.total_blocks, &A.per_xcd);
    if (MODE == MODE_CHEBY && g_fold_now.which) {
      const InterpFold F = g_fold_now;
      if (!P.ghost_free) return record_error(hipErrorInvalidValue, "folded interpolation needs the ghost-free path");
      if (!with_variant(k7ptVariants, variant, &e, [&](auto v) { hipLaunchKernelGGL((stencil7_tile_kernel<v, MODE_CHEBY, TJ, true>), dim3(tgrid), dim3(64, TJ), 0, g_stream, *L, A, F); return 0; })) return refuse_variant();
      profile_end(prof, cells);
      HPGMG_LAUNCH_CHECK("stencil7_tile_kernel (interpolation folded in)");
      return 0;
    }
    if (!with_variant(k7ptVariants, variant, &e, [&](auto v) { hipLaunchKernelGGL((stencil7_tile_kernel<v, TM, TJ>), dim3(tgrid), dim3(64, TJ), 0, g_stream, *L, A); return 0; })) return refuse_variant();
    profile_end(prof, cells);
    HPGMG_LAUNCH_CHECK("stencil7_tile_kernel");
    return 0;
  }
  if (MODE == MODE_CHEBY && g_fold_now.which) {
    const InterpFold F = g_fold_now;
    if (!P.ghost_free || P.defer) return record_error(hipErrorInvalidValue, "folded interpolation needs the ghost-free path with every box local");
    if (!with_variant(k7ptVariants, variant, &e, [&](auto v) { hipLaunchKernelGGL((stencil7_kernel<v, MODE_CHEBY, true>), dim3(grid), block, 0, g_stream, *L, P, F); return 0; })) return refuse_variant();
    profile_end(prof, cells);
    HPGMG_LAUNCH_CHECK("stencil7_kernel (interpolation folded in)");
    return 0;
  }
  if (!with_variant(k7ptVariants, variant, &e, [&](auto v) { hipLaunchKernelGGL((stencil7_kernel<v, MODE>), dim3(grid), block, 0, g_stream, *L, P); return 0; })) return refuse_variant();
  profile_end(prof, cells);
  HPGMG_LAUNCH_CHECK("stencil7_kernel");
  return 0;
}

// ---- fused forms of residual() on the bandwidth-bound fine level (stencil7_wide_kernel, ghost-free, every face local) ----
// residual + restriction + zero_vector on the launch-bound levels (boxes of an even side <= 32, every box local): stencil7_kernel<.., RR>
static int small_fused_ok(const hpgmg_hip_level *L, int variant) {
  if (variant != HPGMG_HIP_7PT_VC_HELMHOLTZ && variant != HPGMG_HIP_7PT_VC_POISSON && variant != HPGMG_HIP_7PT_CC) return 0;
  return knob(K_SMALL_RR) && L->num_boxes > 0 && g_ghost_free && L->box_nbr && !g_defer_mode && !g_tile_part && L->dim % 2 == 0 && (L->dim <= 32 || (L->dim % 64 == 0 && L->dim % 128 != 0));
}
static int launch_small_fused(const hpgmg_hip_level *L, int variant, StencilArgs P, FusedArgs FA, int extra_blocks) {
  dim3 block; int grid, e = 0;
  plan(L, P, block, grid);
  if (L->dim % 64 == 0) {      // boxes of 64^3 (config 2's 128^3 level): the LDS-staged tile kernel carries the form
    constexpr int TJ = 8;
    S7TileArgs A = {};
    A.xn_id = P.xn_id; A.xout_id = P.xout_id; A.rhs_id = P.rhs_id; A.a = P.a; A.b = P.b; A.h2inv = P.h2inv; A.ghost_free = 1;
    A.tiles_i = L->dim / 64; A.tiles_j = L->dim / TJ; A.kchunk = 8; A.chunks_k = L->dim / A.kchunk;
    A.total_blocks = L->num_boxes * A.chunks_k * A.tiles_j * A.tiles_i;
    const int tgrid = grid_for(A.total_blocks, &A.per_xcd) + extra_blocks;
    if (!with_variant(k7ptVariants, variant, &e, [&](auto v) { hipLaunchKernelGGL((stencil7_tile_kernel<v, MODE_RESIDUAL, TJ, false, true>), dim3(tgrid), dim3(64, TJ), 0, g_stream, *L, A, InterpFold{}, FA); return 0; })) return refuse_variant();
    HPGMG_LAUNCH_CHECK("stencil7_tile_kernel (residual + restriction + zero_vector)");
    return 0;
  }
  if (!P.ghost_free || block.x > 32) return record_error(hipErrorInvalidValue, "fused residual on a small level: ghost-free path, boxes of side <= 32");
  if (P.kchunk < 2 || (P.kchunk & 1)) {          // plane PAIRS stay inside a chunk
    P.kchunk = (P.kchunk < 2) ? 2 : P.kchunk + 1;
    P.chunks_k = (L->dim + P.kchunk - 1) / P.kchunk;
    P.total_blocks = L->num_boxes * P.chunks_k * P.tiles_j * P.tiles_i;
    grid = grid_for(P.total_blocks, &P.per_xcd);
  }
  grid += extra_blocks;
  if (!with_variant(k7ptVariants, variant, &e, [&](auto v) { hipLaunchKernelGGL((stencil7_kernel<v, MODE_RESIDUAL, false, true>), dim3(grid), block, 0, g_stream, *L, P, InterpFold{}, FA); return 0; })) return refuse_variant();
  HPGMG_LAUNCH_CHECK("stencil7_kernel (residual + restriction + zero_vector)");
  return 0;
}
static int wide_fused_ok(const hpgmg_hip_level *L, int variant) {
  if (variant != HPGMG_HIP_7PT_VC_HELMHOLTZ && variant != HPGMG_HIP_7PT_VC_POISSON && variant != HPGMG_HIP_7PT_CC) return 0;
  return L->num_boxes > 0 && g_ghost_free && L->box_nbr && !g_defer_mode && L->dim % 128 == 0 && L->jStride % 2 == 0 && L->kStride % 2 == 0 && L->volume % 2 == 0 && (L->flags & 1);
}
// ua: the caller vouched (hpgmg_hip_stencil_uniform_alpha) that alpha is F.alpha_uniform in every interior cell: the Helmholtz pass takes its UA twin
static long long g_wide_ua_launches = 0;
template <int MODE>
static int launch_wide_fused(const hpgmg_hip_level *L, int variant, StencilArgs P, FusedArgs F, int extra_blocks, bool ua) {
  constexpr int wj = 8;
  P.ghost_free = 1;
  P.tiles_i = L->dim / 128; P.tiles_j = L->dim / (2 * wj); P.kchunk = 16; P.chunks_k = (L->dim + 15) / 16;
  F.compute_blocks = L->num_boxes * P.chunks_k * P.tiles_j * P.tiles_i;
  P.total_blocks = F.compute_blocks;
  int grid = grid_for(P.total_blocks, &P.per_xcd);
  if (g_tile_part) {       // one part of the launch (faces on other ranks): part 1 = the tiles at no remote face, under the exchange; part 2 = the others, and the zeroing
    int count = 0;
    P.order = tile_part_order(L, P.tiles_i, P.tiles_j, P.chunks_k, g_tile_part, false, &grid, &P.per_xcd, &count);
    if (g_tile_part == 1) extra_blocks = 0;
    if (grid == 0 && extra_blocks == 0) return 0;
    if (grid > 0 && !P.order) return record_error(hipErrorOutOfMemory, "fused residual: dispatch list of a partial launch");
  }
  grid += extra_blocks;                                                      // the extra (zeroing) workgroups follow the stencil grid
  int e = 0;
  if (ua && variant == HPGMG_HIP_7PT_VC_HELMHOLTZ) {      // the one variant with a UA twin
    hipLaunchKernelGGL((stencil7_wide_kernel<HPGMG_HIP_7PT_VC_HELMHOLTZ, MODE, wj, true>), dim3(grid), dim3(64, wj), 0, g_stream, *L, P, F);
    if (g_tile_part != 1) g_wide_ua_launches++;
  } else if (!with_variant(k7ptVariants, variant, &e, [&](auto v) { hipLaunchKernelGGL((stencil7_wide_kernel<v, MODE, wj>), dim3(grid), dim3(64, wj), 0, g_stream, *L, P, F); return 0; })) return refuse_variant();
  HPGMG_LAUNCH_CHECK("stencil7_wide_kernel (fused residual)");
  return 0;
}
}  // namespace hpgmg
using namespace hpgmg;

extern "C" {

void hpgmg_hip_set_ghost_free(int on) { g_ghost_free = on; }
void hpgmg_hip_set_defer_mode(int mode) { g_defer_mode = mode; }
void hpgmg_hip_set_tile_ghost_free(int on) { g_tile_ghost_free = on; }
void hpgmg_hip_set_27pt_tile32(int on) { knob_set(K_27PT_TILE32, on ? 1 : 0); }
// would smooth / residual / apply_op of this variant run the LDS-tiled kernel on this level (out of place)?
int hpgmg_hip_tile_kernel_applies(const hpgmg_hip_level *L, int variant, int out_of_place) {
  if (L->num_boxes <= 0 || !out_of_place) return 0;
  if (variant == HPGMG_HIP_27PT_CC) return !knob(K_27PT_DIRECT) && L->dim % s27_tile_granule() == 0;
  if (variant == HPGMG_HIP_FV4_VC_HELMHOLTZ || variant == HPGMG_HIP_FV4_VC_POISSON) return !knob(K_FV4_DIRECT) && L->ghosts >= 2 && L->dim % fv4_tile_granule() == 0;
  return 0;
}
int hpgmg_hip_get_ghost_free(void) { return g_ghost_free; }

// the NEXT hpgmg_hip_smooth_cheby launch reads its operand with the piecewise-constant interpolation from (Lc, coarse_id) folded in (InterpFold)
int hpgmg_hip_smooth_cheby_fold_supported(const hpgmg_hip_level *L, int variant) {
  return (variant == HPGMG_HIP_7PT_VC_HELMHOLTZ || variant == HPGMG_HIP_7PT_VC_POISSON || variant == HPGMG_HIP_7PT_CC) && L->box_nbr && L->dim % 128 != 0 && L->dim % 2 == 0 && !g_defer_mode;
}
void hpgmg_hip_stencil_fold_interpolation(const hpgmg_hip_level *Lc, int coarse_id, const int *map, int which) {
  g_fold = InterpFold{}; if (Lc && which) { g_fold.which = which; g_fold.Lc = *Lc; g_fold.coarse_id = coarse_id; g_fold.map = map; }
}
int hpgmg_hip_smooth_cheby(const hpgmg_hip_level *L, int variant, int xn_id, int xnp1_id, int rhs_id,
                           double a, double b, double h2inv, double c1, double c2) {
  StencilArgs P = {}; P.xn_id = xn_id; P.xout_id = xnp1_id; P.rhs_id = rhs_id; P.a = a; P.b = b; P.h2inv = h2inv; P.c1 = c1; P.c2 = c2;
  g_fold_now = g_fold; g_fold = InterpFold{};            // a requested fold belongs to THIS call, also when the launch is skipped (graph replay)
  if (g_fold_now.which && variant != HPGMG_HIP_7PT_VC_HELMHOLTZ && variant != HPGMG_HIP_7PT_VC_POISSON && variant != HPGMG_HIP_7PT_CC) { g_fold_now = InterpFold{}; return record_error(hipErrorInvalidValue, "folded interpolation: 7-point variants only"); }
  const int e = launch<MODE_CHEBY>(L, variant, P, true);
  g_fold_now = InterpFold{};
  return e;
}
// One coloured GSRB half sweep (the colour of `sweep`): in place when xn_id == xnp1_id, else the other colour is copied across.
int hpgmg_hip_smooth_gsrb(const hpgmg_hip_level *L, int variant, int xn_id, int xnp1_id, int rhs_id,
                          double a, double b, double h2inv, int sweep) {
  StencilArgs P = {}; P.xn_id = xn_id; P.xout_id = xnp1_id; P.rhs_id = rhs_id; P.a = a; P.b = b; P.h2inv = h2inv; P.sweep = sweep;
  P.copy_other_colour = (xn_id != xnp1_id);
  return launch<MODE_GSRB>(L, variant, P, true);
}
// Both coloured half sweeps (sweep, sweep + 1; sweep even) of an out-of-place 27-point GSRB sweep in one pass (stencil27_rb.hpp):
// x_id -> out_id, the intermediate vector never stored.  Needs boxes of side 64 m, all of them local, apply_BCs_p2 done on x_id.
static long long g_rb27_launches = 0;
long long hpgmg_hip_rb27_launch_count(void) { return g_rb27_launches; }   // launches of the one-pass red + black kernel so far (tests)
int hpgmg_hip_smooth_gsrb27_rb_supported(const hpgmg_hip_level *L) {
  return !knob(K_27PT_NO_RB) && L->num_boxes > 0 && L->dim % 64 == 0 && L->box_nbr != nullptr && L->ghosts >= 1;
}
int hpgmg_hip_smooth_gsrb27_rb(const hpgmg_hip_level *L, int x_id, int out_id, int rhs_id, double a, double b, double h2inv, int sweep) {
  HPGMG_SKIP_IF_REPLAY();
  if (!hpgmg_hip_smooth_gsrb27_rb_supported(L) || x_id == out_id || (sweep & 1)) return record_error(hipErrorInvalidValue, "smooth_gsrb27_rb: level / arguments not supported");
  constexpr int TJ = 16;                                // rows of a tile; a lane owns two of them
  S27RbArgs A = {};
  A.xn_id = x_id; A.xout_id = out_id; A.rhs_id = rhs_id; A.a = a; A.b = b; A.h2inv = h2inv; A.sweep = sweep;
  A.tiles_i = L->dim / 64; A.tiles_j = L->dim / TJ;
  int kchunk = L->dim;
  // two workgroups fit a CU: 512 workgroups fill the chip, and every k chunk costs three extra planes of loads and a red stage more
  // (measured at 512^3: whole boxes 1.09 ms, chunks of 64 planes 1.19, of 32 planes 1.27)
  while (kchunk > 16 && (long long)L->num_boxes * A.tiles_i * A.tiles_j * (L->dim / kchunk) < 512) kchunk /= 2;
  const int tune_kc = (int)knob(K_27PT_RB_KCHUNK);
  if (tune_kc > 0 && L->dim % tune_kc == 0) kchunk = tune_kc;
  A.kchunk = kchunk; A.chunks_k = (L->dim + kchunk - 1) / kchunk;
  A.total_blocks = L->num_boxes * A.chunks_k * A.tiles_j * A.tiles_i;
  int grid = grid_for(A.total_blocks, &A.per_xcd);
  long long cells = (long long)L->num_boxes * L->dim * L->dim * L->dim;
  const long long whole_cells = cells;
  if (g_tile_part) {      // one part of the launch: part 1 = the tiles that read nothing of an image of another rank's box
    int count = 0;
    A.order = tile_part_order(L, A.tiles_i, A.tiles_j, A.chunks_k, g_tile_part, false, &grid, &A.per_xcd, &count);
    if (grid == 0) return 0;
    if (!A.order) return record_error(hipErrorOutOfMemory, "smooth_gsrb27_rb: dispatch list of a partial launch");
    cells = cells * count / A.total_blocks;
  }
  const int prof = profile_begin(whole_cells);
  hipLaunchKernelGGL((stencil27_rb_kernel<TJ>), dim3(grid), dim3(64, TJ / 2), 0, g_stream, *L, A);
  g_rb27_launches++;
  profile_end(prof, 2 * cells, g_tile_part == 1);     // one launch = two half sweeps over every cell
  HPGMG_LAUNCH_CHECK("stencil27_rb_kernel");
  return 0;
}
// The same on small levels: one workgroup per box of 2^3 ... 16^3 cells (stencil27_rb_box.hpp); forms the boundary ghost cells of x_id itself,
// so the caller runs neither exchange_boundary nor apply_BCs_p2.  Every box local.
// The largest box side it takes is a knob (K_27PT_RB_BOX_MAXDIM).
void hpgmg_hip_set_27pt_rb_box_maxdim(int dim) { knob_set(K_27PT_RB_BOX_MAXDIM, dim); }
int hpgmg_hip_smooth_gsrb27_rb_box_supported(const hpgmg_hip_level *L) {
  return !knob(K_27PT_NO_RB_BOX) && L->num_boxes > 0 && L->box_nbr != nullptr && L->ghosts >= 1 && L->dim <= knob(K_27PT_RB_BOX_MAXDIM) && (L->dim == 2 || L->dim == 4 || L->dim == 8 || L->dim == 16 || L->dim == 32);
}
int hpgmg_hip_smooth_gsrb27_rb_box(const hpgmg_hip_level *L, int x_id, int out_id, int rhs_id, double a, double b, double h2inv, int sweep) {
  HPGMG_SKIP_IF_REPLAY();
  if (!hpgmg_hip_smooth_gsrb27_rb_box_supported(L) || x_id == out_id || (sweep & 1)) return record_error(hipErrorInvalidValue, "smooth_gsrb27_rb_box: level / arguments not supported");
  S27RbBoxArgs A = {}; A.xn_id = x_id; A.xout_id = out_id; A.rhs_id = rhs_id; A.a = a; A.b = b; A.h2inv = h2inv; A.sweep = sweep;
  // cubes of 8^3 for boxes of 8^3 and more (a whole box of 16^3 in one workgroup measured 33 us, slower than the four launches it replaces)
  int e = 0;
  if (!with_variant<8, 4, 2>(L->dim >= 8 ? 8 : L->dim, &e, [&](auto side) {
        constexpr int DD = side, NTT = (DD == 8) ? 512 : (DD == 4) ? 256 : 64;
        A.cubes = L->dim / DD;
        const size_t lds = (size_t)((DD + 4) * (DD + 4) * (DD + 4) + (DD + 2) * (DD + 2) * (DD + 2)) * sizeof(double);
        hipLaunchKernelGGL((stencil27_rb_box_kernel<DD, NTT>), dim3(L->num_boxes * A.cubes * A.cubes * A.cubes), dim3(NTT), lds, g_stream, *L, A);
        return 0; })) return record_error(hipErrorInvalidValue, "smooth_gsrb27_rb_box: level / arguments not supported");
  g_rb27_launches++;
  HPGMG_LAUNCH_CHECK("stencil27_rb_box_kernel");
  return 0;
}
int hpgmg_hip_smooth_jacobi(const hpgmg_hip_level *L, int variant, int xn_id, int xnp1_id, int rhs_id,
                            double a, double b, double h2inv, double weight) {
  StencilArgs P = {}; P.xn_id = xn_id; P.xout_id = xnp1_id; P.rhs_id = rhs_id; P.a = a; P.b = b; P.h2inv = h2inv; P.c2 = weight;
  return launch<MODE_JACOBI>(L, variant, P, true);
}
int hpgmg_hip_blackbox_accumulate(const hpgmg_hip_level *L, int variant, int x_id, int Aii_id, int sumAbs_id, double a, double b, double h2inv) {
  StencilArgs P = {}; P.xn_id = x_id; P.xout_id = Aii_id; P.rhs_id = sumAbs_id; P.a = a; P.b = b; P.h2inv = h2inv;
  if (variant == HPGMG_HIP_27PT_CC) return launch27<MODE_BLACKBOX>(L, P, false);
  return launch_direct<MODE_BLACKBOX>(L, variant, P, false);
}
static bool tiled_variant(int variant) { return variant == HPGMG_HIP_27PT_CC || variant == HPGMG_HIP_FV4_VC_HELMHOLTZ || variant == HPGMG_HIP_FV4_VC_POISSON; }
int hpgmg_hip_residual_fused_supported(const hpgmg_hip_level *L, int variant) {
  if (tiled_variant(variant)) return hpgmg_hip_tile_kernel_applies(L, variant, 1) && L->dim % 2 == 0;   // the tiled kernels carry the fused forms (27-point, fv4)
  return wide_fused_ok(L, variant);
}
// residual + restriction + zero_vector only (not residual + norm): also the launch-bound levels of small boxes
int hpgmg_hip_residual_restrict_supported(const hpgmg_hip_level *L, int variant) {
  return hpgmg_hip_residual_fused_supported(L, variant) || (!tiled_variant(variant) && small_fused_ok(L, variant));
}
// The NEXT fused residual launch (hpgmg_hip_residual_restrict / _restrict_store / _norm; consumed by it, launched or not) may take alpha = value, the one bit pattern of every
// interior cell of the level, from its arguments: the wide Helmholtz pass then runs its UA twin.  Every other form of the launch ignores the request.
static int g_wide_ua_set = 0;
static double g_wide_ua_value = 0.0;
void hpgmg_hip_stencil_uniform_alpha(double value) { g_wide_ua_set = 1; g_wide_ua_value = value; }
long long hpgmg_hip_stencil_uniform_alpha_launches(void) { return g_wide_ua_launches; }
// residual (never stored) -> restriction into vector coarse_id of Lc, plus zero_vector(Lc, zero_id) when zero_id >= 0: the end of
// MGVCycle's down leg (mg.c:1150-1153) in one pass over the fine level.  map[4 b .. 4 b + 3] = coarse box and coarse (i, j, k) under fine box b's first cell.
int hpgmg_hip_residual_restrict_store(const hpgmg_hip_level *L, int variant, int res_id, int x_id, int rhs_id, double a, double b, double h2inv,
                                      const hpgmg_hip_level *Lc, int coarse_id, const int *map, int zero_id);
int hpgmg_hip_residual_restrict(const hpgmg_hip_level *L, int variant, int x_id, int rhs_id, double a, double b, double h2inv,
                                const hpgmg_hip_level *Lc, int coarse_id, const int *map, int zero_id) {
  return hpgmg_hip_residual_restrict_store(L, variant, -1, x_id, rhs_id, a, b, h2inv, Lc, coarse_id, map, zero_id);
}
// res_id >= 0 (7-point only): the residual is stored as residual() would store it as well
int hpgmg_hip_residual_restrict_store(const hpgmg_hip_level *L, int variant, int res_id, int x_id, int rhs_id, double a, double b, double h2inv,
                                      const hpgmg_hip_level *Lc, int coarse_id, const int *map, int zero_id) {
  const bool ua = (g_wide_ua_set != 0 && variant == HPGMG_HIP_7PT_VC_HELMHOLTZ);
  g_wide_ua_set = 0;
  HPGMG_SKIP_IF_REPLAY();
  if (tiled_variant(variant)) {
    if (!hpgmg_hip_residual_fused_supported(L, variant) || Lc->num_boxes <= 0 || res_id >= 0) return record_error(hipErrorInvalidValue, "residual_restrict: level not supported");
    g_tile_fused = TileFused{}; g_tile_fused.kind = 2; g_tile_fused.Lc = *Lc; g_tile_fused.coarse_id = coarse_id; g_tile_fused.map = map;
    StencilArgs T = {}; T.xn_id = x_id; T.xout_id = rhs_id; T.rhs_id = rhs_id; T.a = a; T.b = b; T.h2inv = h2inv;    // xout only has to differ from xn: nothing is stored
    if (int e = launch<MODE_RESIDUAL>(L, variant, T, false)) return e;
    return zero_id >= 0 ? hpgmg_hip_fill(Lc, zero_id, 0.0) : 0;
  }
  if ((!wide_fused_ok(L, variant) && !small_fused_ok(L, variant)) || Lc->num_boxes <= 0) return record_error(hipErrorInvalidValue, "residual_restrict: level not supported");
  if (res_id == x_id || res_id == rhs_id) return record_error(hipErrorInvalidValue, "residual_restrict: the residual may not overwrite its inputs");
  StencilArgs P = {}; P.xn_id = x_id; P.xout_id = (res_id >= 0) ? res_id : x_id; P.rhs_id = rhs_id; P.a = a; P.b = b; P.h2inv = h2inv;
  FusedArgs F = {}; F.Lc = *Lc; F.coarse_id = coarse_id; F.zero_id = zero_id; F.map = map; F.store_res = (res_id >= 0);
  F.zero_chunks_per_box = (Lc->volume + 4095) / 4096;
  if (ua) F.alpha_uniform = g_wide_ua_value;
  if (!wide_fused_ok(L, variant)) return launch_small_fused(L, variant, P, F, zero_id >= 0 ? F.zero_chunks_per_box * Lc->num_boxes : 0);
  return launch_wide_fused<MODE_RESIDUAL_RESTRICT>(L, variant, P, F, zero_id >= 0 ? F.zero_chunks_per_box * Lc->num_boxes : 0, ua);
}
// residual stored to res_id (not stored when res_id < 0) AND its max-abs: residual() + norm() of the convergence check (mg.c:1321-1323) in one pass
int hpgmg_hip_residual_norm(const hpgmg_hip_level *L, int variant, int res_id, int x_id, int rhs_id, double a, double b, double h2inv, double *norm_out) {
  const bool ua = (g_wide_ua_set != 0 && variant == HPGMG_HIP_7PT_VC_HELMHOLTZ);
  g_wide_ua_set = 0;
  if (int e = hpgmg_hip_graph_flush()) return e;
  *norm_out = 0.0;
  if (tiled_variant(variant)) {
    if (!hpgmg_hip_residual_fused_supported(L, variant) || res_id >= 0) return record_error(hipErrorInvalidValue, "residual_norm: level not supported (27-point / fv4: norm only, res_id < 0)");
    const long long cells = (long long)L->num_boxes * L->dim * L->dim * L->dim;
    double *part = reduction_scratch((int)(cells / 512 + 1024));      // one per workgroup: tiles of 512 cells, k chunks down to one plane (HPGMG_TUNE_*_KCHUNK)
    if (!part) return record_error(hipErrorOutOfMemory, "residual_norm: scratch");
    g_tile_fused = TileFused{}; g_tile_fused.kind = 1; g_tile_fused.partials = part;
    StencilArgs T = {}; T.xn_id = x_id; T.xout_id = rhs_id; T.rhs_id = rhs_id; T.a = a; T.b = b; T.h2inv = h2inv;
    if (int e = launch<MODE_RESIDUAL>(L, variant, T, false)) return e;
    return max_of_partials(g_tile_last_blocks, 0.0, norm_out);
  }
  if (!wide_fused_ok(L, variant)) return record_error(hipErrorInvalidValue, "residual_norm: level not supported");
  StencilArgs P = {}; P.xn_id = x_id; P.xout_id = res_id; P.rhs_id = rhs_id; P.a = a; P.b = b; P.h2inv = h2inv;
  const int blocks = L->num_boxes * ((L->dim + 15) / 16) * (L->dim / 16) * (L->dim / 128);
  FusedArgs F = {}; F.partials = reduction_scratch(blocks); F.no_store = (res_id < 0);
  if (res_id < 0) P.xout_id = x_id;
  if (!F.partials) return record_error(hipErrorOutOfMemory, "residual_norm: scratch");
  if (ua) F.alpha_uniform = g_wide_ua_value;
  if (int e = launch_wide_fused<MODE_RESIDUAL_NORM>(L, variant, P, F, 0, ua)) return e;
  if (g_tile_part == 1) return 0;                 // the first part of a two-part launch: the tiles of the second part have not written their maxima yet
  return max_of_partials(blocks, 0.0, norm_out);
}

int hpgmg_hip_residual(const hpgmg_hip_level *L, int variant, int res_id, int x_id, int rhs_id, double a, double b, double h2inv) {
  StencilArgs P = {}; P.xn_id = x_id; P.xout_id = res_id; P.rhs_id = rhs_id; P.a = a; P.b = b; P.h2inv = h2inv;
  if (rhs_id < 0) return launch<MODE_APPLY>(L, variant, P, false);
  return launch<MODE_RESIDUAL>(L, variant, P, false);
}

}  // extern "C"
