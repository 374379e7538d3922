// stencil7_wide.hpp -- the single-sweep kernel of the 7-point operator on the bandwidth-bound fine levels (stencil7_wide_kernel) with its fused
// residual forms.  Included by stencil.hip only, which launches it.
#pragma once
#include "reduce.hpp"
#include "stencil_direct.hpp"

namespace hpgmg {

// ---------------------------------------------------------------------------------------------
// Wide kernel for boxes whose side is a multiple of 128 (the bandwidth-critical fine levels).
// Each lane owns a 2 (i) x 2 (j) patch: a wave covers two full 128-cell rows with 16-byte loads
// (1 KiB per wave-instruction, the coalescing sweet spot); a 64 x WJ workgroup covers 2*WJ rows
// and marches in +k.  Every cell of x is fetched from memory ONCE per workgroup:
//   * k neighbours: the plane k+1 loaded this step is the centre of the next (registers);
//   * j neighbours: the rows owned by the waves above / below come from an LDS copy of the plane
//     (each wave deposits the plane k+1 rows it just loaded; double buffered, one barrier per step);
//     only the two rows outside the workgroup's slab are read from memory;
//   * i neighbours: the neighbouring lane's registers (wave shuffle); lanes 0 / 63 sit on the tile edge.
// (Measured on MI355X: re-reading those neighbours through L1/L2, as the first version did, made the
// L2 miss traffic 10.1 streams per cell instead of 8.4 -- 32 KiB of L1 and 4 MiB of L2 per XCD do not
// hold a plane step of 128 resident workgroups.)
// Interior rows are 16-byte aligned because jStride and kStride are even and the first interior cell
// is 32-byte aligned (create_vectors); the launcher checks this and otherwise uses the generic kernel.
// GSRB: the two cells of a row always have different colours, so every lane updates exactly one
// cell per row (no idle lanes) and stores 8 bytes.
struct alignas(16) d2 { double x, y; };
__device__ __forceinline__ d2 ld2(const double *p) { return *reinterpret_cast<const d2 *>(p); }
__device__ __forceinline__ void st2(double *p, d2 v) { *reinterpret_cast<d2 *>(p) = v; }

// UA (the two fused residual forms of the Helmholtz operator): alpha is the one value F.alpha_uniform in every interior cell of the level, and is not read.
template <int V, int MODE, int WJ, bool UA = false>
__global__ __launch_bounds__(64 * WJ) void stencil7_wide_kernel(const hpgmg_hip_level L, const StencilArgs P, const FusedArgs F) {
  static_assert(!UA || (V == HPGMG_HIP_7PT_VC_HELMHOLTZ && (MODE == MODE_RESIDUAL_RESTRICT || MODE == MODE_RESIDUAL_NORM)), "no UA instance of this kind");
  __shared__ d2 slab[2][2 * WJ][64];                          // plane copy: [buffer][row of the slab][i pair]
  __shared__ double wg_max[WJ];
  // zero_vector(coarse, zero_id) -- whole padded boxes, ghosts included -- by the workgroups appended after the stencil grid (physical
  // order, so they spread over all XCDs instead of landing on the last ones)
  if (MODE == MODE_RESIDUAL_RESTRICT && (int)blockIdx.x >= kXcds * P.per_xcd) {
    const int z = (int)blockIdx.x - kXcds * P.per_xcd, zbox = z / F.zero_chunks_per_box, chunk = z - zbox * F.zero_chunks_per_box;
    if (zbox >= F.Lc.num_boxes) return;
    double *v = F.Lc.box_base[zbox] + (size_t)F.zero_id * (size_t)F.Lc.volume;
    const int lo = chunk * 4096, hi = (lo + 4096 < F.Lc.volume) ? lo + 4096 : F.Lc.volume;
    for (int q = lo + (int)(threadIdx.y * 64 + threadIdx.x); q < hi; q += 64 * WJ) v[q] = 0.0;
    return;
  }
  int logical = xcd_logical_block((int)blockIdx.x, P.per_xcd);
  if (P.order) logical = P.order[logical];
  if (logical >= P.total_blocks) return;
  int t = logical;
  const int ti = t % P.tiles_i; t /= P.tiles_i;
  const int tj = t % P.tiles_j; t /= P.tiles_j;
  const int ck = t % P.chunks_k; t /= P.chunks_k;
  const int box = t;

  const int lane = (int)threadIdx.x, ty = (int)threadIdx.y;
  const int i = ti * 128 + 2 * lane;                         // cells i, i+1
  const int ja = tj * (2 * WJ) + 2 * ty;                     // rows ja, ja+1
  const int k0 = ck * P.kchunk, k1 = (k0 + P.kchunk < L.dim) ? k0 + P.kchunk : L.dim;
  const int jS = L.jStride, kS = L.kStride, last = L.dim - 1;

  constexpr bool kVC = (V != HPGMG_HIP_7PT_CC);
  constexpr bool kHelm = (V == HPGMG_HIP_7PT_VC_HELMHOLTZ);
  constexpr bool kSmooth = (MODE == MODE_CHEBY || MODE == MODE_GSRB || MODE == MODE_JACOBI);
  constexpr bool kRestrict = (MODE == MODE_RESIDUAL_RESTRICT), kNorm = (MODE == MODE_RESIDUAL_NORM);

  typename src_ptr<MODE == MODE_GSRB>::type x = vec_origin(L, box, P.xn_id);
  double *out = ((kRestrict && !F.store_res) || (kNorm && F.no_store)) ? nullptr : vec_origin(L, box, P.xout_id);
  const double *__restrict__ rhs = (MODE == MODE_APPLY) ? nullptr : vec_origin(L, box, P.rhs_id);
  const double *__restrict__ dinv = kSmooth ? vec_origin(L, box, VECTOR_DINV) : nullptr;
  const double *__restrict__ alpha = (kHelm && !UA) ? vec_origin(L, box, VECTOR_ALPHA) : nullptr;
  const double *__restrict__ beta_i = kVC ? vec_origin(L, box, VECTOR_BETA_I) : nullptr;
  const double *__restrict__ beta_j = kVC ? vec_origin(L, box, VECTOR_BETA_J) : nullptr;
  const double *__restrict__ beta_k = kVC ? vec_origin(L, box, VECTOR_BETA_K) : nullptr;
  // fused forms: where this lane's 2 x 2 (x 2 planes) patch lands in the coarse level; running sum / maximum
  double *coarse = nullptr; double racc = 0.0, lane_max = 0.0;
  if (kRestrict) {
    const int *m = F.map + 4 * box;
    coarse = vec_origin(F.Lc, m[0], F.coarse_id) + (m[1] + (i >> 1)) + (m[2] + (ja >> 1)) * F.Lc.jStride + (m[3] + (k0 >> 1)) * F.Lc.kStride;
  }

  const bool gf = P.ghost_free != 0;
  // pair of values just outside this box across face `dir`, for the pair whose centres are `c`
  auto outside2 = [&](int dir, int idx_in_neighbour, int idx_ghost, d2 c) -> d2 {
    const int nb = L.box_nbr[6 * box + dir];
    if (nb >= 0) return ld2(vec_origin(L, nb, P.xn_id) + idx_in_neighbour);
    if (nb == -1) return d2{-c.x, -c.y};
    return ld2(x + idx_ghost);
  };
  auto outside1 = [&](int dir, int idx_in_neighbour, int idx_ghost, double c) -> double {
    const int nb = L.box_nbr[6 * box + dir];
    if (nb >= 0) return vec_origin(L, nb, P.xn_id)[idx_in_neighbour];
    if (nb == -1) return -c;
    return x[idx_ghost];
  };

  int colour000 = 0;
  if (MODE == MODE_GSRB) colour000 = (L.box_low[3 * box] ^ L.box_low[3 * box + 1] ^ L.box_low[3 * box + 2] ^ P.sweep) & 1;

  // cells next to a face another rank owns (P.defer): bit 0 = the pair's first cell, bit 1 = its second cell
  int dm_a = 0, dm_b = 0; bool defer_klo = false, defer_khi = false;
  if (P.defer) {
    const int *nb = L.box_nbr + 6 * box;
    const int di = ((i == 0 && nb[0] == -2) ? 1 : 0) | ((i + 1 == last && nb[1] == -2) ? 2 : 0);
    dm_a = (ja == 0 && nb[2] == -2) ? 3 : di;
    dm_b = (ja + 1 == last && nb[3] == -2) ? 3 : di;
    defer_klo = (nb[4] == -2); defer_khi = (nb[5] == -2);
  }

  int ia = i + ja * jS + k0 * kS;          // index of (i, ja, k); row b is ia + jS
  d2 xc_a = ld2(x + ia), xc_b = ld2(x + ia + jS);
  d2 xm_a = (gf && k0 == 0) ? outside2(4, i + ja * jS + last * kS, ia - kS, xc_a) : ld2(x + ia - kS);
  d2 xm_b = (gf && k0 == 0) ? outside2(4, i + (ja + 1) * jS + last * kS, ia + jS - kS, xc_b) : ld2(x + ia + jS - kS);
  d2 bk0_a = {0, 0}, bk0_b = {0, 0};
  if (kVC) { bk0_a = ld2(beta_k + ia); bk0_b = ld2(beta_k + ia + jS); }
  slab[k0 & 1][2 * ty][lane] = xc_a;
  slab[k0 & 1][2 * ty + 1][lane] = xc_b;
  __syncthreads();

  for (int k = k0; k < k1; k++, ia += kS) {
    const int ib = ia + jS;
    const d2 xp_a = (gf && k == last) ? outside2(5, i + ja * jS, ia + kS, xc_a) : ld2(x + ia + kS);
    const d2 xp_b = (gf && k == last) ? outside2(5, i + (ja + 1) * jS, ib + kS, xc_b) : ld2(x + ib + kS);
    d2 bk1_a = {0, 0}, bk1_b = {0, 0};
    if (kVC) { bk1_a = ld2(beta_k + ia + kS); bk1_b = ld2(beta_k + ib + kS); }
    // rows above and below the 2-row patch: the neighbouring wave's rows (LDS) or, at the slab edge, memory
    d2 xjm_a, xjp_b;
    if (ty > 0) xjm_a = slab[k & 1][2 * ty - 1][lane];
    else        xjm_a = (gf && ja == 0) ? outside2(2, i + last * jS + k * kS, ia - jS, xc_a) : ld2(x + ia - jS);
    if (ty < WJ - 1) xjp_b = slab[k & 1][2 * ty + 2][lane];
    else             xjp_b = (gf && ja + 1 == last) ? outside2(3, i + k * kS, ib + jS, xc_b) : ld2(x + ib + jS);
    // i neighbours of the pair: the cell left of .x and the cell right of .y live in the adjacent lanes
    double xl_a = __shfl_up(xc_a.y, 1, 64), xl_b = __shfl_up(xc_b.y, 1, 64);
    double xr_a = __shfl_down(xc_a.x, 1, 64), xr_b = __shfl_down(xc_b.x, 1, 64);
    if (lane == 0) {
      xl_a = (gf && i == 0) ? outside1(0, last + ja * jS + k * kS, ia - 1, xc_a.x)       : x[ia - 1];
      xl_b = (gf && i == 0) ? outside1(0, last + (ja + 1) * jS + k * kS, ib - 1, xc_b.x) : x[ib - 1];
    }
    if (lane == 63) {
      xr_a = (gf && i + 1 == last) ? outside1(1, ja * jS + k * kS, ia + 2, xc_a.y)       : x[ia + 2];
      xr_b = (gf && i + 1 == last) ? outside1(1, (ja + 1) * jS + k * kS, ib + 2, xc_b.y) : x[ib + 2];
    }
    // beta_j on the face between the two rows serves both (upper face of row a, lower face of row b)
    d2 bj_lo = {0, 0}, bj_mid = {0, 0}, bj_hi = {0, 0};
    if (kVC) { bj_lo = ld2(beta_j + ia); bj_mid = ld2(beta_j + ib); bj_hi = ld2(beta_j + ib + jS); }

    const bool defer_plane = P.defer && ((k == 0 && defer_klo) || (k == last && defer_khi));
#define HPGMG_ROW(IDX, XC, XM, XP, XJM, XJP, XL, XR, BK0, BK1, BJL, BJH, JROW, DM)                                          \
    {                                                                                                                        \
      const int dm = defer_plane ? 3 : DM;                                                                                   \
      d2 bi = {0, 0}, al = {0, 0}; double bir = 0;                                                                           \
      if (kVC) { bi = ld2(beta_i + IDX); bir = __shfl_down(bi.x, 1, 64); if (lane == 63) bir = beta_i[IDX + 2]; }            \
      if (kHelm) { if (UA) al = d2{F.alpha_uniform, F.alpha_uniform}; else al = ld2(alpha + IDX); }                         \
      if (MODE == MODE_GSRB) {                                                                                              \
        const int pp = (JROW ^ k ^ colour000) & 1;              /* the cell of this pair whose colour is swept */           \
        const double c = pp ? XC.y : XC.x;                                                                                  \
        const double Ax = apply_op_7pt<V>(c, pp ? XC.x : XL, pp ? XR : XC.y, pp ? XJM.y : XJM.x, pp ? XJP.y : XJP.x,        \
                                          pp ? XM.y : XM.x, pp ? XP.y : XP.x, pp ? bi.y : bi.x, pp ? bir : bi.y,            \
                                          pp ? BJL.y : BJL.x, pp ? BJH.y : BJH.x, pp ? BK0.y : BK0.x, pp ? BK1.y : BK1.x,   \
                                          pp ? al.y : al.x, P.a, P.b, P.h2inv);                                             \
        const d2 r2 = ld2(rhs + IDX), dv = ld2(dinv + IDX);                                                                 \
        const double xn = c + (pp ? dv.y : dv.x) * ((pp ? r2.y : r2.x) - Ax);                                              \
        if (P.copy_other_colour) st2(out + IDX, pp ? d2{XC.x, xn} : d2{xn, XC.y}); else if (!((dm >> pp) & 1)) out[IDX + pp] = xn; \
      } else {                                                                                                              \
        const double Ax0 = apply_op_7pt<V>(XC.x, XL, XC.y, XJM.x, XJP.x, XM.x, XP.x, bi.x, bi.y, BJL.x, BJH.x, BK0.x, BK1.x, al.x, P.a, P.b, P.h2inv); \
        const double Ax1 = apply_op_7pt<V>(XC.y, XC.x, XR, XJM.y, XJP.y, XM.y, XP.y, bi.y, bir, BJL.y, BJH.y, BK0.y, BK1.y, al.y, P.a, P.b, P.h2inv);  \
        d2 o;                                                                                                               \
        if (MODE == MODE_APPLY) { o.x = Ax0; o.y = Ax1; }                                                                   \
        else {                                                                                                              \
          const d2 r2 = ld2(rhs + IDX);                                                                                     \
          if (MODE == MODE_RESIDUAL || kRestrict || kNorm) { o.x = r2.x - Ax0; o.y = r2.y - Ax1; }                          \
          else {                                                                                                            \
            const d2 dv = ld2(dinv + IDX);                                                                                  \
            if (MODE == MODE_CHEBY) {                                                                                       \
              const d2 old = ld2(out + IDX);                                                                                \
              o.x = XC.x + P.c1 * (XC.x - old.x) + P.c2 * dv.x * (r2.x - Ax0);                                              \
              o.y = XC.y + P.c1 * (XC.y - old.y) + P.c2 * dv.y * (r2.y - Ax1);                                              \
            } else {                                                                                                        \
              o.x = XC.x + P.c2 * dv.x * (r2.x - Ax0);                                                                      \
              o.y = XC.y + P.c2 * dv.y * (r2.y - Ax1);                                                                      \
            }                                                                                                               \
          }                                                                                                                 \
        }                                                                                                                   \
        RES = o;                                                                                                            \
        if ((kRestrict && !F.store_res) || (kNorm && F.no_store)) { }                                                       \
        else if (dm == 0) st2(out + IDX, o);                                                                                \
        else { if (!(dm & 1)) out[IDX] = o.x; if (!(dm & 2)) out[IDX + 1] = o.y; }                                          \
      }                                                                                                                     \
    }
    d2 res_a = {0, 0}, res_b = {0, 0};
#define RES res_a
    HPGMG_ROW(ia, xc_a, xm_a, xp_a, xjm_a, xc_b, xl_a, xr_a, bk0_a, bk1_a, bj_lo, bj_mid, ja, dm_a)
#undef RES
#define RES res_b
    HPGMG_ROW(ib, xc_b, xm_b, xp_b, xc_a, xjp_b, xl_b, xr_b, bk0_b, bk1_b, bj_mid, bj_hi, (ja + 1), dm_b)
#undef RES
#undef HPGMG_ROW
    if (kRestrict) {      // restriction.c:54-57: the eight children in the order (i, i+1) of rows j, j+1 of plane k, then of plane k+1; times 0.125
      if (((k - k0) & 1) == 0) { racc = res_a.x + res_a.y; racc = racc + res_b.x; racc = racc + res_b.y; }
      else {
        racc = racc + res_a.x; racc = racc + res_a.y; racc = racc + res_b.x; racc = racc + res_b.y;
        coarse[((k - k0) >> 1) * F.Lc.kStride] = racc * 0.125;
      }
    }
    if (kNorm) {
      double f;
      f = fabs(res_a.x); lane_max = (f > lane_max) ? f : lane_max;  f = fabs(res_a.y); lane_max = (f > lane_max) ? f : lane_max;
      f = fabs(res_b.x); lane_max = (f > lane_max) ? f : lane_max;  f = fabs(res_b.y); lane_max = (f > lane_max) ? f : lane_max;
    }
    // hand the plane k+1 rows to the neighbouring waves for the next step
    slab[(k + 1) & 1][2 * ty][lane] = xp_a;
    slab[(k + 1) & 1][2 * ty + 1][lane] = xp_b;
    __syncthreads();
    xm_a = xc_a; xc_a = xp_a; bk0_a = bk1_a;
    xm_b = xc_b; xc_b = xp_b; bk0_b = bk1_b;
  }
  if (kNorm) {                                                 // a maximum is exact under any order (misc.c:307-317)
    const int tid = 64 * ty + lane;
    lane_max = block_max<WJ>(lane_max, wg_max, tid);
    if (tid == 0) F.partials[logical] = lane_max;
  }
}

}  // namespace hpgmg
