// stencil7.hpp -- the column-marching kernel of the 7-point operator for boxes of any size (stencil7_kernel: the mid-size, cache-resident levels and
// the launch-bound ones) and the kernel of the cells a deferred launch left out (stencil7_shell_kernel).  Included by stencil.hip only, which
// launches them; the arithmetic and its reference lines: stencil_math.hpp, stencil.hip's header.
#pragma once
#include "stencil_direct.hpp"

namespace hpgmg {

// One lane per (i,j) column, 64 lanes along the unit-stride i direction; the block marches in +k and keeps x[k-1], x[k], x[k+1] and beta_k[k],
// beta_k[k+1] in registers; the +-i / +-j neighbours of x are re-read through the vector L1.
// RR (MODE_RESIDUAL on the launch-bound levels, boxes of side <= 32): residual + restriction + zero_vector of MGVCycle's down leg (mg.c:1150-1153) in
// ONE launch -- a wave holds whole PAIRS of rows (blockDim.x <= 32), so the lane of an even (i, j) gathers its 2 x 2 patch of residuals from its
// neighbours' registers, sums it in restriction.c:54-57's order and carries the sum over the plane pair; the coarse zero_vector rides along as
// extra workgroups; the residual itself is stored only when asked for (FA.store_res: the exact state of the three operators).
template <int V, int MODE, bool IP = false, bool RR = false>
__global__ __launch_bounds__(256) void stencil7_kernel(const hpgmg_hip_level L, const StencilArgs P, const InterpFold F = InterpFold{}, const FusedArgs FA = FusedArgs{}) {
  if (RR && (int)blockIdx.x >= kXcds * P.per_xcd) {      // zero_vector(coarse, zero_id): whole padded boxes, ghosts included
    const int z = (int)blockIdx.x - kXcds * P.per_xcd, zbox = z / FA.zero_chunks_per_box, chunk = z - zbox * FA.zero_chunks_per_box;
    if (zbox >= FA.Lc.num_boxes) return;
    double *v = FA.Lc.box_base[zbox] + (size_t)FA.zero_id * (size_t)FA.Lc.volume;
    const int lo = chunk * 4096, hi = (lo + 4096 < FA.Lc.volume) ? lo + 4096 : FA.Lc.volume, nth = (int)(blockDim.x * blockDim.y);
    for (int q = lo + (int)(threadIdx.y * blockDim.x + threadIdx.x); q < hi; q += nth) v[q] = 0.0;
    return;
  }
  const int logical = xcd_logical_block((int)blockIdx.x, P.per_xcd);
  if (logical >= P.total_blocks) return;
  // logical id -> (box, k chunk, j tile, i tile), i fastest
  int t = logical;
  const int ti = t % P.tiles_i; t /= P.tiles_i;
  const int tj = t % P.tiles_j; t /= P.tiles_j;
  const int ck = t % P.chunks_k; t /= P.chunks_k;
  const int box = t;

  const int i = ti * (int)blockDim.x + (int)threadIdx.x;
  const int j = tj * (int)blockDim.y + (int)threadIdx.y;
  if (i >= L.dim || j >= L.dim) return;
  const int k0 = ck * P.kchunk;
  const int k1 = (k0 + P.kchunk < L.dim) ? k0 + P.kchunk : L.dim;
  const int jS = L.jStride, kS = L.kStride;

  constexpr bool kVC = (V != HPGMG_HIP_7PT_CC);
  constexpr bool kHelm = (V == HPGMG_HIP_7PT_VC_HELMHOLTZ);
  constexpr bool kSmooth = (MODE == MODE_CHEBY || MODE == MODE_GSRB || MODE == MODE_JACOBI);

  typename src_ptr<MODE == MODE_GSRB>::type x = vec_origin(L, box, P.xn_id);
  double *out = vec_origin(L, box, P.xout_id);   // may alias x (in-place GSRB): no __restrict__
  const double *__restrict__ rhs = (MODE == MODE_APPLY) ? nullptr : vec_origin(L, box, P.rhs_id);
  const double *__restrict__ dinv = kSmooth ? vec_origin(L, box, VECTOR_DINV) : nullptr;
  const double *__restrict__ alpha = kHelm ? vec_origin(L, box, VECTOR_ALPHA) : nullptr;
  const double *__restrict__ beta_i = kVC ? vec_origin(L, box, VECTOR_BETA_I) : nullptr;
  const double *__restrict__ beta_j = kVC ? vec_origin(L, box, VECTOR_BETA_J) : nullptr;
  const double *__restrict__ beta_k = kVC ? vec_origin(L, box, VECTOR_BETA_K) : nullptr;

  int colour000 = 0;
  if (MODE == MODE_GSRB) colour000 = (L.box_low[3 * box] ^ L.box_low[3 * box + 1] ^ L.box_low[3 * box + 2] ^ P.sweep) & 1;

  // Value of x just outside this box across face `dir` (0..5 = -i,+i,-j,+j,-k,+k): from the
  // neighbouring local box, from the Dirichlet condition (ghost = -centre), or from the ghost zone.
  const int last = L.dim - 1;
  auto outside = [&](int dir, int idx_in_neighbour, int idx_ghost, double centre) -> double {
    const int nb = L.box_nbr[6 * box + dir];
    if (nb >= 0) return vec_origin(L, nb, P.xn_id)[idx_in_neighbour];
    if (nb == -1) return -centre;
    return x[idx_ghost];
  };
  const bool gf = P.ghost_free != 0;
  // cells whose stencil reaches into a ghost zone another rank fills (box_nbr == -2)
  bool defer_ij = false, defer_klo = false, defer_khi = false;
  if (P.defer) {
    const int *nb = L.box_nbr + 6 * box;
    defer_ij = (i == 0 && nb[0] == -2) || (i == last && nb[1] == -2) || (j == 0 && nb[2] == -2) || (j == last && nb[3] == -2);
    defer_klo = (nb[4] == -2); defer_khi = (nb[5] == -2);
  }

  // IP, sweep 0 of a smooth() with the interpolation folded in: cell (ii, jj, kk) of box bx as stored + the coarse value above it; one step across a
  // face of the box lands in the neighbouring box (every box local) or on the Dirichlet rule applied to the folded centre
  const bool fold_x = IP && F.which == 1;
  auto folded = [&](int bx, int ii, int jj, int kk) -> double { return vec_origin(L, bx, P.xn_id)[ii + jj * jS + kk * kS] + fold_coarse(F, bx, ii, jj, kk); };
  auto folded_step = [&](int dir, int ii, int jj, int kk, double centre) -> double {      // (ii, jj, kk): one step outside this box across face dir
    const int nb = L.box_nbr[6 * box + dir];
    if (nb < 0) return -centre;
    if (dir == 0) ii = last; else if (dir == 1) ii = 0; else if (dir == 2) jj = last; else if (dir == 3) jj = 0; else if (dir == 4) kk = last; else kk = 0;
    return folded(nb, ii, jj, kk);
  };
  double *coarse = nullptr; double racc = 0.0;
  if (RR) {
    const int *m = FA.map + 4 * box;
    coarse = vec_origin(FA.Lc, m[0], FA.coarse_id) + (m[1] + (i >> 1)) + (m[2] + (j >> 1)) * FA.Lc.jStride + (m[3] + (k0 >> 1)) * FA.Lc.kStride;
  }
  int ijk = i + j * jS + k0 * kS;
  double xc = fold_x ? folded(box, i, j, k0) : x[ijk];
  double xm = fold_x ? (k0 == 0 ? folded_step(4, i, j, -1, xc) : folded(box, i, j, k0 - 1))
                     : ((gf && k0 == 0) ? outside(4, i + j * jS + last * kS, ijk - kS, xc) : x[ijk - kS]);
  double bk0 = kVC ? beta_k[ijk] : 0.0;

  for (int k = k0; k < k1; k++, ijk += kS) {
    const double xp = fold_x ? (k == last ? folded_step(5, i, j, k + 1, xc) : folded(box, i, j, k + 1))
                             : ((gf && k == last) ? outside(5, i + j * jS, ijk + kS, xc) : x[ijk + kS]);
    const double bk1 = kVC ? beta_k[ijk + kS] : 0.0;
    bool update = true;
    if (MODE == MODE_GSRB) update = (((i ^ j ^ k ^ colour000) & 1) == 0);
    if (P.defer && (defer_ij || (k == 0 && defer_klo) || (k == last && defer_khi))) update = false;
    if (update) {
      double xim, xip, xjm, xjp;
      if (fold_x) {
        xim = (i == 0)    ? folded_step(0, i - 1, j, k, xc) : folded(box, i - 1, j, k);
        xip = (i == last) ? folded_step(1, i + 1, j, k, xc) : folded(box, i + 1, j, k);
        xjm = (j == 0)    ? folded_step(2, i, j - 1, k, xc) : folded(box, i, j - 1, k);
        xjp = (j == last) ? folded_step(3, i, j + 1, k, xc) : folded(box, i, j + 1, k);
      } else {
        xim = (gf && i == 0)    ? outside(0, last + j * jS + k * kS, ijk - 1, xc)  : x[ijk - 1];
        xip = (gf && i == last) ? outside(1, j * jS + k * kS, ijk + 1, xc)          : x[ijk + 1];
        xjm = (gf && j == 0)    ? outside(2, i + last * jS + k * kS, ijk - jS, xc) : x[ijk - jS];
        xjp = (gf && j == last) ? outside(3, i + k * kS, ijk + jS, xc)              : x[ijk + jS];
      }
      double bi0 = 0.0, bi1 = 0.0, bj0 = 0.0, bj1 = 0.0, al = 0.0;
      if (kVC) { bi0 = beta_i[ijk]; bi1 = beta_i[ijk + 1]; bj0 = beta_j[ijk]; bj1 = beta_j[ijk + jS]; }
      if (kHelm) al = alpha[ijk];
      const double Ax = apply_op_7pt<V>(xc, xim, xip, xjm, xjp, xm, xp, bi0, bi1, bj0, bj1, bk0, bk1, al, P.a, P.b, P.h2inv);
      if (MODE == MODE_CHEBY) {
        double xnm1 = out[ijk];
        if (IP && F.which == 2) xnm1 = xnm1 + fold_coarse(F, box, i, j, k);
        out[ijk] = xc + P.c1 * (xc - xnm1) + P.c2 * dinv[ijk] * (rhs[ijk] - Ax);
      } else if (MODE == MODE_GSRB) {
        out[ijk] = xc + dinv[ijk] * (rhs[ijk] - Ax);
      } else if (MODE == MODE_JACOBI) {
        out[ijk] = xc + P.c2 * dinv[ijk] * (rhs[ijk] - Ax);
      } else if (MODE == MODE_RESIDUAL) {
        const double r = rhs[ijk] - Ax;
        if (!RR || FA.store_res) out[ijk] = r;
        if (RR) {      // the children (i, i+1) of rows j, j+1 of plane k, then of plane k+1; times 0.125 (restriction.c:54-57)
          const int w = (int)blockDim.x;
          const double r10 = __shfl_down(r, 1, 64), r01 = __shfl_down(r, w, 64), r11 = __shfl_down(r, w + 1, 64);
          if (((k - k0) & 1) == 0) { racc = r + r10; racc = racc + r01; racc = racc + r11; }
          else {
            racc = racc + r; racc = racc + r10; racc = racc + r01; racc = racc + r11;
            if (((i | j) & 1) == 0) coarse[((k - k0) >> 1) * FA.Lc.kStride] = racc * 0.125;
          }
        }
      } else {
        out[ijk] = Ax;
      }
    } else if (P.copy_other_colour) {
      out[ijk] = xc;
    }
    xm = xc; xc = xp; bk0 = bk1;
  }
}

// ---------------------------------------------------------------------------------------------
// The cells a deferred launch (StencilArgs.defer) skipped: one lane per cell of every box face whose neighbour
// box lives on another rank, run after that rank's ghost data has been unpacked.  A cell on an edge or corner
// shared by several such faces is computed by the lowest-numbered face only (in-place GSRB must not update twice).
template <int V, int MODE>
__global__ __launch_bounds__(256) void stencil7_shell_kernel(const hpgmg_hip_level L, const StencilArgs P) {
  const int box = blockIdx.y / 6, dir = blockIdx.y % 6;
  const int *nb = L.box_nbr + 6 * box;
  if (nb[dir] != -2) return;
  const int dim = L.dim, last = dim - 1, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= dim * dim) return;
  const int u = t % dim, v = t / dim, side = (dir & 1) ? last : 0;
  int i, j, k;
  if (dir < 2) { i = side; j = u; k = v; } else if (dir < 4) { j = side; i = u; k = v; } else { k = side; i = u; j = v; }
  const int on_face[6] = { i == 0, i == last, j == 0, j == last, k == 0, k == last };
  for (int d = 0; d < dir; d++) if (on_face[d] && nb[d] == -2) return;
  constexpr bool kVC = (V != HPGMG_HIP_7PT_CC);
  constexpr bool kHelm = (V == HPGMG_HIP_7PT_VC_HELMHOLTZ);
  const int jS = L.jStride, kS = L.kStride, ijk = i + j * jS + k * kS;
  if (MODE == MODE_GSRB) {
    const int colour000 = (L.box_low[3 * box] ^ L.box_low[3 * box + 1] ^ L.box_low[3 * box + 2] ^ P.sweep) & 1;
    if (((i ^ j ^ k ^ colour000) & 1) != 0) return;
  }
  const double *x = vec_origin(L, box, P.xn_id);
  double *out = vec_origin(L, box, P.xout_id);
  const double xc = x[ijk];
  auto outside = [&](int d, int idx_in_neighbour, int idx_ghost) -> double {
    const int n = nb[d];
    if (n >= 0) return vec_origin(L, n, P.xn_id)[idx_in_neighbour];
    if (n == -1) return -xc;
    return x[idx_ghost];
  };
  const bool gf = P.ghost_free != 0;
  const double xim = (gf && i == 0)    ? outside(0, last + j * jS + k * kS, ijk - 1)  : x[ijk - 1];
  const double xip = (gf && i == last) ? outside(1, j * jS + k * kS, ijk + 1)          : x[ijk + 1];
  const double xjm = (gf && j == 0)    ? outside(2, i + last * jS + k * kS, ijk - jS) : x[ijk - jS];
  const double xjp = (gf && j == last) ? outside(3, i + k * kS, ijk + jS)              : x[ijk + jS];
  const double xkm = (gf && k == 0)    ? outside(4, i + j * jS + last * kS, ijk - kS) : x[ijk - kS];
  const double xkp = (gf && k == last) ? outside(5, i + j * jS, ijk + kS)              : x[ijk + kS];
  double bi0 = 0, bi1 = 0, bj0 = 0, bj1 = 0, bk0 = 0, bk1 = 0, al = 0;
  if (kVC) {
    const double *bi = vec_origin(L, box, VECTOR_BETA_I), *bj = vec_origin(L, box, VECTOR_BETA_J), *bk = vec_origin(L, box, VECTOR_BETA_K);
    bi0 = bi[ijk]; bi1 = bi[ijk + 1]; bj0 = bj[ijk]; bj1 = bj[ijk + jS]; bk0 = bk[ijk]; bk1 = bk[ijk + kS];
  }
  if (kHelm) al = vec_origin(L, box, VECTOR_ALPHA)[ijk];
  const double Ax = apply_op_7pt<V>(xc, xim, xip, xjm, xjp, xkm, xkp, bi0, bi1, bj0, bj1, bk0, bk1, al, P.a, P.b, P.h2inv);
  if (MODE == MODE_APPLY) { out[ijk] = Ax; return; }
  const double rhs = vec_origin(L, box, P.rhs_id)[ijk];
  if (MODE == MODE_RESIDUAL) { out[ijk] = rhs - Ax; return; }
  const double dinv = vec_origin(L, box, VECTOR_DINV)[ijk];
  if (MODE == MODE_CHEBY)      { const double xnm1 = out[ijk]; out[ijk] = xc + P.c1 * (xc - xnm1) + P.c2 * dinv * (rhs - Ax); }
  else if (MODE == MODE_GSRB)  { out[ijk] = xc + dinv * (rhs - Ax); }
  else                         { out[ijk] = xc + P.c2 * dinv * (rhs - Ax); }
}

}  // namespace hpgmg
