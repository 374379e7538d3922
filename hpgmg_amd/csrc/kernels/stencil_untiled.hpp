// stencil_untiled.hpp -- the two kernels that take any box size and stage nothing in LDS: stencil27_kernel (27-point) and stencil_direct_kernel
// (4th-order fv4, and the black-box probe of every 7-point / fv4 variant).  They run where the tiled kernels (stencil27_tile.hpp, fv4_tile.hpp)
// do not apply.  Included by stencil.hip only, which launches them.
#pragma once
#include "stencil_direct.hpp"

namespace hpgmg {

// ---------------------------------------------------------------------------------------------
// 27-point constant-coefficient operator (reference operators.27pt.c:48-51,60-91).
// One lane per (i,j) column marching in +k with the three 3x3 planes around the cell held in
// registers (27 values, 9 new loads per step instead of 27); streams: x, x_nm1, rhs, Dinv =
// 40 B per cell for Chebyshev.  The weighted partial sums are formed in the reference's order:
// ((C3*corners + C2*edges) + C1*faces) + C0*centre, each group summed left to right as listed.
// MODE_BLACKBOX is the probe of operators/rebuild.c:126-132 (out = Aii, rhs slot = sum|Aij|).
template <int MODE>
__global__ __launch_bounds__(256) void stencil27_kernel(const hpgmg_hip_level L, const StencilArgs P) {
  const int logical = xcd_logical_block((int)blockIdx.x, P.per_xcd);
  if (logical >= P.total_blocks) return;
  int t = logical;
  const int ti = t % P.tiles_i; t /= P.tiles_i;
  const int tj = t % P.tiles_j; t /= P.tiles_j;
  const int ck = t % P.chunks_k; t /= P.chunks_k;
  const int box = t;
  const int i = ti * (int)blockDim.x + (int)threadIdx.x;
  const int j = tj * (int)blockDim.y + (int)threadIdx.y;
  if (i >= L.dim || j >= L.dim) return;
  const int k0 = ck * P.kchunk, k1 = (k0 + P.kchunk < L.dim) ? k0 + P.kchunk : L.dim;
  const int jS = L.jStride, kS = L.kStride;
  constexpr bool kSmooth = (MODE == MODE_CHEBY || MODE == MODE_GSRB || MODE == MODE_JACOBI);

  const double *__restrict__ x = vec_origin(L, box, P.xn_id);      // 27-pt GSRB is always out of place
  double *__restrict__ out = vec_origin(L, box, P.xout_id);
  double *rhs = (MODE == MODE_APPLY) ? nullptr : vec_origin(L, box, P.rhs_id);   // BLACKBOX: the sum|Aij| accumulator
  const double *__restrict__ dinv = kSmooth ? vec_origin(L, box, VECTOR_DINV) : nullptr;
  int colour000 = 0;
  if (MODE == MODE_GSRB) colour000 = (L.box_low[3 * box] ^ L.box_low[3 * box + 1] ^ L.box_low[3 * box + 2] ^ P.sweep) & 1;

  int ijk = i + j * jS + k0 * kS;
  plane9 m = load_plane(x + ijk - kS, jS), c = load_plane(x + ijk, jS);
  for (int k = k0; k < k1; k++, ijk += kS) {
    const plane9 p = load_plane(x + ijk + kS, jS);
    const double xc = c.v[1][1];
    bool update = true;
    if (MODE == MODE_GSRB) update = (((i ^ j ^ k ^ colour000) & 1) == 0);
    if (update) {
      const double Ax = apply_op_27pt(m, c, p, P.a, P.b, P.h2inv);
      if (MODE == MODE_CHEBY)         { const double xnm1 = out[ijk]; out[ijk] = xc + P.c1 * (xc - xnm1) + P.c2 * dinv[ijk] * (rhs[ijk] - Ax); }
      else if (MODE == MODE_GSRB)     { out[ijk] = xc + dinv[ijk] * (rhs[ijk] - Ax); }
      else if (MODE == MODE_JACOBI)   { out[ijk] = xc + P.c2 * dinv[ijk] * (rhs[ijk] - Ax); }
      else if (MODE == MODE_RESIDUAL) { out[ijk] = rhs[ijk] - Ax; }
      else if (MODE == MODE_APPLY)    { out[ijk] = Ax; }
      else { out[ijk] += (xc) * Ax; rhs[ijk] += fabs((1.0 - xc) * Ax); }
    } else {
      out[ijk] = xc;   // out-of-place GSRB copies the other colour (gsrb.c:94-98)
    }
    m = c; c = p;
  }
}


// One lane per (i,j) column walking +k, every operand read through L1/L2 (apply_op_direct, stencil_direct.hpp).
template <int V, int MODE>
__global__ __launch_bounds__(256) void stencil_direct_kernel(const hpgmg_hip_level L, const StencilArgs P) {
  const int logical = xcd_logical_block((int)blockIdx.x, P.per_xcd);
  if (logical >= P.total_blocks) return;
  int t = logical;
  const int ti = t % P.tiles_i; t /= P.tiles_i;
  const int tj = t % P.tiles_j; t /= P.tiles_j;
  const int ck = t % P.chunks_k; t /= P.chunks_k;
  const int box = t;
  // GSRB: a lane owns the PAIR of cells (2 ip, 2 ip + 1) and sweeps whichever of the two has this half sweep's colour, so no
  // lane idles on the other colour (the launcher halves the tiles along i); every other mode: one cell per lane
  const int ip = ti * (int)blockDim.x + (int)threadIdx.x;
  const int i = (MODE == MODE_GSRB) ? 2 * ip : ip;
  const int j = tj * (int)blockDim.y + (int)threadIdx.y;
  if (i >= L.dim || j >= L.dim) return;
  const int k0 = ck * P.kchunk, k1 = (k0 + P.kchunk < L.dim) ? k0 + P.kchunk : L.dim;
  const int jS = L.jStride, kS = L.kStride;
  constexpr bool kSmooth = (MODE == MODE_CHEBY || MODE == MODE_GSRB || MODE == MODE_JACOBI);
  constexpr bool kVC = (V != HPGMG_HIP_7PT_CC);
  constexpr bool kHelm = (V == HPGMG_HIP_7PT_VC_HELMHOLTZ || V == HPGMG_HIP_FV4_VC_HELMHOLTZ);

  const double *x = vec_origin(L, box, P.xn_id);
  double *out = vec_origin(L, box, P.xout_id);           // in-place GSRB (fv2) aliases x
  double *rhs = (MODE == MODE_APPLY) ? nullptr : vec_origin(L, box, P.rhs_id);   // BLACKBOX: the sum|Aij| accumulator
  const double *dinv = kSmooth ? vec_origin(L, box, VECTOR_DINV) : nullptr;
  const double *alpha = kHelm ? vec_origin(L, box, VECTOR_ALPHA) : nullptr;
  const double *bi = kVC ? vec_origin(L, box, VECTOR_BETA_I) : nullptr;
  const double *bj = kVC ? vec_origin(L, box, VECTOR_BETA_J) : nullptr;
  const double *bk = kVC ? vec_origin(L, box, VECTOR_BETA_K) : nullptr;
  int colour000 = 0;
  if (MODE == MODE_GSRB) colour000 = (L.box_low[3 * box] ^ L.box_low[3 * box + 1] ^ L.box_low[3 * box + 2] ^ P.sweep) & 1;

  int row = j * jS + k0 * kS;                            // (0, j, k)
  for (int k = k0; k < k1; k++, row += kS) {
    if (MODE == MODE_GSRB) {
      const int sel = (j ^ k ^ colour000) & 1;             // cell i is swept when (i ^ j ^ k ^ colour000) is even: of the pair, the one with i & 1 == sel
      const int iu = i + sel, io = i + 1 - sel;
      if (iu < L.dim) {
        const int ijk = iu + row;
        const double xc = x[ijk];
        const double Ax = apply_op_direct<V>(x, alpha, bi, bj, bk, ijk, jS, kS, P.a, P.b, P.h2inv);
        out[ijk] = xc + dinv[ijk] * (rhs[ijk] - Ax);
      }
      if (P.copy_other_colour && io < L.dim) out[io + row] = x[io + row];
    } else {
      const int ijk = i + row;
      const double xc = x[ijk];
      const double Ax = apply_op_direct<V>(x, alpha, bi, bj, bk, ijk, jS, kS, P.a, P.b, P.h2inv);
      if (MODE == MODE_CHEBY)         { const double xnm1 = out[ijk]; out[ijk] = xc + P.c1 * (xc - xnm1) + P.c2 * dinv[ijk] * (rhs[ijk] - Ax); }
      else if (MODE == MODE_JACOBI)   { out[ijk] = xc + P.c2 * dinv[ijk] * (rhs[ijk] - Ax); }
      else if (MODE == MODE_RESIDUAL) { out[ijk] = rhs[ijk] - Ax; }
      else if (MODE == MODE_APPLY)    { out[ijk] = Ax; }
      else { out[ijk] += (xc) * Ax; rhs[ijk] += fabs((1.0 - xc) * Ax); }
    }
  }
}

}  // namespace hpgmg
