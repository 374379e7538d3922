// dense_boundary.hip -- inhomogeneous Dirichlet values of the dense-array API (include/hpgmg_operators.h hpgmg_dense_pack_lifted,
// hpgmg_boundary_flux / _restrict / _lift / _interp, their per-face-kind forms for Neumann walls and the Robin forms of those, with
// hpgmg_boundary_check_kappa / _store_walls; the formulas and their order are written there and in DESIGN.md §11.1, §11.2, §11.5).  The arithmetic the host defaults (host/hooks_host.inc) must match bit for bit is not written here but in
// include/hpgmg_boundary_math.h, which both compile.
//
// A boundary array is 6 x n x n doubles (n = the level's cells per side, a cube): [0], [1] i-low / i-high indexed [k][j], [2], [3] j-low /
// j-high [k][i], [4], [5] k-low / k-high [j][i].  w = (2.0 * b) * (1.0 / (h * h)) comes from the host, so every term (w * beta) * g has the
// host default's bits (-ffp-contract=off).
//
// Lifted pack: dense_pack_kernel's single pass over every double of every padded box (grid row y = box, 32-bit offsets inside it,
// consecutive lanes on consecutive doubles), plus T(c) on the interior cells that lie on a domain face, read from the box's own beta
// vectors and g; f and the g values read are validated into the same device word.
// Face kernels (flux, lift, interp): grid row y = box, x over the 6 dim^2 face positions of the box; a position on a box face that is not
// a domain face does nothing.  A cell on several domain faces (edge, corner) is handled once, by the position of the first face it touches
// in the order i-low .. k-high, so no two lanes write one cell.  One launch per level and operation; they are launch bound (6 n^2 cells).
#include "reduce.hpp"
#include "hpgmg_boundary_math.h"

namespace hpgmg {

constexpr int kBndThreads = 256;

// offset, from a cell's padded offset, of its beta on face `face`, and the vector holding it
__device__ __forceinline__ int bnd_beta_vec(int face) { return face < 2 ? VECTOR_BETA_I : face < 4 ? VECTOR_BETA_J : VECTOR_BETA_K; }
__device__ __forceinline__ int bnd_beta_step(const hpgmg_hip_level &L, int face) {
  return !(face & 1) ? 0 : face == 1 ? 1 : face == 3 ? L.jStride : L.kStride;
}

// the face position t of a box: local cell (i, j, k) and whether it is on a domain face and owned (first face it touches)
struct FacePos { int face, i, j, k; bool on; };
__device__ __forceinline__ FacePos bnd_face_pos(const hpgmg_hip_level &L, int li, int lj, int lk, int t) {
  const int dim = L.dim, n = L.dim_i, plane = dim * dim;
  FacePos P;
  P.face = t / plane;
  const int r = t - P.face * plane, q = r / dim, p = r - q * dim, side = (P.face & 1) ? dim - 1 : 0;
  if (P.face < 2) { P.i = side; P.j = p; P.k = q; }
  else if (P.face < 4) { P.i = p; P.j = side; P.k = q; }
  else { P.i = p; P.j = q; P.k = side; }
  const int gi = li + P.i, gj = lj + P.j, gk = lk + P.k;
  P.on = bnd_touches(n, P.face, gi, gj, gk);
  for (int f = 0; f < P.face; f++) P.on = P.on && !bnd_touches(n, f, gi, gj, gk);
  return P;
}

// mask, wall, wn (lifted pack and flux): bit f of mask set = face f is a Neumann wall, whose entry is (wn * wall[e]) * gn with
// wn = b * (1.0 / h) from the host and wall the level's wall-beta array; mask 0 leaves every expression as it was.
// ROBIN, kappa, h (the Robin forms): the level's kappa array and h; a masked face's entry is then bnd_wall_phi's.  The forms
// without a kappa array are instantiations of their own, so that they stay the code they were.
template <bool ROBIN>
__global__ __launch_bounds__(kBndThreads) void dense_pack_lifted_kernel(const hpgmg_hip_level L, int id, const double *__restrict__ src,
                                                                        const double *__restrict__ g, double w, int mask,
                                                                        const double *__restrict__ wall, double wn,
                                                                        const double *__restrict__ kappa, double h, int *flag) {
  const int gh = L.ghosts, dim = L.dim, n = L.dim_i;
  int bits = 0;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    double *dst = L.box_base[box] + (size_t)id * L.volume;
    const double *bi = L.box_base[box] + (size_t)VECTOR_BETA_I * L.volume, *bj = L.box_base[box] + (size_t)VECTOR_BETA_J * L.volume;
    const double *bk = L.box_base[box] + (size_t)VECTOR_BETA_K * L.volume;
    for (int ofs = (int)(blockIdx.x * kBndThreads + threadIdx.x); ofs < L.volume; ofs += (int)(gridDim.x * kBndThreads)) {
      const int pk = ofs / L.kStride, pj = (ofs - pk * L.kStride) / L.jStride, pi = ofs - pk * L.kStride - pj * L.jStride;
      const int i = pi - gh, j = pj - gh, k = pk - gh;
      double v = 0.0;
      if (i >= 0 && i < dim && j >= 0 && j < dim && k >= 0 && k < dim) {
        const int gi = li + i, gj = lj + j, gk = lk + k;
        v = src[((size_t)gk * n + gj) * n + gi];
        if (!isfinite(v)) bits |= HPGMG_DENSE_NOT_FINITE;
        if (gi == 0 || gj == 0 || gk == 0 || gi == n - 1 || gj == n - 1 || gk == n - 1) {
          double T = 0.0;
          for (int face = 0; face < 6; face++) if (bnd_touches(n, face, gi, gj, gk)) {
            const int e = bnd_entry(n, face, gi, gj, gk);
            const double gv = g[e];
            if (!isfinite(gv)) bits |= HPGMG_DENSE_NOT_FINITE;
            const double *beta = face < 2 ? bi : face < 4 ? bj : bk;
            if ((mask >> face) & 1) T = T + (ROBIN ? bnd_wall_phi(wn, wall[e], gv, kappa[e], h) : (wn * wall[e]) * gv);
            else T = T + (w * beta[ofs + bnd_beta_step(L, face)]) * gv;
          }
          v = v + T;
        }
      }
      dst[ofs] = v;
    }
  }
  if (bits) atomicOr(flag, bits);
}

template <bool ROBIN>
__global__ __launch_bounds__(kBndThreads) void boundary_flux_kernel(const hpgmg_hip_level L, double *__restrict__ phi,
                                                                    const double *__restrict__ g, double w, int mask,
                                                                    const double *__restrict__ wall, double wn,
                                                                    const double *__restrict__ kappa, double h, int *flag) {
  const int n = L.dim_i, positions = 6 * L.dim * L.dim;
  int bits = 0;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    for (int t = (int)(blockIdx.x * kBndThreads + threadIdx.x); t < positions; t += (int)(gridDim.x * kBndThreads)) {
      const int face = t / (L.dim * L.dim);
      const int r = t - face * L.dim * L.dim, q = r / L.dim, p = r - q * L.dim, side = (face & 1) ? L.dim - 1 : 0;
      const int i = face < 2 ? side : p, j = face < 2 ? p : face < 4 ? side : q, k = face < 4 ? q : side;
      const int gi = li + i, gj = lj + j, gk = lk + k;
      if (!bnd_touches(n, face, gi, gj, gk)) continue;          // this box face is not a domain face: every entry has one box face that is
      const int e = bnd_entry(n, face, gi, gj, gk);
      const double gv = g[e];
      if (!isfinite(gv)) bits |= HPGMG_DENSE_NOT_FINITE;
      if ((mask >> face) & 1) { phi[e] = ROBIN ? bnd_wall_phi(wn, wall[e], gv, kappa[e], h) : (wn * wall[e]) * gv; continue; }
      const double beta = vec_origin(L, box, bnd_beta_vec(face))[i + j * L.jStride + k * L.kStride + bnd_beta_step(L, face)];
      phi[e] = (w * beta) * gv;
    }
  }
  if (bits) atomicOr(flag, bits);
}

// hpgmg_boundary_check_kappa: one lane per entry of the 6 n^2 array, its bits (bnd_kappa_bits) into the device word
__global__ __launch_bounds__(kBndThreads) void boundary_check_kappa_kernel(const double *__restrict__ kappa, int n, int robin_mask, int *flag) {
  const int total = 6 * n * n;
  int bits = 0;
  for (int e = (int)(blockIdx.x * kBndThreads + threadIdx.x); e < total; e += (int)(gridDim.x * kBndThreads)) bits |= bnd_kappa_bits(n, robin_mask, e, kappa[e]);
  if (bits) atomicOr(flag, bits);
}

// hpgmg_boundary_store_walls: the flux kernel's mapping (grid row y = box, x over its 6 dim^2 face positions, consecutive lanes on consecutive
// entries of a face).  A position on a masked domain face writes that face's beta of its cell -- index 0 of a box on a low wall, the high ghost
// layer dim of a box on a high wall -- from the entry of wall and kappa it alone owns; every other position, and a box on no wall, does nothing.
__global__ __launch_bounds__(kBndThreads) void boundary_store_walls_kernel(const hpgmg_hip_level L, const double *__restrict__ wall,
                                                                           const double *__restrict__ kappa, double h, int mask) {
  const int n = L.dim_i, positions = 6 * L.dim * L.dim;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    for (int t = (int)(blockIdx.x * kBndThreads + threadIdx.x); t < positions; t += (int)(gridDim.x * kBndThreads)) {
      const int face = t / (L.dim * L.dim);
      const int r = t - face * L.dim * L.dim, q = r / L.dim, p = r - q * L.dim, side = (face & 1) ? L.dim - 1 : 0;
      const int i = face < 2 ? side : p, j = face < 2 ? p : face < 4 ? side : q, k = face < 4 ? q : side;
      const int gi = li + i, gj = lj + j, gk = lk + k;
      if (!((mask >> face) & 1) || !bnd_touches(n, face, gi, gj, gk)) continue;
      const int e = bnd_entry(n, face, gi, gj, gk);
      vec_origin(L, box, bnd_beta_vec(face))[i + j * L.jStride + k * L.kStride + bnd_beta_step(L, face)] = bnd_wall_beta(wall[e], kappa ? kappa[e] : 0.0, h);
    }
  }
}

__global__ __launch_bounds__(kBndThreads) void boundary_restrict_kernel(double *__restrict__ gc, const double *__restrict__ gf, int nc) {
  const int nf = 2 * nc, total = 6 * nc * nc;
  for (int e = (int)(blockIdx.x * kBndThreads + threadIdx.x); e < total; e += (int)(gridDim.x * kBndThreads)) {
    const int face = e / (nc * nc), r = e - face * nc * nc, q = r / nc, p = r - q * nc;
    const double *s = gf + (face * nf + 2 * q) * nf + 2 * p;
    gc[e] = (s[0] + s[1] + s[nf] + s[nf + 1]) * 0.25;
  }
}

__global__ __launch_bounds__(kBndThreads) void boundary_lift_kernel(const hpgmg_hip_level L, int id, const double *__restrict__ phi,
                                                                    const double *__restrict__ phi_fine, double sign) {
  const int n = L.dim_i, positions = 6 * L.dim * L.dim;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    double *v = vec_origin(L, box, id);
    for (int t = (int)(blockIdx.x * kBndThreads + threadIdx.x); t < positions; t += (int)(gridDim.x * kBndThreads)) {
      const FacePos P = bnd_face_pos(L, li, lj, lk, t);
      if (!P.on) continue;
      const int gi = li + P.i, gj = lj + P.j, gk = lk + P.k;
      double T = 0.0;
      for (int face = 0; face < 6; face++) if (bnd_touches(n, face, gi, gj, gk)) T = T + phi[bnd_entry(n, face, gi, gj, gk)];
      if (phi_fine) T = T - 0.125 * bnd_fine_sum(n, phi_fine, gi, gj, gk);
      const int c = P.i + P.j * L.jStride + P.k * L.kStride;
      v[c] = v[c] + sign * T;
    }
  }
}

// every ghost lies between Dirichlet walls: bnd_ghost_delta, which bnd_ghost_faces gives under mask 0 too
__global__ __launch_bounds__(kBndThreads) void boundary_interp_kernel(const hpgmg_hip_level L, int id, const double *__restrict__ gc, int nc) {
  const int positions = 6 * L.dim * L.dim;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    double *v = vec_origin(L, box, id);
    for (int t = (int)(blockIdx.x * kBndThreads + threadIdx.x); t < positions; t += (int)(gridDim.x * kBndThreads)) {
      const FacePos P = bnd_face_pos(L, li, lj, lk, t);
      if (!P.on) continue;
      const int gi = li + P.i, gj = lj + P.j, gk = lk + P.k;
      const bnd_p1_cell F = bnd_p1_of(gi, gj, gk);
      double D = 0.0, w;
      int q[3];
#pragma unroll
      for (int s = 1; s < 8; s++) if (bnd_p1_ghost(nc, F, s, q, &w)) D = D + w * bnd_ghost_delta(nc, gc, q[0], q[1], q[2]);
      const int c = P.i + P.j * L.jStride + P.k * L.kStride;
      v[c] = v[c] + D;
    }
  }
}

// the coarse iterate at the in-range cell (i, j, k): read in the box that owns it.  nb > 0: the boxes are in i-fastest order, nb per side
// (checked by the host); else the owner is searched for.
__device__ __forceinline__ double bnd_coarse_cell(const hpgmg_hip_level &Lc, int id, int nb, int i, int j, int k) {
  int box = 0;
  if (nb > 0) box = i / Lc.dim + nb * (j / Lc.dim + nb * (k / Lc.dim));
  else for (; box < Lc.num_boxes - 1; box++) {
    const int li = Lc.box_low[3 * box], lj = Lc.box_low[3 * box + 1], lk = Lc.box_low[3 * box + 2];
    if (i >= li && i < li + Lc.dim && j >= lj && j < lj + Lc.dim && k >= lk && k < lk + Lc.dim) break;
  }
  const int li = Lc.box_low[3 * box], lj = Lc.box_low[3 * box + 1], lk = Lc.box_low[3 * box + 2];
  return vec_origin(Lc, box, id)[(i - li) + (j - lj) * Lc.jStride + (k - lk) * Lc.kStride];
}

// boundary_interp_kernel with per-face kinds: Lc, nb locate the coarse iterate (vector id of the coarse level), hc is the coarse h, kappa the
// coarse level's kappa array (Robin walls; nullptr: the masked walls are Neumann)
template <bool ROBIN>
__global__ __launch_bounds__(kBndThreads) void boundary_interp_faces_kernel(const hpgmg_hip_level L, int id, const hpgmg_hip_level Lc, int nb,
                                                                            const double *__restrict__ gc, double hc, int mask,
                                                                            const double *__restrict__ kappa) {
  const int positions = 6 * L.dim * L.dim, nc = Lc.dim_i;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    double *v = vec_origin(L, box, id);
    for (int t = (int)(blockIdx.x * kBndThreads + threadIdx.x); t < positions; t += (int)(gridDim.x * kBndThreads)) {
      const FacePos P = bnd_face_pos(L, li, lj, lk, t);
      if (!P.on) continue;
      const int gi = li + P.i, gj = lj + P.j, gk = lk + P.k;
      const bnd_p1_cell F = bnd_p1_of(gi, gj, gk);
      double D = 0.0, w;
      int q[3];
#pragma unroll
      for (int s = 1; s < 8; s++) if (bnd_p1_ghost(nc, F, s, q, &w)) {
        const bnd_ghost G = bnd_ghost_faces(nc, gc, hc, mask, ROBIN ? kappa : nullptr, q[0], q[1], q[2]);
        D = D + w * (G.needs_u ? G.c * bnd_coarse_cell(Lc, id, nb, G.P[0], G.P[1], G.P[2]) + G.s : G.s);
      }
      const int c = P.i + P.j * L.jStride + P.k * L.kStride;
      v[c] = v[c] + D;
    }
  }
}

static dim3 bnd_grid(int per_box, int boxes) {       // x: the positions of one box, y: the boxes (the rest of either by grid stride)
  const int blocks = (per_box + kBndThreads - 1) / kBndThreads;
  return dim3(blocks < 16384 ? (blocks > 0 ? blocks : 1) : 16384, boxes < 65535 ? boxes : 65535);
}
static int bnd_cube(const hpgmg_hip_level *L) { return L->dim_i == L->dim_j && L->dim_i == L->dim_k && L->periodic == 0; }

}  // namespace hpgmg

using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

int hpgmg_hip_dense_pack_lifted_faces(const hpgmg_hip_level *L, int id, const double *src, const double *g, double w, int mask, const double *wall,
                                      double wn, int *status);
int hpgmg_hip_boundary_flux_faces(const hpgmg_hip_level *L, double *phi, const double *g, double w, int mask, const double *wall, double wn, int *status);
int hpgmg_hip_dense_pack_lifted_robin(const hpgmg_hip_level *L, int id, const double *src, const double *g, double w, int mask, const double *wall,
                                      double wn, const double *kappa, double h, int *status);
int hpgmg_hip_boundary_flux_robin(const hpgmg_hip_level *L, double *phi, const double *g, double w, int mask, const double *wall, double wn,
                                  const double *kappa, double h, int *status);
int hpgmg_hip_boundary_interp_robin(const hpgmg_hip_level *L, int id, const hpgmg_hip_level *Lc, int boxes_per_side, const double *g_c, double h_c, int mask,
                                    const double *kappa_c);
int hpgmg_hip_dense_pack_lifted(const hpgmg_hip_level *L, int id, const double *src, const double *g, double w, int *status) {
  return hpgmg_hip_dense_pack_lifted_faces(L, id, src, g, w, 0, nullptr, 0.0, status);
}
int hpgmg_hip_boundary_flux(const hpgmg_hip_level *L, double *phi, const double *g, double w, int *status) {
  return hpgmg_hip_boundary_flux_faces(L, phi, g, w, 0, nullptr, 0.0, status);
}

int hpgmg_hip_dense_pack_lifted_faces(const hpgmg_hip_level *L, int id, const double *src, const double *g, double w, int mask, const double *wall,
                                      double wn, int *status) {
  return hpgmg_hip_dense_pack_lifted_robin(L, id, src, g, w, mask, wall, wn, nullptr, 0.0, status);
}
int hpgmg_hip_dense_pack_lifted_robin(const hpgmg_hip_level *L, int id, const double *src, const double *g, double w, int mask, const double *wall,
                                      double wn, const double *kappa, double h, int *status) {
  *status = 0;
  if (mask < 0 || mask > 63 || (mask && !wall)) return record_error(hipErrorInvalidValue, "dense_pack_lifted: a wall mask without the wall betas");
  if (!bnd_cube(L)) return record_error(hipErrorInvalidValue, "dense_pack_lifted: the level is not a Dirichlet cube");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  int *flag;
  if (int e = status_begin(&flag)) return e;
  hipLaunchKernelGGL(kappa ? dense_pack_lifted_kernel<true> : dense_pack_lifted_kernel<false>, bnd_grid(L->volume, L->num_boxes), dim3(kBndThreads), 0, g_stream,
                     *L, id, src, g, w, mask, wall, wn, kappa, h, flag);
  return status_end("dense_pack_lifted_kernel", status);
}

int hpgmg_hip_boundary_flux_faces(const hpgmg_hip_level *L, double *phi, const double *g, double w, int mask, const double *wall, double wn, int *status) {
  return hpgmg_hip_boundary_flux_robin(L, phi, g, w, mask, wall, wn, nullptr, 0.0, status);
}
int hpgmg_hip_boundary_flux_robin(const hpgmg_hip_level *L, double *phi, const double *g, double w, int mask, const double *wall, double wn,
                                  const double *kappa, double h, int *status) {
  *status = 0;
  if (mask < 0 || mask > 63 || (mask && !wall)) return record_error(hipErrorInvalidValue, "boundary_flux: a wall mask without the wall betas");
  if (!bnd_cube(L)) return record_error(hipErrorInvalidValue, "boundary_flux: the level is not a Dirichlet cube");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  int *flag;
  if (int e = status_begin(&flag)) return e;
  hipLaunchKernelGGL(kappa ? boundary_flux_kernel<true> : boundary_flux_kernel<false>, bnd_grid(6 * L->dim * L->dim, L->num_boxes), dim3(kBndThreads), 0, g_stream,
                     *L, phi, g, w, mask, wall, wn, kappa, h, flag);
  return status_end("boundary_flux_kernel", status);
}

int hpgmg_hip_boundary_check_kappa(const double *kappa, int n, int robin_mask, int *status) {
  *status = 0;
  if (!kappa || n <= 0 || n > 9459 || robin_mask < 0 || robin_mask > 63) return record_error(hipErrorInvalidValue, "boundary_check_kappa: no array, or not a face mask");
  if (int e = hpgmg_hip_graph_flush()) return e;
  int *flag;
  if (int e = status_begin(&flag)) return e;
  hipLaunchKernelGGL(boundary_check_kappa_kernel, bnd_grid(6 * n * n, 1), dim3(kBndThreads), 0, g_stream, kappa, n, robin_mask, flag);
  return status_end("boundary_check_kappa_kernel", status);
}

int hpgmg_hip_boundary_store_walls(const hpgmg_hip_level *L, const double *wall, const double *kappa, double h, int mask) {
  if (mask < 0 || mask > 63 || !wall) return record_error(hipErrorInvalidValue, "boundary_store_walls: a wall mask without the wall betas");
  if (!bnd_cube(L) || L->ghosts < 1) return record_error(hipErrorInvalidValue, "boundary_store_walls: the level is not a Dirichlet cube");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0 || !mask) return 0;
  hipLaunchKernelGGL(boundary_store_walls_kernel, bnd_grid(6 * L->dim * L->dim, L->num_boxes), dim3(kBndThreads), 0, g_stream, *L, wall, kappa, h, mask);
  HPGMG_LAUNCH_CHECK("boundary_store_walls_kernel");
  return 0;
}

int hpgmg_hip_boundary_restrict(double *g_c, const double *g_f, int n_c) {
  HPGMG_SKIP_IF_REPLAY();
  if (n_c <= 0) return 0;
  hipLaunchKernelGGL(boundary_restrict_kernel, bnd_grid(6 * n_c * n_c, 1), dim3(kBndThreads), 0, g_stream, g_c, g_f, n_c);
  HPGMG_LAUNCH_CHECK("boundary_restrict_kernel");
  return 0;
}

int hpgmg_hip_boundary_lift(const hpgmg_hip_level *L, int id, const double *phi, const double *phi_fine, double sign) {
  HPGMG_SKIP_IF_REPLAY();
  if (!bnd_cube(L)) return record_error(hipErrorInvalidValue, "boundary_lift: the level is not a Dirichlet cube");
  if (L->num_boxes <= 0) return 0;
  hipLaunchKernelGGL(boundary_lift_kernel, bnd_grid(6 * L->dim * L->dim, L->num_boxes), dim3(kBndThreads), 0, g_stream, *L, id, phi, phi_fine, sign);
  HPGMG_LAUNCH_CHECK("boundary_lift_kernel");
  return 0;
}

int hpgmg_hip_boundary_interp(const hpgmg_hip_level *L, int id, const double *g_c, int n_c) {
  HPGMG_SKIP_IF_REPLAY();
  if (!bnd_cube(L) || 2 * n_c != L->dim_i) return record_error(hipErrorInvalidValue, "boundary_interp: the levels are not a Dirichlet cube and its coarsening");
  if (L->num_boxes <= 0) return 0;
  hipLaunchKernelGGL(boundary_interp_kernel, bnd_grid(6 * L->dim * L->dim, L->num_boxes), dim3(kBndThreads), 0, g_stream, *L, id, g_c, n_c);
  HPGMG_LAUNCH_CHECK("boundary_interp_kernel");
  return 0;
}

int hpgmg_hip_boundary_interp_faces(const hpgmg_hip_level *L, int id, const hpgmg_hip_level *Lc, int boxes_per_side, const double *g_c, double h_c, int mask) {
  return hpgmg_hip_boundary_interp_robin(L, id, Lc, boxes_per_side, g_c, h_c, mask, nullptr);
}
int hpgmg_hip_boundary_interp_robin(const hpgmg_hip_level *L, int id, const hpgmg_hip_level *Lc, int boxes_per_side, const double *g_c, double h_c, int mask,
                                    const double *kappa_c) {
  HPGMG_SKIP_IF_REPLAY();
  if (!bnd_cube(L) || !bnd_cube(Lc) || 2 * Lc->dim_i != L->dim_i || mask < 0 || mask > 63 || Lc->num_boxes <= 0)
    return record_error(hipErrorInvalidValue, "boundary_interp_faces: the levels are not a Dirichlet cube and its coarsening");
  if (boxes_per_side > 0 && (boxes_per_side * Lc->dim != Lc->dim_i || boxes_per_side * boxes_per_side * boxes_per_side != Lc->num_boxes))
    return record_error(hipErrorInvalidValue, "boundary_interp_faces: the coarse boxes do not tile the cube");
  if (L->num_boxes <= 0) return 0;
  hipLaunchKernelGGL(kappa_c ? boundary_interp_faces_kernel<true> : boundary_interp_faces_kernel<false>, bnd_grid(6 * L->dim * L->dim, L->num_boxes), dim3(kBndThreads), 0, g_stream, *L, id, *Lc, boxes_per_side,
                     g_c, h_c, mask, kappa_c);
  HPGMG_LAUNCH_CHECK("boundary_interp_faces_kernel");
  return 0;
}

}  // extern "C"
