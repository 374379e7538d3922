// dense_flux.hip -- face fluxes of a solution into three dense arrays (include/hpgmg_operators.h hpgmg_dense_unpack_flux).
// The arithmetic the host default (host/hooks_host.inc) must match bit for bit is not written here but in include/hpgmg_boundary_math.h, which
// both compile; wq = b * (1.0 / h) comes from the host.
//
// ONE launch writes flux_i, flux_j and flux_k: one lane per interior cell, grid row y = box, box-major then k, j, i (consecutive lanes on
// consecutive i; 32-bit offsets inside a box, as kernels/dense_io.hip).  A lane reads its own u and three betas once and writes the LOW face of
// its cell along each axis; its i-1, j-1, k-1 neighbours are the loads of the lane before it, of the previous row and of the previous plane, so
// they come from cache, and the one across a box face from the ghost zone the caller's exchange_boundary filled.  A lane whose cell lies on a
// domain wall takes the wall expression instead and never reads the ghost outside the domain; on a high wall it writes face dim too, from the
// level's beta in the high ghost layer.  That is dense_pack_kernel's ownership rule for a face array: every entry has exactly one lane.  Only
// lanes on a wall read g, wall and kappa; each g value read is validated, a bad one ORs a bit into one device word that the host reads once.
#include "reduce.hpp"
#include "hpgmg_boundary_math.h"

namespace hpgmg {

constexpr int kFluxThreads = 256;

struct FluxWalls { const double *g, *wall, *kappa; double b, wq, h; int mask; };
// q on wall face `face` of the cell (gi, gj, gk) with value uc; beta: the level's beta there (used on a Dirichlet wall)
__device__ __forceinline__ double flux_wall(const FluxWalls &W, int n, int face, int gi, int gj, int gk, double uc, double beta, int &bits) {
  const int e = bnd_entry(n, face, gi, gj, gk);
  const double gv = W.g ? W.g[e] : 0.0;
  if (!isfinite(gv)) bits |= HPGMG_DENSE_NOT_FINITE;
  if ((W.mask >> face) & 1) return bnd_flux_masked(W.b, W.wall[e], W.kappa ? W.kappa[e] : 0.0, W.h, uc, gv, face & 1);
  return bnd_flux_dirichlet(W.wq, beta, uc, gv, face & 1);
}

__global__ __launch_bounds__(kFluxThreads) void dense_flux_kernel(const hpgmg_hip_level L, int id, const FluxWalls W, double *__restrict__ fi,
                                                                  double *__restrict__ fj, double *__restrict__ fk, int *flag) {
  const int dim = L.dim, plane = dim * dim, cells = plane * dim, n = L.dim_i, jS = L.jStride, kS = L.kStride;
  const bool walls = !L.periodic;
  const size_t nn = (size_t)n, ni = nn + (walls ? 1 : 0);        // flux_i is (n, n, ni), flux_j (n, ni, n), flux_k (ni, n, n)
  int bits = 0;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    const double *u = vec_origin(L, box, id), *bi = vec_origin(L, box, VECTOR_BETA_I), *bj = vec_origin(L, box, VECTOR_BETA_J);
    const double *bk = vec_origin(L, box, VECTOR_BETA_K);
    for (int c = (int)(blockIdx.x * kFluxThreads + threadIdx.x); c < cells; c += (int)(gridDim.x * kFluxThreads)) {
      const int k = c / plane, j = (c - k * plane) / dim, i = c - k * plane - j * dim;
      const int gi = li + i, gj = lj + j, gk = lk + k, ofs = i + j * jS + k * kS;
      const double uc = u[ofs], ci = bi[ofs], cj = bj[ofs], ck = bk[ofs];
      double *qi = fi + ((size_t)gk * nn + (size_t)gj) * ni + (size_t)gi, *qj = fj + ((size_t)gk * ni + (size_t)gj) * nn + (size_t)gi;
      double *qk = fk + ((size_t)gk * nn + (size_t)gj) * nn + (size_t)gi;
      if (walls && gi == 0) *qi = flux_wall(W, n, 0, gi, gj, gk, uc, ci, bits);
      else *qi = bnd_flux_interior(W.wq, ci, u[ofs - 1], uc);
      if (walls && gi == n - 1) qi[1] = flux_wall(W, n, 1, gi, gj, gk, uc, bi[ofs + 1], bits);
      if (walls && gj == 0) *qj = flux_wall(W, n, 2, gi, gj, gk, uc, cj, bits);
      else *qj = bnd_flux_interior(W.wq, cj, u[ofs - jS], uc);
      if (walls && gj == n - 1) qj[nn] = flux_wall(W, n, 3, gi, gj, gk, uc, bj[ofs + jS], bits);
      if (walls && gk == 0) *qk = flux_wall(W, n, 4, gi, gj, gk, uc, ck, bits);
      else *qk = bnd_flux_interior(W.wq, ck, u[ofs - kS], uc);
      if (walls && gk == n - 1) qk[nn * nn] = flux_wall(W, n, 5, gi, gj, gk, uc, bk[ofs + kS], bits);
    }
  }
  if (bits) atomicOr(flag, bits);
}

}  // namespace hpgmg

using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

int hpgmg_hip_dense_unpack_flux(const hpgmg_hip_level *L, int id, const double *g, double b, double wq, double h, int mask, const double *wall,
                                const double *kappa, double *flux_i, double *flux_j, double *flux_k, int *status) {
  *status = 0;
  if (!flux_i || !flux_j || !flux_k) return record_error(hipErrorInvalidValue, "dense_unpack_flux: an output array is missing");
  if (mask < 0 || mask > 63 || (mask && !wall)) return record_error(hipErrorInvalidValue, "dense_unpack_flux: a wall mask without the wall betas");
  if (L->dim_i != L->dim_j || L->dim_i != L->dim_k || L->ghosts < 1) return record_error(hipErrorInvalidValue, "dense_unpack_flux: the level is not a cube with ghost zones");
  if (L->periodic && (g || mask)) return record_error(hipErrorInvalidValue, "dense_unpack_flux: boundary data on a periodic level");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  int *flag;
  if (int e = status_begin(&flag)) return e;
  const FluxWalls W = { g, mask ? wall : nullptr, mask ? kappa : nullptr, b, wq, h, mask };
  const int blocks = (L->dim * L->dim * L->dim + kFluxThreads - 1) / kFluxThreads;
  const dim3 grid(blocks < 16384 ? (blocks > 0 ? blocks : 1) : 16384, L->num_boxes < 65535 ? L->num_boxes : 65535);   // the rest of either by grid stride
  hipLaunchKernelGGL(dense_flux_kernel, grid, dim3(kFluxThreads), 0, g_stream, *L, id, W, flux_i, flux_j, flux_k, flag);
  return status_end("dense_flux_kernel", status);      // synchronises: the caller's arrays are complete on return (a torch tensor is read on another stream)
}

}  // extern "C"
