// dense_sensitivity.hip -- coefficient sensitivities of a state u and an adjoint lam into four dense arrays (include/hpgmg_operators.h
// hpgmg_dense_unpack_sensitivity): d_alpha in alpha's shape, d_beta_i / j / k in the shapes of the beta arrays.  The arithmetic the
// host default (host/hooks_host.inc) must match bit for bit is not written here but in include/hpgmg_boundary_math.h (bnd_sens_*), which both
// compile; the weights w2 = b * (1.0 / (h * h)), w = (2.0 * b) * (1.0 / (h * h)) and wn = b * (1.0 / h) come from the host.
//
// ONE launch writes the four arrays.  Mapped as kernels/dense_flux.hip: one lane per interior cell, grid row y = box, inside a box k, j, i with
// consecutive lanes on consecutive i and 32-bit offsets; the grid is capped as kernels/dense_step.hip caps it (4096 workgroups of 256) and a lane
// takes the rest of its box, a grid row the rest of the boxes, by stride.  A lane reads its own u and lam once and writes d_alpha of its cell and the
// LOW face of its cell along each axis; its i-1, j-1, k-1 neighbours are the loads of the lane before it, of the previous row and of the previous
// plane, so they come from cache, and the ones across a box face from the ghost zones the caller's exchange_boundary filled.  A lane whose cell lies
// on a domain wall takes the wall expression instead and never reads the ghost outside the domain; on a high wall it writes face dim too.  Every
// output entry has exactly one lane; nothing is accumulated.  No beta is read.  Only lanes on a wall read g and kappa; each g value read is
// validated, a bad one ORs a bit into one device word that the host reads once.  48 B per cell (2 reads, 4 writes), 40 B without alpha.
#include "reduce.hpp"
#include "hpgmg_boundary_math.h"

namespace hpgmg {

constexpr int kSensThreads = 256;
constexpr int kSensMaxBlocks = 4096;            // 256 CUs x 16: what the launch is capped to (either axis by grid stride)

struct SensWalls { const double *g, *kappa; double a, w2, w, wn, h; int mask; };
// G of wall face `face` of the cell (gi, gj, gk) with state uc and adjoint lc
__device__ __forceinline__ double sens_wall(const SensWalls &W, int n, int face, int gi, int gj, int gk, double uc, double lc, int &bits) {
  const int e = bnd_entry(n, face, gi, gj, gk);
  const double gv = W.g ? W.g[e] : 0.0;
  if (!isfinite(gv)) bits |= HPGMG_DENSE_NOT_FINITE;
  if ((W.mask >> face) & 1) return bnd_sens_masked(W.wn, W.kappa ? W.kappa[e] : 0.0, W.h, uc, gv, lc);
  return bnd_sens_dirichlet(W.w, uc, gv, lc);
}

// sh = log2(dim) when dim is a power of two, else -1 (the cell index is then divided)
__global__ __launch_bounds__(kSensThreads) void dense_sensitivity_kernel(const hpgmg_hip_level L, int u_id, int lam_id, const SensWalls W, int sh,
                                                                         double *__restrict__ da, double *__restrict__ di, double *__restrict__ dj,
                                                                         double *__restrict__ dk, int *flag) {
  const int dim = L.dim, plane = dim * dim, cells = plane * dim, n = L.dim_i, jS = L.jStride, kS = L.kStride;
  const bool walls = !L.periodic;
  const size_t nn = (size_t)n, ni = nn + (walls ? 1 : 0);        // d_beta_i is (n, n, ni), d_beta_j (n, ni, n), d_beta_k (ni, n, n), d_alpha (n, n, n)
  int bits = 0;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    const gcptr u = gvec_origin(L, box, u_id), lam = gvec_origin(L, box, lam_id);
    for (int c = (int)(blockIdx.x * kSensThreads + threadIdx.x); c < cells; c += (int)(gridDim.x * kSensThreads)) {
      int i, j, k;
      if (sh >= 0) { i = c & (dim - 1); j = (c >> sh) & (dim - 1); k = c >> (2 * sh); }
      else { k = c / plane; j = (c - k * plane) / dim; i = c - k * plane - j * dim; }
      const int gi = li + i, gj = lj + j, gk = lk + k, ofs = i + j * jS + k * kS;
      const double uc = u[ofs], lc = lam[ofs];
      const size_t cell = ((size_t)gk * nn + (size_t)gj) * nn + (size_t)gi;
      double *qi = di + ((size_t)gk * nn + (size_t)gj) * ni + (size_t)gi, *qj = dj + ((size_t)gk * ni + (size_t)gj) * nn + (size_t)gi;
      double *qk = dk + cell;
      if (da) da[cell] = bnd_sens_alpha(W.a, uc, lc);
      if (walls && gi == 0) *qi = sens_wall(W, n, 0, gi, gj, gk, uc, lc, bits);
      else *qi = bnd_sens_interior(W.w2, u[ofs - 1], uc, lam[ofs - 1], lc);
      if (walls && gi == n - 1) qi[1] = sens_wall(W, n, 1, gi, gj, gk, uc, lc, bits);
      if (walls && gj == 0) *qj = sens_wall(W, n, 2, gi, gj, gk, uc, lc, bits);
      else *qj = bnd_sens_interior(W.w2, u[ofs - jS], uc, lam[ofs - jS], lc);
      if (walls && gj == n - 1) qj[nn] = sens_wall(W, n, 3, gi, gj, gk, uc, lc, bits);
      if (walls && gk == 0) *qk = sens_wall(W, n, 4, gi, gj, gk, uc, lc, bits);
      else *qk = bnd_sens_interior(W.w2, u[ofs - kS], uc, lam[ofs - kS], lc);
      if (walls && gk == n - 1) qk[nn * nn] = sens_wall(W, n, 5, gi, gj, gk, uc, lc, bits);
    }
  }
  if (bits) atomicOr(flag, bits);
}

}  // namespace hpgmg

using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

int hpgmg_hip_dense_unpack_sensitivity(const hpgmg_hip_level *L, int u_id, int lam_id, const double *g, double a, double w2, double w, double wn,
                                       double h, int mask, const double *kappa, double *d_alpha, double *d_beta_i, double *d_beta_j,
                                       double *d_beta_k, int *status) {
  *status = 0;
  if (!d_beta_i || !d_beta_j || !d_beta_k) return record_error(hipErrorInvalidValue, "dense_unpack_sensitivity: an output array is missing");
  if (mask < 0 || mask > 63) return record_error(hipErrorInvalidValue, "dense_unpack_sensitivity: the wall mask is not in 0 .. 63");
  if (u_id < 0 || lam_id < 0) return record_error(hipErrorInvalidValue, "dense_unpack_sensitivity: a negative vector id");
  if (L->dim_i != L->dim_j || L->dim_i != L->dim_k || L->ghosts < 1) return record_error(hipErrorInvalidValue, "dense_unpack_sensitivity: the level is not a cube with ghost zones");
  if (L->dim < 1 || L->dim > 1024) return record_error(hipErrorInvalidValue, "dense_unpack_sensitivity: the box side is not in 1 .. 1024");
  if (L->periodic && (g || mask)) return record_error(hipErrorInvalidValue, "dense_unpack_sensitivity: boundary data on a periodic level");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  int *flag;
  if (int e = status_begin(&flag)) return e;
  const SensWalls W = { g, mask ? kappa : nullptr, a, w2, w, wn, h, mask };
  const int dim = L->dim, per_box = (dim * dim * dim + kSensThreads - 1) / kSensThreads;
  const int gy = L->num_boxes < kSensMaxBlocks ? L->num_boxes : kSensMaxBlocks, cap = kSensMaxBlocks / gy;      // the rest of either by grid stride
  const dim3 grid(per_box < cap ? per_box : cap, gy);
  const int sh = (dim & (dim - 1)) == 0 ? __builtin_ctz(dim) : -1;
  hipLaunchKernelGGL(dense_sensitivity_kernel, grid, dim3(kSensThreads), 0, g_stream, *L, u_id, lam_id, W, sh, d_alpha, d_beta_i, d_beta_j, d_beta_k, flag);
  return status_end("dense_sensitivity_kernel", status);      // synchronises: the caller's arrays are complete on return (a torch tensor is read on another stream)
}

}  // extern "C"
