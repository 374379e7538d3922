// dense_cells.hip -- cell-centred conductivities (include/hpgmg_operators.h hpgmg_dense_pack_cell_mean / hpgmg_dense_unpack_cell_sensitivity;
// DESIGN.md §11.10): the coefficient is ONE dense (n, n, n) array kcell, the beta of a face between two cells a mean of the two (harmonic or
// arithmetic; box-to-box and the periodic wrap included) and of a domain wall face its cell's own value.  The arithmetic the host defaults
// (host/hooks_host.inc) must match bit for bit is not written here but in include/hpgmg_boundary_math.h (bnd_mean*, bnd_sens_*), which both compile.
//
// Pack: ONE launch fills VECTOR_BETA_I / J / K, mapped as dense_pack_kernel of kernels/dense_io.hip: a grid row per box, one lane per padded double,
// consecutive lanes on consecutive doubles of a padded row, 32-bit offsets inside a box, that file's grid caps.  A lane loads its own cell of kcell by
// global index and its i-1, j-1, k-1 neighbours (the loads of the lane before it, of the previous row and of the previous plane: cache hits) and
// stores one double into each of the three vectors: the mean, the cell's own value on a wall, 0.0 with the value sent to `wall` on a masked wall
// (each wall entry has one lane), 0.0 wherever the array does not determine the cell -- the bytes dense_pack_kernel / dense_pack_walls_kernel leave
// for the three face arrays.  The three "determined" predicates differ only in which axis carries the high-face layer.  Every kcell entry is
// validated by its own cell's lane, every mean by the lane that writes it.  32 B per cell (one read, three writes).
//
// Cell sensitivity: ONE launch, the structure and caps of dense_sensitivity_kernel (kernels/dense_sensitivity.hip): one lane per interior cell, grid
// row = box, 4096 workgroups of 256, the rest by stride, shifts when the box side is a power of two.  A lane reads u and lam of itself and its six
// neighbours from the box layout (the ghost zones the caller's exchange_boundary filled; a domain wall takes the wall expression and no ghost outside
// the domain is read) and kcell of itself and its six neighbours from the dense array (periodic levels wrap by index; a wall reads no neighbour), and
// writes d_alpha and d_k of its cell.  Every output entry has one lane, nothing is accumulated; the only atomic is the status word.  40 B per cell
// (u, lam, kcell in; two out), 32 B without alpha.
//
// No LDS, no inline assembly, no scratch.
#include "reduce.hpp"
#include "hpgmg_boundary_math.h"

namespace hpgmg {

constexpr int kCellThreads = 256;
constexpr int kCellPackMaxX = 16384, kCellPackMaxY = 65535;      // dense_grid's caps (kernels/dense_io.hip)
constexpr int kCellSensMaxBlocks = 4096;                         // kSensMaxBlocks (kernels/dense_sensitivity.hip)

// beta of the face of axis AXIS on the low side of position (gi, gj, gk), whose coordinate along the axis is 0 .. n (n: the high wall, walls only);
// c: kcell of that position, read by the caller when the coordinate is < n.  The other two coordinates are interior.
template <int AXIS>
__device__ __forceinline__ double cell_face(const double *__restrict__ kc, int n, bool walls, int mean, int mask, double *__restrict__ wall, int gi,
                                            int gj, int gk, double c, int &bits) {
  const int gc = AXIS == 0 ? gi : AXIS == 1 ? gj : gk;
  const size_t nn = (size_t)n, stride = AXIS == 0 ? 1 : AXIS == 1 ? nn : nn * nn;
  const size_t at = ((size_t)gk * nn + (size_t)gj) * nn + (size_t)gi;           // gc == n: one past the cells along the axis; only at - stride is read
  if (walls && (gc == 0 || gc == n)) {
    const int high = gc == n;
    double v = high ? kc[at - stride] : c;
    if ((mask >> (2 * AXIS + high)) & 1) {                                      // a masked wall: its beta goes to the wall array, the vector takes 0.0
      const int q = AXIS == 2 ? gj : gk, p = AXIS == 0 ? gj : gi;
      wall[((2 * AXIS + high) * n + q) * n + p] = v;
      v = 0.0;
    }
    return v;
  }
  const double lo = kc[gc == 0 ? at + (nn - 1) * stride : at - stride];         // the periodic wrap: lo = cell n - 1
  const double m = bnd_mean(mean, lo, c);
  bits |= bnd_mean_bits(lo, c, m);
  return m;
}

__global__ __launch_bounds__(kCellThreads) void dense_pack_cell_mean_kernel(const hpgmg_hip_level L, int id_i, int id_j, int id_k,
                                                                            const double *__restrict__ kc, int mean, int mask,
                                                                            double *__restrict__ wall, int *flag) {
  const int g = L.ghosts, dim = L.dim, n = L.dim_i;
  const bool walls = !L.periodic;
  int bits = 0;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {     // a grid row per box: 32-bit offsets inside it
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    double *bi = L.box_base[box] + (size_t)id_i * L.volume, *bj = L.box_base[box] + (size_t)id_j * L.volume, *bk = L.box_base[box] + (size_t)id_k * L.volume;
    for (int ofs = (int)(blockIdx.x * kCellThreads + threadIdx.x); ofs < L.volume; ofs += (int)(gridDim.x * kCellThreads)) {
      const int pk = ofs / L.kStride, pj = (ofs - pk * L.kStride) / L.jStride, pi = ofs - pk * L.kStride - pj * L.jStride;
      const int i = pi - g, j = pj - g, k = pk - g;
      const int gi = li + i, gj = lj + j, gk = lk + k;
      const bool ci = i >= 0 && i < dim, cj = j >= 0 && j < dim, ck = k >= 0 && k < dim;
      // the high ghost layer along one axis belongs to that axis' vector in a box on the domain's high wall
      const bool hi_i = walls && i == dim && gi == n, hi_j = walls && j == dim && gj == n, hi_k = walls && k == dim && gk == n;
      double c = 0.0, vi = 0.0, vj = 0.0, vk = 0.0;
      if (ci && cj && ck) {
        c = kc[((size_t)gk * n + (size_t)gj) * n + (size_t)gi];
        bits |= bnd_cell_bits(c);
      }
      if ((ci || hi_i) && cj && ck) vi = cell_face<0>(kc, n, walls, mean, mask, wall, gi, gj, gk, c, bits);
      if (ci && (cj || hi_j) && ck) vj = cell_face<1>(kc, n, walls, mean, mask, wall, gi, gj, gk, c, bits);
      if (ci && cj && (ck || hi_k)) vk = cell_face<2>(kc, n, walls, mean, mask, wall, gi, gj, gk, c, bits);
      bi[ofs] = vi;
      bj[ofs] = vj;
      bk[ofs] = vk;
    }
  }
  if (bits) atomicOr(flag, bits);
}

struct CellWalls { const double *g, *kappa; double a, w2, w, wn, h; int mask, mean; };
// G of wall face `face` of the cell (gi, gj, gk) with state uc and adjoint lc (sens_wall of kernels/dense_sensitivity.hip)
__device__ __forceinline__ double cell_sens_wall(const CellWalls &W, int n, int face, int gi, int gj, int gk, double uc, double lc, int &bits) {
  const int e = bnd_entry(n, face, gi, gj, gk);
  const double gv = W.g ? W.g[e] : 0.0;
  if (!isfinite(gv)) bits |= HPGMG_DENSE_NOT_FINITE;
  if ((W.mask >> face) & 1) return bnd_sens_masked(W.wn, W.kappa ? W.kappa[e] : 0.0, W.h, uc, gv, lc);
  return bnd_sens_dirichlet(W.w, uc, gv, lc);
}
// G D of the low and of the high face of axis AXIS of the cell at coordinate gc along it: vs / ks the strides along the axis of the box layout and of kcell
template <int AXIS>
__device__ __forceinline__ void cell_sens_axis(const CellWalls &W, int n, bool walls, gcptr u, gcptr lam, int ofs, int vs, const double *__restrict__ kc,
                                               size_t cell, size_t ks, int gi, int gj, int gk, double uc, double lc, double kcc, double &lo_term,
                                               double &hi_term, int &bits) {
  const int gc = AXIS == 0 ? gi : AXIS == 1 ? gj : gk;
  if (walls && gc == 0) lo_term = cell_sens_wall(W, n, 2 * AXIS, gi, gj, gk, uc, lc, bits);          // D = 1.0
  else {
    const double klo = kc[gc ? cell - ks : cell + (size_t)(n - 1) * ks];
    bits |= bnd_mean_bits(klo, kcc, bnd_mean(W.mean, klo, kcc));                                     // each mean once: by the cell on its high side
    lo_term = bnd_sens_interior(W.w2, u[ofs - vs], uc, lam[ofs - vs], lc) * bnd_mean_dhi(W.mean, klo, kcc);
  }
  if (walls && gc == n - 1) hi_term = cell_sens_wall(W, n, 2 * AXIS + 1, gi, gj, gk, uc, lc, bits);  // D = 1.0
  else {
    const double khi = kc[gc < n - 1 ? cell + ks : cell - (size_t)(n - 1) * ks];
    hi_term = bnd_sens_interior(W.w2, uc, u[ofs + vs], lc, lam[ofs + vs]) * bnd_mean_dlo(W.mean, kcc, khi);
  }
}

// sh = log2(dim) when dim is a power of two, else -1 (the cell index is then divided)
__global__ __launch_bounds__(kCellThreads) void dense_cell_sensitivity_kernel(const hpgmg_hip_level L, int u_id, int lam_id, const CellWalls W, int sh,
                                                                              const double *__restrict__ kc, double *__restrict__ da,
                                                                              double *__restrict__ dk, int *flag) {
  const int dim = L.dim, plane = dim * dim, cells = plane * dim, n = L.dim_i, jS = L.jStride, kS = L.kStride;
  const bool walls = !L.periodic;
  const size_t nn = (size_t)n;
  int bits = 0;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    const gcptr u = gvec_origin(L, box, u_id), lam = gvec_origin(L, box, lam_id);
    for (int c = (int)(blockIdx.x * kCellThreads + threadIdx.x); c < cells; c += (int)(gridDim.x * kCellThreads)) {
      int i, j, k;
      if (sh >= 0) { i = c & (dim - 1); j = (c >> sh) & (dim - 1); k = c >> (2 * sh); }
      else { k = c / plane; j = (c - k * plane) / dim; i = c - k * plane - j * dim; }
      const int gi = li + i, gj = lj + j, gk = lk + k, ofs = i + j * jS + k * kS;
      const size_t cell = ((size_t)gk * nn + (size_t)gj) * nn + (size_t)gi;
      const double uc = u[ofs], lc = lam[ofs], kcc = kc[cell];
      bits |= bnd_cell_bits(kcc);
      double il, ih, jl, jh, kl, kh;
      cell_sens_axis<0>(W, n, walls, u, lam, ofs, 1, kc, cell, 1, gi, gj, gk, uc, lc, kcc, il, ih, bits);
      cell_sens_axis<1>(W, n, walls, u, lam, ofs, jS, kc, cell, nn, gi, gj, gk, uc, lc, kcc, jl, jh, bits);
      cell_sens_axis<2>(W, n, walls, u, lam, ofs, kS, kc, cell, nn * nn, gi, gj, gk, uc, lc, kcc, kl, kh, bits);
      if (da) da[cell] = bnd_sens_alpha(W.a, uc, lc);
      dk[cell] = ((((il + ih) + jl) + jh) + kl) + kh;
    }
  }
  if (bits) atomicOr(flag, bits);
}

}  // namespace hpgmg

using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

int hpgmg_hip_dense_pack_cell_mean(const hpgmg_hip_level *L, int id_i, int id_j, int id_k, const double *kcell, int mean, int mask, double *wall,
                                   int *status) {
  *status = 0;
  if (!kcell || id_i < 0 || id_j < 0 || id_k < 0) return record_error(hipErrorInvalidValue, "dense_pack_cell_mean: no array, or a negative vector id");
  if (mean != HPGMG_MEAN_HARMONIC && mean != HPGMG_MEAN_ARITHMETIC) return record_error(hipErrorInvalidValue, "dense_pack_cell_mean: an unknown mean");
  if (L->dim_i != L->dim_j || L->dim_i != L->dim_k) return record_error(hipErrorInvalidValue, "dense_pack_cell_mean: the level is not a cube");
  if (mask < 0 || mask > 63 || (mask && (!wall || L->periodic))) return record_error(hipErrorInvalidValue, "dense_pack_cell_mean: a wall mask outside 0 .. 63, without the wall array or on a periodic level");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  int *flag;
  if (int e = status_begin(&flag)) return e;
  const int blocks = (L->volume + kCellThreads - 1) / kCellThreads;
  const dim3 grid(blocks < kCellPackMaxX ? (blocks > 0 ? blocks : 1) : kCellPackMaxX, L->num_boxes < kCellPackMaxY ? L->num_boxes : kCellPackMaxY);
  hipLaunchKernelGGL(dense_pack_cell_mean_kernel, grid, dim3(kCellThreads), 0, g_stream, *L, id_i, id_j, id_k, kcell, mean, mask, wall, flag);
  return status_end("dense_pack_cell_mean_kernel", status);      // synchronises: the caller's array may be reused on return (a torch tensor lives on another stream)
}

int hpgmg_hip_dense_unpack_cell_sensitivity(const hpgmg_hip_level *L, int u_id, int lam_id, const double *kcell, int mean, const double *g, double a,
                                            double w2, double w, double wn, double h, int mask, const double *kappa, double *d_alpha, double *d_k,
                                            int *status) {
  *status = 0;
  if (!kcell || !d_k) return record_error(hipErrorInvalidValue, "dense_unpack_cell_sensitivity: an array is missing");
  if (mean != HPGMG_MEAN_HARMONIC && mean != HPGMG_MEAN_ARITHMETIC) return record_error(hipErrorInvalidValue, "dense_unpack_cell_sensitivity: an unknown mean");
  if (mask < 0 || mask > 63) return record_error(hipErrorInvalidValue, "dense_unpack_cell_sensitivity: the wall mask is not in 0 .. 63");
  if (u_id < 0 || lam_id < 0) return record_error(hipErrorInvalidValue, "dense_unpack_cell_sensitivity: a negative vector id");
  if (L->dim_i != L->dim_j || L->dim_i != L->dim_k || L->ghosts < 1) return record_error(hipErrorInvalidValue, "dense_unpack_cell_sensitivity: the level is not a cube with ghost zones");
  if (L->dim < 1 || L->dim > 1024) return record_error(hipErrorInvalidValue, "dense_unpack_cell_sensitivity: the box side is not in 1 .. 1024");
  if (L->periodic && (g || mask)) return record_error(hipErrorInvalidValue, "dense_unpack_cell_sensitivity: boundary data on a periodic level");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  int *flag;
  if (int e = status_begin(&flag)) return e;
  const CellWalls W = { g, mask ? kappa : nullptr, a, w2, w, wn, h, mask, mean };
  const int dim = L->dim, per_box = (dim * dim * dim + kCellThreads - 1) / kCellThreads;
  const int gy = L->num_boxes < kCellSensMaxBlocks ? L->num_boxes : kCellSensMaxBlocks, cap = kCellSensMaxBlocks / gy;      // the rest of either by grid stride
  const dim3 grid(per_box < cap ? per_box : cap, gy);
  const int sh = (dim & (dim - 1)) == 0 ? __builtin_ctz(dim) : -1;
  hipLaunchKernelGGL(dense_cell_sensitivity_kernel, grid, dim3(kCellThreads), 0, g_stream, *L, u_id, lam_id, W, sh, kcell, d_alpha, d_k, flag);
  return status_end("dense_cell_sensitivity_kernel", status);      // synchronises: the caller's arrays are complete on return (a torch tensor is read on another stream)
}

}  // extern "C"
