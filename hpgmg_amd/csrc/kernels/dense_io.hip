// dense_io.hip -- dense N^3 arrays <-> a level's padded boxes (include/hpgmg_operators.h hpgmg_dense_pack / hpgmg_dense_unpack).
//
// Dense layout: C-contiguous float64, indexed [k][j][i] (i fastest, as in a box).  Cell arrays are (N, N, N).  A face array of axis d is
// one longer along d when the domain is Dirichlet (entry d = N is the high domain face) and (N, N, N) when it is periodic (face N is face 0).
//
// Pack: ONE pass over every double of every box (ghosts and row / volume padding included; grid row y = box, 32-bit offsets inside it),
// consecutive lanes on consecutive doubles of a padded row, so the box side and the dense row (for the interior run of the row) are both read / written contiguously.  A padded cell the
// array determines -- interior cells, and for a Dirichlet face array the high ghost layer of the boxes on the domain's high face along d --
// takes its value; every other cell takes 0.0, as initialize_problem's zero-filled staging leaves them.  rebuild_operator's
// exchange_boundary fills the ghost zones afterwards.  Each value read is validated in the same pass (finite; and > 0 or >= 0 when asked);
// a lane that finds a bad value ORs a bit into one device word, which the host reads once per call.
//
// Unpack: one lane per interior cell, box-major then k, j, i; the dense array's interior cells only are written.
#include "reduce.hpp"

namespace hpgmg {

constexpr int kDenseThreads = 256;

__global__ __launch_bounds__(kDenseThreads) void dense_pack_kernel(const hpgmg_hip_level L, int id, const double *__restrict__ src,
                                                                   int ni, int nj, int nk, int check, int *flag) {
  const int g = L.ghosts, dim = L.dim;
  int bits = 0;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {     // a grid row per box: 32-bit offsets inside it
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    double *dst = L.box_base[box] + (size_t)id * L.volume;
    for (int ofs = (int)(blockIdx.x * kDenseThreads + threadIdx.x); ofs < L.volume; ofs += (int)(gridDim.x * kDenseThreads)) {
      const int pk = ofs / L.kStride, pj = (ofs - pk * L.kStride) / L.jStride, pi = ofs - pk * L.kStride - pj * L.jStride;
      const int i = pi - g, j = pj - g, k = pk - g;
      const int gi = li + i, gj = lj + j, gk = lk + k;
      // interior, or the extra high-face layer of a Dirichlet face array (ghost index dim of a box on the domain's high face)
      const bool in_i = i >= 0 && (i < dim || (i == dim && gi == L.dim_i && ni > L.dim_i));
      const bool in_j = j >= 0 && (j < dim || (j == dim && gj == L.dim_j && nj > L.dim_j));
      const bool in_k = k >= 0 && (k < dim || (k == dim && gk == L.dim_k && nk > L.dim_k));
      double v = 0.0;
      if (in_i && in_j && in_k) {
        v = src[((size_t)gk * nj + gj) * ni + gi];
        if (!isfinite(v)) bits |= HPGMG_DENSE_NOT_FINITE;
        else if ((check == HPGMG_DENSE_CHECK_POSITIVE && !(v > 0.0)) || (check == HPGMG_DENSE_CHECK_NONNEGATIVE && !(v >= 0.0))) bits |= HPGMG_DENSE_OUT_OF_RANGE;
      }
      dst[ofs] = v;
    }
  }
  if (bits) atomicOr(flag, bits);
}

// dense_pack_kernel for a face array of axis `axis` of a Dirichlet cube with Neumann walls (hpgmg_dense_pack_walls): the same
// pass, reads and checks.  lo / hi: the low / high domain wall of that axis is masked; a value on a masked wall (index 0 of a box on the low
// wall, the high ghost layer dim of a box on the high wall) goes to its entry of `wall` (face 2 axis / 2 axis + 1 of a 6 n^2 boundary
// array) and the vector takes 0.0.  Each wall value is read by one lane, so no two lanes write one entry.
__global__ __launch_bounds__(kDenseThreads) void dense_pack_walls_kernel(const hpgmg_hip_level L, int id, const double *__restrict__ src,
                                                                         int ni, int nj, int nk, int check, int axis, int lo, int hi,
                                                                         double *__restrict__ wall, int *flag) {
  const int g = L.ghosts, dim = L.dim, n = L.dim_i;
  int bits = 0;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    double *dst = L.box_base[box] + (size_t)id * L.volume;
    for (int ofs = (int)(blockIdx.x * kDenseThreads + threadIdx.x); ofs < L.volume; ofs += (int)(gridDim.x * kDenseThreads)) {
      const int pk = ofs / L.kStride, pj = (ofs - pk * L.kStride) / L.jStride, pi = ofs - pk * L.kStride - pj * L.jStride;
      const int i = pi - g, j = pj - g, k = pk - g;
      const int gi = li + i, gj = lj + j, gk = lk + k;
      const bool in_i = i >= 0 && (i < dim || (i == dim && gi == L.dim_i && ni > L.dim_i));
      const bool in_j = j >= 0 && (j < dim || (j == dim && gj == L.dim_j && nj > L.dim_j));
      const bool in_k = k >= 0 && (k < dim || (k == dim && gk == L.dim_k && nk > L.dim_k));
      double v = 0.0;
      if (in_i && in_j && in_k) {
        v = src[((size_t)gk * nj + gj) * ni + gi];
        if (!isfinite(v)) bits |= HPGMG_DENSE_NOT_FINITE;
        else if ((check == HPGMG_DENSE_CHECK_POSITIVE && !(v > 0.0)) || (check == HPGMG_DENSE_CHECK_NONNEGATIVE && !(v >= 0.0))) bits |= HPGMG_DENSE_OUT_OF_RANGE;
        const int gc = axis == 0 ? gi : axis == 1 ? gj : gk;
        if ((lo && gc == 0) || (hi && gc == n)) {
          const int q = axis == 2 ? gj : gk, p = axis == 0 ? gj : gi;          // in range: the other two axes are interior here
          wall[((2 * axis + (gc == n)) * n + q) * n + p] = v;
          v = 0.0;
        }
      }
      dst[ofs] = v;
    }
  }
  if (bits) atomicOr(flag, bits);
}

__global__ __launch_bounds__(kDenseThreads) void dense_unpack_kernel(const hpgmg_hip_level L, int id, double *__restrict__ dst) {
  const int dim = L.dim, plane = dim * dim, cells = plane * dim;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const int li = L.box_low[3 * box], lj = L.box_low[3 * box + 1], lk = L.box_low[3 * box + 2];
    const double *src = vec_origin(L, box, id);
    for (int c = (int)(blockIdx.x * kDenseThreads + threadIdx.x); c < cells; c += (int)(gridDim.x * kDenseThreads)) {
      const int k = c / plane, j = (c - k * plane) / dim, i = c - k * plane - j * dim;
      dst[((size_t)(lk + k) * L.dim_j + (lj + j)) * L.dim_i + (li + i)] = src[i + j * L.jStride + k * L.kStride];
    }
  }
}

static dim3 dense_grid(int per_box, int boxes) {     // x: the cells of one box, y: the boxes (the rest of either by grid stride)
  const int blocks = (per_box + kDenseThreads - 1) / kDenseThreads;
  return dim3(blocks < 16384 ? (blocks > 0 ? blocks : 1) : 16384, boxes < 65535 ? boxes : 65535);
}

}  // namespace hpgmg

using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

int hpgmg_hip_dense_pack(const hpgmg_hip_level *L, int id, const double *src, int ni, int nj, int nk, int check, int *status) {
  *status = 0;
  if (ni < L->dim_i || ni > L->dim_i + 1 || nj < L->dim_j || nj > L->dim_j + 1 || nk < L->dim_k || nk > L->dim_k + 1)
    return record_error(hipErrorInvalidValue, "dense_pack: array extents do not match the level");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  int *flag;
  if (int e = status_begin(&flag)) return e;
  hipLaunchKernelGGL(dense_pack_kernel, dense_grid(L->volume, L->num_boxes), dim3(kDenseThreads), 0, g_stream, *L, id, src, ni, nj, nk, check, flag);
  return status_end("dense_pack_kernel", status);
}

int hpgmg_hip_dense_pack_walls(const hpgmg_hip_level *L, int id, const double *src, int axis, int check, int mask, double *wall, int *status) {
  *status = 0;
  if (axis < 0 || axis > 2 || mask < 0 || mask > 63 || !wall || L->periodic || L->dim_i != L->dim_j || L->dim_i != L->dim_k)
    return record_error(hipErrorInvalidValue, "dense_pack_walls: not a face array of a Dirichlet cube");
  const int ni = L->dim_i + (axis == 0), nj = L->dim_j + (axis == 1), nk = L->dim_k + (axis == 2);
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  int *flag;
  if (int e = status_begin(&flag)) return e;
  hipLaunchKernelGGL(dense_pack_walls_kernel, dense_grid(L->volume, L->num_boxes), dim3(kDenseThreads), 0, g_stream, *L, id, src, ni, nj, nk, check,
                     axis, (mask >> (2 * axis)) & 1, (mask >> (2 * axis + 1)) & 1, wall, flag);
  return status_end("dense_pack_walls_kernel", status);
}

int hpgmg_hip_dense_unpack(const hpgmg_hip_level *L, int id, double *dst) {
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  hipLaunchKernelGGL(dense_unpack_kernel, dense_grid(L->dim * L->dim * L->dim, L->num_boxes), dim3(kDenseThreads), 0, g_stream, *L, id, dst);
  HPGMG_LAUNCH_CHECK("dense_unpack_kernel");
  HPGMG_CHECK(hipStreamSynchronize(g_stream));      // the caller's array is complete on return (a torch tensor is read on another stream)
  return 0;
}

}  // extern "C"
