// dense_step.hip -- the two streaming passes of the implicit time march of the dense-array solver (include/hpgmg_operators.h hpgmg_step_rhs,
// hpgmg_step_rate).  The two cell expressions the host defaults (host/hooks_host.inc) must match bit for bit are not written here
// but in include/hpgmg_step_math.h, which both compile.
//
//   step_rhs   F = F + ((a alpha) u + c w) ; u_old = u                     4 reads, 2 writes: 48 B per cell
//   step_rate  w = (r + (a alpha) (u - u_old)) - c w ; max |w|             5 reads, 1 write:  48 B per cell
//
// Mapped as kernels/dense_flux.hip: one lane per interior cell, grid row y = box, inside a box k, j, i with consecutive lanes on consecutive i
// (32-bit offsets inside a box), grid stride over both axes.  Ghost and padding cells are neither read nor written.  The grid is capped near
// 16 workgroups per CU; a lane takes the rest of its box by stride, every trip six independent accesses.  step_rate leaves one maximum per workgroup
// in the reduction scratch of kernels/reduce.hip, whose final_max_kernel folds them and publishes the value: a maximum has no order, so the result
// does not depend on the launch shape.  A NaN never becomes the maximum (f > m is false for it), as in pcg_update_kernel.
#include "reduce.hpp"
#include "hpgmg_step_math.h"

namespace hpgmg {

constexpr int kStepThreads = 256;
constexpr int kStepMaxBlocks = 4096;            // 256 CUs x 16: what the launch is capped to (either axis by grid stride)

// offset of interior cell c (k, j, i order) of a box from its first interior cell; sh = log2(dim) when dim is a power of two, else -1
__device__ __forceinline__ int step_offset(int c, int dim, int sh, int jS, int kS) {
  int i, j, k;
  if (sh >= 0) { i = c & (dim - 1); j = (c >> sh) & (dim - 1); k = c >> (2 * sh); }
  else { const int plane = dim * dim; k = c / plane; j = (c - k * plane) / dim; i = c - k * plane - j * dim; }
  return i + j * jS + k * kS;
}

__global__ __launch_bounds__(kStepThreads) void step_rhs_kernel(const hpgmg_hip_level L, int F_id, int u_id, int uold_id, int w_id, double a, double c,
                                                                int sh) {
  const int dim = L.dim, cells = dim * dim * dim, jS = L.jStride, kS = L.kStride;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const gptr F = gvec_origin(L, box, F_id), uold = gvec_origin(L, box, uold_id);
    const gcptr al = gvec_origin(L, box, VECTOR_ALPHA), u = gvec_origin(L, box, u_id), w = gvec_origin(L, box, w_id);
    for (int q = (int)(blockIdx.x * kStepThreads + threadIdx.x); q < cells; q += (int)(gridDim.x * kStepThreads)) {
      const int o = step_offset(q, dim, sh, jS, kS);
      const double uc = u[o];
      F[o] = step_rhs_cell(F[o], al[o], uc, w[o], a, c);
      uold[o] = uc;
    }
  }
}

__global__ __launch_bounds__(kStepThreads) void step_rate_kernel(const hpgmg_hip_level L, int w_id, int r_id, int u_id, int uold_id, double a, double c,
                                                                 int sh, double *__restrict__ partials) {
  __shared__ double smem[kStepThreads / 64];
  const int dim = L.dim, cells = dim * dim * dim, jS = L.jStride, kS = L.kStride;
  double best = 0.0;
  for (int box = (int)blockIdx.y; box < L.num_boxes; box += (int)gridDim.y) {
    const gptr w = gvec_origin(L, box, w_id);
    const gcptr al = gvec_origin(L, box, VECTOR_ALPHA), r = gvec_origin(L, box, r_id), u = gvec_origin(L, box, u_id), uold = gvec_origin(L, box, uold_id);
    for (int q = (int)(blockIdx.x * kStepThreads + threadIdx.x); q < cells; q += (int)(gridDim.x * kStepThreads)) {
      const int o = step_offset(q, dim, sh, jS, kS);
      const double wn = step_rate_cell(r[o], al[o], u[o], uold[o], w[o], a, c);
      w[o] = wn;
      const double f = fabs(wn);
      best = (f > best) ? f : best;
    }
  }
  // (the fold in place, not block_max_store: that form changes this kernel's scalar register count)
  best = wave_max(best);
  if (threadIdx.x % 64 == 0) smem[threadIdx.x / 64] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = smem[0];
    for (int v = 1; v < kStepThreads / 64; v++) m = (smem[v] > m) ? smem[v] : m;
    partials[blockIdx.x + gridDim.x * blockIdx.y] = m;
  }
}

// the level is one the two kernels take: cubic boxes whose cell count fits the 32-bit cell index; the ids name vectors of the level's boxes
static const char *step_refusal(const hpgmg_hip_level *L, const int *ids, int n, int num_vectors) {
  if (L->dim < 1 || L->dim > 1024 || L->ghosts < 0) return "the box side is not in 1 .. 1024";
  if (num_vectors <= VECTOR_ALPHA) return "the level has no alpha vector";
  for (int q = 0; q < n; q++) if (ids[q] < 0 || ids[q] >= num_vectors) return "a vector id is outside the level's vectors";
  return nullptr;
}
static dim3 step_grid(const hpgmg_hip_level *L) {
  const int cells = L->dim * L->dim * L->dim, per_box = (cells + kStepThreads - 1) / kStepThreads;
  const int gy = L->num_boxes < kStepMaxBlocks ? L->num_boxes : kStepMaxBlocks, cap = kStepMaxBlocks / gy;
  return dim3(per_box < cap ? per_box : cap, gy);
}
static int step_shift(int dim) { return (dim & (dim - 1)) == 0 ? __builtin_ctz(dim) : -1; }

}  // namespace hpgmg

using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

int hpgmg_hip_step_rhs(const hpgmg_hip_level *L, int num_vectors, int F_id, int u_id, int uold_id, int w_id, double a, double c) {
  const int ids[4] = { F_id, u_id, uold_id, w_id };
  if (const char *why = step_refusal(L, ids, 4, num_vectors)) return record_error(hipErrorInvalidValue, why);
  if (F_id == u_id || F_id == uold_id || F_id == w_id || uold_id == u_id || uold_id == w_id) return record_error(hipErrorInvalidValue, "step_rhs: an output vector is also an operand");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  hipLaunchKernelGGL(step_rhs_kernel, step_grid(L), dim3(kStepThreads), 0, g_stream, *L, F_id, u_id, uold_id, w_id, a, c, step_shift(L->dim));
  HPGMG_LAUNCH_CHECK("step_rhs_kernel");
  return 0;
}

int hpgmg_hip_step_rate(const hpgmg_hip_level *L, int num_vectors, int w_id, int r_id, int u_id, int uold_id, double a, double c, double *max_abs) {
  const int ids[4] = { w_id, r_id, u_id, uold_id };
  *max_abs = 0.0;
  if (const char *why = step_refusal(L, ids, 4, num_vectors)) return record_error(hipErrorInvalidValue, why);
  if (w_id == r_id || w_id == u_id || w_id == uold_id) return record_error(hipErrorInvalidValue, "step_rate: the rate vector is also an operand");
  if (int e = hpgmg_hip_graph_flush()) return e;
  if (L->num_boxes <= 0) return 0;
  const dim3 grid = step_grid(L);
  const int blocks = (int)(grid.x * grid.y);
  double *partials = reduction_scratch(blocks);
  if (!partials) return record_error(hipErrorOutOfMemory, "step_rate: no scratch");
  hipLaunchKernelGGL(step_rate_kernel, grid, dim3(kStepThreads), 0, g_stream, *L, w_id, r_id, u_id, uold_id, a, c, step_shift(L->dim), partials);
  HPGMG_LAUNCH_CHECK("step_rate_kernel");
  return max_of_partials(blocks, 0.0, max_abs);
}

}  // extern "C"
