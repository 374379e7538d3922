// pcg.hip -- the fine-level passes of the V-cycle-preconditioned CG of the user-problem API (include/hpgmg_operators.h hpgmg_pcg_*):
//   pcg_apply_dot  Ap = A p (7-point, variable coefficients) and p . Ap in one pass: per cell p, three betas (alpha with Helmholtz) in, Ap out
//   pcg_update     x = x + alpha p ; r = r - alpha Ap ; max |r|: four reads, two writes
//   pcg_dot        a . b
//   pcg_dot2       a . b and c . b from one read of the three vectors (the flexible CG's r . z and Ap . z): 24 B per cell for 32
// One mapping for all four: a workgroup of 256 lanes owns 256 consecutive COLUMNS c = i + dim * j of one box (consecutive lanes on consecutive
// doubles of a row) over one SEGMENT of 16 planes, and marches it in +k.  That is the summation order of the header: a lane's chain over its <= 16
// planes is a leaf; lanes fold with shuffles for stride 1 .. 32, the four waves through LDS for stride 64, 128 -- the lower levels of the ONE
// stride-doubling tree over the leaves V[c + W (s + S box)] -- and pcg_fold_kernel folds the workgroups' values (stride 256 upwards) in a second tiny
// launch (a last-workgroup form needs an agent-scope fence per workgroup: blas1.hip measured that 4x slower).  Lanes past dim^2 carry the tree's 0.0.
// The stencil reads a face neighbour where it lives (common.hpp: box_nbr) and a Dirichlet face as -x(centre): apply_op's ghost-free rule, same bits.
#include "pcg_map.hpp"
#include "stencil_math.hpp"

namespace hpgmg {

constexpr int kFoldLanes = 1024;

// where lane (i, j) of box `box` reads its neighbour across face `face` when that neighbour lies outside the box: the column (pointer to its plane 0;
// for the k faces to the cell itself) in the box next door, or -- Dirichlet domain face -- nowhere: the value is -x(centre) (apply_BCs_p1's)
struct PcgNeighbour { gcptr p; bool dirichlet; };
__device__ __forceinline__ PcgNeighbour pcg_outside(const hpgmg_hip_level &L, int box, int id, int face, int i, int j, int k, gcptr own) {
  const int n = L.box_nbr[6 * box + face];
  PcgNeighbour r;
  r.dirichlet = (n == -1);
  if (n < 0) { r.p = own; return r; }             // -1: any valid address (the value is not used); -2 never reaches these kernels (every face is local)
  if (face == 0) i += L.dim; else if (face == 1) i -= L.dim; else if (face == 2) j += L.dim; else if (face == 3) j -= L.dim; else if (face == 4) k += L.dim; else k -= L.dim;
  r.p = gvec_origin(L, n, id) + (i + j * L.jStride + k * L.kStride);
  return r;
}

template <int V>
__global__ __launch_bounds__(kPcgLanes) void pcg_apply_dot_kernel(const hpgmg_hip_level L, int Ap_id, int p_id, double a, double b, double h2inv,
                                                                   int nseg, int ncb, int per_xcd, int items, double *__restrict__ partials) {
  __shared__ double smem[4];
  PcgItem it;
  if (!pcg_item(L, nseg, ncb, per_xcd, items, it)) return;
  double chain = 0.0;
  if (it.live) {
    const int dim = L.dim, jS = L.jStride, kS = L.kStride, i = it.c % dim, j = it.c / dim, col = i + j * jS;
    const gcptr x = gvec_origin(L, it.box, p_id) + col;
    const gptr y = gvec_origin(L, it.box, Ap_id) + col;
    const gcptr bi = gvec_origin(L, it.box, VECTOR_BETA_I) + col, bj = gvec_origin(L, it.box, VECTOR_BETA_J) + col, bk = gvec_origin(L, it.box, VECTOR_BETA_K) + col;
    const gcptr al = (V == HPGMG_HIP_7PT_VC_HELMHOLTZ) ? gvec_origin(L, it.box, VECTOR_ALPHA) + col : x;
    // the four lateral neighbours: columns of this box, or of the box next door (plane 0 of the column in both cases)
    PcgNeighbour im = { x - 1, false }, ip = { x + 1, false }, jm = { x - jS, false }, jp = { x + jS, false };
    if (i == 0)       im = pcg_outside(L, it.box, p_id, 0, -1, j, 0, x);
    if (i == dim - 1) ip = pcg_outside(L, it.box, p_id, 1, dim, j, 0, x);
    if (j == 0)       jm = pcg_outside(L, it.box, p_id, 2, i, -1, 0, x);
    if (j == dim - 1) jp = pcg_outside(L, it.box, p_id, 3, i, dim, 0, x);
    // below the first and above the last plane of the segment: this column, or across a k face
    PcgNeighbour below = { x + (it.k0 - 1) * kS, false }, above = { x + it.k1 * kS, false };
    if (it.k0 == 0)   below = pcg_outside(L, it.box, p_id, 4, i, j, -1, x);
    if (it.k1 == dim) above = pcg_outside(L, it.box, p_id, 5, i, j, dim, x);
    const double x_above = *above.p;
    double xc = x[it.k0 * kS];
    double xkm = below.dirichlet ? -xc : *below.p;
    double bk0 = bk[it.k0 * kS];
    for (int k = it.k0; k < it.k1; k++) {
      const int o = k * kS;
      const double xkp = (k + 1 < it.k1) ? x[o + kS] : (above.dirichlet ? -xc : x_above);
      const double vim = im.p[o], vip = ip.p[o], vjm = jm.p[o], vjp = jp.p[o];
      const double xim = im.dirichlet ? -xc : vim, xip = ip.dirichlet ? -xc : vip, xjm = jm.dirichlet ? -xc : vjm, xjp = jp.dirichlet ? -xc : vjp;
      const double bk1 = bk[o + kS];
      const double alpha = (V == HPGMG_HIP_7PT_VC_HELMHOLTZ) ? al[o] : 0.0;
      const double Ax = apply_op_7pt<V>(xc, xim, xip, xjm, xjp, xkm, xkp, bi[o], bi[o + 1], bj[o], bj[o + jS], bk0, bk1, alpha, a, b, h2inv);
      y[o] = Ax;
      const double q = xc * Ax;
      chain = chain + q;
      xkm = xc; xc = xkp; bk0 = bk1;
    }
  }
  const double sum = pcg_block_sum(chain, smem);
  if (threadIdx.x == 0) partials[it.item] = sum;
}

__global__ __launch_bounds__(kPcgLanes) void pcg_update_kernel(const hpgmg_hip_level L, int x_id, int r_id, int p_id, int Ap_id, double alpha,
                                                                int nseg, int ncb, int per_xcd, int items, double *__restrict__ partials) {
  __shared__ double smem[4];
  PcgItem it;
  if (!pcg_item(L, nseg, ncb, per_xcd, items, it)) return;
  double best = 0.0;
  if (it.live) {
    const int kS = L.kStride, col = it.c % L.dim + (it.c / L.dim) * L.jStride;
    const gptr x = gvec_origin(L, it.box, x_id) + col, r = gvec_origin(L, it.box, r_id) + col;
    const gcptr p = gvec_origin(L, it.box, p_id) + col, Ap = gvec_origin(L, it.box, Ap_id) + col;
#pragma unroll 4
    for (int k = it.k0; k < it.k1; k++) {
      const int o = k * kS;
      const double dx = alpha * p[o], dr = alpha * Ap[o];
      const double xn = x[o] + dx, rn = r[o] - dr;
      x[o] = xn; r[o] = rn;
      const double f = fabs(rn);
      best = (f > best) ? f : best;
    }
  }
  block_max_store<4>(best, smem, partials, it.item);
}

__global__ __launch_bounds__(kPcgLanes) void pcg_dot_kernel(const hpgmg_hip_level L, int a_id, int b_id, int nseg, int ncb, int per_xcd, int items,
                                                             double *__restrict__ partials) {
  __shared__ double smem[4];
  PcgItem it;
  if (!pcg_item(L, nseg, ncb, per_xcd, items, it)) return;
  double chain = 0.0;
  if (it.live) {
    const int kS = L.kStride, col = it.c % L.dim + (it.c / L.dim) * L.jStride;
    const gcptr va = gvec_origin(L, it.box, a_id) + col, vb = gvec_origin(L, it.box, b_id) + col;
#pragma unroll 4
    for (int k = it.k0; k < it.k1; k++) {
      const double q = va[k * kS] * vb[k * kS];
      chain = chain + q;
    }
  }
  const double sum = pcg_block_sum(chain, smem);
  if (threadIdx.x == 0) partials[it.item] = sum;
}

// the workgroups' values of a . b go to partials[item], those of c . b to partials[items + item]: two arrays for the one fold launch below
__global__ __launch_bounds__(kPcgLanes) void pcg_dot2_kernel(const hpgmg_hip_level L, int a_id, int c_id, int b_id, int nseg, int ncb, int per_xcd, int items,
                                                              double *__restrict__ partials) {
  __shared__ double smem[8];
  PcgItem it;
  if (!pcg_item(L, nseg, ncb, per_xcd, items, it)) return;
  double chain_a = 0.0, chain_c = 0.0;
  if (it.live) {
    const int kS = L.kStride, col = it.c % L.dim + (it.c / L.dim) * L.jStride;
    const gcptr va = gvec_origin(L, it.box, a_id) + col, vc = gvec_origin(L, it.box, c_id) + col, vb = gvec_origin(L, it.box, b_id) + col;
#pragma unroll 4
    for (int k = it.k0; k < it.k1; k++) {
      const double vbk = vb[k * kS];
      const double qa = va[k * kS] * vbk, qc = vc[k * kS] * vbk;
      chain_a = chain_a + qa;
      chain_c = chain_c + qc;
    }
  }
  pcg_block_sum2(chain_a, chain_c, smem);
  if (threadIdx.x == 0) { partials[it.item] = chain_a; partials[items + it.item] = chain_c; }
}

// the tree from stride 256 upwards over the workgroups' values, for N arrays of n values at once (partials[q n .. q n + n), q < N): a lane folds its own
// `chunk` (a power of two) consecutive ones in place -- an aligned run of the stride-doubling tree, which no other lane touches -- then the 1024 lanes
// fold through LDS (an array of 8 KB per q, the barriers of one fold); entries past n are the padding's 0.0.  The sum of array 0 is the launch's value,
// that of array 1 its second value: the one sequence number publishes both.
template <int N>
__device__ __forceinline__ void pcg_fold_body(double *__restrict__ partials, int n, int chunk, ResultSlot *result, unsigned long long seq) {
  __shared__ double smem[N][kFoldLanes];
  const int t = (int)threadIdx.x;
  const long long lo = (long long)t * chunk;
  for (int q = 0; q < N; q++) {
    double *P = partials + (long long)q * n;
    for (int stride = 1; stride < chunk; stride *= 2)
      for (long long m = lo; m + stride < n && m < lo + chunk; m += 2 * stride) P[m] = P[m] + P[m + stride];      // past n: + 0.0, which changes no bit
    smem[q][t] = (lo < n) ? P[lo] : 0.0;
  }
  __syncthreads();
  for (int stride = 1; stride < kFoldLanes; stride *= 2) {
    if (t % (2 * stride) == 0) for (int q = 0; q < N; q++) smem[q][t] = smem[q][t] + smem[q][t + stride];
    __syncthreads();
  }
  if (t == 0) { if constexpr (N == 2) publish2(result, smem[0][0], smem[1][0], seq); else publish(result, smem[0][0], seq); }
}
__global__ __launch_bounds__(kFoldLanes) void pcg_fold_kernel(double *__restrict__ partials, int n, int chunk, ResultSlot *result, unsigned long long seq) {
  pcg_fold_body<1>(partials, n, chunk, result, seq);
}
__global__ __launch_bounds__(kFoldLanes) void pcg_fold2_kernel(double *__restrict__ partials, int n, int chunk, ResultSlot *result, unsigned long long seq) {
  pcg_fold_body<2>(partials, n, chunk, result, seq);
}

// fold the scratch's one (out1 == nullptr) or two arrays of `items` values and wait for the sums
int pcg_fold(int items, double *out0, double *out1) {
  int chunk = 1;
  while ((long long)chunk * kFoldLanes < items) chunk *= 2;
  Scalar t;
  if (int e = scalar_begin(&t)) return e;
  hipLaunchKernelGGL(out1 ? pcg_fold2_kernel : pcg_fold_kernel, dim3(1), dim3(kFoldLanes), 0, g_stream, reduction_scratch((out1 ? 2 : 1) * items), items, chunk, t.slot, t.seq);
  HPGMG_LAUNCH_CHECK("pcg_fold_kernel");
  return scalar_wait(t, out0, out1);
}

}  // namespace hpgmg
using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

int hpgmg_hip_pcg_supported(const hpgmg_hip_level *L, int variant) {
  if (variant != HPGMG_HIP_7PT_VC_HELMHOLTZ && variant != HPGMG_HIP_7PT_VC_POISSON) return 0;
  if (!L->box_nbr || L->ghosts < 1) return 0;
  return pcg_geometry_ok(L);
}

int hpgmg_hip_pcg_apply_dot(const hpgmg_hip_level *L, int variant, int Ap_id, int p_id, double a, double b, double h2inv, double *dot) {
  *dot = 0.0;
  if (!hpgmg_hip_pcg_supported(L, variant) || Ap_id == p_id) return record_error(hipErrorInvalidValue, "pcg_apply_dot: level or vectors not supported");
  if (int e = hpgmg_hip_graph_flush()) return e;
  const PcgGrid g = pcg_grid(L);
  double *partials = reduction_scratch(g.items);
  if (!partials) return record_error(hipErrorOutOfMemory, "pcg_apply_dot: no scratch");
  if (variant == HPGMG_HIP_7PT_VC_HELMHOLTZ)
    hipLaunchKernelGGL((pcg_apply_dot_kernel<HPGMG_HIP_7PT_VC_HELMHOLTZ>), dim3(g.grid), dim3(kPcgLanes), 0, g_stream, *L, Ap_id, p_id, a, b, h2inv, g.nseg, g.ncb, g.per_xcd, g.items, partials);
  else
    hipLaunchKernelGGL((pcg_apply_dot_kernel<HPGMG_HIP_7PT_VC_POISSON>), dim3(g.grid), dim3(kPcgLanes), 0, g_stream, *L, Ap_id, p_id, a, b, h2inv, g.nseg, g.ncb, g.per_xcd, g.items, partials);
  HPGMG_LAUNCH_CHECK("pcg_apply_dot_kernel");
  return pcg_fold(g.items, dot);
}

int hpgmg_hip_pcg_update(const hpgmg_hip_level *L, int x_id, int r_id, int p_id, int Ap_id, double alpha, double *rmax) {
  *rmax = 0.0;
  if (!pcg_geometry_ok(L) || x_id == r_id) return record_error(hipErrorInvalidValue, "pcg_update: level or vectors not supported");
  if (int e = hpgmg_hip_graph_flush()) return e;
  const PcgGrid g = pcg_grid(L);
  double *partials = reduction_scratch(g.items);
  if (!partials) return record_error(hipErrorOutOfMemory, "pcg_update: no scratch");
  hipLaunchKernelGGL(pcg_update_kernel, dim3(g.grid), dim3(kPcgLanes), 0, g_stream, *L, x_id, r_id, p_id, Ap_id, alpha, g.nseg, g.ncb, g.per_xcd, g.items, partials);
  HPGMG_LAUNCH_CHECK("pcg_update_kernel");
  return max_of_partials(g.items, 0.0, rmax);
}

int hpgmg_hip_pcg_dot(const hpgmg_hip_level *L, int a_id, int b_id, double *dot) {
  *dot = 0.0;
  if (!pcg_geometry_ok(L)) return record_error(hipErrorInvalidValue, "pcg_dot: level not supported");
  if (int e = hpgmg_hip_graph_flush()) return e;
  const PcgGrid g = pcg_grid(L);
  double *partials = reduction_scratch(g.items);
  if (!partials) return record_error(hipErrorOutOfMemory, "pcg_dot: no scratch");
  hipLaunchKernelGGL(pcg_dot_kernel, dim3(g.grid), dim3(kPcgLanes), 0, g_stream, *L, a_id, b_id, g.nseg, g.ncb, g.per_xcd, g.items, partials);
  HPGMG_LAUNCH_CHECK("pcg_dot_kernel");
  return pcg_fold(g.items, dot);
}

int hpgmg_hip_pcg_dot2(const hpgmg_hip_level *L, int a_id, int c_id, int b_id, double *ab, double *cb) {
  *ab = *cb = 0.0;
  if (!pcg_geometry_ok(L)) return record_error(hipErrorInvalidValue, "pcg_dot2: level not supported");
  if (int e = hpgmg_hip_graph_flush()) return e;
  const PcgGrid g = pcg_grid(L);
  double *partials = reduction_scratch(2 * g.items);
  if (!partials) return record_error(hipErrorOutOfMemory, "pcg_dot2: no scratch");
  hipLaunchKernelGGL(pcg_dot2_kernel, dim3(g.grid), dim3(kPcgLanes), 0, g_stream, *L, a_id, c_id, b_id, g.nseg, g.ncb, g.per_xcd, g.items, partials);
  HPGMG_LAUNCH_CHECK("pcg_dot2_kernel");
  return pcg_fold(g.items, ab, cb);
}

}  // extern "C"
