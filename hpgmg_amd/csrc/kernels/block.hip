// block.hip -- fine-level block linear algebra for the eigen-solver of the user-problem API (include/hpgmg_operators.h hpgmg_block_*):
//   block_gram      G[i][j] = sum over the cells of (w) a_i b_j for up to 36 x 36 pairs: a lane carries a T x T tile of pair chains in registers, a
//                   cell costs 2 T loads (T on a diagonal tile, one more for the weight) for T^2 chains, and blockIdx.y walks the pair tiles
//   block_combine   out_j = sum_i C[i][j] in_i for up to 36 inputs and 12 outputs: nin reads and nout writes per cell, C in a device buffer
//   block_residual  r_j = ax_j - mu_j (w x_j) with max |r_j| and max |w x_j| for up to 12 columns in one launch
// One mapping for all three, pcg.hip's: a workgroup of 256 lanes owns 256 consecutive COLUMNS c = i + dim * j of one box over one SEGMENT of 16 planes
// and marches it in +k.  A lane's chain over its <= 16 planes is a leaf of the ONE stride-doubling tree of include/hpgmg_operators.h; lanes fold with
// shuffles for stride 1 .. 32, the four waves through LDS for stride 64, 128, and block_fold_kernel folds the workgroups' values from stride 256
// upwards, one workgroup per Gram entry -- pcg_fold_body's arithmetic, so an unweighted entry has the bits of hpgmg_hip_pcg_dot on its pair.
// (The lanes-own-pairs form of gram.hip stages cells through LDS and chains a box in k, j, i order: another order, and one workgroup per box.)
#include <string.h>
#include "reduce.hpp"

namespace hpgmg {

constexpr int kBlockLanes = HPGMG_PCG_COLUMNS, kBlockSeg = HPGMG_PCG_SEGMENT, kBlockFoldLanes = 1024;
constexpr int kBlockMaxIn = HPGMG_BLOCK_MAX_IN, kBlockMaxOut = HPGMG_BLOCK_MAX_OUT;
constexpr int kGramTile = HPGMG_HIP_BLOCK_TILE;                                        // T: the pair tile is T x T chains per lane
constexpr int kGramTilesSide = (kBlockMaxIn + kGramTile - 1) / kGramTile;
constexpr int kGramMaxTiles = kGramTilesSide * kGramTilesSide;

struct BlockItem { int item, box, k0, k1, c; bool live; };
__device__ __forceinline__ bool block_item(const hpgmg_hip_level &L, int nseg, int ncb, int per_xcd, int items, BlockItem &it) {
  const int item = xcd_logical_block((int)blockIdx.x, per_xcd);
  if (item >= items) return false;
  it.item = item;
  const int cb = item % ncb, s = (item / ncb) % nseg;
  it.box = item / (ncb * nseg);
  it.k0 = s * kBlockSeg; it.k1 = (it.k0 + kBlockSeg < L.dim) ? it.k0 + kBlockSeg : L.dim;
  it.c = cb * kBlockLanes + (int)threadIdx.x;
  it.live = it.c < L.dim * L.dim;
  return true;
}

// ---- the Gram matrix
struct GramArgs {
  int na, nb, w_id, ntiles, same;                // same: the two id lists are identical -- only tiles with tj >= ti are launched, the host mirrors
  int a[kBlockMaxIn], b[kBlockMaxIn];
  unsigned char ti[kGramMaxTiles], tj[kGramMaxTiles];
};

// one tile of pair chains over the lane's planes.  DIAG: the tile's a and b ids are the same list, so b's values are a's loads
template <int T, bool W, bool DIAG>
__device__ __forceinline__ void gram_tile_chains(const hpgmg_hip_level &L, const GramArgs &A, const BlockItem &it, int ta, int tb, double (&acc)[T][T]) {
  const int kS = L.kStride, col = it.c % L.dim + (it.c / L.dim) * L.jStride;
  gcptr pa[T], pb[T];
#pragma unroll
  for (int u = 0; u < T; u++) {                  // past the end of a list: its last vector again (loaded, never stored)
    pa[u] = gvec_origin(L, it.box, A.a[ta + u < A.na ? ta + u : A.na - 1]) + col;
    pb[u] = gvec_origin(L, it.box, A.b[tb + u < A.nb ? tb + u : A.nb - 1]) + col;
  }
  const gcptr pw = W ? gvec_origin(L, it.box, A.w_id) + col : pa[0];
  for (int k = it.k0; k < it.k1; k++) {
    const int o = k * kS;
    double va[T], vb[T];
#pragma unroll
    for (int u = 0; u < T; u++) va[u] = pa[u][o];
#pragma unroll
    for (int u = 0; u < T; u++) vb[u] = DIAG ? va[u] : pb[u][o];
    if (W) {
      const double w = pw[o];
#pragma unroll
      for (int u = 0; u < T; u++) va[u] = w * va[u];
    }
#pragma unroll
    for (int u = 0; u < T; u++)
#pragma unroll
      for (int v = 0; v < T; v++) { const double q = va[u] * vb[v]; acc[u][v] = acc[u][v] + q; }
  }
}

template <int T, bool W>
__global__ __launch_bounds__(kBlockLanes) void block_gram_kernel(const hpgmg_hip_level L, const GramArgs A, int nseg, int ncb, int per_xcd, int items,
                                                                  double *__restrict__ partials) {
  __shared__ double smem[T * T * 4];
  BlockItem it;
  if (!block_item(L, nseg, ncb, per_xcd, items, it)) return;
  const int ta = A.ti[blockIdx.y] * T, tb = A.tj[blockIdx.y] * T;
  double acc[T][T];
#pragma unroll
  for (int u = 0; u < T; u++)
#pragma unroll
    for (int v = 0; v < T; v++) acc[u][v] = 0.0;
  if (it.live) {
    if (A.same && ta == tb) gram_tile_chains<T, W, true>(L, A, it, ta, tb, acc);
    else gram_tile_chains<T, W, false>(L, A, it, ta, tb, acc);
  }
  // the tree below stride 256 for each of the T^2 chains: V[m] = V[m] + V[m + stride]
#pragma unroll
  for (int u = 0; u < T; u++)
#pragma unroll
    for (int v = 0; v < T; v++) {
      double s = acc[u][v];
#pragma unroll
      for (int stride = 1; stride < 64; stride *= 2) s = s + __shfl_down(s, stride, 64);
      if (threadIdx.x % 64 == 0) smem[(u * T + v) * 4 + threadIdx.x / 64] = s;
    }
  __syncthreads();
  const int e = (int)threadIdx.x;
  if (e < T * T) {
    const int i = ta + e / T, j = tb + e % T;
    if (i < A.na && j < A.nb) {
      const double lo = smem[4 * e] + smem[4 * e + 1], hi = smem[4 * e + 2] + smem[4 * e + 3];
      partials[(size_t)(i * A.nb + j) * items + it.item] = lo + hi;
    }
  }
}

// the tree from stride 256 upwards over the n workgroup values of entry blockIdx.x (partials[e n .. e n + n)), pcg_fold_body's arithmetic: a lane
// folds its own `chunk` (a power of two) consecutive values in place, then the 1024 lanes fold through LDS; entries past n are the padding's 0.0.
// same: entry (i, j < i) is not computed (the host copies it from (j, i)).
__global__ __launch_bounds__(kBlockFoldLanes) void block_fold_kernel(double *__restrict__ partials, int n, int chunk, int nb, int same, double *__restrict__ out) {
  __shared__ double smem[kBlockFoldLanes];
  const int e = (int)blockIdx.x, t = (int)threadIdx.x;
  if (same && e % nb < e / nb) return;
  double *P = partials + (size_t)e * n;
  const long long lo = (long long)t * chunk;
  for (int stride = 1; stride < chunk; stride *= 2)
    for (long long m = lo; m + stride < n && m < lo + chunk; m += 2 * stride) P[m] = P[m] + P[m + stride];
  smem[t] = (lo < n) ? P[lo] : 0.0;
  __syncthreads();
  for (int stride = 1; stride < kBlockFoldLanes; stride *= 2) {
    if (t % (2 * stride) == 0) smem[t] = smem[t] + smem[t + stride];
    __syncthreads();
  }
  if (t == 0) out[e] = smem[0];
}

// ---- the linear combination
struct CombineArgs { int nin, nout; int in[kBlockMaxIn], out[kBlockMaxOut]; };

// NO: the outputs a lane carries (nout rounded up; C has NO columns, the padding's 0.0); the chains of the padding are formed and dropped.
// kCombinePlanes: the cells of its column a lane works on at once (NO x kCombinePlanes chains in registers)
template <int NO, int kCombinePlanes>
__global__ __launch_bounds__(kBlockLanes) void block_combine_kernel(const hpgmg_hip_level L, const CombineArgs A, const double *__restrict__ C,
                                                                     int nseg, int ncb, int per_xcd, int items) {
  BlockItem it;
  if (!block_item(L, nseg, ncb, per_xcd, items, it) || !it.live) return;
  const int kS = L.kStride, col = it.c % L.dim + (it.c / L.dim) * L.jStride;
  // kCombinePlanes cells of the column at a time: their loads of one input are in flight together and share the input's row of C
  for (int k = it.k0; k < it.k1; k += kCombinePlanes) {
    int o[kCombinePlanes];
#pragma unroll
    for (int p = 0; p < kCombinePlanes; p++) o[p] = col + ((k + p < it.k1) ? k + p : it.k1 - 1) * kS;      // past the segment: its last cell again (loaded, never stored)
    double acc[kCombinePlanes][NO];
#pragma unroll
    for (int p = 0; p < kCombinePlanes; p++)
#pragma unroll
      for (int j = 0; j < NO; j++) acc[p][j] = 0.0;
    for (int i = 0; i < A.nin; i++) {
      const gcptr in = gvec_origin(L, it.box, A.in[i]);
      double v[kCombinePlanes];
#pragma unroll
      for (int p = 0; p < kCombinePlanes; p++) v[p] = in[o[p]];
#pragma unroll
      for (int j = 0; j < NO; j++) {
        const double c = C[i * NO + j];
#pragma unroll
        for (int p = 0; p < kCombinePlanes; p++) { const double q = c * v[p]; acc[p][j] = acc[p][j] + q; }
      }
    }
    // every input of these cells has been read: the outputs may be among them
#pragma unroll
    for (int j = 0; j < NO; j++) {
      if (j < A.nout) {
        const gptr out = gvec_origin(L, it.box, A.out[j]);
#pragma unroll
        for (int p = 0; p < kCombinePlanes; p++) if (k + p < it.k1) out[o[p]] = acc[p][j];
      }
    }
  }
}

// ---- the residuals
struct ResidualArgs { int n, w_id; int r[kBlockMaxOut], ax[kBlockMaxOut], x[kBlockMaxOut]; double mu[kBlockMaxOut]; };

// partials[q items + item]: q < n the workgroup's max |r_q|, n <= q < 2 n its max |w x_(q - n)|
template <bool W>
__global__ __launch_bounds__(kBlockLanes) void block_residual_kernel(const hpgmg_hip_level L, const ResidualArgs A, int nseg, int ncb, int per_xcd, int items,
                                                                      double *__restrict__ partials) {
  __shared__ double smem[2 * kBlockMaxOut * 4];
  BlockItem it;
  if (!block_item(L, nseg, ncb, per_xcd, items, it)) return;
  const int kS = L.kStride, col = it.c % L.dim + (it.c / L.dim) * L.jStride;
  for (int q = 0; q < A.n; q++) {
    double rbest = 0.0, mbest = 0.0;
    if (it.live) {
      const gptr r = gvec_origin(L, it.box, A.r[q]) + col;
      const gcptr ax = gvec_origin(L, it.box, A.ax[q]) + col, x = gvec_origin(L, it.box, A.x[q]) + col;
      const gcptr w = W ? gvec_origin(L, it.box, A.w_id) + col : x;
      const double mu = A.mu[q];
#pragma unroll 4
      for (int k = it.k0; k < it.k1; k++) {
        const int o = k * kS;
        const double xv = x[o], mx = W ? w[o] * xv : xv, t = mu * mx, rn = ax[o] - t;
        r[o] = rn;
        const double fr = fabs(rn), fm = fabs(mx);
        rbest = (fr > rbest) ? fr : rbest;
        mbest = (fm > mbest) ? fm : mbest;
      }
    }
    rbest = wave_max(rbest); mbest = wave_max(mbest);
    if (threadIdx.x % 64 == 0) { smem[4 * q + threadIdx.x / 64] = rbest; smem[4 * (A.n + q) + threadIdx.x / 64] = mbest; }
  }
  __syncthreads();
  const int e = (int)threadIdx.x;
  if (e < 2 * A.n) {
    double v = smem[4 * e];
    for (int w = 1; w < 4; w++) v = (smem[4 * e + w] > v) ? smem[4 * e + w] : v;
    partials[(size_t)e * items + it.item] = v;
  }
}

// the maximum of the n workgroup values of array blockIdx.x, from 0.0 (a NaN is never the maximum: final_max_kernel's comparison)
__global__ __launch_bounds__(256) void block_max_kernel(const double *__restrict__ partials, int n, double *__restrict__ out) {
  __shared__ double smem[4];
  const double *P = partials + (size_t)blockIdx.x * n;
  double m = 0.0;
  for (int t = (int)threadIdx.x; t < n; t += 256) m = (P[t] > m) ? P[t] : m;
  m = block_max<4>(m, smem);
  if (threadIdx.x == 0) out[blockIdx.x] = m;
}

struct BlockGrid { int nseg, ncb, items, per_xcd, grid; };
static BlockGrid block_grid(const hpgmg_hip_level *L) {
  BlockGrid g;
  g.nseg = (L->dim + kBlockSeg - 1) / kBlockSeg;
  g.ncb = (L->dim * L->dim + kBlockLanes - 1) / kBlockLanes;
  g.items = g.ncb * g.nseg * L->num_boxes;
  g.grid = grid_for(g.items, &g.per_xcd);
  return g;
}
static int block_ids_ok(const int *ids, int n, int max) {
  if (!ids || n < 1 || n > max) return 0;
  for (int q = 0; q < n; q++) if (ids[q] < 0) return 0;
  return 1;
}
// block_combine's C: two slots, each a pinned host array and its device copy (kBlockMaxIn x kBlockMaxOut doubles), used in turn.  A call fills the
// pinned array of its slot, copies it in stream order and launches; it waits only for the event of the copy that used the slot two calls ago, so the
// host does not stall per call.  Like the reduction scratch (reduce.hip) the slots belong to the device that is current at first use and live as long
// as the process.
struct CombineSlot { double *host, *dev; hipEvent_t copied; bool used; };
static CombineSlot g_block_C[2] = { { nullptr, nullptr, nullptr, false }, { nullptr, nullptr, nullptr, false } };
static unsigned g_block_C_next = 0;

}  // namespace hpgmg
using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

// a box side and a number of workgroups the grid arithmetic holds (the CG passes' bound), with room for 36 x 36 arrays of workgroup values
int hpgmg_hip_block_supported(const hpgmg_hip_level *L) {
  if (L->num_boxes < 1 || L->dim < 1 || L->dim > 1024) return 0;
  const long long items = (long long)((L->dim * L->dim + kBlockLanes - 1) / kBlockLanes) * ((L->dim + kBlockSeg - 1) / kBlockSeg) * L->num_boxes;
  return items < (1LL << 30) / kXcds && items * (kBlockMaxIn * kBlockMaxIn + 1) < (1LL << 31) - 1;
}
int hpgmg_hip_block_tile(void) { return kGramTile; }

int hpgmg_hip_block_gram(const hpgmg_hip_level *L, const int *a_ids, int na, const int *b_ids, int nb, int w_id, double *G_host) {
  if (!hpgmg_hip_block_supported(L) || !G_host || !block_ids_ok(a_ids, na, kBlockMaxIn) || !block_ids_ok(b_ids, nb, kBlockMaxIn))
    return record_error(hipErrorInvalidValue, "block_gram: level or id lists not supported");
  if (int e = hpgmg_hip_graph_flush()) return e;
  GramArgs A;
  memset(&A, 0, sizeof(A));
  A.na = na; A.nb = nb; A.w_id = w_id; A.same = (na == nb);
  for (int q = 0; q < na; q++) A.a[q] = a_ids[q];
  for (int q = 0; q < nb; q++) A.b[q] = b_ids[q];
  for (int q = 0; A.same && q < na; q++) A.same = (a_ids[q] == b_ids[q]);
  for (int ti = 0; ti * kGramTile < na; ti++)
    for (int tj = A.same ? ti : 0; tj * kGramTile < nb; tj++) { A.ti[A.ntiles] = (unsigned char)ti; A.tj[A.ntiles] = (unsigned char)tj; A.ntiles++; }
  const BlockGrid g = block_grid(L);
  const int entries = na * nb;
  double *partials = reduction_scratch(entries * g.items + entries);
  if (!partials) return record_error(hipErrorOutOfMemory, "block_gram: no scratch");
  double *sums = partials + (size_t)entries * g.items;
  if (w_id >= 0)
    hipLaunchKernelGGL((block_gram_kernel<kGramTile, true>), dim3(g.grid, A.ntiles), dim3(kBlockLanes), 0, g_stream, *L, A, g.nseg, g.ncb, g.per_xcd, g.items, partials);
  else
    hipLaunchKernelGGL((block_gram_kernel<kGramTile, false>), dim3(g.grid, A.ntiles), dim3(kBlockLanes), 0, g_stream, *L, A, g.nseg, g.ncb, g.per_xcd, g.items, partials);
  HPGMG_LAUNCH_CHECK("block_gram_kernel");
  int chunk = 1;
  while ((long long)chunk * kBlockFoldLanes < g.items) chunk *= 2;
  hipLaunchKernelGGL(block_fold_kernel, dim3(entries), dim3(kBlockFoldLanes), 0, g_stream, partials, g.items, chunk, nb, A.same, sums);
  HPGMG_LAUNCH_CHECK("block_fold_kernel");
  HPGMG_CHECK(hipMemcpyAsync(G_host, sums, (size_t)entries * sizeof(double), hipMemcpyDeviceToHost, g_stream));
  HPGMG_CHECK(hipStreamSynchronize(g_stream));
  if (A.same) for (int i = 0; i < na; i++) for (int j = 0; j < i; j++) G_host[i * nb + j] = G_host[j * nb + i];
  return 0;
}

int hpgmg_hip_block_combine(const hpgmg_hip_level *L, const int *out_ids, int nout, const int *in_ids, int nin, const double *C_host) {
  if (!hpgmg_hip_block_supported(L) || !C_host || !block_ids_ok(out_ids, nout, kBlockMaxOut) || !block_ids_ok(in_ids, nin, kBlockMaxIn))
    return record_error(hipErrorInvalidValue, "block_combine: level or id lists not supported");
  for (int p = 0; p < nout; p++) for (int q = 0; q < p; q++) if (out_ids[p] == out_ids[q]) return record_error(hipErrorInvalidValue, "block_combine: repeated outputs");
  if (int e = hpgmg_hip_graph_flush()) return e;
  CombineArgs A;
  memset(&A, 0, sizeof(A));
  A.nin = nin; A.nout = nout;
  for (int q = 0; q < nin; q++) A.in[q] = in_ids[q];
  for (int q = 0; q < nout; q++) A.out[q] = out_ids[q];
  const int NO = nout <= 4 ? 4 : nout <= 8 ? 8 : kBlockMaxOut;
  CombineSlot &slot = g_block_C[g_block_C_next++ & 1];
  if (!slot.host) {
    HPGMG_CHECK(hipHostMalloc((void **)&slot.host, kBlockMaxIn * kBlockMaxOut * sizeof(double), hipHostMallocDefault));
    HPGMG_CHECK(hipMalloc((void **)&slot.dev, kBlockMaxIn * kBlockMaxOut * sizeof(double)));
    HPGMG_CHECK(hipEventCreateWithFlags(&slot.copied, hipEventDisableTiming));
  }
  if (slot.used) HPGMG_CHECK(hipEventSynchronize(slot.copied));        // the copy that last read this pinned array has run
  double *C = slot.host;
  for (int i = 0; i < nin; i++) for (int j = 0; j < NO; j++) C[i * NO + j] = j < nout ? C_host[i * nout + j] : 0.0;
  HPGMG_CHECK(hipMemcpyAsync(slot.dev, C, (size_t)nin * NO * sizeof(double), hipMemcpyHostToDevice, g_stream));      // in stream order: after the launch that read this slot's last C
  HPGMG_CHECK(hipEventRecord(slot.copied, g_stream));
  slot.used = true;
  const BlockGrid g = block_grid(L);
  if (NO == 4) hipLaunchKernelGGL((block_combine_kernel<4, 4>), dim3(g.grid), dim3(kBlockLanes), 0, g_stream, *L, A, (const double *)slot.dev, g.nseg, g.ncb, g.per_xcd, g.items);
  else if (NO == 8) hipLaunchKernelGGL((block_combine_kernel<8, 4>), dim3(g.grid), dim3(kBlockLanes), 0, g_stream, *L, A, (const double *)slot.dev, g.nseg, g.ncb, g.per_xcd, g.items);
  else hipLaunchKernelGGL((block_combine_kernel<kBlockMaxOut, 4>), dim3(g.grid), dim3(kBlockLanes), 0, g_stream, *L, A, (const double *)slot.dev, g.nseg, g.ncb, g.per_xcd, g.items);
  HPGMG_LAUNCH_CHECK("block_combine_kernel");
  return 0;
}

int hpgmg_hip_block_residual(const hpgmg_hip_level *L, const int *r_ids, const int *ax_ids, const int *x_ids, int n, int w_id, const double *mu,
                             double *rmax, double *mxmax) {
  if (!hpgmg_hip_block_supported(L) || !mu || !rmax || !mxmax || !block_ids_ok(r_ids, n, kBlockMaxOut) || !block_ids_ok(ax_ids, n, kBlockMaxOut) ||
      !block_ids_ok(x_ids, n, kBlockMaxOut))
    return record_error(hipErrorInvalidValue, "block_residual: level or id lists not supported");
  if (int e = hpgmg_hip_graph_flush()) return e;
  ResidualArgs A;
  memset(&A, 0, sizeof(A));
  A.n = n; A.w_id = w_id;
  for (int q = 0; q < n; q++) { A.r[q] = r_ids[q]; A.ax[q] = ax_ids[q]; A.x[q] = x_ids[q]; A.mu[q] = mu[q]; }
  const BlockGrid g = block_grid(L);
  double *partials = reduction_scratch(2 * n * g.items + 2 * n);
  if (!partials) return record_error(hipErrorOutOfMemory, "block_residual: no scratch");
  double *best = partials + (size_t)2 * n * g.items;
  if (w_id >= 0) hipLaunchKernelGGL((block_residual_kernel<true>), dim3(g.grid), dim3(kBlockLanes), 0, g_stream, *L, A, g.nseg, g.ncb, g.per_xcd, g.items, partials);
  else hipLaunchKernelGGL((block_residual_kernel<false>), dim3(g.grid), dim3(kBlockLanes), 0, g_stream, *L, A, g.nseg, g.ncb, g.per_xcd, g.items, partials);
  HPGMG_LAUNCH_CHECK("block_residual_kernel");
  hipLaunchKernelGGL(block_max_kernel, dim3(2 * n), dim3(256), 0, g_stream, (const double *)partials, g.items, best);
  HPGMG_LAUNCH_CHECK("block_max_kernel");
  double host[2 * kBlockMaxOut];
  HPGMG_CHECK(hipMemcpyAsync(host, best, (size_t)2 * n * sizeof(double), hipMemcpyDeviceToHost, g_stream));
  HPGMG_CHECK(hipStreamSynchronize(g_stream));
  for (int q = 0; q < n; q++) { rmax[q] = host[q]; mxmax[q] = host[n + q]; }
  return 0;
}

}  // extern "C"
