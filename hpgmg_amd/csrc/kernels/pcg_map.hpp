// pcg_map.hpp -- the ONE mapping and summation order of the CG passes (include/hpgmg_operators.h, the comment above hpgmg_pcg_apply_dot), for the files that
// stream in it: pcg.hip and dense_wave.hip.  A workgroup of 256 lanes owns 256 consecutive COLUMNS c = i + dim * j of one box over one SEGMENT of 16
// planes and marches it in +k; a lane's chain over its planes is a leaf, lanes fold with shuffles for stride 1 .. 32, the four waves through LDS for
// stride 64, 128, and pcg_fold (pcg.hip) folds the workgroups' values from stride 256 upwards in a second tiny launch.  One launch arithmetic to hold.
#pragma once
#include "reduce.hpp"

namespace hpgmg {

constexpr int kPcgLanes = HPGMG_PCG_COLUMNS, kPcgSeg = HPGMG_PCG_SEGMENT;

struct PcgItem { int item, box, k0, k1, c; bool live; };
__device__ __forceinline__ bool pcg_item(const hpgmg_hip_level &L, int nseg, int ncb, int per_xcd, int items, PcgItem &it) {
  const int item = xcd_logical_block((int)blockIdx.x, per_xcd);     // an XCD owns a contiguous run of items: rows shared by neighbouring items meet in its L2
  if (item >= items) return false;
  it.item = item;
  const int cb = item % ncb, s = (item / ncb) % nseg;
  it.box = item / (ncb * nseg);
  it.k0 = s * kPcgSeg; it.k1 = (it.k0 + kPcgSeg < L.dim) ? it.k0 + kPcgSeg : L.dim;
  it.c = cb * kPcgLanes + (int)threadIdx.x;
  it.live = it.c < L.dim * L.dim;
  return true;
}

// the tree below stride 256: V[m] = V[m] + V[m + stride], the value of the workgroup's 256 leaves in lane 0
__device__ __forceinline__ double pcg_block_sum(double v, double *smem) {
#pragma unroll
  for (int stride = 1; stride < 64; stride *= 2) v = v + __shfl_down(v, stride, 64);
  if (threadIdx.x % 64 == 0) smem[threadIdx.x / 64] = v;
  __syncthreads();
  const double lo = smem[0] + smem[1], hi = smem[2] + smem[3];
  return lo + hi;
}
// two such trees at once: one barrier for both (smem: 8 doubles)
__device__ __forceinline__ void pcg_block_sum2(double &v, double &w, double *smem) {
#pragma unroll
  for (int stride = 1; stride < 64; stride *= 2) { v = v + __shfl_down(v, stride, 64); w = w + __shfl_down(w, stride, 64); }
  if (threadIdx.x % 64 == 0) { smem[threadIdx.x / 64] = v; smem[4 + threadIdx.x / 64] = w; }
  __syncthreads();
  const double vlo = smem[0] + smem[1], vhi = smem[2] + smem[3], wlo = smem[4] + smem[5], whi = smem[6] + smem[7];
  v = vlo + vhi; w = wlo + whi;
}

struct PcgGrid { int nseg, ncb, items, per_xcd, grid; };
inline PcgGrid pcg_grid(const hpgmg_hip_level *L) {
  PcgGrid g;
  g.nseg = (L->dim + kPcgSeg - 1) / kPcgSeg;
  g.ncb = (L->dim * L->dim + kPcgLanes - 1) / kPcgLanes;
  g.items = g.ncb * g.nseg * L->num_boxes;
  g.grid = grid_for(g.items, &g.per_xcd);
  return g;
}
// what every launch in this mapping needs of the level: a box side and a number of workgroups the grid arithmetic holds
inline int pcg_geometry_ok(const hpgmg_hip_level *L) {
  if (L->num_boxes < 1 || L->dim < 1 || L->dim > 1024) return 0;
  return (long long)((L->dim * L->dim + kPcgLanes - 1) / kPcgLanes) * ((L->dim + kPcgSeg - 1) / kPcgSeg) * L->num_boxes < (1LL << 30) / kXcds;
}
// fold the scratch's one (out1 == nullptr) or two arrays of `items` values (the second at scratch + items) and wait for the sums (pcg.hip)
int pcg_fold(int items, double *out0, double *out1 = nullptr);

}  // namespace hpgmg
