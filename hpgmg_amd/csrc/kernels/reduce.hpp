// reduce.hpp -- the one home of scalar results: the wave / workgroup maximum every kernel folds with, the pinned host slot a
// kernel publishes a scalar to, the ticket the host waits on, the scratch of per-workgroup partials and the device status word
// (host side: reduce.hip).
#pragma once
#include <cstddef>
#include "common.hpp"

namespace hpgmg {

// ---- device side -------------------------------------------------------------------------------
// (a maximum is exact under any order, misc.c:307-317: the shape of these folds is free)
__device__ __forceinline__ double wave_max(double v) {             // the maximum of a wave's 64 lanes, in lane 0
  for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(v, off, 64); v = (o > v) ? o : v; }
  return v;
}
// the maximum of a workgroup of WAVES waves, in thread 0 (tid: the linear thread id): lane 0 of each wave writes smem[wave], one
// barrier, thread 0 folds in wave order.  smem (WAVES doubles) may be LDS the kernel used before: the caller places the barrier
// that ends those reads
template <int WAVES>
__device__ __forceinline__ double block_max(double v, double *smem, int tid = (int)threadIdx.x) {
  v = wave_max(v);
  if ((tid & 63) == 0) smem[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) for (int w = 1; w < WAVES; w++) v = (smem[w] > v) ? smem[w] : v;
  return v;
}
template <int WAVES>
__device__ __forceinline__ void block_max_store(double v, double *smem, double *partials, int index) {
  v = block_max<WAVES>(v, smem);
  if (threadIdx.x == 0) partials[index] = v;
}

// Scalar results go straight to a pinned host record: the last lane stores the value (and the second one of a launch that ends in
// two), fences at system scope, then stores the launch's sequence number; the host polls the number instead of paying a full
// stream synchronisation (reductions gate the host-driven BiCGStab).  The pinned allocation is one 64-byte line of two records,
// "immediate" and "deferred" (byte 32): a scalar the caller collects later does not share a record with those it waits for now.
struct alignas(32) ResultSlot { double value; unsigned long long seq; double second; };
static_assert(sizeof(ResultSlot) == 32 && offsetof(ResultSlot, seq) == 8 && offsetof(ResultSlot, second) == 16, "the slot's layout");
__device__ __forceinline__ void publish_seq(ResultSlot *slot, unsigned long long seq) {      // after the launch's last value
  __threadfence_system();
  __hip_atomic_store(&slot->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ void publish(ResultSlot *slot, double v, unsigned long long seq) { slot->value = v; publish_seq(slot, seq); }
__device__ __forceinline__ void publish2(ResultSlot *slot, double v, double second, unsigned long long seq) {
  slot->second = second;
  publish(slot, v, seq);
}

// ---- host side ---------------------------------------------------------------------------------
// A launch that returns a scalar takes a ticket -- a record and the number it will publish there -- and the host waits for THAT
// number: a wait cannot be answered by another launch's value.  (A record holds one result at a time: a ticket whose number a
// later launch on the same record has overwritten ends in the "never arrived" error, not in a wrong value.)
struct Scalar { ResultSlot *slot; unsigned long long seq; };
int scalar_begin(Scalar *t, bool deferred = false);
int scalar_wait(const Scalar &t, double *value, double *second = nullptr);

double *reduction_scratch(int n);                                    // device scratch of >= n doubles for per-workgroup partials (nullptr: error recorded)
int max_of_partials(int n, double init, const Scalar &t);            // final_max_kernel: fold the scratch's first n maxima, publish on the ticket
int max_of_partials(int n, double init, double *out);                // the same on a ticket of its own, and wait for the value

// around a kernel that ORs validation bits into a device word: the word, cleared; after the launch, copy the bits to *status and
// wait for them.  One word serves every such call: they are synchronous, so they never overlap.
int status_begin(int **word);
int status_end(const char *name, int *status);

}  // namespace hpgmg
