// reduce.hip -- host side of reduce.hpp: the pinned result records and their tickets, the one poll loop, the scratch of partial
// results with the kernel that folds partial maxima, and the device status word.
#include "reduce.hpp"

namespace hpgmg {

__global__ __launch_bounds__(256) void final_max_kernel(const double *partials, int n, double init, ResultSlot *result, unsigned long long seq) {
  __shared__ double smem[4];
  double m = init;
  // four loads in flight per lane: the chain of one load per iteration made 8192 partials a 10 us launch (a maximum is exact under any order)
  double m1 = init, m2 = init, m3 = init;
  int t = threadIdx.x;
  for (; t + 768 < n; t += 1024) {
    const double a0 = partials[t], a1 = partials[t + 256], a2 = partials[t + 512], a3 = partials[t + 768];
    m = (a0 > m) ? a0 : m; m1 = (a1 > m1) ? a1 : m1; m2 = (a2 > m2) ? a2 : m2; m3 = (a3 > m3) ? a3 : m3;
  }
  for (; t < n; t += 256) m = (partials[t] > m) ? partials[t] : m;
  m = (m1 > m) ? m1 : m; m2 = (m3 > m2) ? m3 : m2; m = (m2 > m) ? m2 : m;
  m = block_max<4>(m, smem);
  if (threadIdx.x == 0) publish(result, m, seq);
}

static ResultSlot *g_slots = nullptr;                 // pinned, device-visible: [0] immediate, [1] deferred
static unsigned long long g_seq[2] = { 0, 0 };        // the newest number handed out for each record
int scalar_begin(Scalar *t, bool deferred) {
  if (!g_slots) {
    HPGMG_CHECK(hipHostMalloc((void **)&g_slots, 2 * sizeof(ResultSlot), hipHostMallocDefault));
    for (int q = 0; q < 2; q++) { g_slots[q].value = 0.0; g_slots[q].seq = 0; g_slots[q].second = 0.0; }
  }
  t->slot = g_slots + (deferred ? 1 : 0);
  t->seq = ++g_seq[deferred ? 1 : 0];
  return 0;
}
int scalar_wait(const Scalar &t, double *value, double *second) {
  volatile ResultSlot *slot = t.slot;
  for (long spins = 0; slot->seq != t.seq; spins++) {
    __builtin_ia32_pause();
    if (spins > 20000000L) { HPGMG_CHECK(hipStreamSynchronize(g_stream)); if (slot->seq != t.seq) return record_error(hipErrorUnknown, "reduction result never arrived"); }
  }
  __atomic_thread_fence(__ATOMIC_ACQUIRE);
  *value = slot->value;
  if (second) *second = slot->second;
  return 0;
}

static double *g_scratch = nullptr;  static int g_scratch_len = 0;
double *reduction_scratch(int n) {
  if (n > g_scratch_len) {
    if (g_scratch) { hipStreamSynchronize(g_stream); (void)hipFree(g_scratch); g_scratch = nullptr; g_scratch_len = 0; }
    const int want = n < 65536 ? 65536 : n;
    if (hipError_t e = hipMalloc((void **)&g_scratch, (size_t)want * sizeof(double))) { record_error(e, "reduction_scratch"); g_scratch = nullptr; return nullptr; }
    g_scratch_len = want;
  }
  return g_scratch;
}
int max_of_partials(int n, double init, const Scalar &t) {
  hipLaunchKernelGGL(final_max_kernel, dim3(1), dim3(256), 0, g_stream, (const double *)g_scratch, n, init, t.slot, t.seq);
  HPGMG_LAUNCH_CHECK("final_max_kernel");
  return 0;
}
int max_of_partials(int n, double init, double *out) {
  Scalar t;
  if (int e = scalar_begin(&t)) return e;
  if (int e = max_of_partials(n, init, t)) return e;
  return scalar_wait(t, out);
}

static int *g_status = nullptr;
int status_begin(int **word) {
  if (!g_status) HPGMG_CHECK(hipMalloc((void **)&g_status, sizeof(int)));
  HPGMG_CHECK(hipMemsetAsync(g_status, 0, sizeof(int), g_stream));
  *word = g_status;
  return 0;
}
int status_end(const char *name, int *status) {
  HPGMG_LAUNCH_CHECK(name);
  HPGMG_CHECK(hipMemcpyAsync(status, g_status, sizeof(int), hipMemcpyDeviceToHost, g_stream));
  HPGMG_CHECK(hipStreamSynchronize(g_stream));
  return 0;
}

}  // namespace hpgmg
