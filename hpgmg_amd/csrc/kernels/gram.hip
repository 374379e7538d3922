// gram.hip -- the Gram matrix of the s-step bottom solvers: matmul() of the reference's solvers/matmul.c:6-62 as ONE launch.
//
// Order contract (what makes the entries bit-identical to the reference): entry (mm, nn), nn >= mm, is per box ONE chain over the box's
// dim^3 interior cells in k, j, i order, each product a * b formed first (no FMA: the library is built with -ffp-contract=off), the chain
// starting from 0.0; the level value is the box partials added in box order 0 .. num_boxes - 1, starting from 0.0.  That is not dot()'s
// order (one chain per dim x 8 x 8 tile, blas1.hip), so the Gram matrix cannot be composed from dot() launches.
//
// Launch shape: one workgroup of 256 lanes per box; a lane owns up to four (mm, nn) pairs and runs their chains (17 x 18 -> 170 pairs for
// CABiCGStab at s = 4: three waves).  The box's interior is walked in chunks of kGramChunk consecutive cells (k, j, i order): the whole
// workgroup stages that chunk of every vector the matrix names (each vector read once per box, not once per pair) into LDS, then every
// lane advances its chains over it.  Chunking bounds the LDS (<= 64 vectors x 65 doubles = 33 KB) for any box size, so no box is refused.
// The per-box partials go to device scratch; the host adds them in box order after one copy (a few KB), mirrors the upper triangle
// (matmul.c:45-46) and returns.
#include <string.h>
#include "reduce.hpp"

namespace hpgmg {

constexpr int kGramThreads = 256;
constexpr int kGramChunk = 64;                    // interior cells per vector staged at a time
constexpr int kGramLd = kGramChunk + 1;           // odd row length: the vectors' rows start in different LDS banks
constexpr int kGramMaxSide = 32;                  // rows, cols <= 32: at most 32 x 32 pairs = 4 per lane
constexpr int kGramMaxVecs = 2 * kGramMaxSide;    // distinct vectors among id_A and id_B
constexpr int kGramPerLane = (kGramMaxSide * kGramMaxSide + kGramThreads - 1) / kGramThreads;

struct GramArgs {
  int nvec, rows, cols, npairs;
  int ids[kGramMaxVecs];                          // distinct vector ids, in order of first appearance
  unsigned char slot_a[kGramMaxSide], slot_b[kGramMaxSide];   // id_A[mm] = ids[slot_a[mm]], id_B[nn] = ids[slot_b[nn]]
};

__global__ __launch_bounds__(kGramThreads) void gram_kernel(const hpgmg_hip_level L, const GramArgs A, double *partials) {
  extern __shared__ double stage[];               // [nvec][kGramLd]
  const int box = (int)blockIdx.x, t = (int)threadIdx.x, dim = L.dim, plane = dim * dim, cells = plane * dim;
  int pa[kGramPerLane], pb[kGramPerLane], pid[kGramPerLane];
  double acc[kGramPerLane];
#pragma unroll
  for (int u = 0; u < kGramPerLane; u++) {        // pair p -> (mm, nn) in row-major order of the upper triangle
    int p = t + u * kGramThreads, mm = 0;
    pid[u] = p < A.npairs ? p : -1;
    pa[u] = pb[u] = 0;
    acc[u] = 0.0;
    if (pid[u] < 0) continue;
    while (p >= A.cols - mm) { p -= A.cols - mm; mm++; }
    pa[u] = A.slot_a[mm] * kGramLd;
    pb[u] = A.slot_b[mm + p] * kGramLd;
  }
  for (int q0 = 0; q0 < cells; q0 += kGramChunk) {
    const int len = min(kGramChunk, cells - q0);
    __syncthreads();                              // the previous chunk has been consumed
    for (int e = t; e < A.nvec * kGramChunk; e += kGramThreads) {
      const int s = e / kGramChunk, q = e - s * kGramChunk;
      if (q < len) {
        const int c = q0 + q, k = c / plane, j = (c - k * plane) / dim, i = c - k * plane - j * dim;
        stage[s * kGramLd + q] = gvec_origin(L, box, A.ids[s])[i + j * L.jStride + k * L.kStride];
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kGramPerLane; u++) {
      if (pid[u] < 0) continue;
      const double *a = stage + pa[u], *b = stage + pb[u];
      double s = acc[u];
      for (int q = 0; q < len; q++) { const double prod = a[q] * b[q]; s = s + prod; }      // the chain: k, j, i order
      acc[u] = s;
    }
  }
#pragma unroll
  for (int u = 0; u < kGramPerLane; u++)
    if (pid[u] >= 0) partials[(size_t)box * A.npairs + pid[u]] = acc[u];
}

static double *g_gram_host = nullptr;           // pinned copy of the per-box partials
static size_t g_gram_host_len = 0;

}  // namespace hpgmg

using namespace hpgmg;

extern "C" {
int hpgmg_hip_graph_flush(void);

int hpgmg_hip_gram(const hpgmg_hip_level *L, const int *id_A, int rows, const int *id_B, int cols, double *C_host) {
  if (rows < 1 || cols < 1 || rows > kGramMaxSide || cols > kGramMaxSide) return record_error(hipErrorInvalidValue, "gram: rows and cols must be 1 .. 32");
  if (int e = hpgmg_hip_graph_flush()) return e;
  GramArgs A;
  memset(&A, 0, sizeof(A));
  A.rows = rows; A.cols = cols;
  for (int v = 0; v < rows + cols; v++) {
    const int id = v < rows ? id_A[v] : id_B[v - rows];
    int q = 0;
    while (q < A.nvec && A.ids[q] != id) q++;
    if (q == A.nvec) A.ids[A.nvec++] = id;
    if (v < rows) A.slot_a[v] = (unsigned char)q; else A.slot_b[v - rows] = (unsigned char)q;
  }
  for (int mm = 0; mm < rows; mm++) A.npairs += cols > mm ? cols - mm : 0;
  for (int q = 0; q < rows * cols; q++) C_host[q] = 0.0;
  if (L->num_boxes <= 0) return 0;                // no boxes here: zeros (the allreduce brings the other ranks' sums)
  const size_t n = (size_t)L->num_boxes * A.npairs;
  if (n > (size_t)1 << 30) return record_error(hipErrorInvalidValue, "gram: too many boxes");
  double *partials = reduction_scratch((int)n);
  if (!partials) return record_error(hipErrorOutOfMemory, "gram: scratch");
  if (n > g_gram_host_len) {
    if (g_gram_host) (void)hipHostFree(g_gram_host);
    g_gram_host = nullptr; g_gram_host_len = 0;
    HPGMG_CHECK(hipHostMalloc((void **)&g_gram_host, n * sizeof(double), hipHostMallocDefault));
    g_gram_host_len = n;
  }
  const size_t lds = (size_t)A.nvec * kGramLd * sizeof(double);
  hipLaunchKernelGGL(gram_kernel, dim3(L->num_boxes), dim3(kGramThreads), lds, g_stream, *L, A, partials);
  HPGMG_LAUNCH_CHECK("gram_kernel");
  HPGMG_CHECK(hipMemcpyAsync(g_gram_host, partials, n * sizeof(double), hipMemcpyDeviceToHost, g_stream));
  HPGMG_CHECK(hipStreamSynchronize(g_stream));    // the caller needs the matrix on the host, as after matmul.c's MPI_Allreduce
  for (int mm = 0, p = 0; mm < rows; mm++)
    for (int nn = mm; nn < cols; nn++, p++) {
      double level_sum = 0.0;
      for (int box = 0; box < L->num_boxes; box++) level_sum += g_gram_host[(size_t)box * A.npairs + p];      // box order
      C_host[mm * cols + nn] = level_sum;
      if (mm < cols && nn < rows) C_host[nn * cols + mm] = level_sum;       // matmul.c:45-46
    }
  return 0;
}

}  // extern "C"
