/*
 * plugin_gram.c -- matmul() of the operator plugin: the Gram matrix the s-step bottom solvers (host/solvers.c cabicgstab / cacg) form once per
 * s steps, as ONE device launch (kernels/gram.hip) and ONE transport reduction of the whole matrix (solvers/matmul.c:6-62, its MPI_Allreduce at
 * :49-59).  It replaces the weak host default of host/solvers.c, which would download every box of every vector.
 */
#include "plugin_internal.h"

void matmul(level_type *L, double *C, int *id_A, int *id_B, int rows, int cols, int A_equals_B_transpose) {
  int v;
  (void)A_equals_B_transpose;           /* the reference does not read it either */
  for (v = 0; v < rows + cols; v++) {   /* the kernel addresses vectors by id: an id the level does not have would read past its boxes */
    const int id = v < rows ? id_A[v] : id_B[v - rows];
    if (id < 0 || id >= L->numVectors) { fprintf(stderr, "hpgmg: matmul: vector %d is not one of the level's %d\n", id, L->numVectors); abort(); }
  }
  { TICK(L, blas3, "BLAS3"); HIP_OK(hpgmg_hip_gram(&hp_backend_of(L)->dev, id_A, rows, id_B, cols, C)); TOCK(); }
  hp_allreduce_values(L, C, rows * cols, HPGMG_REDUCE_SUM);
}
