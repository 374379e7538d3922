"""A variant id that no launcher's list holds is refused: a non-zero status, the launcher's own message in hpgmg_hip_last_error(), nothing launched
(kernels/launch_dispatch.hpp: with_variant returns false and the caller records the refusal).

The level is hand-made -- one box of side 4, no box table -- so nothing here touches device memory: every entry point below reaches its variant
dispatch before any device call (argument checks, launch planning and the profiler's "off" test are host arithmetic), and variant 99 ends there.
"""
import ctypes

import pytest

import hpgmg_amd as H

pytestmark = pytest.mark.gpu

NO_SUCH_VARIANT = 99
STENCIL_MESSAGE = b"stencil variant not implemented"


def _kernels():
    K = H.load_kernels()
    c_int, c_dbl, vp, L = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.POINTER(H.HipLevel)
    K.hpgmg_hip_small_level_op.restype = c_int
    K.hpgmg_hip_small_level_op.argtypes = [L] + [c_int] * 7 + [c_dbl] * 3 + [vp, vp, vp, c_int, vp, c_int, c_int, c_int]
    K.hpgmg_hip_bottom_bicgstab.restype = c_int
    K.hpgmg_hip_bottom_bicgstab.argtypes = [L] + [c_int] * 4 + [c_dbl] * 4 + [vp, c_int, c_int, c_int, vp]
    K.hpgmg_hip_small_ops.restype = c_int
    K.hpgmg_hip_small_ops.argtypes = [L, c_int, c_int] + [vp] * 6 + [vp, c_int, c_int, c_int] + [c_dbl] * 3 + [vp, vp]
    return K


def _level():
    """One box of 4^3 cells with one ghost cell, Dirichlet, null box table."""
    side = 4 + 2
    return H.HipLevel(box_base=None, box_low=None, num_boxes=1, dim=4, ghosts=1, jStride=side, kStride=side * side, volume=side ** 3,
                      dim_i=4, dim_j=4, dim_k=4, periodic=0, box_nbr=None, flags=0, box_stride=0)


def _small_ops(K, L):
    kinds, ids, one = (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(0), (ctypes.c_double * 1)(1.0)      # one `add` entry: no value is returned, no ticket taken
    return K.hpgmg_hip_small_ops(L, NO_SUCH_VARIANT, 1, kinds, ids, ids, ids, one, one, None, 0, 0, 0, 1.0, 1.0, 1.0, None, None)


CALLS = {
    "residual": (STENCIL_MESSAGE, lambda K, L: K.hpgmg_hip_residual(L, NO_SUCH_VARIANT, 2, 0, 1, 1.0, 1.0, 1.0)),
    "smooth_cheby": (STENCIL_MESSAGE, lambda K, L: K.hpgmg_hip_smooth_cheby(L, NO_SUCH_VARIANT, 0, 2, 1, 1.0, 1.0, 1.0, 0.5, 0.5)),
    "smooth_gsrb": (STENCIL_MESSAGE, lambda K, L: K.hpgmg_hip_smooth_gsrb(L, NO_SUCH_VARIANT, 0, 0, 1, 1.0, 1.0, 1.0, 0)),
    "smooth_jacobi": (STENCIL_MESSAGE, lambda K, L: K.hpgmg_hip_smooth_jacobi(L, NO_SUCH_VARIANT, 0, 2, 1, 1.0, 1.0, 1.0, 0.5)),
    "small_level_op": (b"small_level_op: variant",
                       lambda K, L: K.hpgmg_hip_small_level_op(L, NO_SUCH_VARIANT, 0, 1, 0, 1, 2, 0, 1.0, 1.0, 1.0, None, None, None, 0, None, 0, 0, 0)),
    "bottom_bicgstab": (b"bottom_bicgstab: variant",
                        lambda K, L: K.hpgmg_hip_bottom_bicgstab(L, NO_SUCH_VARIANT, 0, 1, 4, 1.0, 1.0, 1.0, 1e-3, None, 0, 0, 0, None)),
    "small_ops": (b"small_ops: variant", _small_ops),
}


@pytest.mark.parametrize("entry", sorted(CALLS))
def test_unlisted_variant_is_refused(entry):
    message, call = CALLS[entry]
    K, L = _kernels(), _level()
    status = call(K, ctypes.byref(L))
    assert status != 0, entry
    assert K.hpgmg_hip_last_error().startswith(message), (entry, K.hpgmg_hip_last_error())
