"""User problems on dense arrays: the 7-point variable-coefficient operator  a alpha u - b div(beta grad u)  on an N^3 grid.

    with Solver(256, bc="dirichlet", a=0.0, b=1.0) as s:
        s.set_coefficients(None, beta_i, beta_j, beta_k)     # Poisson: no alpha
        u, info = s.solve(f)                                  # one F-cycle, as the benchmark

Arrays are C-contiguous float64 indexed [k][j][i]; cell (i,j,k) has its centre at ((i+1/2)h, (j+1/2)h, (k+1/2)h).  f, alpha, u, u0 and x
are (N,N,N).  Dirichlet (homogeneous): beta_i is (N,N,N+1), beta_i[k][j][i] on the face between cells i-1 and i (i = 0 and i = N are the
domain faces); beta_j is (N,N+1,N), beta_k (N+1,N,N).  Periodic: all three are (N,N,N), face N being face 0.

Inhomogeneous Dirichlet values: `boundary=` of set_rhs / solve / apply, a (6,N,N) float64 array of face-centre values (the same kind of
array as the call's others): boundary[0], [1] the i-low / i-high faces indexed [k][j]; [2], [3] j-low / j-high indexed [k][i]; [4], [5]
k-low / k-high indexed [j][i].  A boundary cell's ghost is 2 g - u instead of -u, so the solve is A0 u = f + T(g), and
apply(x, boundary=g) is A0 x - T(g).  Solver.boundary_from(fn) samples fn(x, y, z) at the face centres.

Neumann and mixed walls: bc="neumann", or a 6-tuple of "dirichlet" / "neumann" in the face order of `boundary` (i-low, i-high, j-low, j-high,
k-low, k-high).  On a Neumann face the entry of `boundary` is the OUTWARD normal derivative du/dn at the face centre (the ghost is u + h du/dn)
and boundary=None is zero data on every face.  The beta arrays keep their Dirichlet shapes; a Neumann wall's beta (still > 0) weighs its data.
Six Neumann faces without an a alpha term determine u up to a constant: the mean of f + T(boundary) is subtracted (mean_shift) and the
mean-free u is returned.  Periodic cannot be mixed per face.  DESIGN.md §11.2.

Robin (convective) walls: "convective" in the 6-tuple makes that face a Robin wall  du/dn + kappa u = g  (dn outward): a convective, impedance or
surface-reaction wall.  kappa >= 0 comes with the coefficients, set_coefficients(alpha, beta_i, beta_j, beta_k, robin=kappa): a (6,N,N)
array in `boundary`'s layout (the entries of faces that are not "convective" are not read) or six numbers, one per face.  The face's entry of
`boundary` is g (None: zero data); boundary_from(fn, grad, robin=kappa) samples +-grad.n + kappa fn there.  kappa = 0 is the Neumann wall.
The wall adds to the operator's diagonal on every level, with that level's own h.  Six Neumann / Robin faces without an a alpha term are
singular only if kappa is 0 everywhere.  DESIGN.md §11.5.

Coefficients with jumps: solve(f, method="pcg", rtol=..., max_iter=100) runs conjugate gradients preconditioned with one V-cycle per iteration
where method="mg" (20 V-cycles at most) stalls; it reports through info.converged instead of raising.  DESIGN.md §11.3.
method="fpcg" is its flexible form, for grids on which the V-cycle is not one fixed operator -- bc="periodic", or N / box_dim with an odd
factor, where BiCGStab solves the coarsest level to a tolerance: "pcg" can fail to converge there, "fpcg" does not rely on the symmetry it lacks.
Elsewhere the two take the same iterations; "fpcg" pays one more fused inner product each.  DESIGN.md §11.4.

Fluxes: flux(u, boundary=g) returns (flux_i, flux_j, flux_k), q = -b beta grad u on every face -- the heat flux, Darcy velocity or current
density -- in the shapes of beta_i, beta_j, beta_k and positive towards increasing index: flux_i[k][j][i] on the face between cells i-1 and i
(periodic: face 0 lies between cell N-1 and cell 0).  A wall face holds what the wall's ghost gives, with a Neumann or Robin wall's own beta and
kappa, so that cell by cell  a alpha u + (1/h) sum_d (q_d[high face] - q_d[low face])  is apply(u, boundary=g).  wall_flux(fluxes) is the
(6,N,N) OUTWARD flux through the walls in `boundary`'s layout; h^2 times its sum is what leaves the box.  DESIGN.md §11.6.

Time stepping: start(u, f, boundary=g, dt=..., theta=1.0) begins a march of  alpha du/dt = b div(beta grad u) + f  by the theta scheme
alpha (u1 - u0) / dt = theta w1 + (1 - theta) w0,  w = alpha du/dt  (theta = 1: backward Euler, 0.5: Crank-Nicolson; 0.5 <= theta <= 1), on a
solver created with a != 0: one step is one solve with a = 1 / (theta dt), which the march sets (set_shift(a) does so by hand: every level's
diagonal is rebuilt, no coefficient array is packed).  step(f, boundary=g) advances to the next time, f and g being those of that time, with
V-cycles warm-started from the state; dt= / theta= change the step.  The state u and the rate w stay in the library, on the device, between
calls: get_solution() and rate() return them, StepInfo.rate is max |w| and StepInfo.t the time since start().  The rate is exact for the state
the solve stopped at, whatever rtol.  set_coefficients, set_cell_coefficients, set_rhs and solve end a march; get_solution, rate, apply, flux,
sensitivity, cell_sensitivity and set_shift do not.  DESIGN.md §11.8.

Sensitivities: apply(u, boundary=g) = A0 u - T(g) is affine in alpha, in every beta entry and in a Neumann / Robin wall's own beta.
sensitivity(u, lam, boundary=g) returns (d_alpha, d_beta_i, d_beta_j, d_beta_k), G_p = d/dp sum_c lam_c apply(u, boundary=g)_c for every
coefficient entry p, in the shapes of set_coefficients' arguments (d_alpha is None on a Poisson solver).  With t = kappa h:

    alpha[c]                                                              a u_c lam_c
    face between cells lo and hi = lo + 1 (box-to-box, periodic wrap)     (b/h^2) (u_lo - u_hi) (lam_lo - lam_hi)
    Dirichlet wall face of cell c, either side                            (b/h^2) 2 (u_c - g) lam_c
    Neumann / Robin wall face of cell c, either side (Neumann: kappa = 0) (b/h) (2/(2 + t)) (kappa u_c - g) lam_c

None of them reads a beta.  If J depends on the solution u of A u = f + T(g), and lam solves A lam = dJ/du with no boundary data (the operator is
symmetric: the adjoint solve is solve()), then dJ/dp = -G_p and dJ/df = lam -- also on the singular solvers, whose solve subtracts the mean of
any right-hand side.  hpgmg_amd.autograd.solve wraps exactly that as a differentiable torch function.  DESIGN.md §11.9.

Cell-centred conductivities: set_cell_coefficients(alpha, k, mean="harmonic") takes the coefficient as ONE (N,N,N) array, a conductivity,
permeability or density per cell, in place of the three face arrays: the beta of a face between two cells (box-to-box, periodic wrap) is their
harmonic mean 2 lo hi / (lo + hi) -- or, mean="arithmetic", (lo + hi) / 2 -- and a wall face of any kind has its cell's own value.  It is
set_coefficients with those face arrays, bit for bit.  cell_sensitivity(u, lam, k, mean=..., boundary=g) returns (d_alpha, d_k): sensitivity()
with the chain rule through the mean, d_k[c] the sum over the six faces of cell c of G_face d beta_face / d k_c, so that dJ/dk = -d_k.
hpgmg_amd.autograd.solve_cells is the differentiable solve on a cell field.  DESIGN.md §11.10.

Eigenmodes: lam, modes, info = eigs(k, rtol=1e-6, max_iter=60, extra=2) returns the k smallest lambda of  K x = lambda M x  and their modes, K being
-b div(beta grad .) with the solver's walls and zero data (apply() without its a alpha term), M = diag(alpha) on a Helmholtz solver and M = I on a
Poisson solver: the decay rates of the march, the modes of a heterogeneous block, the eigenvalue that bounds an explicit step.  It is LOBPCG with a
block of k + extra <= 12 columns, one V-cycle per unconverged column and iteration.  A Helmholtz solver iterates on A = a M + K with the a in force
(set_shift's, or the last march's), whose eigenvalues are mu = a + lambda > 0 (info.mu): lam = mu - a loses digits when a >> lambda, and set_shift moves
a.  modes is (k,N,N,N), mode j normalised to h^3 x^T M x = 1, sign and the basis inside a degenerate cluster unspecified; info.residuals are
max |A x - mu M x| / (mu max |M x|) of the pairs returned.  Like "pcg" it reports through info.converged instead of raising.  Refused: the singular
solvers (periodic or six Neumann walls without an a alpha term; create the solver with a > 0 and alpha = 1 and the constant mode comes back as
lambda ~ 0) and a Helmholtz solver with alpha == 0 somewhere.  eigs leaves the coefficients (and coefficient_version) alone; it ends a march and
invalidates the stored right-hand side and solution as set_coefficients does.  DESIGN.md §11.11.

The wave equation: wave_start(u, v, f, boundary=g, dt=..., beta=0.25, gamma=0.5, damping=0.0) begins a march of
alpha d2u/dt2 + damping alpha du/dt = b div(beta grad u) + f  -- acoustics, a membrane, structural vibration, the telegraph equation -- from the state u
and the velocity v by the implicit Newmark rule (beta, gamma); the default is the average-acceleration rule: second order, unconditionally stable and
energy conserving.  gamma >= 1/2 and beta >= gamma / 2 are taken (the conditionally stable rules, central differences included, are refused), on a solver
created with a != 0 and alpha > 0 in every cell.  One step is one solve with a = 1 / (beta dt^2) + damping gamma / (beta dt), which the march sets,
warm-started from the predictor.  wave_step(f, boundary=g) advances to the next time, f and g being those of that time; dt= changes the step (a
set_shift and nothing else); beta, gamma and damping stay wave_start's.  u, v and the acceleration stay in the library, on the device, between calls:
get_solution(), velocity() and acceleration() return them.  WaveInfo adds t, kinetic = h^3/2 sum alpha v^2 and potential = h^3/2 u^T K u (K: eigs' K)
to SolveInfo's fields, and energy, their sum; the potential energy comes from the step's closing residual and is exact for the u the solve stopped at.
Only one march is live: step() and rate() refuse on a wave march, wave_step(), velocity() and acceleration() on a theta march; what ends one ends the
other.  DESIGN.md §11.12.

NumPy arrays take the host path.  torch tensors on the library's GPU (float64, contiguous) are read and written in place, and results come
back as tensors on that device.  torch must be imported before this package loads its libraries: both bring a HIP runtime
(libamdhip64.so.7), and a device pointer is only valid inside the runtime that made it.  The C entry points are hpgmg_user_* of
include/hpgmg_fv.h.
"""
import ctypes
from dataclasses import dataclass

import numpy as np

import hpgmg_amd as H

_BC = {"dirichlet": H.BC_DIRICHLET, "periodic": H.BC_PERIODIC}
_FACE = {"dirichlet": H.FACE_DIRICHLET, "neumann": H.FACE_NEUMANN, "convective": H.FACE_ROBIN}
_SMOOTHER = {"cheby": H.SMOOTH_CHEBY, "chebyshev": H.SMOOTH_CHEBY, "gsrb": H.SMOOTH_GSRB, "jacobi": H.SMOOTH_JACOBI}
_OPERATOR = {"7pt": H.OP_7PT, "27pt": H.OP_27PT, "fv4": H.OP_FV4, "fv2": H.OP_FV2}
_MEAN = {"harmonic": H.MEAN_HARMONIC, "arithmetic": H.MEAN_ARITHMETIC}
_METHOD = {"fmg": H.USER_FMG, "mg": H.USER_MG, "pcg": H.USER_PCG, "fpcg": H.USER_FPCG}
_STATUS = {H.USER_BAD_ARGUMENT: "refused by the library", H.USER_CONFLICT: "the process is configured for another live solver",
           H.USER_MULTI_RANK: "only one rank is supported", H.USER_NOT_FINITE: "holds a value that is not finite",
           H.USER_OUT_OF_RANGE: "is out of range (beta must be > 0, alpha >= 0)",
           H.USER_NOT_READY: "no valid coefficients / right-hand side (an earlier call was refused)",
           H.USER_UNSUPPORTED: "only the 7-point operator is supported"}


@dataclass
class SolveInfo:
    residual: float      # |f - A u|_inf (f after the mean shift)
    norm_f: float        # |f|_inf; with boundary values |f + T(g)|_inf, the right-hand side actually solved
    vcycles: int         # V-cycles run from the finest level (an F-cycle ends with one; methods "pcg" and "fpcg": one per iteration)
    converged: bool      # residual < rtol * norm_f
    mean_shift: float    # subtracted from f (periodic without an a alpha term), else 0.0


@dataclass
class StepInfo(SolveInfo):
    """Of one time step (Solver.step): SolveInfo of the step's solve, whose right-hand side is f + T(g) + a alpha u0 + c w0."""
    rate: float          # max |alpha du/dt| at the new time
    t: float             # time since start()


@dataclass
class WaveInfo(SolveInfo):
    """Of Solver.wave_start / wave_step: SolveInfo of the step's solve (wave_start: no solve ran, vcycles = 0, converged False, residual
    and norm_f those of A0 u = f + T(g) at the start), and the discrete energies at the new time."""
    t: float             # time since wave_start()
    kinetic: float       # h^3/2 sum alpha v^2
    potential: float     # h^3/2 u^T K u, K = apply() without its a alpha term and with zero data

    @property
    def energy(self):
        return self.kinetic + self.potential


@dataclass
class EigInfo:
    """Of Solver.eigs."""
    iterations: int          # LOBPCG iterations run
    vcycles: int             # V-cycles run from the finest level: one per unconverged column and iteration
    residuals: np.ndarray    # (k,): max |A x - mu M x| / (mu max |M x|) of the returned pairs, from A x applied at the end
    mu: np.ndarray           # (k,): the eigenvalues of the pencil (A, M) iterated on: a + lam on a Helmholtz solver, lam on a Poisson solver
    converged: bool          # every one of the k residuals is below rtol


def hip_runtimes_mapped():
    """Paths of the libamdhip64 copies mapped into this process."""
    paths = set()
    with open("/proc/self/maps") as f:
        for line in f:
            parts = line.split()
            if len(parts) >= 6 and "libamdhip64" in parts[-1]:
                paths.add(parts[-1])
    return sorted(paths)


def check_single_hip_runtime():
    """Raise unless at most one HIP runtime is mapped (torch's bundled copy and the system one have the same soname; which one the
    project's libraries bind to depends on which was loaded first)."""
    runtimes = hip_runtimes_mapped()
    if len(runtimes) > 1:
        raise RuntimeError("import torch before hpgmg_amd loads its libraries: this process has two HIP runtimes mapped "
                           f"({', '.join(runtimes)}) and a device pointer of one is not valid in the other")


def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


class Solver:
    """One user problem.  `lib` is the driver library to run on (default: the HIP build, hpgmg_amd.load_driver())."""

    def __init__(self, n, box_dim=None, bc="dirichlet", smoother="cheby", a=0.0, b=1.0, h=None, operator="7pt", lib=None, verbose=False):
        faces = None                    # per-face kinds of a solver with at least one Neumann or Robin wall; None: the dirichlet / periodic solver
        if isinstance(bc, str) and bc == "neumann":
            bc = ("neumann",) * 6
        if isinstance(bc, (tuple, list)):
            if len(bc) != 6:
                raise ValueError(f"bc: a tuple needs 6 entries (i-low, i-high, j-low, j-high, k-low, k-high), got {len(bc)}")
            for kind in bc:
                if kind == "periodic":
                    raise ValueError("bc: periodic cannot be mixed per face (pass bc='periodic' for a periodic box)")
                if not isinstance(kind, str) or kind not in _FACE:
                    raise ValueError(f"bc: {kind!r} is not one of {sorted(_FACE)}")
            faces = tuple(bc) if ("neumann" in bc or "convective" in bc) else None
            bc = "dirichlet"            # the shapes and the level's boundary condition; six Dirichlet faces are the "dirichlet" solver
        elif not isinstance(bc, str) or bc not in _BC:
            raise ValueError(f"bc: {bc!r} is not one of {sorted(_BC) + ['neumann']} or a 6-tuple of {sorted(_FACE)}")
        if smoother not in _SMOOTHER:
            raise ValueError(f"smoother: {smoother!r} is not one of {sorted(_SMOOTHER)}")
        if operator not in _OPERATOR:
            raise ValueError(f"operator: {operator!r} is not one of {sorted(_OPERATOR)}")
        self.lib = lib if lib is not None else H.load_driver()
        self.hip = self.lib.hpgmg_backend_name() == b"hip"
        self.n, self.bc, self.faces, self.a, self.b = int(n), bc, faces, float(a), float(b)
        self.h = float(h) if h is not None and h > 0 else 1.0 / self.n
        self.robin_faces = tuple(f for f in range(6) if faces is not None and faces[f] == "convective")
        self._ptr = None
        self._dt = self._theta = None       # of the last start() / step()
        self._wave = None                   # (dt, beta, gamma, damping) of the last wave_start() / wave_step() while that march is live
        self._t = 0.0                       # time since start()
        self.coefficient_version = 0        # counts the calls that may change the operator (set_coefficients, set_shift, a march's new a): autograd.solve
        out = ctypes.c_void_p()
        if faces is None:
            st = self.lib.hpgmg_user_create(self.n, int(box_dim or 0), _BC[bc], _OPERATOR[operator], _SMOOTHER[smoother], self.a, self.b,
                                            float(h or 0.0), ctypes.byref(out))
        else:
            kinds = (ctypes.c_int * 6)(*[_FACE[k] for k in faces])
            st = self.lib.hpgmg_user_create_faces(self.n, int(box_dim or 0), kinds, _OPERATOR[operator], _SMOOTHER[smoother], self.a, self.b,
                                                  float(h or 0.0), ctypes.byref(out))
        self._check(st, "operator" if st == H.USER_UNSUPPORTED else "n, box_dim, a, b or h")
        self._ptr = out.value
        if verbose:
            self.lib.hpgmg_user_set_verbose(self._ptr, 1)

    # ---- shapes
    def _face_shape(self, axis):
        n = self.n
        shape = [n, n, n]
        if self.bc == "dirichlet":
            shape[2 - axis] += 1
        return tuple(shape)

    # ---- arguments
    def _check(self, st, name):
        if st != H.USER_OK:
            raise ValueError(f"{name}: {_STATUS.get(st, f'status {st}')}")

    def _device_ok(self, x, name):
        import torch
        check_single_hip_runtime()
        if not self.hip:
            raise ValueError(f"{name}: a tensor needs the HIP library (this solver runs on {self.lib.hpgmg_backend_name().decode()})")
        if not x.is_cuda:
            raise ValueError(f"{name}: a tensor must be on the GPU (pass a NumPy array for host data)")
        if x.device.index not in (None, torch.cuda.current_device()):
            raise ValueError(f"{name}: the tensor is on {x.device}, the library on cuda:{torch.cuda.current_device()}")

    def _arg(self, x, shape, name, kind=None):
        """(pointer, where, kind) of an input array; kind = 'numpy' / 'torch' must match the other arrays of the call."""
        if _is_tensor(x):
            import torch
            if x.dtype != torch.float64:
                raise ValueError(f"{name}: dtype {x.dtype}, expected torch.float64")
            if tuple(x.shape) != shape:
                raise ValueError(f"{name}: shape {tuple(x.shape)}, expected {shape}")
            if not x.is_contiguous():
                raise ValueError(f"{name}: the tensor is not contiguous")
            self._device_ok(x, name)
            this = "torch"
            ptr, where = x.data_ptr(), H.WHERE_PLUGIN
        elif isinstance(x, np.ndarray):
            if x.dtype != np.float64:
                raise ValueError(f"{name}: dtype {x.dtype}, expected float64")
            if x.shape != shape:
                raise ValueError(f"{name}: shape {x.shape}, expected {shape}")
            if not x.flags.c_contiguous:
                raise ValueError(f"{name}: the array is not C-contiguous")
            this = "numpy"
            ptr, where = x.ctypes.data, H.WHERE_HOST
        else:
            raise ValueError(f"{name}: expected a NumPy array or a torch tensor, got {type(x).__name__}")
        if kind is not None and kind != this:
            raise ValueError(f"{name}: a {this} array among {kind} arrays (one call takes host or device arrays, not both)")
        return ptr, where, this

    @staticmethod
    def _sync_torch(kind):
        if kind == "torch":
            import torch
            torch.cuda.current_stream().synchronize()

    def _first_bad(self, named, st):
        """Which argument a refused pack was about (the library reports the status, not the array)."""
        for name, x, low, strict in named:
            v = x.detach().cpu().numpy() if _is_tensor(x) else x
            if not np.isfinite(v).all():
                return name
            if st == H.USER_OUT_OF_RANGE and ((strict and not (v > low).all()) or (not strict and not (v >= low).all())):
                return name
        return ", ".join(nm for nm, *_ in named)

    def _out(self, out, kind, like, name):
        if out is None:
            if kind == "torch":
                import torch
                return torch.empty((self.n,) * 3, dtype=torch.float64, device=like.device)
            return np.empty((self.n,) * 3, dtype=np.float64)
        self._arg(out, (self.n,) * 3, name, kind)
        return out

    # ---- the API
    def _kappa(self, robin, kind, like=None):
        """robin= as the (6,N,N) array of `kind` ('numpy' / 'torch'; like: a tensor whose device a broadcast goes to): an array of that kind
        is checked like the call's others, six numbers are broadcast per face."""
        if _is_tensor(robin) or isinstance(robin, np.ndarray):
            self._arg(robin, (6, self.n, self.n), "robin", kind)
            return robin
        try:
            values = np.array([float(v) for v in robin], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"robin: expected a (6,N,N) array or 6 numbers, got {type(robin).__name__}") from None
        if values.shape != (6,):
            raise ValueError(f"robin: shape {values.shape}, expected (6, {self.n}, {self.n}) or 6 numbers (one per face)")
        full = np.ascontiguousarray(np.broadcast_to(values[:, None, None], (6, self.n, self.n)))
        if kind == "torch":
            import torch
            return torch.from_numpy(full).to(like.device)
        return full

    def _kappa_bad(self, robin):
        """Whether the library refuses this kappa: a value that is not finite anywhere, or a negative one on a Robin face."""
        v = robin.detach().cpu().numpy() if _is_tensor(robin) else robin
        if not np.isfinite(v).all():
            return "holds a value that is not finite"
        if any((v[f] < 0.0).any() for f in self.robin_faces):
            return "is out of range (kappa must be >= 0 on a Robin face)"
        return None

    def set_coefficients(self, alpha, beta_i, beta_j, beta_k, robin=None):
        """alpha: (N,N,N) or None for Poisson (a = 0); beta_*: the face arrays described in the module docstring.
        robin: kappa of the Robin faces, required exactly when a face is "convective": a (6,N,N) array of the same kind as the others, or 6
        non-negative numbers, one per face (read on the Robin faces only)."""
        if (alpha is None) != (self.a == 0.0):
            raise ValueError("alpha: required when a != 0 (Helmholtz), must be None when a == 0 (Poisson)")
        if robin is None and self.robin_faces:
            raise ValueError("robin: required when a face is 'convective' (kappa of du/dn + kappa u = g: a (6,N,N) array or 6 numbers)")
        if robin is not None and not self.robin_faces:
            raise ValueError("robin: this solver has no 'convective' face (bc=)")
        pi, where, kind = self._arg(beta_i, self._face_shape(0), "beta_i")
        self.coefficient_version += 1
        pj, _, _ = self._arg(beta_j, self._face_shape(1), "beta_j", kind)
        pk, _, _ = self._arg(beta_k, self._face_shape(2), "beta_k", kind)
        pa = self._arg(alpha, (self.n,) * 3, "alpha", kind)[0] if alpha is not None else None
        if robin is not None:
            robin = self._kappa(robin, kind, beta_i)
            pr = self._arg(robin, (6, self.n, self.n), "robin", kind)[0]
        self._sync_torch(kind)
        if robin is None:
            st = self.lib.hpgmg_user_set_coefficients(self._ptr, pa, pi, pj, pk, where)
        else:
            st = self.lib.hpgmg_user_set_coefficients_robin(self._ptr, pa, pi, pj, pk, pr, where)
            if st in (H.USER_NOT_FINITE, H.USER_OUT_OF_RANGE) and self._kappa_bad(robin):      # the library checks kappa first
                raise ValueError(f"robin: {self._kappa_bad(robin)}")
        if st in (H.USER_NOT_FINITE, H.USER_OUT_OF_RANGE):
            named = [("beta_i", beta_i, 0.0, True), ("beta_j", beta_j, 0.0, True), ("beta_k", beta_k, 0.0, True)]
            if alpha is not None:
                named.append(("alpha", alpha, 0.0, False))
            self._check(st, self._first_bad(named, st))
        self._check(st, "alpha, beta_i, beta_j, beta_k" + (", robin" if robin is not None else ""))

    def _mean(self, mean):
        if not isinstance(mean, str) or mean not in _MEAN:
            raise ValueError(f"mean: {mean!r} is not one of {sorted(_MEAN)}")
        return _MEAN[mean]

    @staticmethod
    def _entries_ok(x, strict):
        """Every entry finite and > 0 (strict) or >= 0: what the library asks of k and of alpha entry by entry."""
        v = x.detach().cpu().numpy() if _is_tensor(x) else x
        return bool(np.isfinite(v).all() and ((v > 0.0).all() if strict else (v >= 0.0).all()))

    @staticmethod
    def _mean_bad(st, mean):
        """k's entries pass and the library still refused it: a face mean of two neighbouring cells."""
        return f"a {mean} mean of two neighbouring cells " + ("overflows" if st == H.USER_NOT_FINITE else "underflows to zero")

    def set_cell_coefficients(self, alpha, k, mean="harmonic", robin=None):
        """set_coefficients from ONE cell-centred array k (N,N,N), > 0: the beta of a face between two cells (box-to-box and the periodic wrap
        included) is their mean -- "harmonic": 2 lo hi / (lo + hi), "arithmetic": (lo + hi) / 2 -- and a wall face of any kind has its cell's
        own value.  Bit for bit set_coefficients with those three face arrays, in one pass over k.  alpha, robin: as set_coefficients takes them.
        DESIGN.md §11.10."""
        if (alpha is None) != (self.a == 0.0):
            raise ValueError("alpha: required when a != 0 (Helmholtz), must be None when a == 0 (Poisson)")
        if robin is None and self.robin_faces:
            raise ValueError("robin: required when a face is 'convective' (kappa of du/dn + kappa u = g: a (6,N,N) array or 6 numbers)")
        if robin is not None and not self.robin_faces:
            raise ValueError("robin: this solver has no 'convective' face (bc=)")
        m = self._mean(mean)
        pk, where, kind = self._arg(k, (self.n,) * 3, "k")
        self.coefficient_version += 1
        pa = self._arg(alpha, (self.n,) * 3, "alpha", kind)[0] if alpha is not None else None
        pr = None
        if robin is not None:
            robin = self._kappa(robin, kind, k)
            pr = self._arg(robin, (6, self.n, self.n), "robin", kind)[0]
        self._sync_torch(kind)
        st = self.lib.hpgmg_user_set_cell_coefficients(self._ptr, pa, pk, m, pr, where)
        if st in (H.USER_NOT_FINITE, H.USER_OUT_OF_RANGE):
            if robin is not None and self._kappa_bad(robin):      # the library checks kappa first
                raise ValueError(f"robin: {self._kappa_bad(robin)}")
            if not self._entries_ok(k, True):
                self._check(st, "k")
            if alpha is not None and not self._entries_ok(alpha, False):
                self._check(st, "alpha")
            raise ValueError(f"k: {self._mean_bad(st, mean)}")
        self._check(st, "alpha, k" + (", robin" if robin is not None else ""))

    def _boundary(self, g, kind):
        """(pointer of) the boundary values g: (6,N,N), of the same kind as the call's other arrays; Dirichlet only."""
        if self.bc != "dirichlet":
            raise ValueError(f"boundary: boundary values need a Dirichlet domain (this solver is {self.bc})")
        return self._arg(g, (6, self.n, self.n), "boundary", kind)[0]

    def boundary_from(self, fn, grad=None, robin=None):
        """Boundary values sampled from fn(x, y, z) (NumPy arrays in, an array of their shape out) at the 6 N^2 face centres: cell (i,j,k) is
        centred at ((i+1/2)h, (j+1/2)h, (k+1/2)h), so the faces lie at 0 and N h.  Returns the (6,N,N) NumPy array that boundary= takes.
        A Neumann face takes the outward normal derivative from grad(x, y, z), which returns the three components of grad u; a Robin face
        that derivative plus kappa fn, kappa from robin= (a (6,N,N) NumPy array or 6 numbers, as set_coefficients takes it)."""
        if self.faces is not None and grad is None:
            raise ValueError("grad: required when a face is Neumann or Robin (grad(x, y, z) returns the three components of grad u)")
        if robin is None and self.robin_faces:
            raise ValueError("robin: required when a face is 'convective' (kappa of du/dn + kappa u = g: a (6,N,N) array or 6 numbers)")
        if robin is not None and not self.robin_faces:
            raise ValueError("robin: this solver has no 'convective' face (bc=)")
        kappa = self._kappa(robin, "numpy") if robin is not None else None
        n, h = self.n, self.h
        c = (np.arange(n) + 0.5) * h
        slow, fast = np.meshgrid(c, c, indexing="ij")          # entry [q][p]: p the faster index
        g = np.empty((6, n, n))
        for face in range(6):
            wall = np.full((n, n), n * h if face & 1 else 0.0)
            if face < 2:
                x, y, z = wall, fast, slow                       # [k][j]
            elif face < 4:
                x, y, z = fast, wall, slow                       # [k][i]
            else:
                x, y, z = fast, slow, wall                       # [j][i]
            if self.faces is not None and self.faces[face] != "dirichlet":
                normal = np.asarray(grad(x, y, z)[face // 2], dtype=np.float64)
                g[face] = np.broadcast_to(normal if face & 1 else -normal, (n, n))
                if self.faces[face] == "convective":
                    g[face] = g[face] + kappa[face] * np.broadcast_to(np.asarray(fn(x, y, z), dtype=np.float64), (n, n))
            else:
                g[face] = np.broadcast_to(np.asarray(fn(x, y, z), dtype=np.float64), (n, n))
        return g

    def set_rhs(self, f, boundary=None):
        """Packs f (with boundary values: f + T(boundary)); returns the mean subtracted from it (periodic, or six Neumann faces, without an
        a alpha term), else 0.0."""
        p, where, kind = self._arg(f, (self.n,) * 3, "f")
        shift = ctypes.c_double(0.0)
        if boundary is None:
            self._sync_torch(kind)
            self._check(self.lib.hpgmg_user_set_rhs(self._ptr, p, where, ctypes.byref(shift)), "f")
            return shift.value
        pg = self._boundary(boundary, kind)
        self._sync_torch(kind)
        st = self.lib.hpgmg_user_set_rhs_dirichlet(self._ptr, p, pg, where, ctypes.byref(shift))
        if st == H.USER_NOT_FINITE:
            self._check(st, self._first_bad([("f", f, 0.0, False), ("boundary", boundary, 0.0, False)], st))
        self._check(st, "f, boundary")
        return shift.value

    def solve(self, f, method="fmg", rtol=1e-10, u0=None, out=None, boundary=None, max_iter=100):
        """u, SolveInfo.  method 'fmg': one F-cycle (the benchmark's solve); 'mg': V-cycles until |f - A u| < rtol |f| (20 at most).
        'pcg': conjugate gradients preconditioned with one V-cycle per iteration, until |f - A u| < rtol |f| or for max_iter iterations
        (max_iter is read by the two CG methods only) -- for coefficients with jumps, where 'mg' stalls.  It does not raise when it stops short:
        info.converged is False, u the last iterate and info.residual its residual.  DESIGN.md §11.3.
        'fpcg': the same with the flexible beta = -(Ap.z / p.Ap), for bc='periodic' and N / box_dim with an odd factor, where the V-cycle
        varies between iterations and 'pcg' can fail to converge; same arguments and reporting.  DESIGN.md §11.4.
        u0: start from it ('pcg', 'fpcg': as the first iterate; else u = u0 + e, the correction solved with V-cycles, and method is not used).
        boundary: Dirichlet values, Neumann / Robin data (module docstring); f then stands for f + T(boundary) throughout."""
        if method not in _METHOD:
            raise ValueError(f"method: {method!r} is not one of {sorted(_METHOD)}")
        if not rtol > 0.0:
            raise ValueError(f"rtol: {rtol!r} must be > 0")
        if method in ("pcg", "fpcg") and (isinstance(max_iter, bool) or not isinstance(max_iter, (int, np.integer)) or max_iter < 1):
            raise ValueError(f"max_iter: {max_iter!r} must be an int >= 1")
        _, _, kind = self._arg(f, (self.n,) * 3, "f")
        p0 = self._arg(u0, (self.n,) * 3, "u0", kind)[0] if u0 is not None else None
        if boundary is not None:
            self._boundary(boundary, kind)
        out = self._out(out, kind, f, "out")
        self.set_rhs(f, boundary)
        info = H.UserInfo()
        if method in ("pcg", "fpcg"):
            self._check(self.lib.hpgmg_user_set_max_iterations(self._ptr, int(max_iter)), "max_iter")
        self._sync_torch(kind)
        self._check(self.lib.hpgmg_user_solve(self._ptr, _METHOD[method], float(rtol), p0,
                                              H.WHERE_PLUGIN if kind == "torch" else H.WHERE_HOST, ctypes.byref(info)), "u0")
        self.get_solution(out)
        return out, SolveInfo(info.norm_of_residual, info.norm_of_f, info.vcycles, bool(info.converged), info.mean_shift)

    def get_solution(self, out=None):
        """The last solution into `out` (NumPy array or tensor), or a new NumPy array."""
        if out is None:
            out = np.empty((self.n,) * 3, dtype=np.float64)
        p, where, kind = self._arg(out, (self.n,) * 3, "out")
        self._sync_torch(kind)
        self._check(self.lib.hpgmg_user_get_solution(self._ptr, p, where), "out")
        return out

    def apply(self, x, out=None, boundary=None):
        """y = A x; with boundary values y = A0 x - T(boundary), so that apply(u, boundary=g) - f is the residual of a solution."""
        px, where, kind = self._arg(x, (self.n,) * 3, "x")
        pg = self._boundary(boundary, kind) if boundary is not None else None
        out = self._out(out, kind, x, "out")
        py = self._arg(out, (self.n,) * 3, "out", kind)[0]
        self._sync_torch(kind)
        if pg is None:
            self._check(self.lib.hpgmg_user_apply(self._ptr, px, py, where), "x")
            return out
        st = self.lib.hpgmg_user_apply_dirichlet(self._ptr, px, pg, py, where)
        if st == H.USER_NOT_FINITE:
            self._check(st, self._first_bad([("boundary", boundary, 0.0, False), ("x", x, 0.0, False)], st))
        self._check(st, "x, boundary")
        return out

    def flux(self, u, boundary=None, out=None):
        """(flux_i, flux_j, flux_k): q = -b beta grad u on every face, in the shapes of beta_i, beta_j, beta_k and positive towards increasing
        index (module docstring).  boundary: the data u was solved with (None: zero data).  out: an optional triple of arrays of
        u's kind to write into.  NumPy arrays or tensors according to u."""
        pu, where, kind = self._arg(u, (self.n,) * 3, "u")
        pg = self._boundary(boundary, kind) if boundary is not None else None
        shapes = [self._face_shape(axis) for axis in range(3)]
        if out is None:
            if kind == "torch":
                import torch
                out = tuple(torch.empty(shape, dtype=torch.float64, device=u.device) for shape in shapes)
            else:
                out = tuple(np.empty(shape, dtype=np.float64) for shape in shapes)
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 3:
                raise ValueError("out: expected a triple (flux_i, flux_j, flux_k) of arrays")
            out = tuple(out)
        po = [self._arg(q, shape, f"out[{axis}]", kind)[0] for axis, (q, shape) in enumerate(zip(out, shapes))]
        self._sync_torch(kind)
        st = self.lib.hpgmg_user_flux(self._ptr, pu, pg, po[0], po[1], po[2], where)
        if st == H.USER_NOT_FINITE:
            named = [("u", u, 0.0, False)] + ([("boundary", boundary, 0.0, False)] if boundary is not None else [])
            self._check(st, self._first_bad(named, st))
        self._check(st, "u, boundary" if boundary is not None else "u")
        return out

    def sensitivity(self, u, lam, boundary=None, out=None):
        """(d_alpha, d_beta_i, d_beta_j, d_beta_k): G_p = d/dp sum_c lam_c apply(u, boundary)_c for every coefficient entry p, in the shapes of
        set_coefficients' arguments (module docstring); d_alpha is None on a Poisson solver (a = 0).  With u the solution for
        `boundary` and lam the solution of A lam = dJ/du without boundary data, dJ/dp = -G_p.  boundary: the data u was solved with (None: zero
        data).  out: an optional 4-tuple of arrays of u's kind to write into (out[0] None on a Poisson solver).  NumPy arrays or tensors
        according to u."""
        pu, where, kind = self._arg(u, (self.n,) * 3, "u")
        pl = self._arg(lam, (self.n,) * 3, "lam", kind)[0]
        pg = self._boundary(boundary, kind) if boundary is not None else None
        helm = self.a != 0.0
        shapes = [(self.n,) * 3] + [self._face_shape(axis) for axis in range(3)]
        if out is None:
            if kind == "torch":
                import torch
                out = tuple(torch.empty(shape, dtype=torch.float64, device=u.device) for shape in shapes)
            else:
                out = tuple(np.empty(shape, dtype=np.float64) for shape in shapes)
            if not helm:
                out = (None,) + out[1:]
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 4:
                raise ValueError("out: expected a 4-tuple (d_alpha, d_beta_i, d_beta_j, d_beta_k) of arrays")
            out = tuple(out)
            if (out[0] is None) == helm:
                raise ValueError("out[0]: d_alpha is required when a != 0 (Helmholtz), must be None when a == 0 (Poisson)")
        po = [None if q is None else self._arg(q, shape, f"out[{slot}]", kind)[0] for slot, (q, shape) in enumerate(zip(out, shapes))]
        self._sync_torch(kind)
        st = self.lib.hpgmg_user_sensitivity(self._ptr, pu, pl, pg, po[0], po[1], po[2], po[3], where)
        if st == H.USER_NOT_FINITE:
            named = [("u", u, 0.0, False), ("lam", lam, 0.0, False)] + ([("boundary", boundary, 0.0, False)] if boundary is not None else [])
            self._check(st, self._first_bad(named, st))
        self._check(st, "u, lam, boundary" if boundary is not None else "u, lam")
        return out

    def cell_sensitivity(self, u, lam, k, mean="harmonic", boundary=None, out=None):
        """(d_alpha, d_k) for coefficients set with set_cell_coefficients(alpha, k, mean): d_alpha as sensitivity() returns it (None on a Poisson
        solver), and d_k[c] = sum over the six faces of cell c of G_face d beta_face / d k_c -- sensitivity()'s face arrays gathered through the
        derivative of the mean (1 on a wall), in one pass.  With u the solution for `boundary` and lam the solution of
        A lam = dJ/du without boundary data, dJ/dk = -d_k.  k is passed, not remembered: the chain rule is evaluated at the array handed in.
        out: an optional pair of arrays of u's kind to write into (out[0] None on a Poisson solver)."""
        m = self._mean(mean)
        pu, where, kind = self._arg(u, (self.n,) * 3, "u")
        pl = self._arg(lam, (self.n,) * 3, "lam", kind)[0]
        pk = self._arg(k, (self.n,) * 3, "k", kind)[0]
        pg = self._boundary(boundary, kind) if boundary is not None else None
        helm = self.a != 0.0
        if out is None:
            out = (self._out(None, kind, u, "out[0]") if helm else None, self._out(None, kind, u, "out[1]"))
        else:
            if not isinstance(out, (tuple, list)) or len(out) != 2:
                raise ValueError("out: expected a pair (d_alpha, d_k) of arrays")
            out = tuple(out)
            if (out[0] is None) == helm:
                raise ValueError("out[0]: d_alpha is required when a != 0 (Helmholtz), must be None when a == 0 (Poisson)")
            if out[1] is None:
                raise ValueError("out[1]: d_k is required")
        po = [None if q is None else self._arg(q, (self.n,) * 3, f"out[{slot}]", kind)[0] for slot, q in enumerate(out)]
        self._sync_torch(kind)
        st = self.lib.hpgmg_user_cell_sensitivity(self._ptr, pu, pl, pk, m, pg, po[0], po[1], where)
        if st in (H.USER_NOT_FINITE, H.USER_OUT_OF_RANGE):
            for name, x in (("u", u), ("lam", lam), ("boundary", boundary)):      # these need only be finite; k also > 0
                if x is not None and not np.isfinite(x.detach().cpu().numpy() if _is_tensor(x) else x).all():
                    self._check(H.USER_NOT_FINITE, name)
            if not self._entries_ok(k, True):
                self._check(st, "k")
            raise ValueError(f"k: {self._mean_bad(st, mean)}")      # every entry passes: a face mean of k does not
        self._check(st, "u, lam, k, boundary" if boundary is not None else "u, lam, k")
        return out

    # ---- implicit time stepping (module docstring)
    def set_shift(self, a):
        """A new a (> 0) for a Helmholtz solver: every level's operator is rebuilt from the coefficients already set, without packing an array.
        Afterwards the solver is, bit for bit, one created with that a and given the same coefficients."""
        if self.a == 0.0:
            raise ValueError("a: this solver is Poisson (a = 0) and stays so (create it with a != 0)")
        if isinstance(a, bool) or not isinstance(a, (int, float, np.integer, np.floating)) or not np.isfinite(a) or not a > 0.0:
            raise ValueError(f"a: {a!r} must be a finite number > 0")
        self.coefficient_version += 1
        self._check(self.lib.hpgmg_user_set_shift(self._ptr, float(a)), "a")
        self.a = float(a)

    def _march_args(self, dt, theta):
        if self.a == 0.0:
            raise ValueError("a: time stepping needs a Helmholtz solver (create it with a != 0 and set alpha; a is then set from dt and theta)")
        for name, v in (("dt", dt), ("theta", theta)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                raise ValueError(f"{name}: {v!r} must be a finite number")
        if not dt > 0.0:
            raise ValueError(f"dt: {dt!r} must be > 0")
        if not 0.5 <= theta <= 1.0:
            raise ValueError(f"theta: {theta!r} must lie in [0.5, 1] (1: backward Euler, 0.5: Crank-Nicolson)")
        return float(dt), float(theta)

    def start(self, u, f, boundary=None, dt=None, theta=1.0):
        """Begins a march of  alpha du/dt = b div(beta grad u) + f  at the state u, with the source f and the wall data `boundary` of that time
        (as set_rhs takes them).  Sets a = 1 / (theta dt) and the rate w = alpha du/dt = f - L(u; boundary).  theta = 1: backward Euler,
        0.5: Crank-Nicolson.  The state and the rate stay in the library; step() advances them, get_solution() and rate() return them."""
        if dt is None:
            raise ValueError("dt: required (the time step, > 0)")
        dt, theta = self._march_args(dt, theta)
        pu, where, kind = self._arg(u, (self.n,) * 3, "u")
        pf = self._arg(f, (self.n,) * 3, "f", kind)[0]
        pg = self._boundary(boundary, kind) if boundary is not None else None
        self._sync_torch(kind)
        self.coefficient_version += 1        # the march sets a = 1 / (theta dt)
        st = self.lib.hpgmg_user_start(self._ptr, pu, pf, pg, where, dt, theta)
        if st == H.USER_NOT_FINITE:
            named = [("u", u, 0.0, False), ("f", f, 0.0, False)] + ([("boundary", boundary, 0.0, False)] if boundary is not None else [])
            self._check(st, self._first_bad(named, st))
        if st == H.USER_UNSUPPORTED:
            raise ValueError("alpha: zero everywhere, so there is no du/dt term to march")
        self._check(st, "u, f, boundary, dt or theta")
        self.a, self._dt, self._theta, self._t, self._wave = 1.0 / (theta * dt), dt, theta, 0.0, None

    def step(self, f, boundary=None, dt=None, theta=None, rtol=1e-8):
        """One theta step to the next time; f and `boundary` are those of the NEW time.  dt, theta None: as in the call before (a change rebuilds
        the operator's diagonals, nothing else).  V-cycles from the state run until the residual of the step's equation is below rtol times its
        right-hand side (20 at most).  Returns StepInfo: SolveInfo's fields for that solve, rate = max |alpha du/dt| at the new time and t, the
        time since start().  The rate is exact for the state the solve stopped at, whatever rtol."""
        if self._dt is None:
            raise ValueError("step: no march is live (start() begins one; set_coefficients, set_rhs and solve end it)")
        if not rtol > 0.0:
            raise ValueError(f"rtol: {rtol!r} must be > 0")
        dt, theta = self._march_args(self._dt if dt is None else dt, self._theta if theta is None else theta)
        pf, where, kind = self._arg(f, (self.n,) * 3, "f")
        pg = self._boundary(boundary, kind) if boundary is not None else None
        self._sync_torch(kind)
        info, rate = H.UserInfo(), ctypes.c_double(0.0)
        if 1.0 / (theta * dt) != self.a:
            self.coefficient_version += 1
        st = self.lib.hpgmg_user_step(self._ptr, pf, pg, where, dt, theta, float(rtol), ctypes.byref(info), ctypes.byref(rate))
        if st == H.USER_NOT_FINITE:
            named = [("f", f, 0.0, False)] + ([("boundary", boundary, 0.0, False)] if boundary is not None else [])
            self._check(st, self._first_bad(named, st))
        if st == H.USER_NOT_READY:
            raise ValueError("step: no march is live (start() begins one; set_coefficients, set_rhs and solve end it)")
        self._check(st, "f, boundary, dt or theta")
        self.a, self._dt, self._theta, self._t = 1.0 / (theta * dt), dt, theta, self._t + dt
        return StepInfo(info.norm_of_residual, info.norm_of_f, info.vcycles, bool(info.converged), info.mean_shift, rate.value, self._t)

    def rate(self, out=None):
        """The rate w = alpha du/dt of the march's state into `out` (NumPy array or tensor), or a new NumPy array."""
        if out is None:
            out = np.empty((self.n,) * 3, dtype=np.float64)
        p, where, kind = self._arg(out, (self.n,) * 3, "out")
        self._sync_torch(kind)
        st = self.lib.hpgmg_user_get_rate(self._ptr, p, where)
        if st == H.USER_NOT_READY:
            raise ValueError("rate: no march is live (start() begins one; set_coefficients, set_rhs and solve end it)")
        self._check(st, "out")
        return out

    # ---- the wave equation (module docstring)
    _NO_WAVE = "no wave march is live (wave_start() begins one; set_coefficients, set_rhs, solve, eigs and start end it)"

    @staticmethod
    def _wave_shift(dt, beta, gamma, damping):
        """a of one Newmark step, in the library's written order (inf where a divisor underflows to zero, as in C)."""
        with np.errstate(all="ignore"):
            return float(np.float64(1.0) / np.float64(beta * (dt * dt)) + np.float64(damping * gamma) / np.float64(beta * dt))

    def _wave_args(self, dt, beta, gamma, damping):
        if self.a == 0.0:
            raise ValueError("a: the wave march needs a Helmholtz solver (create it with a != 0 and set alpha; a is then set from dt, beta, gamma and damping)")
        for name, v in (("dt", dt), ("beta", beta), ("gamma", gamma), ("damping", damping)):
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not np.isfinite(v):
                raise ValueError(f"{name}: {v!r} must be a finite number")
        if not dt > 0.0:
            raise ValueError(f"dt: {dt!r} must be > 0")
        if not damping >= 0.0:
            raise ValueError(f"damping: {damping!r} must be >= 0")
        if not gamma >= 0.5:
            raise ValueError(f"gamma: {gamma!r} must be >= 0.5 (a smaller gamma is unstable)")
        if not beta >= gamma / 2.0:
            raise ValueError(f"beta: {beta!r} must be >= gamma / 2 = {gamma / 2.0!r} (smaller values, central differences included, are conditionally stable)")
        dt, beta, gamma, damping = float(dt), float(beta), float(gamma), float(damping)
        if not np.isfinite(self._wave_shift(dt, beta, gamma, damping)):
            raise ValueError(f"dt: {dt!r} gives a shift a = 1 / (beta dt^2) + damping gamma / (beta dt) that is not finite")
        return dt, beta, gamma, damping

    @staticmethod
    def _wave_info(info):
        return WaveInfo(info.norm_of_residual, info.norm_of_f, info.vcycles, bool(info.converged), info.mean_shift, info.t, info.kinetic, info.potential)

    def wave_start(self, u, v, f, boundary=None, dt=None, beta=0.25, gamma=0.5, damping=0.0):
        """Begins a march of  alpha d2u/dt2 + damping alpha du/dt = b div(beta grad u) + f  at the state u and the velocity v, with the source f and the wall
        data `boundary` of that time (as set_rhs takes them), by the Newmark rule (beta, gamma): gamma >= 1/2, beta >= gamma / 2.  Sets
        a = 1 / (beta dt^2) + damping gamma / (beta dt) and the acceleration (f - L(u; boundary)) / alpha - damping v, which needs alpha > 0 in every cell.
        Returns WaveInfo with t = 0, vcycles = 0 and the energies of the start.  wave_step() advances; get_solution(), velocity() and acceleration() return
        the state."""
        if dt is None:
            raise ValueError("dt: required (the time step, > 0)")
        dt, beta, gamma, damping = self._wave_args(dt, beta, gamma, damping)
        pu, where, kind = self._arg(u, (self.n,) * 3, "u")
        pv = self._arg(v, (self.n,) * 3, "v", kind)[0]
        pf = self._arg(f, (self.n,) * 3, "f", kind)[0]
        pg = self._boundary(boundary, kind) if boundary is not None else None
        self._sync_torch(kind)
        self.coefficient_version += 1        # the march sets a
        info = H.UserWaveInfo()
        st = self.lib.hpgmg_user_wave_start(self._ptr, pu, pv, pf, pg, where, dt, beta, gamma, damping, ctypes.byref(info))
        if st in (H.USER_OK, H.USER_NOT_FINITE):
            self._dt = self._wave = None     # past its checks the library has ended whatever march was live
        if st == H.USER_NOT_FINITE:
            named = [("u", u, 0.0, False), ("v", v, 0.0, False), ("f", f, 0.0, False)] + ([("boundary", boundary, 0.0, False)] if boundary is not None else [])
            self._check(st, self._first_bad(named, st))
        if st == H.USER_OUT_OF_RANGE:
            raise ValueError("alpha: zero in some cell, so the acceleration (f - L u) / alpha is not defined there (the wave march needs alpha > 0 everywhere)")
        self._check(st, "u, v, f, boundary, dt, beta, gamma or damping")
        self.a, self._t, self._wave = self._wave_shift(dt, beta, gamma, damping), 0.0, (dt, beta, gamma, damping)
        return self._wave_info(info)

    def wave_step(self, f, boundary=None, dt=None, rtol=1e-8):
        """One Newmark step to the next time; f and `boundary` are those of the NEW time.  dt None: as in the call before (a change rebuilds the operator's
        diagonals, nothing else).  V-cycles from the predictor run until the residual of the step's equation is below rtol times its right-hand side (20 at
        most).  Returns WaveInfo: SolveInfo's fields for that solve, t, and the kinetic and potential energy at the new time."""
        if self._wave is None:
            raise ValueError(f"wave_step: {self._NO_WAVE}")
        if not rtol > 0.0:
            raise ValueError(f"rtol: {rtol!r} must be > 0")
        dt, beta, gamma, damping = self._wave_args(self._wave[0] if dt is None else dt, *self._wave[1:])
        pf, where, kind = self._arg(f, (self.n,) * 3, "f")
        pg = self._boundary(boundary, kind) if boundary is not None else None
        self._sync_torch(kind)
        a, info = self._wave_shift(dt, beta, gamma, damping), H.UserWaveInfo()
        if a != self.a:
            self.coefficient_version += 1
        st = self.lib.hpgmg_user_wave_step(self._ptr, pf, pg, where, dt, float(rtol), ctypes.byref(info))
        if st == H.USER_NOT_FINITE:
            named = [("f", f, 0.0, False)] + ([("boundary", boundary, 0.0, False)] if boundary is not None else [])
            self._check(st, self._first_bad(named, st))
        if st == H.USER_NOT_READY:
            self._wave = None
            raise ValueError(f"wave_step: {self._NO_WAVE}")
        self._check(st, "f, boundary or dt")
        self.a, self._t, self._wave = a, self._t + dt, (dt, beta, gamma, damping)
        return self._wave_info(info)

    def _wave_get(self, call, name, out):
        if out is None:
            out = np.empty((self.n,) * 3, dtype=np.float64)
        p, where, kind = self._arg(out, (self.n,) * 3, "out")
        self._sync_torch(kind)
        st = call(self._ptr, p, where)
        if st == H.USER_NOT_READY:
            raise ValueError(f"{name}: {self._NO_WAVE}")
        self._check(st, "out")
        return out

    def velocity(self, out=None):
        """The velocity v = du/dt of the wave march's state into `out` (NumPy array or tensor), or a new NumPy array."""
        return self._wave_get(self.lib.hpgmg_user_get_velocity, "velocity", out)

    def acceleration(self, out=None):
        """The acceleration d2u/dt2 of the wave march's state into `out` (NumPy array or tensor), or a new NumPy array."""
        return self._wave_get(self.lib.hpgmg_user_get_acceleration, "acceleration", out)

    # ---- eigenmodes (module docstring)
    def eigs(self, k, rtol=1e-6, max_iter=60, extra=2, x0=None, out=None):
        """lam, modes, EigInfo: the k smallest lambda of K x = lambda M x (K = -b div(beta grad .) with the solver's walls and zero data, M = diag(alpha)
        or I) as a float64 array (k,), ascending, and their modes (k,N,N,N), each normalised to h^3 x^T M x = 1 (sign, and the basis inside a degenerate
        cluster, unspecified).  LOBPCG with k + extra <= 12 columns and one V-cycle per unconverged column and iteration, until the k residuals
        max |A x - mu M x| / (mu max |M x|) are below rtol or for max_iter iterations; it does not raise when it stops short (info.converged).
        A Helmholtz solver iterates on A = a M + K with the a in force: info.mu = a + lam, and lam loses digits when a >> lam (set_shift moves a).
        x0: a start block (k + extra,N,N,N); None: a deterministic one, so the same call twice gives the same bits.  out: where the modes go -- a NumPy
        array (the host path) or a GPU float64 tensor written in place, of the same kind as x0; None: a new NumPy array (a tensor when x0 is one).
        Ends a march and invalidates the stored right-hand side and solution; the coefficients and coefficient_version stay."""
        for name, v, low in (("k", k, 1), ("extra", extra, 0), ("max_iter", max_iter, 1)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < low:
                raise ValueError(f"{name}: {v!r} must be an int >= {low}")
        k, extra, m = int(k), int(extra), int(k) + int(extra)
        if m > H.USER_EIGS_MAX_BLOCK:
            raise ValueError(f"k + extra: {m} columns, at most {H.USER_EIGS_MAX_BLOCK} are iterated on")
        if m > self.n ** 3:
            raise ValueError(f"k + extra: {m} columns, the problem has {self.n ** 3} unknowns")
        if isinstance(rtol, bool) or not isinstance(rtol, (int, float, np.integer, np.floating)) or not rtol > 0.0:
            raise ValueError(f"rtol: {rtol!r} must be > 0")
        kind, p0 = None, None
        if x0 is not None:
            p0, _, kind = self._arg(x0, (m,) + (self.n,) * 3, "x0")
        if out is None:
            if kind == "torch":
                import torch
                out = torch.empty((k,) + (self.n,) * 3, dtype=torch.float64, device=x0.device)
            else:
                out = np.empty((k,) + (self.n,) * 3, dtype=np.float64)
        po, where, kind = self._arg(out, (k,) + (self.n,) * 3, "out", kind)
        self._sync_torch(kind)
        lam, info = np.empty(k, dtype=np.float64), H.UserEigInfo()
        st = self.lib.hpgmg_user_eigs(self._ptr, k, extra, float(rtol), int(max_iter), p0, where,
                                      lam.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), po, ctypes.byref(info))
        if st == H.USER_UNSUPPORTED:
            raise ValueError("eigs: this solver is singular (no a alpha term on a periodic box or between six Neumann walls): create it with a > 0 "
                             "and alpha = 1, and the constant mode comes back as lambda ~ 0")
        if st == H.USER_OUT_OF_RANGE:
            raise ValueError("alpha: zero in some cell, so M = diag(alpha) is not positive definite (eigs needs alpha > 0 everywhere)")
        if st == H.USER_NOT_READY:
            raise ValueError("eigs: no valid coefficients (an earlier set_coefficients was refused)")
        self._check(st, "x0" if st == H.USER_NOT_FINITE else "k, extra, rtol, max_iter, x0 or out")
        self._dt = self._wave = None        # a march is over
        return lam, out, EigInfo(info.iterations, info.vcycles, np.array(info.residuals[:k]), np.array(info.mu[:k]), bool(info.converged))

    def wall_flux(self, fluxes):
        """The OUTWARD flux through the six walls as a (6,N,N) array in `boundary`'s layout, from the triple flux() returned: the wall entries
        of the three arrays, those of the low walls negated.  Its sum times h^2 is what leaves the box."""
        if self.bc != "dirichlet":
            raise ValueError(f"fluxes: a {self.bc} solver has no walls")
        if not isinstance(fluxes, (tuple, list)) or len(fluxes) != 3:
            raise ValueError("fluxes: expected the triple (flux_i, flux_j, flux_k) of flux()")
        kind = None
        for axis, q in enumerate(fluxes):
            kind = self._arg(q, self._face_shape(axis), f"fluxes[{axis}]", kind)[2]
        qi, qj, qk = fluxes
        n = self.n
        faces = [-qi[:, :, 0], qi[:, :, n], -qj[:, 0, :], qj[:, n, :], -qk[0], qk[n]]
        if kind == "torch":
            import torch
            return torch.stack(faces).contiguous()
        return np.ascontiguousarray(np.stack(faces))

    def close(self):
        if self._ptr is not None:
            self.lib.hpgmg_user_destroy(self._ptr)
            self._ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
