"""Solver.eigs (hpgmg_user_eigs) on the CPU oracle.

Exact reference: at N = 8 and N = 12 in boxes of 4 (512 and 1728 unknowns; 12 / 4 = 3 boxes a side, an odd factor) the dense operator is built column
by column through Solver.apply and numpy.linalg.eigh gives the spectrum of M^-1/2 A M^-1/2.  Each returned pair is accepted by a bound that is
rigorous, not tuned: with rho = |A x - mu M x|_{M^-1} / |x|_M (user_eigs_lib.rho, from the returned mode and the dense A) some exact eigenvalue lies
within rho of mu, so the j-th returned mu must be within rho_j + 64 eps mu_j of the j-th smallest exact one -- which also proves no mode was skipped,
k being chosen with lambda_k < lambda_k+1.  Closed forms hold the constant-coefficient operators at N = 16 in boxes of 8 the same way.

Iterations: ITERATIONS holds what the oracle took at rtol = 1e-6 when the feature was written; the gate is + 25 %, the margin of the CG tests.
"""
import ctypes

import numpy as np
import pytest

import hpgmg_amd as H
import hpgmg_testlib as T
import user_eigs_lib as E
from hpgmg_amd.problem import EigInfo, Solver

K, RTOL = 3, 1e-6
# (case, N) -> iterations at rtol = 1e-6, k = 3, extra = 2, max_iter = 60, as measured on the oracle
ITERATIONS = {("contrast", 8): 12, ("contrast", 12): 14, ("corners", 8): 11, ("corners", 12): 11, ("dirichlet", 8): 10, ("dirichlet", 12): 11,
              ("neumann", 8): 10, ("neumann", 12): 10, ("periodic", 8): 18, ("periodic", 12): 20, ("poisson", 8): 10, ("poisson", 12): 11,
              ("random-alpha", 8): 11, ("random-alpha", 12): 10, ("robin", 8): 9, ("robin", 12): 10}
CLOSED_ITERATIONS = {"dirichlet": 10, "neumann": 7, "periodic": 8}      # N = 16, k = 4
CONTRAST_16 = 13                                                          # the contrast-100 block field at N = 16: extra = 2 is enough


@pytest.fixture(scope="module")
def lib():
    be = T.Backend.oracle()
    return be.lib


def gate(measured, recorded):
    return measured <= int(np.floor(1.25 * recorded))


@pytest.mark.parametrize("n", [8, 12])
@pytest.mark.parametrize("name", sorted(E.CASES))
def test_pairs_against_the_dense_spectrum(lib, name, n):
    a = E.CASES[name][1]
    with Solver(n, box_dim=4, bc=E.bc_of(name), a=a, b=E.B, lib=lib) as s:
        alpha = E.set_case(s, name, n)
        version = s.coefficient_version
        lam, modes, info = s.eigs(K, rtol=RTOL)
        assert s.coefficient_version == version
        A = E.dense_operator(s)
    assert isinstance(info, EigInfo) and lam.shape == (K,) and lam.dtype == np.float64 and modes.shape == (K, n, n, n)
    assert info.residuals.shape == (K,) and info.mu.shape == (K,)
    m = np.ones(n ** 3) if alpha is None else alpha.reshape(-1)
    exact = E.exact_spectrum(A, m)
    assert exact[0] > 0.0 and exact[K] - exact[K - 1] > 1e-8 * exact[K], exact[:K + 1]          # A is SPD; lambda_k < lambda_k+1
    print(f"{name} N={n}: iterations {info.iterations} vcycles {info.vcycles} residuals {info.residuals} mu {info.mu} exact {exact[:K]}")
    assert info.converged and (info.residuals < RTOL).all() and 0 <= info.iterations <= 60
    assert np.array_equal(lam, info.mu - a) and (np.diff(lam) >= 0.0).all()
    X = modes.reshape(K, -1)
    for j in range(K):
        Ax = A @ X[j]
        bound = E.rho(Ax, m, info.mu[j], X[j]) + 64.0 * E.EPS * info.mu[j]
        assert abs(info.mu[j] - exact[j]) <= bound, (j, info.mu[j], exact[j], bound)
        own = E.residual_measure(Ax, m, info.mu[j], X[j])
        slack = 32.0 * E.EPS * (np.abs(A) @ np.abs(X[j]) + info.mu[j] * np.abs(m * X[j])).max() / (info.mu[j] * np.abs(m * X[j]).max())
        assert abs(info.residuals[j] - own) <= slack, (j, info.residuals[j], own, slack)
    gram = (X * m) @ X.T * s.h ** 3
    assert np.abs(gram - np.eye(K)).max() <= 1e-10, gram
    assert (name, n) in ITERATIONS and gate(info.iterations, ITERATIONS[name, n]), (info.iterations, ITERATIONS.get((name, n)))


@pytest.mark.parametrize("kind,a", [("dirichlet", 0.0), ("neumann", 1.0), ("periodic", 1.0)])
def test_closed_forms(lib, kind, a):
    """Constant coefficients at N = 16 in boxes of 8, k = 4: the cluster {111}, {211, 121, 112} (Neumann: {000}, {100, 010, 001}; periodic: {000} and
    three of the six-fold {+-100, 0+-10, 00+-1})."""
    n, k = 16, 4
    with Solver(n, box_dim=8, bc=kind, a=a, b=E.B, lib=lib) as s:
        lam, modes, info = s.eigs(k, rtol=RTOL)
        Ax = [s.apply(np.ascontiguousarray(x)).reshape(-1) for x in modes]
    want = E.closed_form(n, E.B, 1.0 / n, k, kind)
    print(f"closed form {kind}: iterations {info.iterations} lam {lam} want {want}")
    assert info.converged
    m = np.ones(n ** 3)
    for j in range(k):
        bound = E.rho(Ax[j], m, info.mu[j], modes[j].reshape(-1)) + 64.0 * E.EPS * info.mu[j]
        assert abs(info.mu[j] - (a + want[j])) <= bound, (j, lam[j], want[j], bound)
    if kind == "neumann":
        assert abs(lam[0]) <= E.rho(Ax[0], m, info.mu[0], modes[0].reshape(-1)) + 64.0 * E.EPS * info.mu[0]
    assert kind in CLOSED_ITERATIONS and gate(info.iterations, CLOSED_ITERATIONS[kind]), info.iterations


def test_contrast_100_converges_within_60(lib):
    """The contrast-100 block field at N = 16 in boxes of 8 with the default extra = 2."""
    n = 16
    with Solver(n, box_dim=8, a=E.CASES["contrast"][1], b=E.B, lib=lib) as s:
        E.set_case(s, "contrast", n)
        lam, modes, info = s.eigs(K, rtol=RTOL, max_iter=60)
    print(f"contrast N={n}: iterations {info.iterations} residuals {info.residuals}")
    assert info.converged and info.iterations <= 60 and gate(info.iterations, CONTRAST_16)


def refused(call, *args, **kwargs):
    try:
        call(*args, **kwargs)
    except ValueError as e:
        return str(e)
    raise AssertionError("the call was accepted")


def test_lifecycle(lib):
    n, k = 8, 2
    rng = np.random.default_rng(5)
    f, u0 = rng.random((n, n, n)) - 0.5, rng.random((n, n, n))
    with Solver(n, box_dim=4, bc=E.bc_of("corners"), a=1.3, b=E.B, lib=lib) as s, Solver(n, box_dim=4, bc=E.bc_of("corners"), a=1.3, b=E.B, lib=lib) as fresh:
        E.set_case(s, "corners", n); E.set_case(fresh, "corners", n)
        version = s.coefficient_version
        lam, modes, info = s.eigs(k, rtol=RTOL)
        again = s.eigs(k, rtol=RTOL)
        assert lam.tobytes() == again[0].tobytes() and modes.tobytes() == again[1].tobytes()           # the same call twice: the same bytes
        assert info.iterations == again[2].iterations and info.residuals.tobytes() == again[2].residuals.tobytes()
        out = np.full((k, n, n, n), np.nan)
        got = s.eigs(k, rtol=RTOL, out=out)
        assert got[1] is out and out.tobytes() == modes.tobytes()                                    # out= is written in place
        # the returned block with two guards: nothing left to do but the guards' business
        x0 = np.concatenate([modes, rng.random((2, n, n, n)) - 0.5])
        lam1, modes1, info1 = s.eigs(k, rtol=RTOL, x0=x0)
        assert info1.converged and info1.iterations <= 1 and np.abs(lam1 - lam).max() <= 1e-9 * lam.max()
        # a march dies; a solve still works and gives a fresh solver's bytes; the coefficients were not touched
        s.start(u0, f, dt=0.1)
        a_march = s.a
        s.step(f)
        s.eigs(k, rtol=RTOL)
        assert "no march is live" in refused(s.step, f)
        assert s.coefficient_version == version + 1 and s.a == a_march                               # the march's shift, not eigs
        fresh.set_shift(a_march)
        u, _ = s.solve(f, method="mg", rtol=1e-9)
        v, _ = fresh.solve(f, method="mg", rtol=1e-9)
        assert u.tobytes() == v.tobytes()
        lam_m = s.eigs(k, rtol=RTOL)[0]
        assert np.abs(lam_m - lam).max() <= 1e-5 * lam.max()                                         # lambda does not depend on the shift


def test_refusals(lib):
    n = 8
    out = np.full((2, n, n, n), np.nan)
    untouched = lambda: np.isnan(out).all()  # noqa: E731
    with Solver(n, box_dim=4, bc="periodic", a=0.0, lib=lib) as s:
        assert "singular" in refused(s.eigs, 2, out=out) and "a > 0 and alpha = 1" in refused(s.eigs, 2, out=out) and untouched()
    with Solver(n, box_dim=4, bc="neumann", a=0.0, lib=lib) as s:
        assert "singular" in refused(s.eigs, 2, out=out) and untouched()
    with Solver(n, box_dim=4, a=1.0, lib=lib) as s:
        alpha, bi, bj, bk = E.random_coefficients(n, "dirichlet", True, 3)
        holed = alpha.copy()
        holed[1, 2, 3] = 0.0
        s.set_coefficients(holed, bi, bj, bk)
        assert refused(s.eigs, 2, out=out).startswith("alpha: zero in some cell") and untouched()
        s.set_coefficients(alpha, bi, bj, bk)
        for kwargs, text in ((dict(k=0), "k: 0 must be an int >= 1"), (dict(k=2, extra=-1), "extra: -1 must be an int >= 0"), (dict(k=2.0), "k: 2.0 must be"),
                             (dict(k=11, extra=2), "k + extra: 13 columns, at most 12"), (dict(k=2, rtol=0.0), "rtol:"), (dict(k=2, max_iter=0), "max_iter:"),
                             (dict(k=2, x0=np.zeros((3, n, n, n))), "x0: shape"), (dict(k=3, out=out), "out: shape")):
            assert refused(s.eigs, **{"out": out, **kwargs} if "out" not in kwargs else kwargs).startswith(text), kwargs
        bad = np.zeros((4, n, n, n))
        bad[2, 1, 1, 1] = np.inf
        assert refused(s.eigs, 2, x0=bad, out=out).startswith("x0: holds a value that is not finite") and untouched()
        negative = bi.copy()
        negative[0, 0, 0] = -1.0
        assert "out of range" in refused(s.set_coefficients, alpha, negative, bj, bk)
        assert "no valid coefficients" in refused(s.eigs, 2, out=out) and untouched()
        s.set_coefficients(alpha, bi, bj, bk)
        lam, modes, info = s.eigs(2, out=out)                                                        # zero start vectors break down: reported, not raised
        assert modes is out and info.converged
        lam0, _, info0 = s.eigs(2, x0=np.zeros((4, n, n, n)))
        assert not info0.converged
        # the process reconfigured under the live solver: refused, nothing written, and fine again once the configuration is back
        other = H.Config(H.OP_7PT, H.SMOOTH_GSRB, 1, 1)
        assert lib.hpgmg_configure(ctypes.byref(other)) == 0
        try:
            out[:] = np.nan
            assert "configured for another" in refused(s.eigs, 2, out=out) and untouched()
        finally:
            mine = H.Config(H.OP_7PT, H.SMOOTH_CHEBY, 1, 1)
            assert lib.hpgmg_configure(ctypes.byref(mine)) == 0
        assert s.eigs(2, out=out)[2].converged
    # "more columns than unknowns" cannot be provoked: the smallest solver there is has 4^3 = 64 unknowns and a block has at most 12 columns
    assert "n, box_dim" in refused(Solver, 3, box_dim=3, lib=lib) and "n, box_dim" in refused(Solver, 2, box_dim=2, lib=lib)
    with Solver(4, box_dim=4, a=1.0, lib=lib) as s:                                                 # 64 unknowns: every block size fits
        lam, modes, info = s.eigs(10, extra=2, rtol=RTOL)
        assert info.converged and (np.diff(lam) >= 0.0).all()
