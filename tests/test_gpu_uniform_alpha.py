"""Uniform alpha (HPGMG_UNIFORM_ALPHA / hpgmg_set_uniform_alpha): where rebuild_operator finds VECTOR_ALPHA to be ONE bit pattern over every interior cell of the
level, the sweep pairs that form Dinv (kernels/cheby_pair.hpp, UA instances) and the two wide fused residual passes (kernels/stencil7_wide.hpp, launched from kernels/stencil.hip) take alpha from their arguments
instead of streaming the vector.  The vector is the contract: whichever instance runs, the bits are those of the oracle, which always reads it.  Every comparison here is
bit for bit; hpgmg_uniform_alpha_launches() says which instance ran.  The uniform value is 0.7, not 1.0: a kernel that dropped the term or assumed 1.0 fails.

The waves per workgroup and the k chunk are chosen once per process (HPGMG_TUNE_PAIR_NW / _KC), so the smooth() cases run in a worker process per launch shape: this
file run as a script does all of them and prints one JSON line each.
"""
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, HERE)
    import conftest  # noqa: F401  (the OpenMP environment of the suite, before any runtime loads)

import numpy as np
import pytest

import hpgmg_amd as H
from hpgmg_testlib import ROOT, Backend, Level, load_golden, seeded_field
from test_gpu_operators import VARIANTS

pytestmark = pytest.mark.gpu

VARIANT, A, B = "7pt-cheby-helm", 1.0, 1.0
ALPHA = 0.7
U, F, R, TEMP = H.VECTOR_U, H.VECTOR_F, H.VECTOR_R, H.VECTOR_TEMP
# (boxes per side, box side): one box of 128^3 (walls on every side), 128^3 in boxes of 64 (the NARROW instances), 2^3 boxes of 128^3 (an interior tile edge in i: the
# EDGEW instances with 10 waves, the pre-pass with 12; two k chunks)
GEOMS = {"1x128": (1, 128), "2x64": (2, 64), "2x128": (2, 128)}
MODES = ("smooth", "cycle", "interp")      # smooth(): x1 kept; the in-cycle form: x1 of the second pair not stored; the up leg: interpolation folded into the first pair
c_int, c_dbl, c_ll, vp = ctypes.c_int, ctypes.c_double, ctypes.c_longlong, ctypes.c_void_p


def declare(lib):
    lib.hpgmg_set_uniform_alpha.argtypes = [c_int]
    lib.hpgmg_uniform_alpha_launches.restype = c_ll
    lib.hpgmg_pair_formed_dinv_launches.restype = c_ll
    lib.hpgmg_smooth_in_cycle.restype = c_int
    lib.hpgmg_smooth_in_cycle.argtypes = [vp, c_int, c_int, c_dbl, c_dbl]
    lib.hpgmg_interp_smooth_fused.restype = c_int
    lib.hpgmg_interp_smooth_fused.argtypes = [vp, c_int, c_int, vp, c_dbl, c_dbl]
    lib.hpgmg_residual_restrict_zero_fused.restype = c_int
    lib.hpgmg_residual_restrict_zero_fused.argtypes = [vp, c_int, vp, c_int, c_int, c_dbl, c_dbl, c_int]
    lib.hpgmg_residual_norm_fused.restype = c_int
    lib.hpgmg_residual_norm_fused.argtypes = [vp, c_int, c_int, c_int, c_dbl, c_dbl, ctypes.POINTER(c_dbl)]
    return lib


def bits(x):
    return np.ascontiguousarray(x).view(np.uint64)


def same_bits(x, y):
    return all(np.array_equal(bits(p), bits(q)) for p, q in zip(x, y))


class TwoLevel:
    """The same fine level (and the coarse level under it) on both backends: seeded data in [-1, 1], positive seeded betas, alpha = 0.7 in every cell."""

    def __init__(self, hip, oracle, geom, seed=4100):
        self.hip, self.oracle, self.geom = hip, oracle, geom
        self.lib = declare(hip.lib)
        self.fine, self.mg = [], []
        for be in (hip, oracle):
            be.configure(**VARIANTS[VARIANT])
            fine = be.level(*geom)
            for vid in range(fine.num_vectors):
                d = seeded_field(fine, seed + vid)
                if vid >= H.VECTOR_DINV:
                    d = np.abs(d) + 0.5
                if vid == H.VECTOR_ALPHA:
                    d = np.full_like(d, ALPHA)
                fine.write_all(vid, d)
            for vid in range(H.VECTOR_DINV, fine.num_vectors):
                be.lib.exchange_boundary(fine.ptr, vid, H.STENCIL_SHAPE_BOX)
            self.fine.append(fine)
            self.mg.append(be.lib.hpgmg_mg_create(fine.ptr, A, B, 1))
            be.lib.rebuild_operator(fine.ptr, None, A, B)
        self.lh, self.lo = self.fine
        self.ch, self.co = (Level(be, be.lib.hpgmg_mg_level(m, 1)) for be, m in zip((hip, oracle), self.mg))
        coarse_e = seeded_field(self.ch, seed + 77)
        for c in (self.ch, self.co):
            c.write_all(U, coarse_e)
        self.start = {v: self.lh.read_all(v) for v in (U, TEMP, F)}
        self.alpha_is = "uniform"

    def use(self):
        for be in (self.hip, self.oracle):
            be.configure(**VARIANTS[VARIANT])

    def reset(self, lv):
        for v, d in self.start.items():
            lv.write_all(v, d)

    def set_alpha(self, per_box, tag, rebuild=True):
        """VECTOR_ALPHA of both backends := per_box [box][volume]; then (rebuild) rebuild_operator with the a, b of the tests."""
        for lv in (self.lh, self.lo):
            lv.write_all(H.VECTOR_ALPHA, per_box)
            if rebuild:
                lv.b.lib.rebuild_operator(lv.ptr, None, A, B)
        self.alpha_is = tag

    def uniform(self):
        if self.alpha_is != "uniform":
            self.set_alpha(np.full((self.lh.num_boxes, self.lh.volume), ALPHA), "uniform")

    def cell(self, k, j, i):
        g = self.lh.ghosts
        return (i + g) + (j + g) * self.lh.jStride + (k + g) * self.lh.kStride

    def count(self):
        return self.lib.hpgmg_uniform_alpha_launches()

    def destroy(self):
        for be, f, m in zip((self.hip, self.oracle), self.fine, self.mg):
            be.lib.hpgmg_mg_destroy(m); f.destroy()


def run_mode(P, lv, mode, a=A, b=B):
    """One smooth() of `mode` on a backend's fine level from the seeded start; what it leaves in the interior (the in-cycle forms promise nothing about VECTOR_TEMP)."""
    lib = lv.b.lib
    P.reset(lv)
    if lv is P.lo:
        if mode == "interp":
            lib.interpolation_vcycle(lv.ptr, U, 1.0, P.co.ptr, U)
        lib.smooth(lv.ptr, U, F, a, b)
    elif mode == "smooth":
        lib.smooth(lv.ptr, U, F, a, b)
    elif mode == "cycle":
        assert lib.hpgmg_smooth_in_cycle(lv.ptr, U, F, a, b) == 1
    else:
        assert lib.hpgmg_interp_smooth_fused(lv.ptr, U, F, P.ch.ptr, a, b) == 1
    return [lv.interior(v) for v in ((U, TEMP) if mode == "smooth" else (U,))]


def on_off_oracle(P, mode):
    lib = P.lib
    try:
        lib.hpgmg_set_uniform_alpha(1)
        n0 = P.count()
        on = run_mode(P, P.lh, mode)
        n1 = P.count()
        lib.hpgmg_set_uniform_alpha(0)
        off = run_mode(P, P.lh, mode)
        n2 = P.count()
    finally:
        lib.hpgmg_set_uniform_alpha(1)
    ref = run_mode(P, P.lo, mode)
    sha = hashlib.sha256(b"".join(x.tobytes() for x in on)).hexdigest()
    return {"on_is_off": same_bits(on, off), "on_is_oracle": same_bits(on, ref), "rise_on": n1 - n0, "rise_off": n2 - n1, "sha": sha}


def worker(names):
    hip, oracle = Backend.hip(), Backend.oracle()
    for name in names:
        P = TwoLevel(hip, oracle, GEOMS[name])
        try:
            for mode in MODES:
                print("CASE " + json.dumps(dict(on_off_oracle(P, mode), case=name + "-" + mode)), flush=True)
        finally:
            P.destroy()


_RUNS = {}


def run_with(nw, kc=0):
    """The worker with HPGMG_TUNE_PAIR_NW = nw; kc > 0: also HPGMG_TUNE_PAIR_KC = kc, on the one box of 128^3 only (every step a general step with kc = 1, segment
    bounds everywhere with 3)."""
    if (nw, kc) not in _RUNS:
        names = list(GEOMS) if kc == 0 else ["1x128"]
        env = dict(os.environ, HPGMG_TUNE_PAIR_NW=str(nw))
        if kc:
            env["HPGMG_TUNE_PAIR_KC"] = str(kc)
        out = subprocess.run([sys.executable, os.path.abspath(__file__)] + names, capture_output=True, text=True, timeout=900, env=env)
        assert out.returncode == 0, (out.stdout[-800:], out.stderr[-800:])
        rows = [json.loads(l[5:]) for l in out.stdout.splitlines() if l.startswith("CASE ")]
        _RUNS[(nw, kc)] = {r["case"]: r for r in rows}
        assert sorted(_RUNS[(nw, kc)]) == sorted(n + "-" + m for n in names for m in MODES)
    return _RUNS[(nw, kc)]


@pytest.mark.parametrize("nw", [10, 12, 16])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_smooth_takes_alpha_from_its_arguments(geom, mode, nw):
    """Both pairs of a smooth() (c1 = 0 and c1 != 0), x1 kept and not, the interpolation folded in: 10 and 12 waves run the UA twins (two launches), 16 waves have
    none; the switch off: nobody does.  All equal the oracle, and each other across wave counts."""
    r = run_with(nw)[geom + "-" + mode]
    print(geom, mode, nw, r)
    assert r["on_is_off"] and r["on_is_oracle"]
    assert r["rise_off"] == 0
    assert r["rise_on"] == (0 if nw == 16 else 2)
    assert r["sha"] == run_with(10)[geom + "-" + mode]["sha"]


@pytest.mark.parametrize("kc", [1, 3])
@pytest.mark.parametrize("mode", MODES)
def test_smooth_in_short_k_chunks(mode, kc):
    """Chunks of one plane (every step of the march a general step) and of three (a segment of one step wherever one fits) on one box of 128^3."""
    r = run_with(10, kc)["1x128-" + mode]
    print(mode, kc, r)
    assert r["on_is_off"] and r["on_is_oracle"]
    assert (r["rise_on"], r["rise_off"]) == (2, 0)
    assert r["sha"] == run_with(10)["1x128-" + mode]["sha"]


_kept = {}


@pytest.fixture
def two_level(hip, oracle):
    def get(name):
        if name not in _kept:
            _kept[name] = TwoLevel(hip, oracle, GEOMS[name])
        _kept[name].use()
        return _kept[name]
    return get


def switch_on_then_off(P, run):
    """run() with the switch on, then off: (result on, result off, rise on, rise off)."""
    try:
        P.lib.hpgmg_set_uniform_alpha(1)
        n0 = P.count(); on = run(); n1 = P.count()
        P.lib.hpgmg_set_uniform_alpha(0)
        off = run(); n2 = P.count()
    finally:
        P.lib.hpgmg_set_uniform_alpha(1)
    return on, off, n1 - n0, n2 - n1


@pytest.mark.parametrize("geom", ["1x128", "2x128"])
def test_residual_restriction_zero_vector(two_level, geom):
    """residual + restriction + zero_vector in one pass: the residual not stored (the call), and stored (the operator queue behind the reference's call order, after a
    smooth() in its in-cycle form: two UA pairs and the UA pass)."""
    P = two_level(geom)
    P.uniform()
    lh, lo, ch, co = P.lh, P.lo, P.ch, P.co
    junk = seeded_field(ch, 1301)

    def call():
        P.reset(lh)
        ch.write_all(U, junk); ch.write_all(R, junk)
        assert P.lib.hpgmg_residual_restrict_zero_fused(ch.ptr, R, lh.ptr, U, F, A, B, U) == 1
        return [ch.interior(R), ch.interior(U)]

    on, off, rise_on, rise_off = switch_on_then_off(P, call)
    P.reset(lo)
    co.write_all(U, junk); co.write_all(R, junk)
    lo.b.lib.residual(lo.ptr, TEMP, U, F, A, B)
    lo.b.lib.restriction(co.ptr, R, lo.ptr, TEMP, H.RESTRICT_CELL)
    lo.b.lib.zero_vector(co.ptr, U)
    assert same_bits(on, off) and same_bits(on, [co.interior(R), co.interior(U)])
    assert (rise_on, rise_off) == (1, 0)

    def queued(lv, c):
        lib = lv.b.lib
        P.reset(lv)
        c.write_all(U, junk); c.write_all(F, junk)
        lib.smooth(lv.ptr, U, F, A, B)
        lib.residual(lv.ptr, TEMP, U, F, A, B)
        lib.restriction(c.ptr, F, lv.ptr, TEMP, H.RESTRICT_CELL)      # (MGVCycle restricts into the vector it smooths against, mg.c:1152: what the queue recognises)
        lib.zero_vector(c.ptr, U)
        lib.hpgmg_operators_flush()
        return [lv.interior(U), lv.interior(TEMP), c.interior(F), c.interior(U)]

    on, off, rise_on, rise_off = switch_on_then_off(P, lambda: queued(lh, ch))
    assert same_bits(on, off) and same_bits(on, queued(lo, co))
    assert (rise_on, rise_off) == (3, 0)


def norm_places(geom):
    """{name: (box, k, j, i)}: the first and the last cell, either side of the 128-cell tile edge (boxes of 128: the box face in i) and of a 16-plane chunk edge."""
    nb, d = GEOMS[geom]
    last = nb ** 3 - 1
    out = {"first": (0, 0, 0, 0), "last": (last, d - 1, d - 1, d - 1), "k-15": (last // 2, 15, 50, 70), "k-16": (last // 2, 16, 50, 70)}
    if nb > 1:
        out.update({"i-127": (0, 100, 100, 127), "i-128": (1, 100, 100, 0)})
    return out


NORM_CASES = [(g, w) for g in ("1x128", "2x128") for w in norm_places(g)]


@pytest.mark.parametrize("geom,where", NORM_CASES)
def test_residual_norm_wherever_the_maximum_sits(two_level, geom, where):
    """residual + norm, stored and not: the data in [-1, 1] and one right-hand-side cell at 2^44 (the placement rule of DESIGN.md section 3)."""
    P = two_level(geom)
    P.uniform()
    lh, lo = P.lh, P.lo
    box, k, j, i = norm_places(geom)[where]
    value = 2.0 ** 44 if (len(where) % 2) else -(2.0 ** 44)
    f = P.start[F][box].copy()
    f[P.cell(k, j, i)] = value
    P.reset(lo)
    lo.write_raw(box, F, f)
    lo.b.lib.residual(lo.ptr, TEMP, U, F, A, B)
    want = lo.b.lib.norm(lo.ptr, TEMP)
    res = lo.interior(TEMP)
    assert want == np.abs(res).max() > 0.5 * 2.0 ** 44
    for stored in (True, False):
        def call():
            P.reset(lh)
            lh.write_raw(box, F, f)
            out = c_dbl(-1.0)
            assert P.lib.hpgmg_residual_norm_fused(lh.ptr, TEMP if stored else -1, U, F, A, B, ctypes.byref(out)) == 1
            return [np.array([out.value]), lh.interior(TEMP)]
        on, off, rise_on, rise_off = switch_on_then_off(P, call)
        assert same_bits(on, off)
        assert on[0][0] == want, (on[0][0], want, where, stored)
        if stored:
            assert np.array_equal(bits(on[1]), bits(res)), "the stored residual"
        assert (rise_on, rise_off) == (1, 0)


def smooth_and_norm(P, lv, a=A, b=B):
    """smooth() and residual + norm from the seeded start: the interior of the iterate and of VECTOR_TEMP after the smooth(), then the norm."""
    lib = lv.b.lib
    P.reset(lv)
    lib.smooth(lv.ptr, U, F, a, b)
    out = [lv.interior(U), lv.interior(TEMP)]
    if lv is P.lo:
        lib.residual(lv.ptr, TEMP, U, F, a, b)
        return out + [np.array([lib.norm(lv.ptr, TEMP)])]
    v = c_dbl(-1.0)
    assert lib.hpgmg_residual_norm_fused(lv.ptr, -1, U, F, a, b, ctypes.byref(v)) == 1
    return out + [np.array([v.value])]


ULP_PLACES = {"first-cell-of-box-0": (0, 0, 0, 0), "last-cell-of-the-last-box": (7, 127, 127, 127), "mid-row": (3, 60, 61, 77)}


@pytest.mark.parametrize("where", list(ULP_PLACES))
def test_one_cell_one_ulp_away_prevents_the_record(two_level, where):
    """alpha = 0.7 but for ONE interior cell one ulp away -- the cell the reference value is read from, the last one, one in mid-row: no launch takes alpha from its
    arguments, and the bits are the oracle's."""
    P = two_level("2x128")
    box, k, j, i = ULP_PLACES[where]
    alpha = np.full((P.lh.num_boxes, P.lh.volume), ALPHA)
    alpha[box, P.cell(k, j, i)] = np.nextafter(ALPHA, 1.0)
    P.set_alpha(alpha, where)
    n0 = P.count()
    got = smooth_and_norm(P, P.lh)
    assert P.count() == n0
    assert same_bits(got, smooth_and_norm(P, P.lo))


def test_ghost_cells_and_the_sign_of_zero(two_level):
    """A ghost cell of alpha with another value does not prevent the record (no 7-point kernel reads alpha there); -0.0 in one cell of an all-0.0 alpha does (the
    compare is of bits), and an all-0.0 alpha is a uniform one whose value is 0.0, not 0.7."""
    P = two_level("1x128")
    alpha = np.full((1, P.lh.volume), ALPHA)
    alpha[0, 0] = 0.9                                            # the ghost corner of the box, outside the domain: no exchange overwrites it
    alpha[0, P.cell(5, -1, 7)] = 0.9                             # a ghost cell next to the interior
    P.set_alpha(alpha, "ghosts")
    n0 = P.count()
    got = smooth_and_norm(P, P.lh)
    assert P.count() - n0 == 3
    assert same_bits(got, smooth_and_norm(P, P.lo))
    zero = np.zeros((1, P.lh.volume))
    P.set_alpha(zero, "zeros")
    n0 = P.count()
    got = smooth_and_norm(P, P.lh)
    assert P.count() - n0 == 3
    assert same_bits(got, smooth_and_norm(P, P.lo))
    zero[0, P.cell(64, 64, 64)] = -0.0
    P.set_alpha(zero, "minus-zero")
    n0 = P.count()
    got = smooth_and_norm(P, P.lh)
    assert P.count() == n0
    assert same_bits(got, smooth_and_norm(P, P.lo))


def test_the_record_lives_as_long_as_the_dinv_record(two_level):
    P = two_level("1x128")
    formed = P.lib.hpgmg_pair_formed_dinv_launches

    def check(rise, formed_rise, a=A, b=B):
        n0, f0 = P.count(), formed()
        got = smooth_and_norm(P, P.lh, a, b)
        assert (P.count() - n0, formed() - f0) == (rise, formed_rise)
        assert same_bits(got, smooth_and_norm(P, P.lo, a, b))

    P.set_alpha(np.full((1, P.lh.volume), ALPHA), "uniform")
    check(3, 2)                                                  # two pairs and the residual pass
    rough = np.abs(seeded_field(P.lh, 4242)) + 0.5
    P.set_alpha(rough, "rough", rebuild=False)                   # written, not rebuilt: both backends read the same stale Dinv, nobody forms it or assumes alpha
    check(0, 0)
    P.set_alpha(rough, "rough")                                  # rebuilt: Dinv is formed again, alpha is read
    check(0, 2)
    P.set_alpha(np.full((1, P.lh.volume), 0.9), "0.9")           # a cached 0.7 would fail here
    check(3, 2)
    check(1, 0, a=2.0)                                           # another a than the rebuild's: no FORM twin, hence no UA twin, in the pairs; the residual pass does not read Dinv
    check(3, 2)
    P.uniform()
    check(3, 2)


@pytest.mark.parametrize("size", ["7 8", "6 8"])
def test_the_whole_cycle_prints_the_same_lines(size):
    """hpgmg-fv --helmholtz: the analytic problem's alpha is 1.0 in every cell, so by default every fine-level pair and residual pass takes it from its arguments.
    Switch on and off print the same pinned lines, and the f-cycle norms are the reference's where they are recorded."""
    from test_gpu_parity_sweep import pinned_lines
    exe = os.path.join(ROOT, "hpgmg_amd", "bin", "hpgmg-fv")
    on = pinned_lines(exe, "--helmholtz", size, HPGMG_UNIFORM_ALPHA="1")
    off = pinned_lines(exe, "--helmholtz", size, HPGMG_UNIFORM_ALPHA="0")
    assert len(on) >= 10 and on == off
    gold = load_golden("fcycle_norms.json").get("7pt-cheby-helm " + size)
    assert gold or size != "7 8"
    if gold:
        printed = [re.search(r"norm=(\S+)", l).group(1) for l in on if "f-cycle" in l]
        assert [g for g in gold["norms"] if g in printed] == gold["norms"], (gold["norms"], printed[:6])


@pytest.mark.parametrize("alpha", [None, ALPHA])
def test_dense_array_solver(alpha):
    """The dense-array Solver with a != 0: left with the alpha = 1 it starts with (no coefficients given), and given alpha = 0.7 with seeded betas.  The F-cycle's solution
    is the same with the switch on and off and on the oracle, and with it on launches take alpha from their arguments."""
    from hpgmg_amd.problem import Solver
    from user_problem_lib import random_coefficients
    n = 128
    hip, oracle = declare(Backend.hip().lib), Backend.oracle().lib
    assert H.load_kernels().hpgmg_hip_set_device(0) == 0
    _, bi, bj, bk = random_coefficients(n, "dirichlet", True, seed=1281)
    f = np.random.default_rng(n).random((n, n, n)) - 0.3

    def fcycle(lib):
        lib.hpgmg_set_verbose(0)
        with Solver(n, box_dim=128, smoother="cheby", a=1.0, b=1.0, lib=lib) as s:
            if alpha is not None:
                s.set_coefficients(np.full((n, n, n), alpha), bi, bj, bk)
            u, info = s.solve(f, method="fmg", rtol=1.0)
        return u, info.residual

    try:
        hip.hpgmg_set_uniform_alpha(1)
        n0 = hip.hpgmg_uniform_alpha_launches()
        on = fcycle(hip)
        assert hip.hpgmg_uniform_alpha_launches() > n0
        hip.hpgmg_set_uniform_alpha(0)
        n1 = hip.hpgmg_uniform_alpha_launches()
        off = fcycle(hip)
        assert hip.hpgmg_uniform_alpha_launches() == n1
    finally:
        hip.hpgmg_set_uniform_alpha(1)
    ref = fcycle(oracle)
    assert on[0].tobytes() == off[0].tobytes() == ref[0].tobytes()
    assert on[1] == off[1] == ref[1]


if __name__ == "__main__":
    worker(sys.argv[1:])
