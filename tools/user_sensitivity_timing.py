#!/usr/bin/env python3
"""Times Solver.sensitivity's entry point (hpgmg_user_sensitivity of include/hpgmg_fv.h) at 256^3 Helmholtz in 2^3 boxes of 128^3,
Dirichlet walls with boundary values, device arrays (torch tensors, in place), three ways in ONE run, alternating them repeat by repeat:

    call    the whole hpgmg_user_sensitivity: two packs, g copied, two ghost exchanges, the pass
    pass    the pass alone (hpgmg_dense_unpack_sensitivity on the vectors the call has packed: one launch for the four arrays)
    torch   the same four arrays by plain slicing, differencing and multiplying on the dense tensors, temporaries and all: what a user writes today

hipEvent pairs: for the library on its launch stream around each call (every call synchronises before it returns, so the pair brackets all of its
device work), for torch on torch's stream around the expressions.  Prints one JSON line of medians in ms, the pass's rate against its minimum
traffic of 48 B per cell (u, lam in; four arrays out), and the largest difference between the library's and torch's arrays relative to the
largest entry (rounding: torch evaluates in another order).

    python tools/user_sensitivity_timing.py [--n 256] [--box 128] [--repeats 9]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import hpgmg_amd as H  # noqa: E402
from hpgmg_amd.problem import Solver  # noqa: E402


def by_slicing(u, lam, g, a, b, h):
    """(d_alpha, d_beta_i, d_beta_j, d_beta_k) of a Dirichlet box from the dense tensors: the table of DESIGN.md §11.9 written with torch slices."""
    n = u.shape[0]
    w2 = b / (h * h)
    out = [a * u * lam]
    for axis in range(3):
        ax = 2 - axis
        U, L = u.movedim(ax, 0), lam.movedim(ax, 0)
        shape = [n, n, n]
        shape[ax] += 1
        G = torch.empty(shape, dtype=u.dtype, device=u.device)
        V = G.movedim(ax, 0)
        V[1:n] = w2 * (U[:-1] - U[1:]) * (L[:-1] - L[1:])
        V[0] = 2.0 * w2 * (U[0] - g[2 * axis]) * L[0]
        V[n] = 2.0 * w2 * (U[n - 1] - g[2 * axis + 1]) * L[n - 1]
        out.append(G)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--box", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=9)
    args = ap.parse_args()
    n, a, b = args.n, 1.3, 0.7
    lib, K = H.load_driver(), H.load_kernels()
    lib.hpgmg_set_verbose(0)
    assert K.hpgmg_hip_set_device(torch.cuda.current_device()) == 0
    dev = torch.device("cuda", torch.cuda.current_device())
    e0, e1 = K.hpgmg_hip_event_create(), K.hpgmg_hip_event_create()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def library(fn):
        K.hpgmg_hip_event_record(e0)
        assert fn() == 0
        K.hpgmg_hip_event_record(e1)
        return K.hpgmg_hip_event_elapsed_ms(e0, e1)

    def on_torch(fn):
        torch.cuda.synchronize()
        t0.record()
        out = fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1), out

    gen = torch.Generator(device=dev).manual_seed(0)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device=dev, generator=gen)  # noqa: E731
    shapes = ((n, n, n + 1), (n, n + 1, n), (n + 1, n, n))
    alpha, betas = 1.0 + rand(n, n, n), [1.0 + rand(*s) for s in shapes]
    u, lam, g = rand(n, n, n) - 0.5, rand(n, n, n) - 0.5, rand(6, n, n) - 0.5
    out = [torch.empty((n, n, n), dtype=torch.float64, device=dev)] + [torch.empty(s, dtype=torch.float64, device=dev) for s in shapes]
    P = [q.data_ptr() for q in out]
    times = {"call": [], "pass": [], "torch": []}
    with Solver(n, box_dim=args.box, bc="dirichlet", smoother="cheby", a=a, b=b, lib=lib) as s:
        S, h = s._ptr, s.h
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
        x_id = lib.hpgmg_vectors_reserved()                    # the solver's operand vector; lam goes to VECTOR_R
        s.set_coefficients(alpha, *betas)
        torch.cuda.synchronize()
        for _ in range(args.repeats + 1):                      # the first round allocates (boundary arrays, validation word, torch's pool): not counted
            times["call"].append(library(lambda: lib.hpgmg_user_sensitivity(S, u.data_ptr(), lam.data_ptr(), g.data_ptr(), *P, H.WHERE_PLUGIN)))
            times["pass"].append(library(lambda: lib.hpgmg_dense_unpack_sensitivity(L, x_id, H.VECTOR_R, g.data_ptr(), a, b, 0, None, None, *P,
                                                                                    H.WHERE_PLUGIN)))
            ms, ref = on_torch(lambda: by_slicing(u, lam, g, a, b, h))
            times["torch"].append(ms)
        worst = max(float((q - r).abs().max() / r.abs().max()) for q, r in zip(out, ref))
    cells = float(n) ** 3
    res = {"n": n, "box": args.box, "repeats": args.repeats}
    for key, v in times.items():
        res[f"{key}_ms"] = statistics.median(v[1:])
    res["pass_min_bytes"] = 48.0 * cells
    res["pass_TBps"] = 48.0 * cells / (res["pass_ms"] * 1e-3) / 1e12
    res["call_over_torch"] = res["call_ms"] / res["torch_ms"]
    res["max_rel_difference_to_torch"] = worst
    K.hpgmg_hip_event_destroy(e0)
    K.hpgmg_hip_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
