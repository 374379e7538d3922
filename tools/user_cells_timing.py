#!/usr/bin/env python3
"""Times the cell-centred conductivity path (hpgmg_user_set_cell_coefficients, hpgmg_user_cell_sensitivity of include/hpgmg_fv.h)
against the face route it replaces, at 256^3 Helmholtz in 2^3 boxes of 128^3, Dirichlet walls with boundary values, device arrays (torch tensors, in
place), the alternatives interleaved repeat by repeat in ONE run:

    set_cells        hpgmg_user_set_cell_coefficients(alpha, k)
    set_faces        the face mean written in torch (three face arrays materialised) plus hpgmg_user_set_coefficients: the route before
    pack_cells       the pack hook alone: hpgmg_dense_pack_cell_mean, one launch for the three vectors
    pack_faces       the three existing packs of the three face arrays (hpgmg_dense_pack, FACE_I / J / K), the face arrays given
    sens_cells       hpgmg_user_cell_sensitivity(u, lam, k)
    sens_faces       hpgmg_user_sensitivity plus the gather of its three face arrays back to cells in torch
    pass_cells       the new pass alone: hpgmg_dense_unpack_cell_sensitivity on the vectors the call has packed
    pass_faces       the existing pass alone: hpgmg_dense_unpack_sensitivity

hipEvent pairs: for the library on its launch stream around each call (every call synchronises before it returns, so the pair brackets all of its
device work), for torch on torch's stream around the expressions; a route with both is the sum of the two.  Prints one JSON line of medians in ms,
the two new launches' rates against their minimum traffic (32 B per cell for the pack; 40 B for the pass: u, lam, k in, two out), and the largest
difference between d_k of the two routes relative to its largest entry (rounding: torch gathers in another order).

    python tools/user_cells_timing.py [--n 256] [--box 128] [--repeats 9] [--mean harmonic]
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


def face_mean(k, harmonic):
    """The three face arrays of a Dirichlet box from the cell tensor: a wall face takes its cell's value."""
    out = []
    for dim in (2, 1, 0):
        n = k.shape[dim]
        lo, hi = k.narrow(dim, 0, n - 1), k.narrow(dim, 1, n - 1)
        inner = (2.0 * (lo * hi)) / (lo + hi) if harmonic else 0.5 * (lo + hi)
        out.append(torch.cat([k.narrow(dim, 0, 1), inner, k.narrow(dim, n - 1, 1)], dim=dim).contiguous())
    return out


def gather(k, G, harmonic):
    """d_k from the three face arrays of sensitivities: each face's G times the derivative of its mean to the cell, 1 on a wall."""
    d = torch.zeros_like(k)
    for dim, Gf in zip((2, 1, 0), G):
        n = k.shape[dim]
        lo, hi = k.narrow(dim, 0, n - 1), k.narrow(dim, 1, n - 1)
        inner = Gf.narrow(dim, 1, n - 1)
        if harmonic:
            s = lo + hi
            d_lo, d_hi = 2.0 * (hi / s) ** 2, 2.0 * (lo / s) ** 2
        else:
            d_lo = d_hi = 0.5
        d.narrow(dim, 0, n - 1).add_(inner * d_lo)
        d.narrow(dim, 1, n - 1).add_(inner * d_hi)
        d.narrow(dim, 0, 1).add_(Gf.narrow(dim, 0, 1))
        d.narrow(dim, n - 1, 1).add_(Gf.narrow(dim, n, 1))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--box", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--mean", choices=("harmonic", "arithmetic"), default="harmonic")
    args = ap.parse_args()
    n, a, b = args.n, 1.3, 0.7
    harmonic = args.mean == "harmonic"
    mean = H.MEAN_HARMONIC if harmonic else H.MEAN_ARITHMETIC
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
    alpha, k = 1.0 + rand(n, n, n), 0.5 + rand(n, n, n)
    u, lam, g = rand(n, n, n) - 0.5, rand(n, n, n) - 0.5, rand(6, n, n) - 0.5
    d_alpha, d_k = torch.empty_like(k), torch.empty_like(k)
    G = [torch.empty(s, dtype=torch.float64, device=dev) for s in shapes]
    PG = [q.data_ptr() for q in G]
    betas = (H.VECTOR_BETA_I, H.VECTOR_BETA_J, H.VECTOR_BETA_K)
    layouts = (H.DENSE_FACE_I, H.DENSE_FACE_J, H.DENSE_FACE_K)
    keys = ("set_cells", "set_faces", "pack_cells", "pack_faces", "sens_cells", "sens_faces", "pass_cells", "pass_faces")
    times = {key: [] for key in keys}
    with Solver(n, box_dim=args.box, bc="dirichlet", smoother="cheby", a=a, b=b, lib=lib) as s:
        S = s._ptr
        L = lib.hpgmg_solver_level(lib.hpgmg_user_solver_of(S), 0)
        x_id = lib.hpgmg_vectors_reserved()                    # the solver's operand vector; lam goes to VECTOR_R
        W = H.WHERE_PLUGIN
        for _ in range(args.repeats + 1):                      # the first round allocates (boundary arrays, validation word, torch's pool): not counted
            times["set_cells"].append(library(lambda: lib.hpgmg_user_set_cell_coefficients(S, alpha.data_ptr(), k.data_ptr(), mean, None, W)))
            ms, F = on_torch(lambda: face_mean(k, harmonic))
            times["set_faces"].append(ms + library(lambda: lib.hpgmg_user_set_coefficients(S, alpha.data_ptr(), *[q.data_ptr() for q in F], W)))
            times["pack_cells"].append(library(lambda: lib.hpgmg_dense_pack_cell_mean(L, k.data_ptr(), W, mean, 0, None)))
            times["pack_faces"].append(sum(library(lambda v=v, q=q, lay=lay: lib.hpgmg_dense_pack(L, v, q.data_ptr(), W, lay, H.DENSE_CHECK_POSITIVE))
                                           for v, q, lay in zip(betas, F, layouts)))
            times["sens_cells"].append(library(lambda: lib.hpgmg_user_cell_sensitivity(S, u.data_ptr(), lam.data_ptr(), k.data_ptr(), mean, g.data_ptr(),
                                                                                       d_alpha.data_ptr(), d_k.data_ptr(), W)))
            lib_ms = library(lambda: lib.hpgmg_user_sensitivity(S, u.data_ptr(), lam.data_ptr(), g.data_ptr(), d_alpha.data_ptr(), *PG, W))
            ms, ref = on_torch(lambda: gather(k, G, harmonic))
            times["sens_faces"].append(lib_ms + ms)
            times["pass_cells"].append(library(lambda: lib.hpgmg_dense_unpack_cell_sensitivity(L, x_id, H.VECTOR_R, k.data_ptr(), mean, g.data_ptr(), a, b, 0,
                                                                                               None, None, d_alpha.data_ptr(), d_k.data_ptr(), W)))
            times["pass_faces"].append(library(lambda: lib.hpgmg_dense_unpack_sensitivity(L, x_id, H.VECTOR_R, g.data_ptr(), a, b, 0, None, None,
                                                                                          d_alpha.data_ptr(), *PG, W)))
        worst = float((d_k - ref).abs().max() / ref.abs().max())
    cells = float(n) ** 3
    res = {"n": n, "box": args.box, "repeats": args.repeats, "mean": args.mean}
    for key in keys:
        res[f"{key}_ms"] = statistics.median(times[key][1:])
    res["pack_cells_TBps"] = 32.0 * cells / (res["pack_cells_ms"] * 1e-3) / 1e12
    res["pack_faces_TBps"] = 48.0 * cells / (res["pack_faces_ms"] * 1e-3) / 1e12
    res["pass_cells_TBps"] = 40.0 * cells / (res["pass_cells_ms"] * 1e-3) / 1e12
    res["pass_faces_TBps"] = 48.0 * cells / (res["pass_faces_ms"] * 1e-3) / 1e12
    res["max_rel_difference_of_d_k"] = worst
    K.hpgmg_hip_event_destroy(e0)
    K.hpgmg_hip_event_destroy(e1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
