"""Writes tests/golden/window_bits.npz, the fixture of tests/test_gpu_window_bits.py: the worldlines, and the arrays that
atm_read() and bop_read() return for them on the MI355X.  Run by hand, on a commit whose kernels are trusted, and never by
a test:

  python tests/golden/make_window_bits.py [--out tests/golden/window_bits.npz]

The shapes, the walker list and the calls are those of the test module (imported from it).  The worldlines are the
jittered lattices of tau_numpy.lattice_paths, five slices of three walkers per (dim, Np); up to six particles they are
drawn together to half the spacing, so that every pair lies within half the box.  Nothing is written unless
  * no pair of any slice comes near coincidence,
  * the sizes do what they are there for (one triplet at Np = 3, every triplet at 5 and 6, a vertex with more than 64 legs
    at 131, bonds at every bop size), and
  * every recorded array agrees with atm_numpy / bop_numpy at the tolerances of test_gpu_atm.py and test_gpu_bop.py (their
    own comparison functions): a wrong build cannot be pinned."""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                            # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))           # the repository

import atm_numpy  # noqa: E402
import bop_numpy  # noqa: E402
import test_gpu_atm  # noqa: E402
import test_gpu_bop  # noqa: E402
import test_gpu_window_bits as wb  # noqa: E402
from pathintegralgroundstate_amd import SystemConfig, api  # noqa: E402
from tau_numpy import lattice_paths, min_max_distance  # noqa: E402


def inputs():
    """The boxes, the worldlines and the neighbour radii."""
    fix = {}
    for dim in (2, 3):
        for Np in sorted(set(wb.ATM_NP) | set(wb.BOP_NP)):
            cfg = SystemConfig(dim=dim, Np=Np, Nb=2, density=wb.DENSITY[dim])
            scale = 0.5 if Np <= 6 else 1.0
            P = lattice_paths(cfg, 3, np.random.default_rng(100000 * dim + Np)) * scale
            n = int(np.ceil(Np ** (1.0 / dim) - 1e-9))
            lo, hi = min_max_distance(P, cfg)
            assert lo > 0.6 * scale * cfg.Lbox[0] / n, (dim, Np, lo)        # no pair comes near coincidence
            assert Np > 6 or hi < cfg.rcut, (dim, Np, hi)
            fix[f"box_d{dim}_n{Np}"] = np.float64(cfg.Lbox[0])
            fix[f"paths_d{dim}_n{Np}"] = P
            if Np in wb.BOP_NP:                                             # as test_gpu_bop.py draws its `shell` radius
                fix[f"rnb_d{dim}_n{Np}"] = np.float64(min(test_gpu_bop._radius(dim, cfg.density, 12 if dim == 3 else 6), cfg.rcut))
    return fix


def verify(fix):
    """The recorded arrays against the numpy restatements, and what the sizes are there for."""
    for dim in (2, 3):
        for Nb, window in wb.WINDOWS:
            for Np in wb.ATM_NP:
                cfg, P = wb.config(fix, dim, Np, Nb), wb.worldlines(fix, dim, Np, Nb)
                exp = atm_numpy.Window(P, Nb, window, cfg.Lbox).expected(wb.ORDER, cfg.rcut)
                pre = f"atm_d{dim}_n{Np}_b{Nb}_"
                test_gpu_atm._assert_same({k: fix[pre + k] for k in ("T", "ntrip", "samples")}, exp, pre)
                if Np <= 6:
                    assert np.all(exp["ntrip"] == Np * (Np - 1) * (Np - 2) // 6), pre
                if Np == 131:
                    legs = atm_numpy.pair_r2(P[0, Nb], cfg.Lbox)[0, 1:] <= cfg.rcut2
                    assert legs.sum() > 64, (pre, int(legs.sum()))
            for Np in wb.BOP_NP:
                cfg, P = wb.config(fix, dim, Np, Nb), wb.worldlines(fix, dim, Np, Nb)
                win = bop_numpy.Window(P, cfg.Lbox, cfg.rcut2, float(fix[f"rnb_d{dim}_n{Np}"]))
                for Nr in wb.BOP_NR:
                    exp = win.expected(wb.ORDER, Nb, window, Nr, cfg.rcut / Nr if Nr else 0.0)
                    pre = f"bop_d{dim}_n{Np}_b{Nb}_r{Nr}_"
                    test_gpu_bop._check({k: fix[pre + k] for k in ("S", "H", "G", "GN", "samples")}, exp, Np, wb.NH, window, pre)
                    assert np.all(exp["S"][:, 6] > 0) and (Nr == 0 or np.all(exp["GN"].sum(axis=1) > 0)), pre


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "window_bits.npz"))
    a = ap.parse_args()
    api.load_library()
    assert api.device_count() >= 1, "needs a GPU"
    fix = inputs()
    for dim in (2, 3):
        for Nb, window in wb.WINDOWS:
            for Np in wb.ATM_NP:
                fix.update(wb.atm_arrays(api, fix, dim, Np, Nb, window))
            for Np in wb.BOP_NP:
                fix.update(wb.bop_arrays(api, fix, dim, Np, Nb, window))
    verify(fix)
    np.savez_compressed(a.out, **fix)
    print(f"{a.out}: {len(fix)} arrays, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
