"""tests/nk_numpy.py, the restatement that the GPU tests of pigs_nk_* compare with, and profiles.normalize_nk /
normalize_nrvec, pinned on the CPU: to a lattice of samples whose sums are known in closed form, to the reference's
NormalizeNr of the same samples' radial histogram (the oracle's OBDM), and to the sum rule sum_k n(k) = Np rho1(0)/density."""
import math

import numpy as np
import pytest

from nk_numpy import cos_sums, fold, grid_counts, half_space, inside_count, sums
from pathintegralgroundstate_amd.profiles import normalize_nk, normalize_nrvec, shell_average

BOX = {2: [3.0, 4.5], 3: [3.0, 4.5, 3.75]}


def _lattice(dim, M, L):
    j = np.stack(np.meshgrid(*([np.arange(M)] * dim), indexing="ij"), -1).reshape(-1, dim)
    x = np.zeros((M ** dim, 2, dim))
    x[:, 0] = j * np.asarray(L[:dim]) / M
    return x


@pytest.mark.parametrize("dim", [2, 3])
def test_lattice_of_samples_sums_to_zero_off_k_zero(dim):
    M, nmax = 4, 3
    L = BOX[dim]
    s = sums(_lattice(dim, M, L), L, nmax, M, (0.5 * min(L)) ** 2)
    assert s["nopen"] == M ** dim                            # C(0): the sum of cos(0) over the samples
    assert s["C"].shape == (((2 * nmax + 1) ** dim - 1) // 2,)
    assert np.abs(s["C"]).max() <= 1e-12 * M ** dim
    # one sample per bin of the M^dim grid of the minimum-image cell, except the points on the cell's open upper faces
    # (x_k = +L_k/2 is not folded and lies outside [-L/2, L/2)): j_k = 2 on some axis
    assert s["H"].shape == (M,) * dim and s["H"].max() == 1 and s["H"].sum() == 3 ** dim


def test_enumeration_is_the_half_space_in_lexicographic_order():
    n = half_space(3, 1)
    assert n[:5].tolist() == [[0, 0, 1], [0, 1, -1], [0, 1, 0], [0, 1, 1], [1, -1, -1]] and n[-1].tolist() == [1, 1, 1]
    assert len(half_space(2, 3)) == 24 and half_space(1, 4).ravel().tolist() == [1, 2, 3, 4]


def test_fold_is_one_compare_per_side():
    L = [3.0, 4.5]
    xe = np.array([[[1.5, 0.0], [0.0, 0.0]], [[np.nextafter(1.5, 2), 0.0], [0.0, 0.0]], [[-1.5, 2.25], [0.0, 0.0]],
                   [[0.2, np.nextafter(-2.25, -3)], [0.0, 0.0]], [[0.7, 0.7], [0.7, 0.7]]])
    v = fold(xe, L)
    assert v[0].tolist() == [1.5, 0.0] and v[1, 0] == np.nextafter(1.5, 2) - 3.0 and v[2].tolist() == [-1.5, 2.25]
    assert v[3, 1] == np.nextafter(-2.25, -3) + 4.5 and v[4].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("dim", [2, 3])
def test_radial_rebinning_is_the_reference_s_normalised_histogram(oracle, dim):
    """The samples inside rcut, re-binned radially and divided as normalize_nk divides, over the ideal shell count: the
    reference's NormalizeNr (sample_mod.f90:706-732) of the OBDM histogram (m = 0) of the same samples."""
    from oracle.pyoracle import System
    Np, Nbin, cworm, nobdm, zconf = 16, 20, 0.5, 4, 37.0
    S = System(dim=dim, Np=Np, Nb=2, density=0.3, Nbin=Nbin, Npw=0, CWorm=cworm)
    L = np.asarray(S.Lbox[:dim], np.float64)
    rbin = S.rbin
    rng = np.random.default_rng(dim)
    xend = rng.uniform(-0.5, 0.5, (300, 2, dim)) * L
    nrho = np.zeros((Nbin, 1))
    for p in xend:
        nrho += oracle.obdm(S, p)
    x = fold(xend, L)
    r = np.sqrt((x * x).sum(axis=1))
    inside = x[(x * x).sum(axis=1) <= S.rcut2]
    assert 0 < len(inside) < len(x) and len(inside) == inside_count(x, S.rcut2) == nrho.sum()
    radial = np.bincount((r[(x * x).sum(axis=1) <= S.rcut2] / rbin).astype(int), minlength=Nbin)[:Nbin]
    assert np.array_equal(radial, nrho[:, 0])
    got = normalize_nk({"C": radial.astype(np.float64), "nopen": len(x)}, cworm, zconf, nobdm, Np)["nk"]
    k_n = math.pi ** (0.5 * dim) / math.gamma(0.5 * dim + 1.0)
    want = np.zeros(Nbin)
    for ibin in range(1, Nbin + 1):                          # NormalizeNr, line by line
        rr = (float(ibin) - 0.5) * rbin
        nid = S.density * k_n * ((rr + 0.5 * rbin) ** dim - (rr - 0.5 * rbin) ** dim)
        want[ibin - 1] = nrho[ibin - 1, 0] / (cworm * nid * zconf * float(nobdm))
        got[ibin - 1] = got[ibin - 1] / nid
    assert np.allclose(got, want, rtol=1e-15, atol=0)


@pytest.mark.parametrize("dim", [2, 3])
def test_sum_rule_over_a_full_period(dim):
    """Samples on the M-point lattice x = j L/M with arbitrary weights (multiplicities); vectors over a full period of the
    lattice, n_k = -M/2 .. M/2 - 1 (n_k = +-M/2 alias, so +M/2 of the stored grid is left out).  The sum over all those k
    of n(k), the stored half space counted for +k and -k, is M^dim times the weight at x = 0 over the divisor: with the
    lattice as the quadrature of the cell this is Np * rho1(0)/density."""
    M, L, Np = 4, BOX[dim], 16
    cworm, nobdm, zconf = 0.5, 3, 11.0
    rng = np.random.default_rng(40 + dim)
    mult = rng.integers(0, 4, M ** dim)
    mult[0] = 5                                              # the weight at x = 0
    xend = np.repeat(_lattice(dim, M, L), mult, axis=0)
    nmax = M // 2
    n = half_space(dim, nmax)
    s = sums(xend, L, nmax, M, (0.5 * min(L)) ** 2)
    out = normalize_nk(s, cworm, zconf, nobdm, Np, n=n, Lbox=L)
    # a stored vector stands for +k and -k; of the two, those with every component in -M/2 .. M/2 - 1 are in the period
    wgt = np.all(n < nmax, axis=1).astype(np.float64) + np.all(n > -nmax, axis=1).astype(np.float64)
    total = out["nk0"] + float((out["nk"] * wgt).sum())
    den = cworm * zconf * nobdm
    assert abs(total - M ** dim * mult[0] / den) <= 1e-12 * len(xend) * (2 * nmax + 1) ** dim / den
    assert out["n0"] == out["nk0"] / Np and out["nk0"] == len(xend) / den
    # the shells are shell_average's
    k, mean, m = shell_average(n, L, out["nk"])
    assert np.array_equal(out["k"], k) and np.array_equal(out["nk_shell"], mean) and np.array_equal(out["mult"], m)
    # and rho1/density at the origin's bin in normalize_nrvec's normalisation
    rho = normalize_nrvec(s, cworm, zconf, nobdm, Np / float(np.prod(L)), L, dim)
    b = np.asarray(L[:dim]) / M
    centre = (M // 2,) * dim                                 # the bin [0, b): x = 0 sits on its lower edge
    assert rho["rho1"].shape == (M,) * dim
    assert rho["rho1"][centre] == mult[0] / (den * (Np / float(np.prod(L))) * float(np.prod(b)))
    assert np.allclose(rho["x"][0], -0.5 * L[0] + (np.arange(M) + 0.5) * b[0], rtol=0, atol=0)


def test_normalize_nk_broadcasts_over_walkers():
    C = np.arange(12.0).reshape(3, 4)
    out = normalize_nk({"C": C, "nopen": np.array([4, 0, 8])}, 0.5, np.array([2.0, 0.0, 4.0]), 2, 10)
    assert np.array_equal(out["nk"][0], C[0] / 2.0) and not np.isfinite(out["nk"][1]).any() and np.isnan(out["n0"][1])
    assert out["nk0"][2] == 2.0 and out["n0"][2] == 0.2
