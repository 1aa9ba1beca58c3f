"""tests/atm_numpy.py, the restatement that the GPU tests of pigs_atm_* compare with, pinned on the CPU: to a literal triple
loop over i < j < k written from the definition in include/pigs_hip.h, to triangles whose term is known in closed form, to
the triangle count of the radius graph, to permutation invariance, and to the triplet whose nearest images do not close."""
import itertools
import math

import numpy as np
import pytest

from atm_numpy import Window, pair_r2, slice_sums, terms


def _r2_literal(xa, xb, Lbox):
    r2 = 0.0
    for k in range(len(xa)):
        v = float(xa[k]) - float(xb[k])
        if v > 0.5 * Lbox[k]:
            v = v - Lbox[k]
        if v < -0.5 * Lbox[k]:
            v = v + Lbox[k]
        r2 = r2 + v * v
    return r2


def _literal(X, Lbox, rc2):
    """The definition, one scalar operation at a time: (T, Sum|t|, ntrip, the terms)."""
    Np = X.shape[0]
    T, A, n, ts = 0.0, 0.0, 0, []
    for i in range(Np):
        for j in range(i + 1, Np):
            a2 = _r2_literal(X[i], X[j], Lbox)
            for k in range(j + 1, Np):
                b2 = _r2_literal(X[i], X[k], Lbox)
                c2 = _r2_literal(X[j], X[k], Lbox)
                if not (a2 <= rc2 and b2 <= rc2 and c2 <= rc2):
                    continue
                p = (a2 * b2) * c2
                s = math.sqrt(p)
                num = ((a2 + b2 - c2) * (a2 + c2 - b2)) * (b2 + c2 - a2)
                den = (p * p) * s
                top = p + 0.375 * num
                t = top / den if den != 0.0 else (math.nan if top == 0.0 or top != top else math.copysign(math.inf, top))
                T += t
                A += abs(t)
                n += 1
                ts.append(t)
    return T, A, n, ts


def _put(points, dim):
    X = np.zeros((len(points), dim))
    X[:, :2] = points
    return X


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("Np", [3, 4, 5, 9])
def test_restatement_is_the_literal_triple_loop(dim, Np):
    rng = np.random.default_rng(10 * dim + Np)
    L = [3.0, 4.0, 3.5][:dim]
    for trial in range(3):
        X = rng.uniform(-0.5, 0.5, (Np, dim)) * np.asarray(L)
        if trial == 1:
            X[Np - 1, 0] = np.nan                                         # drops every triplet of that particle
        for rc in (0.5 * min(L), 0.3 * min(L)):
            T, A, n = slice_sums(X, L, rc * rc)
            lT, lA, ln, ts = _literal(X, L, rc * rc)
            assert n == ln and np.isfinite(lT)
            # the same terms in another order: at most 84 of them, each partial sum within an ulp of Sum|t|
            assert abs(T - lT) <= 1e-13 * lA and abs(A - lA) <= 1e-13 * lA, (trial, rc)
            if n == 1:
                assert T == lT == ts[0]                                   # one term: its bits
    # every term of the vectorised form has the literal term's bits
    X = rng.uniform(-0.5, 0.5, (Np, dim)) * np.asarray(L)
    r2 = pair_r2(X, L)
    got = sorted(float(terms(r2[i, j], r2[i, k], r2[j, k])) for i, j, k in itertools.combinations(range(Np), 3))
    assert got == sorted(_literal(X, L, np.inf)[3])


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("r", [0.75, 1.0, 1.3])
def test_equilateral_and_collinear_triangles(dim, r):
    """Equilateral, side r: the three cosines are 1/2, t = (1 + 3/8)/r^9 = 11/(8 r^9).  Collinear, sides r, r, 2r: the
    cosines are 1, 1, -1, t = (1 - 3)/(r r 2r)^3 = -2/(8 r^9) = -1/(4 r^9)."""
    L = [20.0] * dim
    h = r * math.sqrt(3.0) / 2.0
    T, A, n = slice_sums(_put([(0.0, 0.0), (r, 0.0), (0.5 * r, h)], dim), L, 9.0)
    assert n == 1 and abs(T - 11.0 / (8.0 * r ** 9)) <= 1e-13 * abs(T) and A == abs(T)
    T, A, n = slice_sums(_put([(-r, 0.0), (0.0, 0.0), (r, 0.0)], dim), L, 9.0)
    assert n == 1 and abs(T + 1.0 / (4.0 * r ** 9)) <= 1e-13 * abs(T) and A == abs(T)
    # with the cutoff below the long side the collinear triplet is gone, whichever pair is the long one
    for order in itertools.permutations([(-r, 0.0), (0.0, 0.0), (r, 0.0)]):
        assert slice_sums(_put(list(order), dim), L, (1.5 * r) ** 2)[2] == 0


@pytest.mark.parametrize("dim,Np", [(2, 24), (3, 40)])
def test_ntrip_counts_the_triangles_of_the_radius_graph(dim, Np):
    rng = np.random.default_rng(5 + dim)
    L = [3.0, 4.0, 5.0][:dim]
    X = rng.uniform(-0.5, 0.5, (Np, dim)) * np.asarray(L)
    for rc in (0.5 * min(L), 0.3 * min(L)):
        adj = (pair_r2(X, L) <= rc * rc).astype(np.int64)
        np.fill_diagonal(adj, 0)
        triangles = int(np.trace(adj @ adj @ adj)) // 6
        assert slice_sums(X, L, rc * rc)[2] == triangles > 0


@pytest.mark.parametrize("dim,Np", [(2, 17), (3, 30)])
def test_permuting_the_particles_changes_only_the_order_of_the_sum(dim, Np):
    """A permutation renames a2, b2, c2 within a term, which is symmetric in them up to rounding (a few ulps of the
    term), and reorders the sum: |dT| <= 1e-12 Sum|t|, the bound the GPU tests use; the count is equal."""
    rng = np.random.default_rng(21 + dim)
    L = [3.0, 4.0, 5.0][:dim]
    X = rng.uniform(-0.5, 0.5, (Np, dim)) * np.asarray(L)
    rc2 = (0.5 * min(L)) ** 2
    T, A, n = slice_sums(X, L, rc2)
    for _ in range(3):
        Tp, Ap, npm = slice_sums(X[rng.permutation(Np)], L, rc2)
        assert npm == n > 0 and abs(Tp - T) <= 1e-12 * A and abs(Ap - A) <= 1e-12 * A


@pytest.mark.parametrize("dim", [2, 3])
def test_triplet_whose_nearest_images_do_not_close(dim):
    """Three particles on the x axis of a cubic box of side L at 0, 0.4 L and 0.8 L, rc = L/2: the nearest-image sides are
    0.4 L, 0.2 L (0 and 0.8 L, round the box) and 0.4 L, an isosceles triangle, not the collinear 0.4, 0.8, 0.4."""
    Lx = 5.0
    L = [Lx] * dim
    X = _put([(0.0, 0.0), (0.4 * Lx, 0.0), (0.8 * Lx, 0.0)], dim) - 0.4 * Lx       # (inside the box: -0.4 L, 0, 0.4 L)
    r2 = pair_r2(X, L)
    assert np.allclose(np.sqrt([r2[0, 1], r2[0, 2], r2[1, 2]]), [0.4 * Lx, 0.2 * Lx, 0.4 * Lx], rtol=1e-14)
    T, A, n = slice_sums(X, L, (0.5 * Lx) ** 2)
    a, b = 0.4 * Lx, 0.2 * Lx
    cos_apex = (2 * a * a - b * b) / (2 * a * a)                          # between the two sides a
    cos_base = b / (2 * a)
    want = (1.0 + 3.0 * cos_apex * cos_base * cos_base) / (a * a * b) ** 3
    collinear = (1.0 - 3.0) / (a * (2 * a) * a) ** 3
    assert n == 1 and abs(T - want) <= 1e-13 * abs(want) and want > 0 > collinear


def test_window_adds_walkers_as_listed():
    rng = np.random.default_rng(3)
    L = [3.0, 3.0, 3.0]
    Nb, window, W, Np = 2, 1, 2, 6
    P = rng.uniform(-0.5, 0.5, (W, 2 * Nb + 1, Np, 3)) * 3.0
    win = Window(P, Nb, window, L)
    e = win.expected([1, 0, 1], 1.5)
    assert e["samples"].tolist() == [1, 2] and e["T"].shape == (W, 3)
    for js in range(3):
        T, A, n = slice_sums(P[1, Nb - window + js], L, 2.25)
        assert e["T"][1, js] == 2.0 * T and e["abs"][1, js] == 2.0 * A and e["ntrip"][1, js] == 2 * n
