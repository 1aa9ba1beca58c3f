"""tests/g3_numpy.py, the restatement that the GPU tests of pigs_g3_* compare with, pinned on the CPU: to a literal triple
loop over (i, j, k) written from the definition in include/pigs_hip.h, to the counting identities, to grv_numpy's radial
counts, and to configurations whose angle bin is known in closed form."""
import math

import numpy as np
import pytest

import g3_numpy
from g3_numpy import Window, packed_index, slice_counts
from grv_numpy import Window as GrvWindow


def _literal(X, Lbox, Nr, rbin, Na):
    """The definition, one scalar operation at a time."""
    Np, dim = X.shape
    P = Nr * (Nr + 1) // 2
    trip = np.zeros((P, Na), np.int64)
    pair = np.zeros(Nr, np.int64)
    nleg = np.zeros(Np, np.int64)
    for i in range(Np):
        leg = []
        for j in range(Np):
            if j == i:
                continue
            d, r2 = [], 0.0
            for k in range(dim):
                v = float(X[i, k]) - float(X[j, k])
                if v > 0.5 * Lbox[k]:
                    v = v - Lbox[k]
                if v < -0.5 * Lbox[k]:
                    v = v + Lbox[k]
                d.append(v)
                r2 = r2 + v * v
            if not (0.0 < r2):
                continue
            s = math.sqrt(r2) if r2 != math.inf else math.inf
            u = s / rbin
            if not (u < Nr):
                continue
            leg.append((d, s, int(u)))
            pair[int(u)] += 1
        nleg[i] = len(leg)
        for a in range(len(leg)):
            for b in range(a + 1, len(leg)):
                (dj, sj, bj), (dk, sk, bk) = leg[a], leg[b]
                dot = dj[0] * dk[0]
                for e in range(1, dim):
                    dot = dot + dj[e] * dk[e]
                den = sj * sk
                c = dot / den if den != 0.0 else (math.nan if dot == 0.0 else math.copysign(math.inf, dot))
                v = (c + 1.0) * (0.5 * Na)
                if v != v:
                    continue
                q = 0 if v < 0 else (Na - 1 if v >= Na else min(int(v), Na - 1))
                lo, hi = min(bj, bk), max(bj, bk)
                trip[lo * Nr - lo * (lo - 1) // 2 + (hi - lo), q] += 1
    return trip, pair, nleg


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("Np", [2, 3, 5, 7])
def test_restatement_is_the_literal_triple_loop(dim, Np):
    rng = np.random.default_rng(10 * dim + Np)
    L = [3.0, 4.0, 3.5][:dim]
    for trial in range(4):
        X = rng.uniform(-0.5, 0.5, (Np, dim)) * np.asarray(L)
        if trial == 1 and Np > 2:
            X[1] = X[0]                                                   # a coincident pair
        if trial == 2:
            X[Np - 1, 0] = np.nan
        if trial == 3:
            X[0, dim - 1] = np.inf
        for Nr, rbin, Na in ((3, 0.5, 4), (6, 0.25, 5), (1, 1.5, 1)):
            t, p, n = slice_counts(X, L, Nr, rbin, Na)
            lt, lp, ln = _literal(X, L, Nr, rbin, Na)
            assert np.array_equal(t, lt) and np.array_equal(p, lp) and np.array_equal(n, ln), (trial, Nr, Na)


@pytest.mark.parametrize("dim,Np", [(2, 20), (3, 33)])
def test_counting_identities_and_the_radial_counts_of_grv_numpy(dim, Np):
    rng = np.random.default_rng(7 + dim)
    L = [3.0, 4.0, 5.0][:dim]
    rcut = 0.5 * min(L)
    Nb, window, W, Nr, Na = 3, 2, 2, 11, 6
    rbin = rcut / Nr
    P = rng.uniform(-0.5, 0.5, (W, 2 * Nb + 1, Np, dim)) * np.asarray(L)
    win = Window(P, Nb, window, L)
    exp = win.expected([1, 0, 1], Nr, rbin, Na)
    assert exp["samples"].tolist() == [1, 2]
    for w, times in ((0, 1), (1, 2)):
        n = np.concatenate([slice_counts(P[w, a], L, Nr, rbin, Na)[2] for a in range(Nb - window, Nb + window + 1)])
        assert exp["trip"][w].sum() == times * (n * (n - 1) // 2).sum() > 0
        assert exp["pair"][w].sum() == times * n.sum()
    # no two particles coincide and rmax = rcut: the ordered pairs are twice grv_numpy's pairs, bin for bin
    _, R, cnt, _ = GrvWindow(P, Nb, window, L, rcut * rcut).expected([1, 0, 1], 2, Nr, rbin)
    assert R.sum() > 0 and np.array_equal(exp["pair"], 2 * R) and np.array_equal(exp["samples"], cnt)


@pytest.mark.parametrize("dim", [2, 3])
def test_collinear_and_equilateral_triplets_land_in_their_bins(dim):
    L = [10.0] * dim
    Nr, rbin = 4, 1.0

    def put(points):
        X = np.zeros((len(points), dim))
        X[:, :2] = points
        return X
    for Na in (1, 4, 7, 10):
        # three collinear particles a unit apart: from an end cos = +1 (bin Na-1), from the middle cos = -1 (bin 0)
        t, p, n = slice_counts(put([(0.0, 0.0), (1.0, 0.0), (2.0, 0.0)]), L, Nr, rbin, Na)
        assert n.tolist() == [2, 2, 2] and t.sum() == 3
        assert t[packed_index(1, 2, Nr), Na - 1] == 2 and t[packed_index(1, 1, Nr), 0] == 1
        # along a diagonal, where c = dot/(s s) is rounded: still an end bin
        t, _, _ = slice_counts(put([(0.1, 0.3), (0.8, 1.0), (1.5, 1.7)]), L, Nr, rbin, Na)
        assert t.sum() == 3 and (Na == 1 or (t[:, 0].sum() == 1 and t[:, Na - 1].sum() == 2))
        # an equilateral triangle of side 1.5: every vertex sees cos = 1/2, leg bins (1, 1)
        h = 1.5 * math.sqrt(3.0) / 2.0
        t, _, _ = slice_counts(put([(0.0, 0.0), (1.5, 0.0), (0.75, h)]), L, Nr, rbin, Na)
        q = min(int((0.5 + 1.0) * (0.5 * Na)), Na - 1)
        near_edge = abs((0.5 + 1.0) * (0.5 * Na) - round((0.5 + 1.0) * (0.5 * Na))) < 1e-9
        if not near_edge:                                               # (Na = 4: c = 1/2 sits on an edge; rounding decides)
            assert t.sum() == 3 and t[packed_index(1, 1, Nr), q] == 3, Na
        else:
            assert t.sum() == 3 and t[packed_index(1, 1, Nr), q - 1:q + 1].sum() == 3, Na


def test_packed_index_walks_the_upper_triangle_row_by_row():
    for Nr in (1, 2, 5, 9):
        lo, hi = np.triu_indices(Nr)
        assert np.array_equal(packed_index(lo, hi, Nr), np.arange(Nr * (Nr + 1) // 2))
        assert g3_numpy.n_leg_pairs(Nr) == len(lo)
