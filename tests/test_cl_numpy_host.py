"""tests/cl_numpy.py, the yardstick of the cluster family, against literal cases and closed forms (no GPU): a literal flood
fill written from the definition, lattices below and above their spacing, the radius of gyration of a straight chain, and
the identities of the integer sums."""
import numpy as np
import pytest

import cl_numpy as cn
from pathintegralgroundstate_amd.profiles import normalize_cl


def _flood(bond):
    """Components by a literal flood fill, labelled by their smallest index."""
    n = bond.shape[0]
    label = -np.ones(n, np.int64)
    for i in range(n):
        if label[i] >= 0:
            continue
        todo, label[i] = [i], i
        while todo:
            a = todo.pop()
            for b in np.nonzero(bond[a] | bond[:, a])[0]:
                if label[b] < 0:
                    label[b] = i
                    todo.append(int(b))
    return label


def _lattice(dim, n, a):
    g = np.stack(np.meshgrid(*[np.arange(n)] * dim, indexing="ij"), axis=-1).reshape(-1, dim)
    return (g - 0.5 * n) * a + 0.25 * a


@pytest.mark.parametrize("dim", [2, 3])
def test_lattice_below_and_above_its_spacing(dim):
    a, n = 1.25, 4
    X = _lattice(dim, n, a)
    L = [n * a] * dim
    Np = n ** dim
    nsize, smax, nbond, G, label = cn.slice_sums(X, L, 0.99 * a)
    assert nsize.tolist() == [Np] + [0] * (Np - 1) and smax == 1 and nbond == 0 and not np.any(G)
    assert label.tolist() == list(range(Np))
    nsize, smax, nbond, G, label = cn.slice_sums(X, L, 1.01 * a)
    assert nsize.tolist() == [0] * (Np - 1) + [1] and smax == Np and not np.any(label)
    assert nbond == dim * Np                                            # every site bonds its 2 dim neighbours through the faces
    assert np.count_nonzero(G) == 1 and G[Np - 1] > 0


@pytest.mark.parametrize("s", [2, 3, 7, 40])
@pytest.mark.parametrize("order", ["ascending", "shuffled", "ends"])
def test_straight_chain_has_the_closed_form(s, order):
    """Rg^2 of s points at spacing a on a line: a^2 (s^2 - 1) / 12 (dyadic a: every term is exact)."""
    a = 0.125
    idx = {"ascending": np.arange(s), "shuffled": np.random.default_rng(s).permutation(s), "ends": cn.order_both_ends(s)}[order]
    assert sorted(idx.tolist()) == list(range(s))
    X = cn.chain(s, a, idx, dim=3, origin=[-3.0, 0.5, 0.25])
    nsize, smax, nbond, G, label = cn.slice_sums(X, [16.0, 8.0, 8.0], 1.5 * a)
    assert smax == s and nbond == s - 1 and nsize[s - 1] == 1 and nsize.sum() == 1 and not np.any(label)
    assert G[s - 1] == a * a * (s * s - 1) / 12.0


def test_both_ends_order():
    assert cn.order_both_ends(5).tolist() == [0, 2, 4, 3, 1] and cn.order_both_ends(4).tolist() == [0, 2, 3, 1]


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_union_find_against_a_flood_fill_and_the_identities(dim):
    Np, Nb, W = 90, 2, 2
    L = np.array([9.0, 7.0, 11.0])[:dim] * (Np / 90.0)
    rho = Np / float(np.prod(L))
    rc = cn.threshold_rc(dim, rho, L)
    P = cn.random_paths(W, 2 * Nb + 1, Np, L, np.random.default_rng(dim))
    for w in range(W):
        for a in range(2 * Nb + 1):
            r2 = cn.pair_r2(P[w, a], L)
            bond = (r2 > 0) & (r2 < rc * rc)
            assert np.array_equal(bond, bond.T)
            nsize, smax, nbond, G, label = cn.slice_sums(P[w, a], L, rc)
            assert np.array_equal(label, _flood(bond))
            assert nbond == bond.sum() // 2 and smax == np.bincount(label).max()
            assert np.array_equal(nsize, np.bincount(np.bincount(label)[np.bincount(label) > 0], minlength=Np + 1)[1:])
    win = cn.Window(P, Nb, Nb, L, rc)
    exp = win.expected([0, 1, 1])
    s = np.arange(1, Np + 1)
    assert exp["samples"].tolist() == [5, 10]
    assert np.array_equal((s * exp["nsize"]).sum(axis=1), Np * exp["samples"])
    assert np.array_equal(exp["nlarge"].sum(axis=1), exp["samples"])
    assert np.array_equal(exp["nsize"][1], 2 * win.expected([1])["nsize"][1])         # listed twice: counted twice
    assert not np.any(exp["rg2"][:, 0]) and np.all(exp["rg2"] >= 0)
    assert np.array_equal(exp["rg2"] > 0, (exp["nsize"] > 0) & (s > 1))


def test_a_pair_through_the_face_a_touching_pair_and_a_coincident_pair():
    L = [8.0, 4.0]
    X = np.array([[3.75, 0.0], [-3.75, 0.0], [0.0, 1.0], [0.0, 1.0]])
    nsize, smax, nbond, G, label = cn.slice_sums(X, L, 0.75)
    assert label.tolist() == [0, 0, 2, 3] and nbond == 1 and G[1] == 0.25 / 4.0          # coincident: no bond
    nsize, smax, nbond, G, label = cn.slice_sums(X, L, 0.5)
    assert label.tolist() == [0, 1, 2, 3] and nbond == 0                                 # r2 == rc2: no bond
    assert cn.slice_sums(X, L, np.nextafter(0.5, np.inf))[2] == 1


def test_normalize_cl():
    Np = 6
    got = {"nsize": np.array([[2, 2, 0, 0, 0, 0], [0, 0, 4, 0, 0, 0]]), "nlarge": np.array([[0, 2, 0, 0, 0, 0], [0, 0, 2, 0, 0, 0]]),
           "nbond": np.array([2, 8]), "samples": np.array([1 + 1, 2]), "rg2": np.array([[0, 0.5, 0, 0, 0, 0], [0, 0, 2.0, 0, 0, 0]])}
    n = normalize_cl(got, Np)
    assert n["n"][0].tolist() == [1, 1, 0, 0, 0, 0] and n["fraction"][0].tolist() == [1 / 6, 2 / 6, 0, 0, 0, 0]
    assert n["p_largest"][1].tolist() == [0, 0, 1, 0, 0, 0] and n["rg2"][0, 1] == 0.25 and n["rg2"][1, 2] == 0.5
    assert np.isnan(n["rg2"][0, 2]) and n["rg2"][0, 0] == 0
    assert n["n_clusters"].tolist() == [2, 2] and n["smax"].tolist() == [2 / 6, 3 / 6]
    assert n["mean_size"].tolist() == [(2 + 8) / (2 + 4), 3.0] and n["bonds"].tolist() == [2 / 12, 8 / 12]
    t = normalize_cl(got, Np, summed=True)
    assert t["n"].tolist() == [0.5, 0.5, 1, 0, 0, 0] and t["bonds"] == 10 / 24 and t["mean_size"] == (2 + 8 + 36) / 18
    one = normalize_cl({k: v[1] for k, v in got.items()}, Np)
    assert one["mean_size"] == 3.0 and one["n"].tolist() == n["n"][1].tolist()
    with pytest.raises(ValueError):
        normalize_cl(got, Np + 1)
