"""tests/pc_numpy.py, the yardstick of the percolation family, against literal cases and closed forms (no GPU): a
breadth-first flood fill that carries image numbers, rings that wrap and a cut ring longer than half the box, a
staircase through two faces, lattices, a pair through a face, and the identities that tie its sums to tests/cl_numpy.py."""
import numpy as np
import pytest

import cl_numpy as cn
import pc_numpy as pn

HB = pn.hand_built()


def _flood(bond, n):
    """Breadth first from the smallest index of every component: label, image numbers m (m_j = m_i - n_ij along the tree)
    and the mask of every bond that the image numbers do not explain, at the root."""
    Np, dim = bond.shape[0], n.shape[2]
    label = -np.ones(Np, np.int64)
    m = np.zeros((Np, dim), np.int64)
    for r in range(Np):
        if label[r] >= 0:
            continue
        queue, label[r] = [r], r
        while queue:
            i = queue.pop(0)
            for j in np.nonzero(bond[i])[0]:
                if label[j] < 0:
                    label[j], m[j] = r, m[i] - n[i, j]
                    queue.append(int(j))
    mask = np.zeros(Np, np.int64)
    for i, j in zip(*np.nonzero(bond)):
        for k in range(dim):
            if m[i, k] - m[j, k] != n[i, j, k]:
                mask[label[i]] |= 1 << k
    return label, m, mask[label]


@pytest.mark.parametrize("factor", [1.0, 0.8])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_union_find_against_a_flood_fill_and_the_identities(dim, factor):
    Np, Nb, W, ntau = 90, 2, 2, 3
    L = np.array([9.0, 7.0, 11.0])[:dim] * (Np / 90.0)
    rc = factor * cn.threshold_rc(dim, Np / float(np.prod(L)), L)
    P = cn.random_paths(W, 2 * Nb + 1, Np, L, np.random.default_rng(dim))
    P[1, 3:] = P[1, 2]                                                  # slices that repeat: persistence that is not all loss
    masks = set()
    for w in range(W):
        for a in range(2 * Nb + 1):
            X = P[w, a]
            n = pn.fold_numbers(X, L)
            assert np.array_equal(n, -n.transpose(1, 0, 2))
            bond = pn.bonds_of(X, L, rc)
            label, m, mask = pn.components(bond, n)
            fl, fm, fmask = _flood(bond, n)
            assert np.array_equal(label, fl) and np.array_equal(mask, fmask)
            assert np.array_equal(label, cn.slice_sums(X, L, rc)[4])
            fin = mask == 0
            assert np.array_equal(m[fin], fm[fin])                      # unique in a finite cluster
            assert not np.any(m[label == np.arange(Np)])
            masks |= set(mask.tolist())
    if dim > 1 and factor == 1.0:
        assert len(masks - {0}) >= 2 and 0 in masks
    lists = [0, 1, 1]
    exp = pn.Window(P, Nb, Nb, L, rc, ntau).expected(lists)
    cl = cn.Window(P, Nb, Nb, L, rc).expected(lists)
    s = np.arange(1, Np + 1)
    assert exp["samples"].tolist() == [5, 10] and np.array_equal(exp["samples"], cl["samples"])
    assert np.array_equal(exp["nwrap"].sum(axis=1), cl["nsize"].sum(axis=1))
    assert np.all(exp["nfin"] <= cl["nsize"])
    assert np.array_equal(exp["mwrap"][:, 0], (s * exp["nfin"]).sum(axis=1))
    assert np.array_equal(exp["mwrap"].sum(axis=1), Np * exp["samples"])
    assert np.array_equal(exp["swrap"].sum(axis=1), exp["samples"])
    assert np.array_equal(exp["first"][:, 0], (s * (s - 1) // 2 * cl["nsize"]).sum(axis=1))
    assert np.array_equal(exp["first"][:, 0], exp["second"][:, 0]) and np.array_equal(exp["first"][:, 0], exp["both"][:, 0])
    assert np.all(exp["both"] <= np.minimum(exp["first"], exp["second"]))
    assert exp["norig"][0].tolist() == [5, 4, 3, 2] and exp["norig"][1].tolist() == [10, 8, 6, 4]
    assert np.all(exp["nwrap"][:, 1 << dim:] == 0)
    assert np.all(exp["both"][0, 1:] < exp["first"][0, 1:]) or exp["first"][0, 1:].sum() == 0


def test_identical_slices_keep_every_pair():
    L = np.array([7.0, 11.0])
    X = cn.random_paths(1, 1, 60, L, np.random.default_rng(8))[0, 0]
    exp = pn.Window(cn.as_paths(X, 5), 2, 2, L, cn.threshold_rc(2, 60 / 77.0, L), 4).expected([0])
    assert exp["first"][0, 0] > 0 and exp["norig"][0].tolist() == [5, 4, 3, 2, 1]
    assert np.array_equal(exp["both"], exp["first"]) and np.array_equal(exp["both"], exp["second"])
    assert np.array_equal(exp["first"][0], exp["first"][0, 0] // 5 * exp["norig"][0])


@pytest.mark.parametrize("name", ["ring300_ascending", "ring300_shuffled", "ring300_ends", "ring_1d"])
def test_ring_wraps_along_x(name):
    X, L, rc = HB[name]
    n = X.shape[0]
    nwrap, mwrap, smask, nfin, G, label, mask = pn.slice_sums(X, L, rc)
    assert L[0] / n < rc and not np.any(label) and smask == 1
    assert nwrap.tolist() == [0, 1, 0, 0, 0, 0, 0, 0] and mwrap[1] == n and not np.any(nfin) and not np.any(G)
    assert cn.slice_sums(X, L, rc)[2] == n                              # n bonds on n particles: one closes the ring


def test_cut_ring_is_finite_and_longer_than_half_the_box():
    X, L, rc = HB["cut_ring"]
    s, a = X.shape[0], L[0] / 300
    nwrap, mwrap, smask, nfin, G, label, mask = pn.slice_sums(X, L, rc)
    assert s == 299 and smask == 0 and nwrap[0] == 1 and mwrap[0] == s and nfin[s - 1] == 1 and nfin.sum() == 1
    assert (s - 1) * a > 0.5 * L[0] and 2 * a > rc
    want = a * a * (s * s - 1) / 12.0
    assert abs(G[s - 1] - want) <= 1e-12 * want                         # the chain's closed form, unfolded
    folded = cn.slice_sums(X, L, rc)[3][s - 1]
    assert folded < 0.6 * want                                          # the folded r_ij are no separations along the chain


def test_staircase_closes_through_two_faces():
    X, L, rc = HB["staircase"]
    nwrap, mwrap, smask, nfin, G, label, mask = pn.slice_sums(X, L, rc)
    assert not np.any(label) and smask == 3 and nwrap[3] == 1 and mwrap[3] == 30 and cn.slice_sums(X, L, rc)[2] == 30


@pytest.mark.parametrize("dim", [2, 3])
def test_lattice_below_and_above_its_spacing(dim):
    X, L, rc = HB[f"lattice{dim}d_bonded"]
    Np = 4 ** dim
    nwrap, mwrap, smask, nfin, G, label, mask = pn.slice_sums(X, L, rc)
    full = (1 << dim) - 1
    assert smask == full and nwrap[full] == 1 and mwrap[full] == Np and nwrap.sum() == 1 and not np.any(nfin)
    X, L, rc = HB[f"lattice{dim}d_single"]
    nwrap, mwrap, smask, nfin, G, label, mask = pn.slice_sums(X, L, rc)
    assert smask == 0 and nwrap[0] == Np and mwrap[0] == Np and nfin[0] == Np and nfin.sum() == Np and not np.any(G)


def test_pair_through_a_face_is_finite_with_the_folded_g():
    X, L, rc = HB["pair_through_face"]
    nwrap, mwrap, smask, nfin, G, label, mask = pn.slice_sums(X, L, rc)
    assert label.tolist() == [0, 0, 2] and smask == 0 and nfin.tolist() == [1, 1, 0]
    assert G[1] == 0.25 / 4.0 == cn.slice_sums(X, L, rc)[3][1]


def test_cluster_across_the_mask_words_and_a_face():
    X, L, rc = HB["words_and_face"]
    nwrap, mwrap, smask, nfin, G, label, mask = pn.slice_sums(X, L, rc)
    want = np.arange(300)
    want[[64, 255, 256]] = 63
    assert np.array_equal(label, want) and smask == 0 and nfin[3] == 1 and nfin[0] == 296
    assert np.any(pn.fold_numbers(X, L)[63, 64] != 0)                   # the bond 63-64 goes through the face
    assert G[3] == cn.slice_sums(X, L, rc)[3][3] and G[3] > 0
