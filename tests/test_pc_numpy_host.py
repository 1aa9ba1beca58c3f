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


# ---- image numbers far from zero ---------------------------------------------------------------------------------------
FAR = pn.far_images()


def _crossings(U, L, root=0):
    """Per particle and axis, the faces between the root's cell and the particle's, signed, from the unfolded points."""
    cell = np.floor((U + 0.5 * np.asarray(L)) / np.asarray(L)).astype(np.int64)
    return cell - cell[root]


def check_helix(X, L, rc, U, axes):
    """One finite cluster of all n particles whose image numbers are the cells of the unfolded line (far from zero along
    `axes`, both signs), and whose unfolded Rg^2 is the closed form of n collinear points at equal spacing."""
    n, dim = X.shape
    bond, nf = pn.bonds_of(X, L, rc), pn.fold_numbers(X, L)
    assert int(np.triu(bond, 1).sum()) == n - 1                         # the bonds of the line, none between turns
    label, m, mask = pn.components(bond, nf)
    assert np.unique(label).size == 1 and not np.any(label) and not np.any(mask)
    cross = _crossings(U, L)
    assert np.array_equal(np.abs(m), np.abs(cross)) and (np.array_equal(m, cross) or np.array_equal(m, -cross))
    for k in range(dim):
        if k in axes:
            assert np.abs(m[:, k]).max() == np.abs(cross[:, k]).max() >= 15 and m[:, k].min() <= -5 and m[:, k].max() >= 5
        else:
            assert not np.any(m[:, k])
    fl, fm, fmask = _flood(bond, nf)
    assert np.array_equal(fl, label) and np.array_equal(fm, m) and not np.any(fmask)
    nwrap, mwrap, smask, nfin, G, _, _ = pn.slice_sums(X, L, rc)
    assert smask == 0 and nwrap.tolist() == [1] + [0] * 7 and mwrap[0] == n and nfin[n - 1] == 1 and nfin.sum() == 1
    return m, G[n - 1]


@pytest.mark.parametrize("name", ["helix2d_plus", "helix2d_minus", "helix3d_plus", "helix3d_minus", "double_helix_same",
                                  "double_helix_opposite"])
def test_helix_is_one_finite_cluster_with_the_closed_form(name):
    X, L, rc, U = FAR[name]
    n = X.shape[0]
    axes = (0, 1) if name.startswith("double") else (0,)
    m, g = check_helix(X, L, rc, U, axes)
    climb = X.shape[1] - 1 if name.startswith("double") else 1          # the axis that never wraps sorts the line
    s = U[np.argsort(U[:, climb])]
    d2 = float(((s[1] - s[0]) ** 2).sum())
    assert np.allclose(np.diff(s, axis=0), s[1] - s[0], rtol=0, atol=1e-9)     # collinear, equal steps
    want = d2 * (n * n - 1) / 12.0
    tol = (n * (n - 1) / 2 + n + 8) * 2.0 ** -53
    print(f"{name}: max |m| {np.abs(m).max(axis=0).tolist()}, rg2u / closed form - 1 = {g / want - 1.0:.3e} (bound {tol:.3e})")
    assert abs(g - want) <= tol * want
    assert np.array_equal(X, pn.hand_built()[name][0])                 # the slice the GPU test runs
    folded = cn.slice_sums(X, L, rc)[3][n - 1]
    assert 0 < folded < 0.1 * want                                      # the folded r_ij stay within half the short side
    if name == "double_helix_opposite":
        assert np.array_equal(np.sign(m[:, 0]) * np.sign(m[:, 1]) <= 0, np.ones(n, bool)) and np.any(m[:, 0] * m[:, 1] < -25)
    if name == "double_helix_same":
        assert np.all(m[:, 0] * m[:, 1] >= 0) and np.any(m[:, 0] * m[:, 1] > 25)


def test_helix_windings_mirror_each_other():
    """Towards +x and towards -x: the image numbers along x have opposite signs, particle by particle."""
    for dim in (2, 3):
        a = pn.components(pn.bonds_of(*FAR[f"helix{dim}d_plus"][:3]), pn.fold_numbers(*FAR[f"helix{dim}d_plus"][:2]))[1]
        b = pn.components(pn.bonds_of(*FAR[f"helix{dim}d_minus"][:3]), pn.fold_numbers(*FAR[f"helix{dim}d_minus"][:2]))[1]
        assert np.abs(a[:, 0]).max() >= 20 and np.abs(np.abs(a[:, 0]) - np.abs(b[:, 0])).max() <= 1
        assert np.all(a[:, 0] * b[:, 0] <= 0)


def test_double_winding_wraps_with_mask_3_and_a_mismatch_of_two():
    X, L, rc, U = FAR["double_winding"]
    n = X.shape[0]
    bond, nf = pn.bonds_of(X, L, rc), pn.fold_numbers(X, L)
    assert int(np.triu(bond, 1).sum()) == n                             # n bonds on n particles: one closes the line
    label, m, mask = pn.components(bond, nf)
    assert not np.any(label) and np.all(mask == 3)
    i, j = np.nonzero(np.triu(bond, 1))
    mis = m[i] - m[j] - nf[i, j]
    bad = np.nonzero(np.any(mis != 0, axis=1))[0]
    assert bad.size == 1 and np.abs(mis[bad[0]]).tolist() == [2, 1]
    assert np.array_equal(_flood(bond, nf)[2], mask)
    nwrap, mwrap, smask, nfin, G, _, _ = pn.slice_sums(X, L, rc)
    assert smask == 3 and nwrap[3] == 1 and mwrap[3] == n and nwrap.sum() == 1 and not np.any(nfin) and not np.any(G)


@pytest.mark.parametrize("dim", [2, 3])
def test_helix_at_the_size_limit(dim):
    """The slice tests/test_gpu_cl_pc_limits.py runs at kClNpMax = 2048: |m_x| passes 150."""
    n = 2048
    X, L, rc, U = pn.helix(n, dim)
    m, g = check_helix(X, L, rc, U, (0,))
    s = U[np.argsort(U[:, 1])]
    want = float(((s[1] - s[0]) ** 2).sum()) * (n * n - 1) / 12.0
    assert abs(g - want) <= (n * (n - 1) / 2 + n + 8) * 2.0 ** -53 * want
    assert np.abs(m[:, 0]).max() >= 150 and m[:, 0].min() <= -70
