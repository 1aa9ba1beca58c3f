"""numpy restatement of the sums that pigs_pc_* accumulates (include/pigs_hip.h has the definition), written from the
definition and sharing no code with the library: a union-find that carries, for every particle, the offset vector of its
image numbers to its parent -- another algorithm than the device's sweeps from the roots --, the wrap mask from the bonds
that close a walk inside one tree, the unfolded separations of the finite clusters with the same IEEE operations in the
same order, and a plain double loop over origins and lags for the persistence counts.  Pinned to a flood fill with image
numbers, to rings, lattices and closed forms by tests/test_pc_numpy_host.py.  The input builders of the percolation tests
are here too (among them the helices, whose image numbers run far from zero); those of cl_numpy serve as they are.

Paths are [walker, slice, particle, axis]."""
import numpy as np

import cl_numpy as cn


def fold_numbers(X, L):
    """n[i, j, k]: +1 where min_image takes d - L for d = x(i) - x(j) along k, -1 where it takes d + L, else 0."""
    half = 0.5 * np.asarray(L, dtype=np.float64)
    d = X[:, None, :] - X[None, :, :]
    with np.errstate(invalid="ignore"):
        return np.where(d > half, 1, np.where(d < -half, -1, 0)).astype(np.int64)


def bonds_of(X, L, rc):
    r2 = cn.pair_r2(X, L)
    with np.errstate(invalid="ignore"):
        bond = (r2 > 0.0) & (r2 < float(rc) * float(rc))
    np.fill_diagonal(bond, False)
    return bond


def components(bond, n):
    """(label [Np], m [Np, dim], mask [Np]): the smallest index of i's component, the image numbers relative to it
    (m_i = m_j + n_ij along the tree the union-find built) and, at every particle, the wrap mask of its component."""
    Np, dim = bond.shape[0], n.shape[2]
    parent = list(range(Np))
    off = np.zeros((Np, dim), np.int64)                                 # m_a - m_parent(a)

    def find(a):
        chain = []
        while parent[a] != a:
            chain.append(a)
            a = parent[a]
        acc = np.zeros(dim, np.int64)
        for b in reversed(chain):                                       # from the root's child down: off becomes m_b - m_root
            acc = acc + off[b]
            off[b] = acc
            parent[b] = a
        return a, (off[chain[0]].copy() if chain else np.zeros(dim, np.int64))

    closing = []                                                        # (a particle of the tree, the mismatch of a closing bond)
    for i, j in zip(*np.nonzero(np.triu(bond, 1))):
        i, j = int(i), int(j)
        (ri, oi), (rj, oj) = find(i), find(j)
        if ri == rj:
            closing.append((i, oi - oj - n[i, j]))                      # m_i - m_j - n_ij inside one tree
        elif ri < rj:
            parent[rj], off[rj] = ri, oi - oj - n[i, j]                 # m_rj - m_ri from m_i = m_j + n_ij
        else:
            parent[ri], off[ri] = rj, oj + n[i, j] - oi
    label = np.empty(Np, np.int64)
    m = np.zeros((Np, dim), np.int64)
    for i in range(Np):
        label[i], m[i] = find(i)
    rootmask = np.zeros(Np, np.int64)
    for i, mis in closing:
        rootmask[label[i]] |= sum(1 << k for k in range(dim) if mis[k] != 0)
    return label, m, rootmask[label]


def slice_sums(X, L, rc):
    """One slice X [Np, dim]: (nwrap [8], mwrap [8], slice mask, nfin [Np], G [Np], label [Np], mask per particle [Np])."""
    X = np.asarray(X, dtype=np.float64)
    L = np.asarray(L, dtype=np.float64)
    Np, dim = X.shape
    label, m, mask = components(bonds_of(X, L, rc), fold_numbers(X, L))
    t = np.zeros(Np)
    for i in range(Np):
        if mask[i]:
            continue
        js = np.nonzero(label[i + 1:] == label[i])[0] + i + 1
        if js.size:
            ru2 = np.zeros(js.size)
            for k in range(dim):
                c = (m[i, k] - m[js, k]).astype(np.float64)
                du = (X[i, k] - X[js, k]) - c * L[k]                    # the product first, then the subtraction
                ru2 = ru2 + du * du
            t[i] = np.cumsum(ru2)[-1]                                   # one addition after the other from the first term
    nwrap, mwrap = np.zeros(8, np.int64), np.zeros(8, np.int64)
    nfin, G = np.zeros(Np, np.int64), np.zeros(Np)
    smask = 0
    for r in np.nonzero(label == np.arange(Np))[0]:                     # roots ascending
        mem = np.nonzero(label == r)[0]
        s, mk = mem.size, int(mask[r])
        nwrap[mk] += 1
        mwrap[mk] += s
        smask |= mk
        if mk == 0:
            T = 0.0
            for i in mem:
                T = T + t[i]
            nfin[s - 1] += 1
            G[s - 1] = G[s - 1] + T / (float(s) * float(s))
    return nwrap, mwrap, smask, nfin, G, label, mask


def together(label):
    """The pairs i < j of one slice that carry the same label, as a boolean matrix (upper triangle)."""
    return np.triu(label[:, None] == label[None, :], 1)


class Window:
    """The slices Nb-window..Nb+window of every walker of P, their slice sums computed once."""

    def __init__(self, P, Nb, window, L, rc, ntau=0):
        self.P = np.asarray(P, dtype=np.float64)
        self.Np = self.P.shape[2]
        self.slices = list(range(Nb - window, Nb + window + 1))
        self.L, self.rc, self.ntau = np.asarray(L, dtype=np.float64), float(rc), int(ntau)
        self._sums, self._pers = {}, {}

    def sums(self, w):
        if w not in self._sums:
            self._sums[w] = [slice_sums(self.P[w, a], self.L, self.rc) for a in self.slices]
        return self._sums[w]

    def persistence(self, w):
        """first, second, both, norig [ntau + 1] of one sample of walker w: origins and lags in a plain double loop."""
        if w not in self._pers:
            tog = [together(s[5]) for s in self.sums(w)]
            out = np.zeros((4, self.ntau + 1), np.int64)
            for a in range(len(tog)):
                for l in range(self.ntau + 1):
                    if a + l >= len(tog):
                        continue
                    out[0, l] += int(tog[a].sum())
                    out[1, l] += int(tog[a + l].sum())
                    out[2, l] += int((tog[a] & tog[a + l]).sum())
                    out[3, l] += 1
            self._pers[w] = out
        return self._pers[w]

    def expected(self, walkers):
        """The sums after one sample of each entry of `walkers` (a walker listed twice counts twice), all walkers of P."""
        W, Np, nl = self.P.shape[0], self.Np, self.ntau + 1
        out = {k: np.zeros((W, 8), np.int64) for k in ("nwrap", "mwrap", "swrap")}
        out.update({"nfin": np.zeros((W, Np), np.int64), "samples": np.zeros(W, np.int64), "rg2u": np.zeros((W, Np))})
        out.update({k: np.zeros((W, nl), np.int64) for k in ("first", "second", "both", "norig")})
        terms = np.zeros((W, Np), np.int64)                             # the non-zero terms an element of rg2u holds
        for w in walkers:
            for nwrap, mwrap, smask, nfin, G, _, _ in self.sums(w):
                out["nwrap"][w] += nwrap
                out["mwrap"][w] += mwrap
                out["swrap"][w, smask] += 1
                out["nfin"][w] += nfin
                out["samples"][w] += 1
                out["rg2u"][w] = out["rg2u"][w] + G                     # slices ascending, one add per slice and size
                terms[w] += (G != 0.0)
            pers = self.persistence(w)
            for q, k in enumerate(("first", "second", "both", "norig")):
                out[k][w] += pers[q]
        out["terms"] = terms
        return out


# ---- input builders ---------------------------------------------------------------------------------------------------
def ring(n, L, dim, order=None, axis=0, origin=None):
    """n points at spacing L[axis]/n along `axis`, wrapped into the cell; particle order[p] sits at point p."""
    L = np.asarray(L, dtype=np.float64)
    X = np.zeros((n, dim))
    if origin is not None:
        X[:] = np.asarray(origin, dtype=np.float64)
    order = np.arange(n) if order is None else np.asarray(order)
    X[order, axis] = X[order, axis] + np.arange(n) * (L[axis] / n)
    return cn.wrap(X, L[:dim])


def staircase(n, L):
    """2D: n points on the diagonal of the cell, point p at p (L/n): the chain closes through both faces at once."""
    L = np.asarray(L, dtype=np.float64)[:2]
    return cn.wrap(np.arange(n)[:, None] * (L / n)[None, :] + 0.1 * L, L)


def lattice(n, L, dim):
    """n^dim points of a square or cubic lattice that fills the cell."""
    L = np.asarray(L, dtype=np.float64)[:dim]
    g = np.stack(np.meshgrid(*([np.arange(n)] * dim), indexing="ij"), axis=-1).reshape(-1, dim)
    return cn.wrap((g + 0.25) * (L / n), L)


def root_mid_chain(n, at, seed):
    """A shuffled order whose particle 0 -- the root of a cluster that holds it -- sits at point `at` of the line."""
    order = np.random.default_rng(seed).permutation(n)
    z = int(np.nonzero(order == 0)[0][0])
    order[z], order[at] = order[at], 0
    return order


def _line(n, step, origin, L, order):
    """(X, U): n points at origin + p step, particle order[p] at point p; U unfolded, X wrapped into the cell."""
    U = np.zeros((n, len(step)))
    U[np.asarray(order)] = np.asarray(origin, dtype=np.float64) + np.arange(n)[:, None] * np.asarray(step, dtype=np.float64)
    return wrap_cell(U, L), U


def wrap_cell(U, L):
    X = cn.wrap(U, np.asarray(L, dtype=np.float64))
    assert np.all(np.abs(X) < 0.5 * np.asarray(L)), "a point on a face"
    return X


HELIX_LX, HELIX_DX, HELIX_CLIMB = 8.0, 0.9, 1.2                         # in units of rc


def helix(n, dim, sign=1, rc=1.0, order=None):
    """A chain with steps of 0.9 rc along x (sign: towards +x or -x) in a cell of Lx = 8 rc, which climbs 1.2 rc along y per
    turn in a cell too tall to wrap in y (3D: z constant, Lz = 8 rc): neighbours along the line are 0.91 rc apart, second
    neighbours 1.82 rc and successive turns 1.19 rc, so the bonds are those of the line and the cluster is ONE finite
    cluster that goes through the x faces once every 8.9 steps.  Returns (X, L, rc, U): U the unfolded points, on a
    line at equal spacing; particle order[p] at point p (default: root_mid_chain at n // 3)."""
    assert dim in (2, 3)
    dy = HELIX_CLIMB * HELIX_DX / HELIX_LX
    L = [HELIX_LX * rc, (n * dy + 4.0) * rc] + [8.0 * rc] * (dim - 2)
    step = [sign * HELIX_DX * rc, dy * rc] + [0.0] * (dim - 2)
    origin = [0.05 * rc, -0.5 * (n - 1) * dy * rc] + [1.0 * rc] * (dim - 2)
    order = root_mid_chain(n, n // 3, n + dim) if order is None else order
    X, U = _line(n, step, origin, L, order)
    return X, L, rc, U


def double_helix(n, sy=1, rc=1.0, order=None):
    """3D: the line advances by (0.64, 0.48 sy) rc per step along the diagonal of a cell of 8 rc x 6 rc -- 12.5 steps per turn
    through the x AND the y faces, after which it is back over its own track -- and climbs 1.2 rc along z per turn: one
    finite cluster whose image numbers along x and y grow together (sy = +1) or with opposite signs (sy = -1)."""
    dz = HELIX_CLIMB * 0.64 / 8.0
    L = [8.0 * rc, 6.0 * rc, (n * dz + 4.0) * rc]
    order = root_mid_chain(n, n // 3, n + 7 + sy) if order is None else order
    X, U = _line(n, [0.64 * rc, 0.48 * sy * rc, dz * rc], [0.05 * rc, 0.03 * rc, -0.5 * (n - 1) * dz * rc], L, order)
    return X, L, rc, U


def double_winding(n, rc=1.0, order=None):
    """2D: a closed line of n points that goes twice round x and once round y before its last point bonds to its first:
    one wrapping cluster of mask 3 whose one closing bond has a mismatch of 2 along x and 1 along y.  Steps of
    (0.6, 0.4) rc; the two strands are half the cell apart."""
    L = [0.3 * n * rc, 0.4 * n * rc]
    order = root_mid_chain(n, n // 3, n + 11) if order is None else order
    X, U = _line(n, [2.0 * L[0] / n, L[1] / n], [0.05 * rc, 0.03 * rc], L, order)
    return X, L, rc, U


def far_images(n=300):
    """name -> (X, L, rc, U): the slices whose image numbers leave {-1, 0, +1}."""
    out = {}
    for dim in (2, 3):
        for sign, tag in ((1, "plus"), (-1, "minus")):
            out[f"helix{dim}d_{tag}"] = helix(n, dim, sign)
    out["double_helix_same"] = double_helix(n, 1)
    out["double_helix_opposite"] = double_helix(n, -1)
    out["double_winding"] = double_winding(n)
    return out


RING_L = [270.0, 8.0, 8.0]                                              # 300 points at spacing 0.9 close a ring along x
FACE_L = [600.0, 8.0, 8.0]


def hand_built():
    """name -> (X [Np, dim], L, rc): the slices that tests/test_pc_numpy_host.py pins and tests/test_gpu_pc.py runs."""
    out = {}
    n = 300
    orders = {"ascending": np.arange(n), "shuffled": np.random.default_rng(300).permutation(n), "ends": cn.order_both_ends(n)}
    for name, order in orders.items():
        out[f"ring300_{name}"] = (ring(n, RING_L, 3, order, origin=[-140.0, 1.0, -2.0]), RING_L, 1.0)
    out["ring_1d"] = (ring(40, [36.0], 1, np.random.default_rng(40).permutation(40), origin=[3.0]), [36.0], 1.0)
    out["cut_ring"] = (np.delete(ring(n, RING_L, 3, origin=[-140.0, 1.0, -2.0]), 117, axis=0), RING_L, 1.0)
    out["staircase"] = (staircase(30, [24.0, 30.0]), [24.0, 30.0], 1.5)
    for dim in (2, 3):
        out[f"lattice{dim}d_bonded"] = (lattice(4, [5.0] * dim, dim), [5.0] * dim, 1.01 * 1.25)
        out[f"lattice{dim}d_single"] = (lattice(4, [5.0] * dim, dim), [5.0] * dim, 0.99 * 1.25)
    out["pair_through_face"] = (np.array([[3.75, 0.0, 0.0], [-3.75, 0.0, 0.0], [2.0, 4.0, 1.0]]), [8.0, 16.0, 4.0], 0.75)
    X = np.zeros((n, 3))
    X[:, 0] = -290.0 + 1.9 * np.arange(n)
    X[[63, 64, 255, 256]] = [[299.75, 2.0, 1.0], [-299.875, 2.0, 1.0], [-299.875, 2.375, 1.0], [-299.875, 2.375, 1.375]]
    out["words_and_face"] = (X, FACE_L, 0.5)
    out.update({name: v[:3] for name, v in far_images(n).items()})
    return out
