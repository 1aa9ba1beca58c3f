"""numpy restatement of the cluster sums that pigs_cl_* accumulates (include/pigs_hip.h has the definition), written from
the definition and sharing no code with the library: the bond list of a slice, a plain union-find over it, and the sums
with the same IEEE operations per term in the same order.  Pinned to literal cases and closed forms by
tests/test_cl_numpy_host.py.  Also the input builders of the cluster tests.

Paths are [walker, slice, particle, axis]."""
import numpy as np


def fold(d, L):
    """min_image: the two compares one after the other, each against L/2, nothing fused."""
    L = np.asarray(L, dtype=np.float64)
    half = 0.5 * L
    d = np.where(d > half, d - L, d)
    return np.where(d < -half, d + L, d)


def pair_r2(X, L):
    """r2[i, j]: the squares of d = x(i) - x(j), folded once, summed left to right from 0.0."""
    d = fold(X[:, None, :] - X[None, :, :], L)
    r2 = np.zeros(d.shape[:2])
    for k in range(d.shape[2]):
        r2 = r2 + d[..., k] * d[..., k]
    return r2


def labels_of(bond):
    """label[i]: the smallest index of i's connected component, by a plain union-find over the bond list (i < j)."""
    n = bond.shape[0]
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    for i, j in zip(*np.nonzero(np.triu(bond, 1))):
        a, b = find(int(i)), find(int(j))
        if a != b:
            parent[max(a, b)] = min(a, b)                               # the smaller index stays the root
    return np.array([find(i) for i in range(n)], dtype=np.int64)


def slice_sums(X, L, rc):
    """One slice X [Np, dim]: (nsize [Np] int64, smax, nbond, G [Np] float64, label [Np])."""
    Np = X.shape[0]
    rc2 = float(rc) * float(rc)
    r2 = pair_r2(np.asarray(X, dtype=np.float64), L)
    with np.errstate(invalid="ignore"):
        bond = (r2 > 0.0) & (r2 < rc2)
    np.fill_diagonal(bond, False)
    label = labels_of(bond)
    t = np.zeros(Np)
    for i in range(Np):
        js = np.nonzero(label[i + 1:] == label[i])[0] + i + 1
        if js.size:
            t[i] = np.cumsum(r2[i, js])[-1]                             # one addition after the other from the first term
    nsize = np.zeros(Np, np.int64)
    G = np.zeros(Np)
    smax = 0
    for r in np.nonzero(label == np.arange(Np))[0]:                     # roots ascending
        mem = np.nonzero(label == r)[0]
        s = mem.size
        T = 0.0
        for i in mem:
            T = T + t[i]
        g = T / (float(s) * float(s))
        nsize[s - 1] += 1
        G[s - 1] = G[s - 1] + g
        smax = max(smax, s)
    return nsize, smax, int(np.triu(bond, 1).sum()), G, label


class Window:
    """The slices Nb-window..Nb+window of every walker of P, their slice sums computed once."""

    def __init__(self, P, Nb, window, L, rc):
        self.P = np.asarray(P, dtype=np.float64)
        self.Np = self.P.shape[2]
        self.slices = list(range(Nb - window, Nb + window + 1))
        self.L, self.rc = np.asarray(L, dtype=np.float64), float(rc)
        self._sums = {}

    def sums(self, w):
        if w not in self._sums:
            self._sums[w] = [slice_sums(self.P[w, a], self.L, self.rc) for a in self.slices]
        return self._sums[w]

    def expected(self, walkers):
        """The sums after one sample of each entry of `walkers` (a walker listed twice counts twice), all walkers of P."""
        W, Np = self.P.shape[0], self.Np
        out = {"nsize": np.zeros((W, Np), np.int64), "nlarge": np.zeros((W, Np), np.int64), "nbond": np.zeros(W, np.int64),
               "samples": np.zeros(W, np.int64), "rg2": np.zeros((W, Np))}
        terms = np.zeros((W, Np), np.int64)                             # the non-zero terms an element of rg2 holds
        for w in walkers:
            for nsize, smax, nbond, G, _ in self.sums(w):
                out["nsize"][w] += nsize
                out["nlarge"][w, smax - 1] += 1
                out["nbond"][w] += nbond
                out["samples"][w] += 1
                out["rg2"][w] = out["rg2"][w] + G                       # slices ascending, one add per slice and size
                terms[w] += (G != 0.0)
        out["terms"] = terms
        return out


# ---- input builders ---------------------------------------------------------------------------------------------------
def wrap(X, L):
    L = np.asarray(L, dtype=np.float64)
    return X - L * np.floor((X + 0.5 * L) / L)


def random_paths(W, M, Np, L, rng):
    """Independent uniform points in the cell [-L/2, L/2) for every walker and slice."""
    L = np.asarray(L, dtype=np.float64)
    return rng.uniform(-0.5, 0.5, (W, M, Np, L.size)) * L


def threshold_rc(dim, density, L):
    """A bond radius near the connectivity threshold of uniform points of this density: continuum percolation of spheres
    of diameter rc (filling 1.128 in 2D gives 1.20 rho^-1/2, 0.3418 in 3D gives 0.87 rho^-1/3), a little above it so that
    a finite sample has a large cluster beside small ones; in 1D, where there is none, a bond probability of 0.95 per gap.
    Never beyond half the shortest side."""
    c = {1: 3.0, 2: 1.3, 3: 0.95}[dim]
    return min(c * float(density) ** (-1.0 / dim), 0.5 * float(np.min(np.asarray(L)[:dim])))


def chain(n, spacing, order, dim=3, origin=None):
    """n points on a line along x, point p at origin + p spacing; particle order[p] sits at point p."""
    X = np.zeros((n, dim))
    if origin is not None:
        X[:] = np.asarray(origin, dtype=np.float64)
    pos = np.concatenate([[0.0], np.cumsum(np.broadcast_to(np.asarray(spacing, dtype=np.float64), (n - 1,)))]) if n > 1 \
        else np.zeros(1)
    X[np.asarray(order), 0] = X[np.asarray(order), 0] + pos
    return X


def order_both_ends(n):
    """0 at one end, 1 at the other, 2 next to 0, 3 next to 1, ..: the particle at point p."""
    order = np.empty(n, np.int64)
    lo, hi = 0, n - 1
    for idx in range(n):
        if idx % 2 == 0:
            order[lo] = idx
            lo += 1
        else:
            order[hi] = idx
            hi -= 1
    return order


def as_paths(X, M):
    """One walker whose M slices all hold the slice X."""
    return np.broadcast_to(X, (1, M) + X.shape).copy()
