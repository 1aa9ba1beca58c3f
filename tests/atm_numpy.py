"""numpy restatement of the Axilrod-Teller-Muto sums that pigs_atm_* accumulates (include/pigs_hip.h has the definition),
with the same IEEE operations per term: per pair the coordinate difference x(lower) - x(higher), one fold per coordinate by
two compares against LboxHalf, r2 summed left to right; per triplet i < j < k with a2 = r2(i,j), b2 = r2(i,k), c2 = r2(j,k),
counted iff a2 <= rc2 and b2 <= rc2 and c2 <= rc2 in double:
    p = (a2*b2)*c2;  s = sqrt(p);  num = ((a2 + b2 - c2)*(a2 + c2 - b2))*(b2 + c2 - a2);  t = (p + 0.375*num)/((p*p)*s)
Every term has the device's bits; only the order of the sum differs, so a comparison of sums is bounded by Sum|t|, which
is returned beside T and the count.

Vectorised per vertex i over the pairs j < k of its partners beyond i."""
import numpy as np


def pair_r2(X, Lbox):
    """r2 [Np, Np] of the slice X [Np, dim] from d = x(row) - x(col), folded once, squares summed left to right.  (The fold
    is odd in d, so r2 is symmetric to the bit.)"""
    Np, dim = X.shape
    L = np.asarray(Lbox, np.float64)[:dim]
    Lh = 0.5 * L
    with np.errstate(invalid="ignore", over="ignore"):
        d = X[:, None, :] - X[None, :, :]
        d = np.where(d > Lh, d - L, d)
        d = np.where(d < -Lh, d + L, d)
        r2 = np.zeros((Np, Np))
        for k in range(dim):
            r2 = r2 + d[:, :, k] * d[:, :, k]
    return r2


def terms(a2, b2, c2):
    """The term of every triplet of sides (a2, b2, c2), elementwise, in the definition's order of operations."""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        p = (a2 * b2) * c2
        s = np.sqrt(p)
        num = ((a2 + b2 - c2) * (a2 + c2 - b2)) * (b2 + c2 - a2)
        return (p + 0.375 * num) / ((p * p) * s)


def slice_sums(X, Lbox, rc2):
    """One slice X [Np, dim]: (T, Sum|t|, ntrip)."""
    Np = X.shape[0]
    r2 = pair_r2(X, Lbox)
    T, A, n = 0.0, 0.0, 0
    with np.errstate(invalid="ignore"):
        near = r2 <= rc2                                                # NaN compares false
    for i in range(Np - 2):
        legs = np.nonzero(near[i, i + 1:])[0] + i + 1
        if len(legs) < 2:
            continue
        j, k = np.triu_indices(len(legs), 1)
        j, k = legs[j], legs[k]
        keep = near[j, k]
        j, k = j[keep], k[keep]
        if not len(j):
            continue
        t = terms(r2[i, j], r2[i, k], r2[j, k])
        T += float(t.sum())
        A += float(np.abs(t).sum())
        n += len(j)
    return T, A, n


class Window:
    """The sums of the window slices Nb-window..Nb+window of every walker of paths [W, M, Np, dim], computed once per
    (walker, rc2) and then only added up."""

    def __init__(self, paths, Nb, window, Lbox, slices=None):
        """slices: the dict of another Window over the SAME paths (its .slices), to share the per-slice sums with it."""
        self.paths, self.Nb, self.window, self.Lbox = paths, Nb, window, Lbox
        self.W = paths.shape[0]
        self.ns = 2 * window + 1
        self.slices = {} if slices is None else slices
        self._c = {}

    def _slice(self, w, a, rc2):
        key = (w, a, rc2)
        if key not in self.slices:
            self.slices[key] = slice_sums(self.paths[w, a], self.Lbox, rc2)
        return self.slices[key]

    def walker(self, w, rc2):
        key = (w, rc2)
        if key not in self._c:
            T, A, n = np.zeros(self.ns), np.zeros(self.ns), np.zeros(self.ns, np.int64)
            for js in range(self.ns):
                T[js], A[js], n[js] = self._slice(w, self.Nb - self.window + js, rc2)
            self._c[key] = (T, A, n)
        return self._c[key]

    def expected(self, walkers, rc):
        """Accumulated sums for the walker list `walkers` (entries may repeat), rc2 = rc*rc as the host computes it: dict of
        T [W, ns], abs [W, ns] (Sum|t|, the scale of a bound on T), ntrip [W, ns] and samples [W]."""
        rc2 = float(rc) * float(rc)
        T, A = np.zeros((self.W, self.ns)), np.zeros((self.W, self.ns))
        n, cnt = np.zeros((self.W, self.ns), np.int64), np.zeros(self.W, np.int64)
        for w in walkers:
            t, a, c = self.walker(w, rc2)
            T[w] += t
            A[w] += a
            n[w] += c
            cnt[w] += 1
        return {"T": T, "abs": A, "ntrip": n, "samples": cnt}
