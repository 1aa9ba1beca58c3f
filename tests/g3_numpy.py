"""numpy restatement of the triplet counts that pigs_g3_* accumulates (include/pigs_hip.h has the definition), with the
same IEEE operations in the same order: d_k = x_k(i) - x_k(j), one fold per coordinate by two compares against LboxHalf,
r2 summed left to right, s = sqrt(r2), u = s/rbin decided in double before any conversion; per pair of legs the dot
product summed left to right, c = dot/(s_j s_k), v = (c + 1.0)(0.5 Na), clamped in double.  All integer counts: every
comparison with the device is exact.

Vectorised per vertex: the legs of a vertex are at most Np - 1, their pairs at most (Np - 1)(Np - 2)/2."""
import numpy as np


def n_leg_pairs(Nr):
    return Nr * (Nr + 1) // 2


def packed_index(lo, hi, Nr):
    """p of the leg bins lo <= hi on the packed upper triangle."""
    return lo * Nr - lo * (lo - 1) // 2 + (hi - lo)


def legs(X, i, Lbox, Nr, rbin):
    """The legs of vertex i of the slice X [Np, dim], in ascending j: (d [n, dim], s [n], b [n])."""
    Np, dim = X.shape
    L = np.asarray(Lbox, np.float64)[:dim]
    Lh = 0.5 * L
    with np.errstate(invalid="ignore", over="ignore"):
        d = X[i][None, :] - X
        d = np.where(d > Lh, d - L, d)
        d = np.where(d < -Lh, d + L, d)
        r2 = np.zeros(Np)
        for k in range(dim):
            r2 = r2 + d[:, k] * d[:, k]
        s = np.sqrt(r2)
        u = s / rbin
        leg = (0.0 < r2) & (u < float(Nr))                            # NaN and Inf compare false
    leg[i] = False
    return d[leg], s[leg], u[leg].astype(np.int64)


def angle_bins(d, s, Na):
    """For every unordered pair j < k of the legs (d, s): (j, k, q, keep), q the bin of cos(theta), keep False where v is
    NaN."""
    n, dim = d.shape
    j, k = np.triu_indices(n, 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dot = d[j, 0] * d[k, 0]
        for e in range(1, dim):
            dot = dot + d[j, e] * d[k, e]
        c = dot / (s[j] * s[k])
        v = (c + 1.0) * (0.5 * Na)
        keep = ~np.isnan(v)
        vv = np.where(keep, v, 0.0)
        q = np.where(vv < 0.0, 0, np.where(vv >= float(Na), Na - 1, np.minimum(vv, float(Na)).astype(np.int64)))
    return j, k, q.astype(np.int64), keep


def slice_counts(X, Lbox, Nr, rbin, Na):
    """One slice X [Np, dim]: (trip [Nr(Nr+1)/2, Na], pair [Nr], legs per vertex [Np]), int64."""
    Np = X.shape[0]
    P = n_leg_pairs(Nr)
    trip = np.zeros(P * Na, np.int64)
    pair = np.zeros(Nr, np.int64)
    nleg = np.zeros(Np, np.int64)
    for i in range(Np):
        d, s, b = legs(X, i, Lbox, Nr, rbin)
        nleg[i] = len(s)
        pair += np.bincount(b, minlength=Nr)
        if len(s) < 2:
            continue
        j, k, q, keep = angle_bins(d, s, Na)
        lo, hi = np.minimum(b[j], b[k]), np.maximum(b[j], b[k])
        idx = packed_index(lo, hi, Nr) * Na + q
        trip += np.bincount(idx[keep], minlength=P * Na)
    return trip.reshape(P, Na), pair, nleg


class Window:
    """The counts of the window slices Nb-window..Nb+window of every walker of paths [W, M, Np, dim], computed once per
    (walker, grid) and then only added up."""

    def __init__(self, paths, Nb, window, Lbox):
        self.paths, self.Nb, self.window, self.Lbox = paths, Nb, window, Lbox
        self.W = paths.shape[0]
        self._c = {}

    def walker(self, w, Nr, rbin, Na):
        key = (w, Nr, rbin, Na)
        if key not in self._c:
            T, Pr = np.zeros((n_leg_pairs(Nr), Na), np.int64), np.zeros(Nr, np.int64)
            for a in range(self.Nb - self.window, self.Nb + self.window + 1):
                t, p, _ = slice_counts(self.paths[w, a], self.Lbox, Nr, rbin, Na)
                T += t
                Pr += p
            self._c[key] = (T, Pr)
        return self._c[key]

    def expected(self, walkers, Nr, rbin, Na):
        """Accumulated counts for the walker list `walkers` (entries may repeat): dict of trip [W, Nr(Nr+1)/2, Na],
        pair [W, Nr] and samples [W], all int64."""
        T = np.zeros((self.W, n_leg_pairs(Nr), Na), np.int64)
        Pr = np.zeros((self.W, Nr), np.int64)
        cnt = np.zeros(self.W, np.int64)
        for w in walkers:
            t, p = self.walker(w, Nr, rbin, Na)
            T[w] += t
            Pr[w] += p
            cnt[w] += 1
        return {"trip": T, "pair": Pr, "samples": cnt}
