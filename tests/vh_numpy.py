"""numpy restatement of the van Hove histograms that pigs_vh_* accumulates (include/pigs_hip.h has the definition), with
the same IEEE operations in the same order: d_k = x_k(i, a+l) - x_k(j, a), one fold per coordinate by two compares against
LboxHalf, r2 summed left to right, u = sqrt(r2)/bin decided in double before any conversion.  All integer counts: every
comparison with the device is exact.

The folded r2 of a window depend on neither grid, so `Window` computes them once per (walker, lag) and bins them per
request."""
import numpy as np


def n_pairs(window, Ntau):
    """Slice pairs (a, a+l) of the window per lag l = 0..Ntau."""
    return 2 * window + 1 - np.arange(Ntau + 1)


def r2_matrix(Xl, Xa, Lbox):
    """Xl, Xa: slices a+l and a, [Np, dim].  r2[i, j] of d = x(i, a+l) - x(j, a), folded once."""
    Np, dim = Xa.shape
    L = np.asarray(Lbox, np.float64)[:dim]
    Lh = 0.5 * L                                                      # vpi.f90:118
    with np.errstate(invalid="ignore", over="ignore"):
        d = Xl[:, None, :] - Xa[None, :, :]
        d = np.where(d > Lh, d - L, d)                                # pbc_mod.f90:40
        d = np.where(d < -Lh, d + L, d)                               # pbc_mod.f90:41
        r2 = np.zeros((Np, Np))
        for k in range(dim):
            r2 = r2 + d[:, :, k] * d[:, :, k]
    return r2


def bin_distinct(r2, rcut2, Nr, rbin):
    """r2: the off-diagonal elements.  K7's radial rule: r2 <= rcut2, u = sqrt(r2)/rbin < Nr, bin int(u)."""
    with np.errstate(invalid="ignore", over="ignore"):
        inside = r2 <= rcut2                                          # NaN compares false: decided in double
        u = np.sqrt(r2[inside]) / rbin
    u = u[u < float(Nr)]
    return np.bincount(u.astype(np.int64), minlength=Nr).astype(np.int64)


def bin_self(r2, Ns, sbin):
    """r2: the diagonal elements.  u = sqrt(r2)/sbin < Ns, bin int(u); no cutoff."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.sqrt(r2) / sbin
        u = u[u < float(Ns)]                                          # NaN and Inf compare false
    return np.bincount(u.astype(np.int64), minlength=Ns).astype(np.int64)


class Window:
    """r2 of every slice pair (a, a+l), a = Nb-window .. Nb+window-l, l = 0..Ntau, of every walker of
    paths[W, M, Np, dim]: per (walker, lag) the off-diagonal and the diagonal elements."""

    def __init__(self, paths, Nb, window, Ntau, Lbox, rcut2):
        self.W, self.Np = paths.shape[0], paths.shape[2]
        self.window, self.Ntau, self.rcut2 = window, Ntau, rcut2
        off = ~np.eye(self.Np, dtype=bool)
        self.dist, self.self = {}, {}
        for w in range(self.W):
            for l in range(Ntau + 1):
                m = [r2_matrix(paths[w, a + l], paths[w, a], Lbox) for a in range(Nb - window, Nb + window - l + 1)]
                self.dist[(w, l)] = np.concatenate([x[off] for x in m])
                self.self[(w, l)] = np.concatenate([np.diagonal(x) for x in m])
        self._bins = {}                                               # per (walker, grids): binned once

    def expected(self, walkers, Nr, rbin, Ns, sbin):
        """Accumulated counts for the walker list `walkers` (entries may repeat): dict of self [W, Ntau+1, Ns],
        distinct [W, Ntau+1, Nr] and samples [W], all int64."""
        S = np.zeros((self.W, self.Ntau + 1, Ns), np.int64)
        D = np.zeros((self.W, self.Ntau + 1, Nr), np.int64)
        cnt = np.zeros(self.W, np.int64)
        for w in walkers:
            key = (w, Nr, rbin, Ns, sbin)
            if key not in self._bins:
                self._bins[key] = (np.stack([bin_self(self.self[(w, l)], Ns, sbin) for l in range(self.Ntau + 1)]),
                                   np.stack([bin_distinct(self.dist[(w, l)], self.rcut2, Nr, rbin) for l in range(self.Ntau + 1)]))
            S[w] += self._bins[key][0]
            D[w] += self._bins[key][1]
            cnt[w] += 1
        return {"self": S, "distinct": D, "samples": cnt}


def expected(paths, walkers, Nb, window, Ntau, Lbox, rcut2, Nr, rbin, Ns, sbin):
    return Window(paths, Nb, window, Ntau, Lbox, rcut2).expected(walkers, Nr, rbin, Ns, sbin)
