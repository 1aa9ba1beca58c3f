"""numpy restatement of the pair distribution that pigs_grv_* accumulates (include/pigs_hip.h has the definition), with
the same IEEE operations in the same order: one fold per coordinate by two compares against LboxHalf, r2 summed left to
right, t_k = (d_k + LboxHalf[k]) / b_k decided in double before any conversion.  All integer counts: every comparison
with the device is exact.

The folded displacements of a window depend on neither grid, so `Window` computes them once and bins them per request."""
import numpy as np


def folded(X, Lbox):
    """X: one slice [Np, dim].  (d [pairs, dim], r2 [pairs]) of the pairs i < j: d = x(i) - x(j) folded once."""
    Np, dim = X.shape
    L = np.asarray(Lbox, np.float64)[:dim]
    Lh = 0.5 * L                                                      # vpi.f90:118
    i, j = np.triu_indices(Np, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        d = X[i] - X[j]
        d = np.where(d > Lh, d - L, d)                                # pbc_mod.f90:40
        d = np.where(d < -Lh, d + L, d)                               # pbc_mod.f90:41
        r2 = np.zeros(d.shape[0])
        for k in range(dim):
            r2 = r2 + d[:, k] * d[:, k]
    return d, r2


def bin_vector(d, Lbox, Nbin):
    """(vec [Nbin]*dim int64 with x on the LAST axis, pairs dropped)."""
    dim = d.shape[1]
    L = np.asarray(Lbox, np.float64)[:dim]
    Lh = 0.5 * L
    b = L / float(Nbin)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (d + Lh) / b
        keep = np.all((t >= 0.0) & (t < float(Nbin)), axis=1)         # NaN compares false: decided in double
    jj = t[keep].astype(np.int64)
    flat = np.zeros(jj.shape[0], np.int64)
    for k in range(dim):
        flat += jj[:, k] * Nbin ** k                                  # x fastest
    vec = np.bincount(flat, minlength=Nbin ** dim).astype(np.int64).reshape((Nbin,) * dim)
    return vec, int(d.shape[0] - keep.sum())


def bin_radial(r2, rcut2, Nr, rbin):
    with np.errstate(invalid="ignore", over="ignore"):
        inside = r2 <= rcut2
        u = np.sqrt(r2[inside]) / rbin
    u = u[u < float(Nr)]
    return np.bincount(u.astype(np.int64), minlength=Nr).astype(np.int64)


class Window:
    """The folded displacements of the slices Nb-window..Nb+window of every walker of paths[W, M, Np, dim]."""

    def __init__(self, paths, Nb, window, Lbox, rcut2):
        self.W, self.dim = paths.shape[0], paths.shape[3]
        self.Lbox, self.rcut2 = Lbox, rcut2
        self.d, self.r2 = [], []
        for w in range(self.W):
            parts = [folded(paths[w, a], Lbox) for a in range(Nb - window, Nb + window + 1)]
            self.d.append(np.concatenate([p[0] for p in parts]))
            self.r2.append(np.concatenate([p[1] for p in parts]))
        self._vec, self._rad = {}, {}                                 # per (walker, grid): binned once

    def expected(self, walkers, Nbin, Nr, rbin):
        """Accumulated counts for the walker list `walkers` (entries may repeat): vec [W, Nbin..], radial [W, Nr],
        samples [W], and the pairs that the vector grid dropped (summed over the list)."""
        V = np.zeros((self.W,) + (Nbin,) * self.dim, np.int64)
        R = np.zeros((self.W, Nr), np.int64)
        cnt = np.zeros(self.W, np.int64)
        dropped = 0
        for w in walkers:
            if (w, Nbin) not in self._vec:
                self._vec[(w, Nbin)] = bin_vector(self.d[w], self.Lbox, Nbin)
            if (w, Nr, rbin) not in self._rad:
                self._rad[(w, Nr, rbin)] = bin_radial(self.r2[w], self.rcut2, Nr, rbin)
            V[w] += self._vec[(w, Nbin)][0]
            R[w] += self._rad[(w, Nr, rbin)]
            dropped += self._vec[(w, Nbin)][1]
            cnt[w] += 1
        return V, R, cnt, dropped


def expected(paths, walkers, Nb, window, Lbox, rcut2, Nbin, Nr, rbin):
    return Window(paths, Nb, window, Lbox, rcut2).expected(walkers, Nbin, Nr, rbin)
