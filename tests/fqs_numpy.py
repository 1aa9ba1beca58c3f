"""Numpy restatement of the self part of F(q,tau) and the imaginary-time displacement, as pigs_fqs_* accumulate them
(include/pigs_hip.h).

The vectors are those of sqv_numpy.  The FULL phase sum_k real(n_k) * qbin_k * x_k(i, a) is formed per (vector,
particle, slice) and cos/sin are called on it: nothing is factorised, so the check does not share the kernel's algebra.
The loop over the lags and pairs is that of fqv_numpy.correlate.  One accumulate call adds, for l = 0..Ntau,
    F[l][iqv] += sum over a = Nb-W .. Nb+W-l and the particles i of c_i(a)*c_i(a+l) + s_i(a)*s_i(a+l)
    D[l][0]   += sum over a, i of r2,   D[l][1] += sum over a, i of r2*r2
with r2 the squared length of x_i(a+l) - x_i(a) folded once by the two compares of pbc_mod.f90:40-41.

Bounds per element and call:
    F: 1e-12 * n_pairs(l) * Np -- the `+ Np` term of the project's S(k) bound per slice pair; every particle term has
       modulus 1.
    D: 1e-12 * the sum of the terms -- the terms are the kernel's own bits and only the summation order differs; a
       sequential sum of n positive terms errs by at most n * 2^-53 of the sum, so callers keep Np*(2W+1) <= 4000.
"""
import numpy as np

from sqv_numpy import n_vectors, vectors  # noqa: F401  (re-exported: one enumeration)


def n_pairs(window, Ntau):
    return 2 * window + 1 - np.arange(Ntau + 1)


def phasors(slices, n, Lbox):
    """c, s [ns, Np, Nq] of slices[ns, Np, dim] at the vectors n[Nq, dim], from the full phase."""
    slices = np.asarray(slices, np.float64)
    dim = slices.shape[-1]
    qbin = 2.0 * np.pi / np.asarray(Lbox, np.float64)[:dim]            # vpi.f90:119
    nf = np.asarray(n).astype(np.float32).astype(np.float64)
    ph = np.zeros(slices.shape[:-1] + (nf.shape[0],))
    for k in range(dim):
        ph = ph + (nf[:, k] * qbin[k]) * slices[..., k, None]
    return np.cos(ph), np.sin(ph)


def fold(d, L):
    """The two compares of pbc_mod.f90:40-41, one fold."""
    d = np.where(d > 0.5 * L, d - L, d)
    return np.where(d < -0.5 * L, d + L, d)


def fqs_sums(path, Nb, window, Ntau, n, Lbox):
    """Raw sums of ONE accumulate call for one walker's path[M, Np, dim]: (F, Fbound) [Ntau+1, Nq] and (D, Dbound)
    [Ntau+1, 2]."""
    x = np.asarray(path, np.float64)[Nb - window:Nb + window + 1]      # [ns, Np, dim]
    ns, Np, dim = x.shape
    L = np.asarray(Lbox, np.float64)[:dim]
    c, s = phasors(x, n, Lbox)
    F = np.zeros((Ntau + 1, n.shape[0]))
    D = np.zeros((Ntau + 1, 2))
    for l in range(Ntau + 1):
        for a in range(ns - l):
            F[l] = F[l] + (c[a] * c[a + l] + s[a] * s[a + l]).sum(axis=0)
            d = fold(x[a + l] - x[a], L)
            r2 = np.zeros(Np)
            for k in range(dim):
                r2 = r2 + d[:, k] * d[:, k]
            D[l, 0] = D[l, 0] + r2.sum()
            D[l, 1] = D[l, 1] + (r2 * r2).sum()
    Fb = 1e-12 * (n_pairs(window, Ntau) * float(Np))[:, None] * np.ones((1, n.shape[0]))
    return F, Fb, D, 1e-12 * D


def expected(paths, walkers, Nb, window, Ntau, n, Lbox):
    """Accumulated raw sums, bounds and samples for the walker list `walkers` (entries may repeat) over
    paths[W, M, Np, dim]: a dict F, Fb [W, Ntau+1, Nq], D, Db [W, Ntau+1, 2], samples [W]."""
    W = paths.shape[0]
    out = {"F": np.zeros((W, Ntau + 1, n.shape[0])), "D": np.zeros((W, Ntau + 1, 2)), "samples": np.zeros(W, np.int64)}
    out["Fb"], out["Db"] = np.zeros_like(out["F"]), np.zeros_like(out["D"])
    cache = {}
    for w in walkers:
        if w not in cache:
            cache[w] = fqs_sums(paths[w], Nb, window, Ntau, n, Lbox)
        for key, val in zip(("F", "Fb", "D", "Db"), cache[w]):
            out[key][w] = out[key][w] + val
        out["samples"][w] += 1
    return out
