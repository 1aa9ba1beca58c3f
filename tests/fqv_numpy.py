"""Numpy restatement of F(q,tau) on the full reciprocal grid, as pigs_fqv_* accumulate it (include/pigs_hip.h).

The vectors and rho_q = C + i S are those of sqv_numpy (the FULL phase per (vector, particle), nothing factorised, so
the check does not share the kernel's algebra); the loop over the lags and pairs is that of fqt_numpy.fqt_sums.  One
accumulate call adds, for the lags l = 0..Ntau,
    acc[l][iqv] += sum over a = Nb-W .. Nb+W-l (ascending) of C(a)*C(a+l) + S(a)*S(a+l)
and the estimator is acc / (samples * n_pairs(l) * Np) with n_pairs(l) = 2W + 1 - l.
"""
import numpy as np

from sqv_numpy import n_vectors, rho, vectors  # noqa: F401  (re-exported: one enumeration)


def n_pairs(window, Ntau):
    return 2 * window + 1 - np.arange(Ntau + 1)


def correlate(C, S, Ntau, Np):
    """(acc, bound) [Ntau+1, ...] from C, S [ns, ...]: fqt_numpy.fqt_sums' loop over (l, a).
    bound = 1e-12 * sum over the pairs of (|rho(a)|*|rho(a+l)| + Np): the project's S(k) bound, applied per pair."""
    mod = np.sqrt(C * C + S * S)
    ns = C.shape[0]
    acc = np.zeros((Ntau + 1,) + C.shape[1:])
    bound = np.zeros_like(acc)
    for l in range(Ntau + 1):
        for a in range(ns - l):
            acc[l] = acc[l] + (C[a] * C[a + l] + S[a] * S[a + l])
            bound[l] = bound[l] + (mod[a] * mod[a + l] + Np)
    return acc, 1e-12 * bound


def fqv_sums(path, Nb, window, Ntau, n, Lbox):
    """Raw sums of ONE accumulate call for one walker's path[M, Np, dim]: (acc, bound), both [Ntau+1, Nq]."""
    C, S = rho(path[Nb - window:Nb + window + 1], n, Lbox)            # [ns, Nq]
    return correlate(C, S, Ntau, path.shape[1])


def expected(paths, walkers, Nb, window, Ntau, n, Lbox):
    """Accumulated raw sums, bounds and samples for the walker list `walkers` (entries may repeat) over
    paths[W, M, Np, dim]."""
    W = paths.shape[0]
    F = np.zeros((W, Ntau + 1, n.shape[0]))
    B = np.zeros_like(F)
    cnt = np.zeros(W, np.int64)
    cache = {}
    for w in walkers:
        if w not in cache:
            cache[w] = fqv_sums(paths[w], Nb, window, Ntau, n, Lbox)
        F[w] = F[w] + cache[w][0]
        B[w] = B[w] + cache[w][1]
        cnt[w] += 1
    return F, B, cnt
