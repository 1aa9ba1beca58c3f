"""Numpy restatement of the imaginary-time density correlations that pigs_fqt_* accumulate (include/pigs_hip.h).

For axis k and harmonic iq = 1..Nk: q = real(iq) * (2*pi/Lbox[k]), phase = q * x_k(i, s),
C(s) = sum_i cos(phase), S(s) = sum_i sin(phase).  One accumulate call adds, for the lags l = 0..Ntau,
    acc[l][iq][k] += sum over a = Nb-W .. Nb+W-l (ascending) of C(a)*C(a+l) + S(a)*S(a+l)
and the estimator is acc / (samples * n_pairs(l) * Np) with n_pairs(l) = 2W + 1 - l.
"""
import numpy as np


def rho(slices, Nk, Lbox):
    """C, S of slices[..., Np, dim]: arrays [..., Nk, dim]."""
    slices = np.asarray(slices, np.float64)
    dim = slices.shape[-1]
    L = np.asarray(Lbox, np.float64)[:dim]
    qbin = 2.0 * np.pi / L                                             # vpi.f90:119
    q = np.arange(1, Nk + 1).astype(np.float32).astype(np.float64)[:, None] * qbin[None, :]      # [Nk, dim]
    with np.errstate(invalid="ignore"):
        ph = q * slices[..., :, None, :]                               # [..., Np, Nk, dim]
        return np.cos(ph).sum(axis=-3), np.sin(ph).sum(axis=-3)


def n_pairs(window, Ntau):
    return 2 * window + 1 - np.arange(Ntau + 1)


def fqt_sums(path, Nb, window, Ntau, Nk, Lbox):
    """Raw sums of ONE accumulate call for one walker's path[M, Np, dim]: (acc, bound), both [Ntau+1, Nk, dim].
    bound = 1e-12 * sum over the pairs of (|rho(a)|*|rho(a+l)| + Np): the S(k) bound 1e-12*(|want| + Np) of
    test_gpu_parity.py::test_structure_estimators_vs_oracle, applied per pair."""
    Np = path.shape[1]
    C, S = rho(path[Nb - window:Nb + window + 1], Nk, Lbox)            # [ns, Nk, dim]
    mod = np.sqrt(C * C + S * S)
    ns = 2 * window + 1
    acc = np.zeros((Ntau + 1,) + C.shape[1:])
    bound = np.zeros_like(acc)
    for l in range(Ntau + 1):
        for a in range(ns - l):
            acc[l] = acc[l] + (C[a] * C[a + l] + S[a] * S[a + l])
            bound[l] = bound[l] + (mod[a] * mod[a + l] + Np)
    return acc, 1e-12 * bound


def expected(paths, walkers, Nb, window, Ntau, Nk, Lbox):
    """Accumulated raw sums, bounds and samples for the walker list `walkers` (entries may repeat) over
    paths[W, M, Np, dim]."""
    W = paths.shape[0]
    dim = paths.shape[-1]
    F = np.zeros((W, Ntau + 1, Nk, dim))
    B = np.zeros_like(F)
    n = np.zeros(W, np.int64)
    cache = {}
    for w in walkers:
        if w not in cache:
            cache[w] = fqt_sums(paths[w], Nb, window, Ntau, Nk, Lbox)
        F[w] = F[w] + cache[w][0]
        B[w] = B[w] + cache[w][1]
        n[w] += 1
    return F, B, n
