"""Numpy restatement of the vector structure factor that pigs_sqv_* accumulate (include/pigs_hip.h).

Vectors: the integers n = (n_1..n_dim), |n_k| <= nmax, whose first non-zero component is positive, in ascending
lexicographic order (n_1 slowest): Nq = ((2*nmax + 1)**dim - 1)/2 of them.  For each the FULL phase
    phase(i) = sum_k real(n_k) * qbin_k * x_k(i),   qbin_k = 2*pi/Lbox[k]
is formed per (vector, particle) and cos/sin are called on it: nothing is factorised here, so the check does not share
the kernel's algebra.  One accumulate call adds
    acc[iqv] += sum over a = Nb-W .. Nb+W (ascending) of C(a)**2 + S(a)**2
and the estimator is acc / (samples * (2W + 1) * Np).
"""
import itertools

import numpy as np


def vectors(dim, nmax):
    """[Nq, dim] int32: the half space in ascending lexicographic order."""
    r = range(-nmax, nmax + 1)
    zero = (0,) * dim
    return np.array([n for n in itertools.product(r, repeat=dim) if n > zero], np.int32).reshape(-1, dim)


def n_vectors(dim, nmax):
    return ((2 * nmax + 1) ** dim - 1) // 2


def rho(slices, n, Lbox, chunk=512):
    """C, S of slices[..., Np, dim] at the vectors n[Nq, dim]: arrays [..., Nq]."""
    slices = np.asarray(slices, np.float64)
    dim = slices.shape[-1]
    qbin = 2.0 * np.pi / np.asarray(Lbox, np.float64)[:dim]            # vpi.f90:119
    nf = np.asarray(n).astype(np.float32).astype(np.float64)
    C = np.zeros(slices.shape[:-2] + (n.shape[0],))
    S = np.zeros_like(C)
    with np.errstate(invalid="ignore"):
        for v0 in range(0, n.shape[0], chunk):
            v = nf[v0:v0 + chunk]
            ph = np.zeros(slices.shape[:-1] + (v.shape[0],))          # [..., Np, nv]
            for k in range(dim):
                ph = ph + (v[:, k] * qbin[k]) * slices[..., k, None]
            C[..., v0:v0 + chunk] = np.cos(ph).sum(axis=-2)
            S[..., v0:v0 + chunk] = np.sin(ph).sum(axis=-2)
    return C, S


def sqv_sums(path, Nb, window, n, Lbox):
    """Raw sums of ONE accumulate call for one walker's path[M, Np, dim]: (acc, bound), both [Nq].
    bound = 1e-12 * sum over the window slices of (|rho_q(a)|^2 + Np): the S(k) bound 1e-12*(|want| + Np) of
    test_gpu_parity.py::test_structure_estimators_vs_oracle, applied per slice."""
    Np = path.shape[1]
    C, S = rho(path[Nb - window:Nb + window + 1], n, Lbox)            # [ns, Nq]
    mod2 = C * C + S * S
    acc = np.zeros(n.shape[0])
    bound = np.zeros(n.shape[0])
    for a in range(mod2.shape[0]):
        acc = acc + mod2[a]
        bound = bound + (mod2[a] + Np)
    return acc, 1e-12 * bound


def expected(paths, walkers, Nb, window, n, Lbox):
    """Accumulated raw sums, bounds and samples for the walker list `walkers` (entries may repeat) over
    paths[W, M, Np, dim]."""
    W = paths.shape[0]
    A = np.zeros((W, n.shape[0]))
    B = np.zeros_like(A)
    cnt = np.zeros(W, np.int64)
    cache = {}
    for w in walkers:
        if w not in cache:
            cache[w] = sqv_sums(paths[w], Nb, window, n, Lbox)
        A[w] = A[w] + cache[w][0]
        B[w] = B[w] + cache[w][1]
        cnt[w] += 1
    return A, B, cnt
