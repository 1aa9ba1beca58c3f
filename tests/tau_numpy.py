"""Numpy restatement of the four per-slice sums that pigs_tau_* accumulate (include/pigs_hip.h), in the reference's plain
arithmetic: Interpolate opt 0 / opt 1 (interpolate.f90:13-28), the single fold of MinimumImage (pbc_mod.f90:40-49), the
cutoff of PotentialEnergy (sample_mod.f90:98) and of ThermEnergy's link term (sample_mod.f90:377, quirk Q8), TrapPot
(system_mod.f90:238-252).  Per slice b of one worldline path[M, Np, dim]:
    Q[b][0] Vpair = sum_{i<j} v(r_ij)            Q[b][1] Vext = sum_i sum_k 0.5 x_k(i)^2 / a_ho(k)^4   (trap; else 0)
    Q[b][2] W     = sum_{i<j} r_ij v'(r_ij)      Q[b][3] D2   = sum_i |x_i(b) - x_i(b+1)|^2            (0 for b = 2Nb)
and, per element, the sum of the terms' absolute values (the scale of the summation error).
"""
import numpy as np


def interpolate(opt, N, dx, F, x):
    """interpolate.f90 for arrays of arguments x >= 0.  The cell index is clamped to the table exactly where the
    library and the oracle clamp it (ix <= N; F(ix-2) not below F(0)): an identity wherever the reference is defined."""
    F = np.asarray(F, np.float64)
    x = np.asarray(x, np.float64)
    ix = (x / dx).astype(np.int64) + 1                                 # :13
    a1 = x - (ix - 1).astype(np.float64) * dx                          # :14
    a2 = dx - a1                                                       # :15
    ix = np.minimum(ix, N)
    if opt == 0:
        return (a1 * F[ix] + a2 * F[ix - 1]) / dx                      # :21
    before = (a1 * F[ix - 1] + a2 * F[np.maximum(ix - 2, 0)]) / dx     # :25
    after = (a1 * F[ix + 1] + a2 * F[ix]) / dx                         # :26
    return 0.5 * (after - before) / dx                                 # :28


def fold(d, Lbox):
    """pbc_mod.f90:40-41 on d[..., dim]: one fold per coordinate, each compare against Lbox/2."""
    L = np.asarray(Lbox, np.float64)[:d.shape[-1]]
    h = 0.5 * L
    d = np.where(d > h, d - L, d)
    return np.where(d < -h, d + L, d)


def r2_of(d):
    """Sum of the squares, left to right (the reference's loop)."""
    r2 = np.zeros(d.shape[:-1])
    for k in range(d.shape[-1]):
        r2 = r2 + d[..., k] * d[..., k]
    return r2


def tau_sums(path, VT, S):
    """One accumulate call for one worldline path[M, Np, dim] of the system S (dim, Np, Nmax, dr, rcut2, Lbox, trap,
    a_ho: an oracle.pyoracle.System or a SystemConfig).  Returns (Q, A, n): Q [M, 4] the sums, A [M, 4] the sums of the
    terms' absolute values, n [M, 2] the numbers of counted pairs and links."""
    path = np.asarray(path, np.float64)
    M, Np, dim = path.shape
    Q, A, n = np.zeros((M, 4)), np.zeros((M, 4)), np.zeros((M, 2), np.int64)
    iu, ju = np.triu_indices(Np, 1)
    with np.errstate(all="ignore"):
        for b in range(M):
            R = path[b]
            d = R[iu] - R[ju]
            if S.trap:
                r2 = r2_of(d)
                keep = np.ones(r2.shape, bool)
            else:
                r2 = r2_of(fold(d, S.Lbox))
                keep = r2 <= S.rcut2
            r = np.sqrt(r2[keep])
            v = interpolate(0, S.Nmax, S.dr, VT, r)
            w = r * interpolate(1, S.Nmax, S.dr, VT, r)
            Q[b, 0], A[b, 0] = v.sum(), np.abs(v).sum()
            Q[b, 2], A[b, 2] = w.sum(), np.abs(w).sum()
            n[b, 0] = int(keep.sum())
            if S.trap:
                ext = 0.0
                for k in range(dim):
                    a = float(S.a_ho[k])
                    a4 = a * a * a * a
                    ext = ext + (0.5 * (R[:, k] * R[:, k]) / a4).sum()
                Q[b, 1] = A[b, 1] = ext
            if b + 1 < M:
                d = R - path[b + 1]
                if S.trap:
                    l2 = r2_of(d)
                else:
                    l2 = r2_of(fold(d, S.Lbox))
                    l2 = l2[l2 <= S.rcut2]
                Q[b, 3] = A[b, 3] = l2.sum()
                n[b, 1] = l2.size
    return Q, A, n


def expected(paths, walkers, VT, S):
    """Accumulated raw sums Q [W, M, 4], the sums of absolute terms A and the samples for the walker list `walkers`
    (entries may repeat) over paths[W, M, Np, dim]."""
    W, M = paths.shape[:2]
    Q, A = np.zeros((W, M, 4)), np.zeros((W, M, 4))
    n = np.zeros(W, np.int64)
    cache = {}
    for w in walkers:
        if w not in cache:
            cache[w] = tau_sums(paths[w], VT, S)
        Q[w] = Q[w] + cache[w][0]
        A[w] = A[w] + cache[w][1]
        n[w] += 1
    return Q, A, n


# ---- the test inputs: jittered lattices, not uniform random points (which come within dr of each other in 1D) --------
def lattice_paths(S, W, rng):
    """Periodic: sites of an n^dim grid (n = ceil(Np^(1/dim)), spacing a = L/n), every bead with its own uniform jitter
    of +-0.1 a per coordinate, wrapped into [-L/2, L/2).  Pair distances are >= 0.65 a: the table's head is never read."""
    dim, Np, M = S.dim, S.Np, 2 * S.Nb + 1
    n = int(np.ceil(Np ** (1.0 / dim) - 1e-9))
    L = np.asarray(S.Lbox[:dim], float)
    a = L / n
    idx = np.stack(np.unravel_index(np.arange(Np), (n,) * dim), axis=1).astype(float)
    P = (idx[None, None] + 0.5 + rng.uniform(-0.1, 0.1, (W, M, Np, dim))) * a - 0.5 * L
    return P - L * np.floor((P + 0.5 * L) / L)


def trap_paths(S, W, rng):
    """Trapped: a grid of spacing s around the origin with jitter +-0.1 s, small enough for every pair distance to stay
    below rcut - 2 dr (no table clamp)."""
    dim, Np, M = S.dim, S.Np, 2 * S.Nb + 1
    n = int(np.ceil(Np ** (1.0 / dim) - 1e-9))
    s = 0.9 * (S.rcut - 2.0 * S.dr) / ((n - 0.8) * np.sqrt(dim))
    idx = np.stack(np.unravel_index(np.arange(Np), (n,) * dim), axis=1).astype(float)
    return (idx[None, None] - 0.5 * (n - 1) + rng.uniform(-0.1, 0.1, (W, M, Np, dim))) * s


def min_max_distance(P, S):
    """Smallest and largest pair distance over all slices of P[W, M, Np, dim] (folded for a periodic system)."""
    iu, ju = np.triu_indices(S.Np, 1)
    d = P[:, :, iu] - P[:, :, ju]
    r = np.sqrt(r2_of(d if S.trap else fold(d, S.Lbox)))
    return float(r.min()), float(r.max())
