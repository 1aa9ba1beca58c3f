"""numpy restatement of what pigs_nk_* accumulates (include/pigs_hip.h has the definition), written from the definition and
not from the kernel: the end-to-end vector x = head - tail folded once per coordinate by two compares against LboxHalf,
then, per sample,
    C[iq]   += cos(k_iq . x), k = 2 pi n / Lbox, a straight np.cos of the dot product (no phasor tables, no recurrences)
    H[flat] += 1 on the Cartesian grid of the minimum-image cell, t_k = (x_k + LboxHalf_k)/(Lbox_k/nbin), decided in double
    nopen   += 1;    ninside += 1 iff r2 <= rcut2 with r2 the squares summed left to right
The counts have the device's bits; the cosine sums differ from the device's by the rounding of the phase and the order, so
they are compared within 1e-12 per unit-modulus term."""
import numpy as np


def half_space(dim, nmax):
    """The vectors of pigs_sqv_vectors: |n_k| <= nmax, ascending lexicographic order (n_1 slowest), those after n = 0."""
    S = 2 * nmax + 1
    ranks = np.arange(S ** dim)
    n = np.zeros((S ** dim, dim), np.int64)
    r = ranks.copy()
    for k in range(dim - 1, -1, -1):
        n[:, k] = r % S - nmax
        r //= S
    zero = (S ** dim - 1) // 2
    return n[zero + 1:]


def fold(xend, Lbox):
    """xend [ns, 2, dim] (head, tail) -> the once-folded differences [ns, dim], as the OBDM histogram folds them."""
    xend = np.asarray(xend, np.float64)
    dim = xend.shape[-1]
    L = np.asarray(Lbox, np.float64)[:dim]
    Lh = 0.5 * L
    v = xend[:, 0, :] - xend[:, 1, :]
    v = np.where(v > Lh, v - L, v)
    v = np.where(v < -Lh, v + L, v)
    return v


def cos_sums(x, n, Lbox):
    """C [Nq] of the folded samples x [ns, dim] on the vectors n [Nq, dim]."""
    x = np.asarray(x, np.float64)
    dim = x.shape[-1]
    kvec = 2.0 * np.pi * np.asarray(n, np.float64) / np.asarray(Lbox, np.float64)[:dim]
    if x.shape[0] == 0:
        return np.zeros(len(n))
    return np.cos(x @ kvec.T).sum(axis=0)


def grid_counts(x, Lbox, nbin):
    """H [nbin, ..dim times] (array axis -1-k is axis k of the box: x fastest in memory) of the folded samples."""
    x = np.asarray(x, np.float64)
    dim = x.shape[-1]
    L = np.asarray(Lbox, np.float64)[:dim]
    Lh = 0.5 * L
    b = L / float(nbin)
    H = np.zeros(nbin ** dim, np.int64)
    for s in range(x.shape[0]):
        flat, stride, inside = 0, 1, True
        for k in range(dim):
            t = (x[s, k] + Lh[k]) / b[k]
            if t >= 0.0 and t < float(nbin):
                flat += int(t) * stride
            else:
                inside = False
            stride *= nbin
        if inside:
            H[flat] += 1
    return H.reshape((nbin,) * dim)


def inside_count(x, rcut2):
    """The samples with r2 <= rcut2, r2 summed left to right."""
    x = np.asarray(x, np.float64)
    r2 = np.zeros(x.shape[0])
    for k in range(x.shape[1]):
        r2 = r2 + x[:, k] * x[:, k]
    return int(np.count_nonzero(r2 <= rcut2))


def sums(xend, Lbox, nmax, nbin, rcut2):
    """One walker's samples xend [ns, 2, dim]: the dict of one walker's slice of nk_read."""
    xend = np.asarray(xend, np.float64)
    dim = xend.shape[-1]
    x = fold(xend, Lbox) if xend.shape[0] else np.zeros((0, dim))
    return {"C": cos_sums(x, half_space(dim, nmax), Lbox), "H": grid_counts(x, Lbox, nbin), "nopen": x.shape[0],
            "ninside": inside_count(x, rcut2)}
