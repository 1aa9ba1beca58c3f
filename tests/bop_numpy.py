"""numpy restatement of the bond-orientational order that pigs_bop_* accumulates (include/pigs_hip.h has the definition).

It shares no formula with the kernel: there are no spherical harmonics here.  By the addition theorem
  q_l(i)^2 = (1/n_i^2) sum_{j,k in nb(i)} P_l(d^_ij . d^_ik)
  Q_l^2    = (1/Np^2) sum_{i,i'} (1/(n_i n_i')) sum_{j in nb(i), k in nb(i')} P_l(d^_ij . d^_i'k)
  c_ii'    = the inner sum of Q_6^2 for one pair of particles
and in 2D P_l(cos gamma) is replaced by cos(n (theta_ij - theta_i'k)).  So a slice is one bond x bond matrix (built in
row chunks), summed over the bonds of a particle on both sides into the particle x particle matrix C_l: its diagonal is
q_l(i)^2, its mean Q_l^2, and C_6 itself is c.

Bonds and radial bins come from grv_numpy's min-image and r2 arithmetic (the same IEEE operations as the device, so the
neighbour sets, n_i and the pair counts GN are exact)."""
import numpy as np

from grv_numpy import folded

CHUNK = 1024                                                           # bond rows per block of the bond x bond matrix


def _p4(x):
    x2 = x * x
    return (35.0 * x2 * x2 - 30.0 * x2 + 3.0) / 8.0


def _p6(x):
    x2 = x * x
    return (231.0 * x2 * x2 * x2 - 315.0 * x2 * x2 + 105.0 * x2 - 5.0) / 16.0


def _kernels(dim):
    """(f4, f6): bond x bond matrix blocks from the bond descriptors (unit vectors in 3D, angles in 2D)."""
    if dim == 3:
        return (lambda a, b: _p4(np.clip(a @ b.T, -1.0, 1.0)), lambda a, b: _p6(np.clip(a @ b.T, -1.0, 1.0)))
    return (lambda a, b: np.cos(4.0 * (a[:, None] - b[None, :])), lambda a, b: np.cos(6.0 * (a[:, None] - b[None, :])))


def _particle_matrix(f, desc, owner, wgt, Np):
    """C[i, i'] = sum over the bonds b of i and b' of i' of wgt_b wgt_b' f(desc_b, desc_b'); bonds sorted by owner."""
    C = np.zeros((Np, Np))
    nb = owner.shape[0]
    if nb == 0:
        return C
    owners, start = np.unique(owner, return_index=True)               # the particles that have bonds, first bond of each
    for b0 in range(0, nb, CHUNK):
        b1 = min(nb, b0 + CHUNK)
        blk = f(desc[b0:b1], desc) * wgt[None, :] * wgt[b0:b1, None]    # [rows of the chunk, all bonds]
        cols = np.add.reduceat(blk, start, axis=1)                    # summed over the bonds of i'
        own, first = np.unique(owner[b0:b1], return_index=True)       # a particle's bonds may span two chunks: +=
        C[np.ix_(own, owners)] += np.add.reduceat(cols, first, axis=0)
    return C


class SliceOrder:
    """One slice X [Np, dim]: n [Np], q4 [Np], q6 [Np] (the local invariants), Q4sq, Q6sq (the slice invariants' squares),
    and for the pairs i < j: r2 and c = C_6[i, j]."""

    def __init__(self, X, Lbox, rnb):
        Np, dim = X.shape
        iu, ju = np.triu_indices(Np, 1)
        d, r2 = folded(X, Lbox)                                        # pairs i < j: d = x(i) - x(j)
        with np.errstate(invalid="ignore"):
            bond = (r2 > 0.0) & (r2 < rnb * rnb)                       # NaN compares false
        # every bond counts for both ends: (i, j) with d and (j, i) with -d
        owner = np.concatenate([iu[bond], ju[bond]])
        vec = np.concatenate([d[bond], -d[bond]])
        order = np.argsort(owner, kind="stable")
        owner, vec = owner[order], vec[order]
        self.n = np.bincount(owner, minlength=Np).astype(np.int64)
        wgt = 1.0 / self.n[owner]
        if dim == 3:
            desc = vec / np.sqrt(np.sum(vec * vec, axis=1))[:, None]
        else:
            desc = np.arctan2(vec[:, 1], vec[:, 0])
        f4, f6 = _kernels(dim)
        C4 = _particle_matrix(f4, desc, owner, wgt, Np)
        C6 = _particle_matrix(f6, desc, owner, wgt, Np)
        self.q4 = np.sqrt(np.maximum(np.diag(C4), 0.0))
        self.q6 = np.sqrt(np.maximum(np.diag(C6), 0.0))
        self.Q4sq = max(float(C4.sum()) / float(Np) ** 2, 0.0)
        self.Q6sq = max(float(C6.sum()) / float(Np) ** 2, 0.0)
        self.r2 = r2
        self.c = C6[iu, ju]

    def radial(self, rcut2, Nr, rbin):
        """(G [Nr], GN [Nr]) of this slice: K7's rule, as grv_numpy.bin_radial."""
        if Nr == 0:
            return np.zeros(0), np.zeros(0, np.int64)
        with np.errstate(invalid="ignore", over="ignore"):
            inside = self.r2 <= rcut2
            u = np.sqrt(self.r2[inside]) / rbin
        keep = u < float(Nr)
        b = u[keep].astype(np.int64)
        G = np.bincount(b, weights=self.c[inside][keep], minlength=Nr)
        return G, np.bincount(b, minlength=Nr).astype(np.int64)


class Window:
    """The slices of paths[W, M, Np, dim], restated on demand and kept (a slice depends on rnb alone)."""

    def __init__(self, paths, Lbox, rcut2, rnb):
        self.paths, self.Lbox, self.rcut2, self.rnb = paths, Lbox, rcut2, rnb
        self._s = {}

    def slice(self, w, a):
        if (w, a) not in self._s:
            self._s[(w, a)] = SliceOrder(self.paths[w, a], self.Lbox, self.rnb)
        return self._s[(w, a)]

    def expected(self, walkers, Nb, window, Nr, rbin):
        """Per walker of paths: S [W, 8], G [W, Nr], GN [W, Nr], samples [W], the local invariants of every slice added
        (q4, q6: lists of arrays per walker) and the slice invariants added (Q4, Q6: lists per walker)."""
        W = self.paths.shape[0]
        Np = self.paths.shape[2]
        out = {"S": np.zeros((W, 8)), "G": np.zeros((W, Nr)), "GN": np.zeros((W, Nr), np.int64),
               "samples": np.zeros(W, np.int64), "q4": [[] for _ in range(W)], "q6": [[] for _ in range(W)],
               "Q4": [[] for _ in range(W)], "Q6": [[] for _ in range(W)]}
        for w in walkers:
            out["samples"][w] += 1
            for a in range(Nb - window, Nb + window + 1):
                s = self.slice(w, a)
                Q4, Q6 = np.sqrt(s.Q4sq), np.sqrt(s.Q6sq)
                out["S"][w] += [Q4, s.Q4sq, Q6, s.Q6sq, s.q4.sum() / Np, s.q6.sum() / Np, float(s.n.sum()), 0.0]
                G, GN = s.radial(self.rcut2, Nr, rbin)
                out["G"][w] += G
                out["GN"][w] += GN
                out["q4"][w].append(s.q4)
                out["q6"][w].append(s.q6)
                out["Q4"][w].append(Q4)
                out["Q6"][w].append(Q6)
        return out


def histogram(q, Nh):
    """The counts of min(int(q Nh), Nh - 1) over the values q >= 0."""
    b = np.minimum((np.asarray(q) * float(Nh)).astype(np.int64), Nh - 1)
    return np.bincount(b, minlength=Nh).astype(np.int64)


# ---- perfect lattices and their closed forms (Steinhardt, Nelson and Ronchetti 1983 for fcc, to the digits quoted)
def _grid(n, a=1.0):
    """n[k] sites per axis at spacing a, centred on the origin; (X, Lbox)."""
    ax = [(np.arange(m) - 0.5 * m + 0.25) * a for m in n]
    X = np.stack(np.meshgrid(*ax, indexing="ij"), axis=-1).reshape(-1, len(n))
    return X, [m * a for m in n] + [1.0] * (3 - len(n))


def sc(n=3):
    return _grid([n] * 3)


def fcc(n=2):
    X, L = _grid([n] * 3)
    basis = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    return (X[:, None, :] + basis[None]).reshape(-1, 3), L


def square(n=4):
    return _grid([n] * 2)


def triangular(nx=4, ny=4):
    """Rows at distance sqrt(3)/2, every other row shifted by half a spacing: box sides nx : sqrt(3)/2 ny (ny even)."""
    h = 0.5 * np.sqrt(3.0)
    X = np.array([[ix + 0.5 * (iy % 2) - 0.5 * nx + 0.125, (iy - 0.5 * ny + 0.25) * h] for iy in range(ny) for ix in range(nx)])
    return X, [float(nx), ny * h, 1.0]


LATTICES = {            # name: (builder, rnb, Q4, Q6, digits known)
    "sc": (sc, 1.2, np.sqrt(7.0 / 12.0), np.sqrt(1.0 / 8.0), 1e-13),
    "fcc": (fcc, 0.85, 0.19094, 0.57452, 5e-6),
    "square": (square, 1.2, 1.0, 0.0, 1e-13),
    "triangular": (triangular, 1.3, None, 1.0, 1e-13),
}
COORDINATION = {"sc": 6, "fcc": 12, "square": 4, "triangular": 6}
