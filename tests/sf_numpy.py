"""numpy restatement of the sums that pigs_sf_* accumulates (include/pigs_hip.h has the definition), with the same IEEE
operations in the same order: a link d = x(a+1) - x(a) folded once by two compares against LboxHalf; the unfolded path
U by a sequential cumsum from 0.0; the link sum over the particles in the kernel's order (lane_sum: 256 lanes, lane j takes
the particles j, j + 256, .. ascending from 0.0, the butterfly v = v + v[idx ^ m] per wave of 64 for m = 32 .. 1, the
four waves in wave order from 0.0); W by a sequential cumsum; C by one running sum over a; D by a running sum per lane over
(particle ascending, a ascending), then lane_sum's butterfly and waves.  C and D of ONE call have the device's bits; a
second call adds a second value to the accumulator."""
import numpy as np

LANES, WAVE = 256, 64


def fold(d, Lbox):
    """The two compares of min_image, and the number of components on which one fired."""
    L = np.asarray(Lbox, np.float64)[:d.shape[-1]]
    Lh = 0.5 * L
    with np.errstate(invalid="ignore"):
        up, dn = d > Lh, d < -Lh
        f = np.where(up, d - L, d)
        f = np.where(f < -Lh, f + L, f)
    return f, int(up.sum() + dn.sum())


def butterfly(lanes):
    """lanes [.., 256]: the wave_sum of every wave of 64 (lane 0's value), then the waves in wave order from 0.0."""
    v = lanes.reshape(lanes.shape[:-1] + (LANES // WAVE, WAVE))
    idx = np.arange(WAVE)
    m = WAVE // 2
    with np.errstate(invalid="ignore", over="ignore"):
        while m >= 1:
            v = v + v[..., idx ^ m]
            m //= 2
        tot = np.zeros(lanes.shape[:-1])
        for g in range(LANES // WAVE):
            tot = tot + v[..., g, 0]
    return tot


def lane_sum(x):
    """x [.., Np] -> [..]: lane j adds x[j], x[j + 256], .. from 0.0, then butterfly."""
    Np = x.shape[-1]
    rounds = -(-Np // LANES)
    pad = np.zeros(x.shape[:-1] + (rounds * LANES,))
    pad[..., :Np] = x
    lanes = np.zeros(x.shape[:-1] + (LANES,))
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(rounds):
            lanes = lanes + pad[..., r * LANES:(r + 1) * LANES]
    return butterfly(lanes)


def unfold(X, Lbox):
    """X [ns, Np, dim], the window slices of one walker -> d [ns-1, Np, dim], U [ns, Np, dim], W [ns, dim], nwrap."""
    ns, Np, dim = X.shape
    with np.errstate(invalid="ignore", over="ignore"):
        d, nwrap = fold(X[1:] - X[:-1], Lbox)
        U = np.cumsum(np.concatenate((np.zeros((1, Np, dim)), d)), axis=0)
        s = lane_sum(np.moveaxis(d, 1, 2))                                  # [ns-1, dim]
        W = np.cumsum(np.concatenate((np.zeros((1, dim)), s)), axis=0)
    return d, U, W, nwrap


def seq_sum(t, axis):
    """One running sum from 0.0, one addition after the other (every term here is a square: 0.0 + t is t)."""
    return np.take(np.cumsum(t, axis=axis), -1, axis=axis)


def lag_sums(U, W, Ntau):
    """C, D [Ntau+1, dim] of one call."""
    ns, Np, dim = U.shape
    rounds = -(-Np // LANES)
    Up = np.zeros((ns, rounds * LANES, dim))
    Up[:, :Np] = U
    C, D = np.zeros((Ntau + 1, dim)), np.zeros((Ntau + 1, dim))
    with np.errstate(invalid="ignore", over="ignore"):
        for l in range(Ntau + 1):
            dW = W[l:] - W[:ns - l]
            C[l] = seq_sum(dW * dW, 0)
            dU = Up[l:] - Up[:ns - l]                                       # [n_pairs, rounds*256, dim]
            t = (dU * dU).reshape(ns - l, rounds, LANES, dim)
            t = np.moveaxis(t, 0, 1).reshape(rounds * (ns - l), LANES, dim)     # (particle round, a) ascending
            D[l] = butterfly(np.moveaxis(seq_sum(t, 0), 0, 1))
    return C, D


class Window:
    """P [W, 2 Nb + 1, Np, dim]: the sums of one call per walker."""

    def __init__(self, P, Nb, window, Lbox, Ntau):
        self.W, self.dim, self.Ntau = P.shape[0], P.shape[3], Ntau
        self.C, self.D, self.nwrap, self.U, self.Wcm = [], [], [], [], []
        for w in range(self.W):
            d, U, Wc, nw = unfold(P[w, Nb - window:Nb + window + 1], Lbox)
            C, D = lag_sums(U, Wc, Ntau)
            self.C.append(C); self.D.append(D); self.nwrap.append(nw); self.U.append(U); self.Wcm.append(Wc)

    def expected(self, walkers):
        """What accumulate calls over `walkers` leave (a walker listed n times holds n times one call: n <= 2 is exact)."""
        out = {"C": np.zeros((self.W, self.Ntau + 1, self.dim)), "D": np.zeros((self.W, self.Ntau + 1, self.dim)),
               "nwrap": np.zeros(self.W, np.int64), "samples": np.zeros(self.W, np.int64)}
        with np.errstate(invalid="ignore", over="ignore"):
            for w in walkers:
                out["C"][w] = out["C"][w] + self.C[w]
                out["D"][w] = out["D"][w] + self.D[w]
                out["nwrap"][w] += self.nwrap[w]
                out["samples"][w] += 1
        return out


GRID = 65536.0


def on_grid(x):
    """x rounded to the 2^-16 grid: with dyadic box sides every operation of the family is then exact."""
    return np.round(np.asarray(x, np.float64) * GRID) / GRID


def wrap(P, Lbox):
    L = np.asarray(Lbox, np.float64)
    return P - L * np.floor((P + 0.5 * L) / L)


def drift(Np, M, Lbox, c, sign, rng):
    """[1, M, Np, dim]: particle i moves by sign[i] * c per link from a start on the 2^-16 grid, wrapped into the cell."""
    L = np.asarray(Lbox, np.float64)
    x0 = on_grid(rng.uniform(-0.5, 0.5, (Np, L.size)) * L)
    P = x0[None] + np.arange(M)[:, None, None] * (np.asarray(sign, np.float64)[:, None] * np.asarray(c, np.float64))[None]
    return wrap(P, L)[None]


def random_walk(W, M, Np, Lbox, rng, step):
    """[W, M, Np, dim]: every particle starts uniformly in the cell and takes Gaussian steps of `step` times the box side
    per axis and link; every bead is wrapped into [-L/2, L/2).  Particle 0 starts next to the upper faces, so that the
    smallest system crosses them too."""
    L = np.asarray(Lbox, np.float64)
    dim = L.size
    x0 = rng.uniform(-0.5, 0.5, (W, 1, Np, dim)) * L
    x0[:, :, 0] = 0.4999 * L
    P = x0 + np.cumsum(rng.normal(0.0, step, (W, M, Np, dim)) * L, axis=1)
    return P - L * np.floor((P + 0.5 * L) / L)
