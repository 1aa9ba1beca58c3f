"""numpy restatement of the lattice sums that pigs_lat_* accumulates (include/pigs_hip.h has the definition), with the same
IEEE operations per term: per particle and site d = x - R, one fold per coordinate by two compares against LboxHalf, r2
summed left to right; the assigned site by a plain loop over the sites in ascending order with a strict `<` from
+infinity (the smallest index of the minimum; NaN and +infinity never win: the particle is lost, site -1); u the folded d
of that site; with cm the centre of mass c_k = (0.0 + u_k(0) + u_k(1) + ..)/n_assigned by a sequential cumsum (a lost
particle adds 0.0); v = u - c; m2 = sum_k v_k*v_k left to right; the bins decided in double before the conversion.
Every term and every count has the device's bits; only the order of the sums of mom differs, so their comparison is
bounded by Sum|terms|, which equals the sums themselves (every term is a square)."""
import numpy as np


def fold(d, Lbox):
    L = np.asarray(Lbox, np.float64)[:d.shape[-1]]
    Lh = 0.5 * L
    with np.errstate(invalid="ignore"):
        d = np.where(d > Lh, d - L, d)
        d = np.where(d < -Lh, d + L, d)
    return d


def r2_of(d):
    r2 = np.zeros(d.shape[:-1])
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(d.shape[-1]):
            r2 = r2 + d[..., k] * d[..., k]
    return r2


def assign(X, R, Lbox):
    """X [Np, dim], R [nsite, dim]: (site [Np] with -1 for a lost particle, u [Np, dim] with 0.0 for a lost one)."""
    Np, dim = X.shape
    best = np.full(Np, np.inf)
    site = np.full(Np, -1, np.int64)
    u = np.zeros((Np, dim))
    for s in range(R.shape[0]):
        d = fold(X - R[s], Lbox)
        r2 = r2_of(d)
        with np.errstate(invalid="ignore"):
            m = r2 < best
        best = np.where(m, r2, best)
        site = np.where(m, s, site)
        u = np.where(m[:, None], d, u)
    return site, u


def slice_sums(X, R, Lbox, nbin, rmax, cm):
    """One slice: dict of mom [2 + dim], nassigned, nlost, occ [4], hr [nbin], hx [dim, 2 nbin], site [Np]."""
    Np, dim = X.shape
    site, u = assign(X, R, Lbox)
    ok = site >= 0
    nass = int(ok.sum())
    v = u
    if cm and nass > 0:
        c = np.array([np.cumsum(np.concatenate(([0.0], u[:, k])))[-1] for k in range(dim)]) / float(nass)
        v = u - c
    v = v[ok]
    m2 = r2_of(v)
    mom = np.array([m2.sum(), (m2 * m2).sum()] + [(v[:, k] * v[:, k]).sum() for k in range(dim)])
    rbin = float(rmax) / float(nbin)
    t = np.sqrt(m2) / rbin
    hr = np.bincount(t[t < float(nbin)].astype(np.int64), minlength=nbin)
    hx = np.zeros((dim, 2 * nbin), np.int64)
    for k in range(dim):
        t = (v[:, k] + float(rmax)) / rbin
        hx[k] = np.bincount(t[(t >= 0.0) & (t < float(2 * nbin))].astype(np.int64), minlength=2 * nbin)
    per_site = np.bincount(site[ok], minlength=R.shape[0])
    occ = np.bincount(np.minimum(per_site, 3), minlength=4)
    return {"mom": mom, "nassigned": nass, "nlost": Np - nass, "occ": occ, "hr": hr, "hx": hx, "site": site}


def hops(sites):
    """sites [ns, Np] along the window: (hop1, hopw); a lost end (site -1) drops the comparison."""
    a, b = sites[:-1], sites[1:]
    hop1 = int(((a >= 0) & (b >= 0) & (a != b)).sum())
    f, l = sites[0], sites[-1]
    return hop1, int(((f >= 0) & (l >= 0) & (f != l)).sum())


class Window:
    """The sums of the window slices Nb-window..Nb+window of every walker of paths [W, M, Np, dim], computed once per walker
    and then only added up."""

    def __init__(self, paths, Nb, window, Lbox, sites, nbin, rmax, cm):
        self.paths, self.Nb, self.window, self.Lbox = paths, Nb, window, Lbox
        self.R = np.ascontiguousarray(sites, np.float64)
        self.nbin, self.rmax, self.cm = nbin, rmax, cm
        self.W, self.dim = paths.shape[0], paths.shape[-1]
        self.ns = 2 * window + 1
        self._c = {}

    def walker(self, w):
        if w not in self._c:
            sl = [slice_sums(self.paths[w, self.Nb - self.window + js], self.R, self.Lbox, self.nbin, self.rmax, self.cm)
                  for js in range(self.ns)]
            h1, hw = hops(np.stack([s["site"] for s in sl]))
            self._c[w] = {"mom": np.stack([s["mom"] for s in sl]), "nassigned": np.array([s["nassigned"] for s in sl]),
                          "nlost": sum(s["nlost"] for s in sl), "occ": np.stack([s["occ"] for s in sl]),
                          "hr": sum(s["hr"] for s in sl), "hx": sum(s["hx"] for s in sl), "hop1": h1, "hopw": hw,
                          "samples": 1}
        return self._c[w]

    def expected(self, walkers):
        """Accumulated sums for the walker list `walkers` (entries may repeat): the dict of PigsContext.lat_read."""
        W, ns, dim, nb = self.W, self.ns, self.dim, self.nbin
        i64 = lambda *s: np.zeros(s, np.int64)
        out = {"mom": np.zeros((W, ns, 2 + dim)), "nassigned": i64(W, ns), "nlost": i64(W), "occ": i64(W, ns, 4),
               "hr": i64(W, nb), "hx": i64(W, dim, 2 * nb), "hop1": i64(W), "hopw": i64(W), "samples": i64(W)}
        for w in walkers:
            for k, v in self.walker(w).items():
                out[k][w] += v
        return out


INT_KEYS = ("nassigned", "nlost", "occ", "hr", "hx", "hop1", "hopw", "samples")


def grid_sites(dim, n, Lbox, nsite=None):
    """The first nsite (default: all) of the n^dim cell centres of a simple grid in the box, [nsite, dim], in [-L/2, L/2)."""
    L = np.asarray(Lbox, np.float64)[:dim]
    idx = np.stack(np.unravel_index(np.arange(n ** dim), (n,) * dim), axis=1).astype(np.float64)
    R = (idx + 0.5) * (L / n) - 0.5 * L
    return R if nsite is None else R[:nsite]


def jittered(R, W, M, Np, Lbox, rng, amp):
    """paths [W, M, Np, dim]: particle i of every bead at site i (mod the sites) plus a uniform jitter of +-amp, wrapped
    into the primary cell."""
    dim = R.shape[1]
    L = np.asarray(Lbox, np.float64)[:dim]
    P = R[np.arange(Np) % R.shape[0]][None, None] + rng.uniform(-amp, amp, (W, M, Np, dim))
    return P - L * np.floor((P + 0.5 * L) / L)
