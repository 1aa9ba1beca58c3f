"""Normalisation of the accumulators that PigsContext.density_read (trapped systems, pigs_density_*),
PigsContext.fqt_read, PigsContext.sqv_read, PigsContext.fqv_read, PigsContext.fqs_read and PigsContext.grv_read (periodic
systems, pigs_fqt_*, pigs_sqv_*, pigs_fqv_*, pigs_fqs_*, pigs_grv_*) and PigsContext.tau_read (both, pigs_tau_*) return.

Trapped-system profiles:

With S = the samples of a walker and V_d(r) = unit_ball(d) * r**d (the reference's ball volume,
pigs_estimators.f90 unit_ball):
  planar  c_j / (S * b**min(dim,2))                          b  = (2.0*h)/Nbin, grid [-h, h)
  radial  c_j / (S * (V_d((j+1)*br) - V_d(j*br)))            br = h/Nbin, grid [0, h)
  pair    c_j / (S * Np * (V_d((j+1)*br) - V_d(j*br)))
With every particle inside the grid the planar and radial profiles integrate to Np and the pair distribution to Np-1.

Imaginary-time density correlations (normalize_fqt): raw[l][iq][k] holds, per sample, the n_pairs(l) = 2*window + 1 - l
products C(a)C(a+l) + S(a)S(a+l) of the window slices, so
  F(q, tau_l) = raw / (S * n_pairs(l) * Np),   q = iq * (2*pi/Lbox[k]) for iq = 1..Nk,   tau_l = l*dt
and F(q, 0) is S(q) averaged over the window.

Vector structure factor (normalize_sqv, shell_average): raw[iqv] holds, per sample, the 2*window + 1 values C^2 + S^2 of
the window slices at the integer vector n[iqv] (q_k = n_k * 2*pi/Lbox[k]; half space, so q stands for -q too):
  S(q) = raw / (S * (2*window + 1) * Np)
and the vectors of equal |q| form a shell over which S(q) of an isotropic system is averaged.

F(q,tau) on the vector grid (normalize_fqv, shell_average): raw[l][iqv] holds, per sample, the n_pairs(l) products
C(a)C(a+l) + S(a)S(a+l) of the window slices at the vector n[iqv] of the S(q) grid above:
  F(q, tau_l) = raw / (S * n_pairs(l) * Np)
Its l = 0 row is normalize_sqv's S(q); shell_average(n, Lbox, F) gives the table per lag and |q| shell.

Self part of F(q,tau) and imaginary-time displacement (normalize_fqs, normalize_msd): F[l][iqv] holds, per sample, the
n_pairs(l) * Np single-particle products cos(q.(x_i(a+l) - x_i(a))), D[l] the sums of r^2 and r^4 of the once-folded
displacement x_i(a+l) - x_i(a) over the same pairs and particles:
  F_s(q, tau_l) = F / (S * n_pairs(l) * Np),   <dr^2>(tau_l) = D[l][0] / (S * n_pairs(l) * Np),
  alpha_2(tau_l) = dim * <dr^4> / ((dim + 2) * <dr^2>^2) - 1      (0 for a Gaussian displacement in dim dimensions)
F_s(q, 0) = 1 and <dr^2>(0) = 0; the distinct part is normalize_fqv - normalize_fqs.

Pair distribution on the vector grid (normalize_grv): vec[j] counts, per sample, the pairs i < j of the 2*window + 1
window slices whose folded displacement x(i) - x(j) falls into bin j of the minimum-image cell (width b_k = Lbox[k]/Nbin);
the partner -d is added by index reflection, and
  g(r_vec) = (vec[j] + vec[Nbin-1-j on every axis]) / (S * (2*window + 1) * Np * density * prod_k b_k)
which is 1 - 1/Np for an ideal gas.  radial[j] counts the same pairs by distance (bin width rbin, inside the cutoff):
  g(r_j) = 2 * radial[j] / (S * (2*window + 1) * Np * density * kn * ((r_j + rbin/2)^dim - (r_j - rbin/2)^dim))
with kn the volume of the unit ball: the reference's normalisation (sample_mod.f90, Normalize / NormAvGr).

Imaginary-time profiles (normalize_tau, pressure_virial): raw[b] holds, per sample, Vpair, Vext, W = sum r v'(r) and
D2 = sum_i |x_i(b) - x_i(b+1)|^2 of slice b = 0..2Nb, so per particle
  vpair, vext, w = raw[..., 0..2] / (S * Np),   klink[b] = dim/(2*dt) - D2[b] / (2*dt**2 * Np * S)  for the 2Nb links,
at tau_b = (b - Nb)*dt; the plateau of vpair + vext around tau = 0 is the converged part of the path.  The pressure of a
periodic system is P = density/dim * (2*K/N - W/N).

Bond-orientational order (normalize_bop, PigsContext.bop_read, pigs_bop_*): S holds, per sample, the sums over the
2*window + 1 window slices of Q4, Q4^2, Q6, Q6^2, the particle means of q4(i) and q6(i), and sum_i n_i; H the counts of
q4(i), q6(i) in Nh bins over [0, 1]; G and GN the sums of c_ij and the pairs per radial bin:
  <Q_l> = S / (S_w * (2*window + 1)),  coordination = S[6] / (S_w * (2*window + 1) * Np),
  P(q_l) = H * Nh / (S_w * (2*window + 1) * Np),   G6(r_j) = G[j] / GN[j]   (S_w the walker's samples)

Van Hove functions (normalize_vh, PigsContext.vh_read, pigs_vh_*): `distinct` counts |x_i(a+l) - x_j(a)| over the ordered
pairs i != j and `self` counts |x_i(a+l) - x_i(a)|, per lag l = 0..Ntau, over the n_pairs(l) = 2*window + 1 - l slice pairs
of the window; with dV_b the volume of the shell of bin b (radial grid Nr, rbin; self grid Ns, sbin):
  G_d(r_b, tau_l) = distinct / (S_w * n_pairs(l) * Np * density * dV_b)     (g(r) at tau = 0; 1 - 1/Np for an ideal gas)
  G_s(r_b, tau_l) = self / (S_w * n_pairs(l) * Np * dV_b)                   (a probability density: sum_b G_s dV_b = 1)

Triplet distribution (normalize_g3, PigsContext.g3_read, pigs_g3_*): `pair` counts the legs of every vertex per radial bin
(ordered pairs) and `trip` the unordered pairs of legs of a vertex per (lo, hi, q): lo <= hi their radial bins, packed at
p = lo*Nr - lo*(lo-1)/2 + hi - lo, and q the bin of cos(theta) on [-1, 1]; with S = S_w * (2*window + 1):
  g2(b)         = pair / (S * Np * density * dV_b)
  g3(lo, hi, q) = trip / (S * Np * density**2 * dV_lo * dV_hi * w_q * m),   m = 1 for lo < hi, 1/2 for lo = hi,
  w_q = 1/Na in 3D, (acos(c_q) - acos(c_{q+1}))/pi in 2D with c_q = -1 + 2q/Na      (1 + O(1/Np) without correlations)
bond_angle sums trip over the legs of the first bins into P(cos theta); kirkwood_g3 is g(r) g(s) g(t) on the same grid.

Axilrod-Teller-Muto three-body energy (normalize_atm, PigsContext.atm_read, pigs_atm_*): T sums, per window slice, the
geometric term (1 + 3 cos cos cos)/(r_ij r_ik r_jk)**3 over the triplets whose three nearest-image sides lie within rc, and
ntrip counts them; with the coupling nu in the run's own units (energy * length**9; the library knows no element):
  V3/N(tau_a) = nu * T / (S_w * Np)                     (its window mean is the perturbative <V3>/N)
  P3          = 9 * density * (V3/N) / dim              (pressure_atm: the sum is homogeneous of degree -9; cut at rc, no tail)

Momentum distribution and one-body density matrix (normalize_nk, normalize_nrvec, PigsContext.nk_read, pigs_nk_*): C sums
cos(k.x) over the end-to-end vectors x of the open worldlines on the box-commensurate vectors, nopen counts them (the sum of
k = 0) and H bins them on the Cartesian grid of the minimum-image cell.  In the reference's NormalizeNr convention (zconf
the diagonal configurations of the block, rho1(r)/density -> 1 at r -> 0):
  n(k)              = C / (CWorm * zconf * Nobdm),   n(0) = nopen / (CWorm * zconf * Nobdm),   n0 = n(0) / Np
  rho1(bin)/density = H / (CWorm * zconf * Nobdm * density * bin volume)
and the sum of n(k) over all k, -k included, is Np.
Lattice estimators of a crystal (normalize_lat, nearest_neighbour_distance, PigsContext.lat_read, pigs_lat_*): every
particle of a window slice is assigned to its nearest lattice site, u is its displacement from it (less the slice's mean
displacement with cm), and with N_a = nassigned of slice a, S = samples and ns = 2 window + 1:
  <u^2>(tau_a) = mom[a, 0] / N_a,  <u_k^2>(tau_a) = mom[a, 2 + k] / N_a;  over the window: sum_a mom / sum_a N_a
  gamma   = sqrt(<u^2>) / a_nn                                           (the Lindemann ratio)
  alpha_2 = dim <u^4> / ((dim + 2) <u^2>^2) - 1                          (normalize_msd's expression; 0 for a Gaussian)
  vacant  = sum_a occ[a, 0] / (S ns nsite),   multiple = sum_a (occ[a, 2] + occ[a, 3]) / (S ns nsite)
  hops per particle and link = hop1 / (S Np (ns - 1)),   across the window = hopw / (S Np)
  rho_site(r) = hr / (S ns nsite shell volume),   P(u_k) = hx[k] / (sum_a N_a rbin)
Superfluid fraction at T = 0 (normalize_sf, superfluid_fraction, PigsContext.sf_read, pigs_sf_*): every link of the window
is folded once and the folded links are added up, so the displacement over a lag is the unfolded one; with
n_pairs(l) = 2 window + 1 - l, S = samples, tau_l = l dt and lam = hbar^2/2m (1/2 in the run's units):
  Dcm[l, k]  = C / (S n_pairs Np)        <(sum_i dx_k(i))^2> / Np: Np times the squared displacement of the centre of mass
  rhos[l, k] = Dcm / (2 lam tau_l)       -> rho_s,k / rho for tau -> inf; 1 for a free gas; NaN at l = 0
  msd[l, k]  = D / (S n_pairs Np)        the single-particle displacement per axis, with no half-box limit
  cross      = Dcm - msd                 sum_{i != j} <dx_i dx_j> / Np
and rho_s,k / rho is the slope of Dcm over tau at large tau, divided by 2 lam (superfluid_fraction).
Clusters (normalize_cl, PigsContext.cl_read, pigs_cl_*): i and j are bonded iff 0 < r_ij^2 < rc^2 and a cluster is a
connected component of that graph in one window slice; with S = samples (slices) and s = 1..Np:
  n(s) = nsize / S,   fraction(s) = s n(s) / Np,   P_largest(s) = nlarge / S,   <Rg^2>(s) = rg2 / nsize (NaN: no such cluster)
  clusters per slice = sum_s n(s),   <smax>/Np = sum_s s nlarge / (S Np),   S_mean = sum s^2 nsize / sum s nsize
  bonds per particle = nbond / (S Np)
Wrapping clusters and persistence (normalize_pc, PigsContext.pc_read, pigs_pc_*): cl's bonds and clusters; a cluster's wrap
mask has bit k set when it closes on itself through the faces along axis k; with S = samples and mask = 0..7:
  P_wrap,k = sum_{mask with bit k} swrap / S,   P_any = sum_{mask != 0} swrap / S,   P_all = swrap[2^dim - 1] / S
  P_inf = sum_{mask != 0} mwrap / (Np S),   n_fin(s) / Np = nfin / (Np S),   S_fin = sum s^2 nfin / sum s nfin
  <Rg^2>(s) = rg2u / nfin  (finite clusters, from unfolded separations),   C(l) = both / first,
  J(l) = both / (first + second - both);   NaN where a denominator is zero
Pure numpy: it needs no GPU.
"""
from __future__ import annotations

import math

import numpy as np


def unit_ball(dim):
    """Volume of the unit dim-ball."""
    return math.pi ** (0.5 * dim) / math.gamma(0.5 * dim + 1.0)


def bin_widths(Nbin, half_width):
    """(b, br): the planar and the radial bin width, by the library's expressions."""
    return (2.0 * half_width) / Nbin, half_width / Nbin


def shell_volumes(dim, Nbin, half_width):
    """V_d((j+1)*br) - V_d(j*br) for j = 0..Nbin-1."""
    _, br = bin_widths(Nbin, half_width)
    kn = unit_ball(dim)
    j = np.arange(Nbin, dtype=np.float64)
    return kn * ((j + 1.0) * br) ** dim - kn * (j * br) ** dim


def normalize_profiles(counts, dim, Np, Nbin, half_width):
    """counts: the dict of density_read (per walker, leading axis W) or one walker's slice of it.
    Returns a dict: planar, radial, pair (float arrays of the same shapes) and the bin centres x (planar axis) and r
    (radial and pair).  A walker without samples gives NaN."""
    b, br = bin_widths(Nbin, half_width)
    dp = min(dim, 2)
    S = np.asarray(counts["samples"], dtype=np.float64)
    dv = shell_volumes(dim, Nbin, half_width)
    Sp = S.reshape(S.shape + (1,) * dp)
    Sr = S.reshape(S.shape + (1,))
    with np.errstate(divide="ignore", invalid="ignore"):
        planar = np.asarray(counts["planar"], np.float64) / (Sp * b ** dp)
        radial = np.asarray(counts["radial"], np.float64) / (Sr * dv)
        pair = np.asarray(counts["pair"], np.float64) / (Sr * Np * dv)
    x = -half_width + (np.arange(Nbin) + 0.5) * b
    r = (np.arange(Nbin) + 0.5) * br
    return {"planar": planar, "radial": radial, "pair": pair, "x": x, "r": r}


def normalize_fqt(raw, Np, window, dt, Lbox):
    """raw: the dict of fqt_read (F [W, Ntau+1, Nk, dim] raw sums, samples [W]) or one walker's slice of it.
    Returns (F, q, tau): F of the same shape as raw["F"], q [Nk, dim] (column k: iq * 2*pi/Lbox[k], iq = 1..Nk) and
    tau [Ntau+1] = l*dt.  A walker without samples gives NaN."""
    A = np.asarray(raw["F"], dtype=np.float64)
    S = np.asarray(raw["samples"], dtype=np.float64)
    nl, Nk, dim = A.shape[-3:]
    l = np.arange(nl, dtype=np.float64)
    n_pairs = 2.0 * window + 1.0 - l
    if nl > 2 * window + 1:
        raise ValueError("more lags than the window holds")
    with np.errstate(divide="ignore", invalid="ignore"):
        F = A / (S.reshape(S.shape + (1, 1, 1)) * n_pairs[:, None, None] * float(Np))
    L = np.asarray(Lbox, dtype=np.float64)[:dim]
    q = np.arange(1, Nk + 1, dtype=np.float64)[:, None] * (2.0 * np.pi / L)[None, :]
    return F, q, l * dt


def normalize_sqv(raw, samples, Np, window):
    """raw: the sums of sqv_read ([W, Nq] or one walker's [Nq]), samples: [W] or a scalar.  Returns S(q) of the same
    shape as raw: raw / (samples * (2*window + 1) * Np).  A walker without samples gives NaN."""
    A = np.asarray(raw, dtype=np.float64)
    S = np.asarray(samples, dtype=np.float64)
    if S.ndim > 0:
        S = S.reshape(S.shape + (1,))
    with np.errstate(divide="ignore", invalid="ignore"):
        return A / (S * (2.0 * window + 1.0) * float(Np))


def normalize_fqv(raw, samples, Np, window):
    """raw: the sums of fqv_read ([W, Ntau+1, Nq] or one walker's [Ntau+1, Nq]), samples: [W] or a scalar.  Returns
    F(q, tau_l) of the same shape as raw: raw / (samples * n_pairs(l) * Np), n_pairs(l) = 2*window + 1 - l.  A walker
    without samples gives NaN."""
    A = np.asarray(raw, dtype=np.float64)
    S = np.asarray(samples, dtype=np.float64)
    nl = A.shape[-2]
    if nl > 2 * window + 1:
        raise ValueError("more lags than the window holds")
    if S.ndim > 0:
        S = S.reshape(S.shape + (1, 1))
    n_pairs = 2.0 * window + 1.0 - np.arange(nl, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return A / (S * n_pairs[:, None] * float(Np))


def normalize_fqs(raw, samples, Np, window):
    """raw: the sums F of fqs_read ([W, Ntau+1, Nq] or one walker's [Ntau+1, Nq]), samples: [W] or a scalar.  Returns
    F_s(q, tau_l) of the same shape: raw / (samples * n_pairs(l) * Np), the normalisation of normalize_fqv.  A walker
    without samples gives NaN."""
    return normalize_fqv(raw, samples, Np, window)


def normalize_msd(raw, samples, Np, window, dim):
    """raw: the sums D of fqs_read ([W, Ntau+1, 2] or one walker's [Ntau+1, 2]), samples: [W] or a scalar.  Returns
    (msd, alpha2), each [.., Ntau+1]: msd = <|x_i(tau_l) - x_i(0)|^2> = D[..., 0] / (samples * n_pairs(l) * Np) and the
    non-Gaussian parameter alpha2 = dim * <dr^4> / ((dim + 2) * msd^2) - 1, NaN where msd is 0 (lag 0).  A walker
    without samples gives NaN."""
    A = np.asarray(raw, dtype=np.float64)
    S = np.asarray(samples, dtype=np.float64)
    nl = A.shape[-2]
    if A.shape[-1] != 2:
        raise ValueError("D must be [.., Ntau+1, 2]")
    if nl > 2 * window + 1:
        raise ValueError("more lags than the window holds")
    if S.ndim > 0:
        S = S.reshape(S.shape + (1,))
    n_pairs = 2.0 * window + 1.0 - np.arange(nl, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = S * n_pairs * float(Np)
        msd = A[..., 0] / norm
        r4 = A[..., 1] / norm
        alpha2 = dim * r4 / ((dim + 2.0) * msd * msd) - 1.0
    return msd, alpha2


def shell_average(n, Lbox, Sq):
    """n: the stored vectors [Nq, dim] (sqv_vectors), Lbox: the box lengths, Sq: [..., Nq].
    Returns (q, mean, mult): per shell, in ascending |q|, the modulus, the mean of Sq over the shell's stored vectors
    (shape [..., n_shells]) and the multiplicity counting both +q and -q (twice the stored vectors of the shell).
    With all box lengths bitwise equal the shell key is the integer sum of n_k^2; otherwise vectors whose |q|^2 agree
    to 1e-12 relative share a shell."""
    n = np.asarray(n, dtype=np.int64)
    Sq = np.asarray(Sq, dtype=np.float64)
    dim = n.shape[1]
    L = np.asarray(Lbox, dtype=np.float64)[:dim]
    qb = 2.0 * np.pi / L
    q2 = ((n * qb[None, :]) ** 2).sum(axis=1)
    if np.all(L == L[0]):
        key = (n * n).sum(axis=1)
        order = np.argsort(key, kind="stable")
        start = np.flatnonzero(np.r_[True, np.diff(key[order]) != 0])
    else:
        order = np.argsort(q2, kind="stable")
        s = q2[order]
        start = np.flatnonzero(np.r_[True, np.diff(s) > 1e-12 * s[1:]])
    cnt = np.diff(np.r_[start, n.shape[0]])
    q = np.sqrt(np.add.reduceat(q2[order], start) / cnt)
    mean = np.add.reduceat(Sq[..., order], start, axis=-1) / cnt
    return q, mean, 2 * cnt


def normalize_grv(counts, Np, window, density, Lbox, rbin, dim):
    """counts: the dict of grv_read (vec [W, Nbin, ..dim times], radial [W, Nr], samples [W]) or one walker's slice of
    it.  Returns a dict: g_vec (same shape as vec), the bin centres x (a list of dim arrays, x[k] along axis k of the
    box; array axis -1-k), g_r (same shape as radial) and its bin centres r.  A walker without samples gives NaN."""
    vec = np.asarray(counts["vec"], dtype=np.float64)
    rad = np.asarray(counts["radial"], dtype=np.float64)
    S = np.asarray(counts["samples"], dtype=np.float64)
    Nbin, Nr = vec.shape[-1], rad.shape[-1]
    L = np.asarray(Lbox, dtype=np.float64)[:dim]
    b = L / float(Nbin)
    axes = tuple(range(vec.ndim - dim, vec.ndim))
    sym = vec + np.flip(vec, axis=axes)                              # c[j] + c[Nbin-1-j] on every axis
    ns = 2.0 * window + 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        g_vec = sym / (S.reshape(S.shape + (1,) * dim) * ns * float(Np) * density * float(np.prod(b)))
        # the reference's g(r): centres (j - 1/2) rbin, ideal-gas count of the shell, 2 per pair
        r = (np.arange(1, Nr + 1, dtype=np.float64) - 0.5) * rbin
        nid = density * unit_ball(dim) * ((r + 0.5 * rbin) ** dim - (r - 0.5 * rbin) ** dim)
        g_r = 2.0 * rad / (nid * (S.reshape(S.shape + (1,)) * ns * float(Np)))
    x = [-0.5 * L[k] + (np.arange(Nbin) + 0.5) * b[k] for k in range(dim)]
    return {"g_vec": g_vec, "x": x, "g_r": g_r, "r": r}


def normalize_tau(raw, Np, dim, dt):
    """raw: the dict of tau_read (Q [W, 2Nb+1, 4] raw sums, samples [W]) or one walker's slice of it.
    Returns a dict: vpair, vext, w (per particle, [.., 2Nb+1]), klink ([.., 2Nb]: the kinetic estimator of the link
    between slices b and b+1, dim/(2*dt) - D2/(2*dt**2 * Np * samples)) and tau [2Nb+1] = (b - Nb)*dt.  A walker without
    samples gives NaN."""
    Q = np.asarray(raw["Q"], dtype=np.float64)
    S = np.asarray(raw["samples"], dtype=np.float64)
    M = Q.shape[-2]
    if Q.shape[-1] != 4 or M < 3 or M % 2 == 0:
        raise ValueError("Q must be [.., 2Nb+1, 4]")
    Nb = (M - 1) // 2
    Sb = S.reshape(S.shape + (1,))
    with np.errstate(divide="ignore", invalid="ignore"):
        per = Q[..., :3] / (Sb[..., None] * float(Np))
        klink = dim / (2.0 * dt) - Q[..., :M - 1, 3] / (2.0 * dt * dt * float(Np) * Sb)
    tau = (np.arange(M, dtype=np.float64) - Nb) * dt
    return {"vpair": per[..., 0], "vext": per[..., 1], "w": per[..., 2], "klink": klink, "tau": tau}


def normalize_bop(raw, Np, window, rbin=None):
    """raw: the dict of bop_read (S [W, 8], H [W, 2, Nh], G [W, Nr], GN [W, Nr], samples [W]) or one walker's slice of
    it.  With n = samples * (2*window + 1) slices, returns a dict: Q4, Q4sq, Q6, Q6sq (the slice invariants and their
    squares per slice), q4, q6 (the particle means of the local invariants per slice), coordination = sum n_i / (Np n),
    P4, P6 ([.., Nh]: the distributions of q4(i), q6(i) as probability densities on [0, 1]) with the bin centres q, and
    G6 = G / GN ([.., Nr]; NaN in a bin without pairs) with the bin centres r where rbin is given.  In 2D Psi_4, Psi_6
    and |psi_n(i)| stand in the same places.  A walker without samples gives NaN."""
    S = np.asarray(raw["S"], dtype=np.float64)
    H = np.asarray(raw["H"], dtype=np.float64)
    G = np.asarray(raw["G"], dtype=np.float64)
    GN = np.asarray(raw["GN"], dtype=np.float64)
    n = np.asarray(raw["samples"], dtype=np.float64) * (2.0 * window + 1.0)
    if S.shape[-1] != 8 or H.shape[-2] != 2:
        raise ValueError("S must be [.., 8] and H [.., 2, Nh]")
    Nh, Nr = H.shape[-1], G.shape[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        per = S / n[..., None]
        P = H * float(Nh) / (n[..., None, None] * float(Np))           # counts / (particles counted * bin width 1/Nh)
        G6 = np.where(GN > 0, G / GN, np.nan)
    out = {"Q4": per[..., 0], "Q4sq": per[..., 1], "Q6": per[..., 2], "Q6sq": per[..., 3], "q4": per[..., 4],
           "q6": per[..., 5], "coordination": per[..., 6] / float(Np), "P4": P[..., 0, :], "P6": P[..., 1, :],
           "q": (np.arange(Nh, dtype=np.float64) + 0.5) / float(Nh), "G6": G6}
    if rbin is not None:
        out["r"] = (np.arange(1, Nr + 1, dtype=np.float64) - 0.5) * rbin
    return out


def normalize_vh(counts, Np, window, density, rbin, sbin, dim, dt=None):
    """counts: the dict of vh_read (self [W, Ntau+1, Ns], distinct [W, Ntau+1, Nr], samples [W]) or one walker's slice
    of it.  Returns a dict: G_d (same shape as distinct) with its bin centres r, G_s (same shape as self) with its bin
    centres rs, the slice pairs n_pairs [Ntau+1] and, where dt is given, tau [Ntau+1] = l*dt.  The shell volumes are the
    reference's (NormAvGr), so the lag 0 of G_d is normalize_grv's g_r.  A walker without samples gives NaN."""
    dist = np.asarray(counts["distinct"], dtype=np.float64)
    slf = np.asarray(counts["self"], dtype=np.float64)
    S = np.asarray(counts["samples"], dtype=np.float64)
    nl, Nr, Ns = dist.shape[-2], dist.shape[-1], slf.shape[-1]
    if slf.shape[-2] != nl or nl > 2 * window + 1:
        raise ValueError("self and distinct must have the same lags, at most 2*window + 1 of them")
    n_pairs = 2.0 * window + 1.0 - np.arange(nl, dtype=np.float64)
    r = (np.arange(1, Nr + 1, dtype=np.float64) - 0.5) * rbin
    rs = (np.arange(1, Ns + 1, dtype=np.float64) - 0.5) * sbin
    kn = unit_ball(dim)
    nid = density * kn * ((r + 0.5 * rbin) ** dim - (r - 0.5 * rbin) ** dim)
    dv = 1.0 * kn * ((rs + 0.5 * sbin) ** dim - (rs - 0.5 * sbin) ** dim)
    norm = S.reshape(S.shape + (1, 1)) * n_pairs[:, None] * float(Np)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = {"G_d": dist / (nid * norm), "r": r, "G_s": slf / (dv * norm), "rs": rs, "n_pairs": n_pairs}
    if dt is not None:
        out["tau"] = np.arange(nl, dtype=np.float64) * dt
    return out


def g3_pairs(Nr):
    """(lo, hi): the radial bins of the two legs at every index p of the packed upper triangle, p = lo*Nr - lo*(lo-1)/2 +
    hi - lo (rows lo = 0..Nr-1, hi = lo..Nr-1 within a row)."""
    lo, hi = np.triu_indices(int(Nr))
    return lo, hi


def g3_nr(npairs):
    """Nr of a packed triangle of npairs = Nr*(Nr+1)/2 leg-bin pairs."""
    Nr = (math.isqrt(8 * int(npairs) + 1) - 1) // 2
    if Nr * (Nr + 1) // 2 != int(npairs):
        raise ValueError("%d is not Nr*(Nr+1)/2" % npairs)
    return Nr


def unpack_g3(packed):
    """[.., Nr*(Nr+1)/2, Na] on the packed triangle -> [.., Nr, Nr, Na], symmetric in the two legs (counts of a diagonal
    bin lo = hi are not doubled)."""
    a = np.asarray(packed)
    Nr = g3_nr(a.shape[-2])
    lo, hi = g3_pairs(Nr)
    out = np.zeros(a.shape[:-2] + (Nr, Nr, a.shape[-1]), a.dtype)
    out[..., lo, hi, :] = a
    out[..., hi, lo, :] = a
    return out


def g3_angle_weights(Na, dim):
    """w_q, q = 0..Na-1: the share of bin q of cos(theta) for two independent directions; sums to 1."""
    if dim == 3:
        return np.full(int(Na), 1.0 / float(Na))
    if dim != 2:
        raise ValueError("the triplet distribution is defined in 2D and 3D")
    c = np.clip(-1.0 + 2.0 * np.arange(int(Na) + 1, dtype=np.float64) / float(Na), -1.0, 1.0)
    return (np.arccos(c[:-1]) - np.arccos(c[1:])) / math.pi


def normalize_g3(counts, Np, window, density, rbin, dim):
    """counts: the dict of g3_read (trip [W, Nr(Nr+1)/2, Na], pair [W, Nr], samples [W]) or one walker's slice of it.
    Returns a dict: r [Nr] and cos [Na] the bin mid-points, g2 (same shape as pair), g3 (same shape as trip, on the packed
    triangle: unpack_g3 gives [.., Nr, Nr, Na]), lo and hi the leg bins of the packed index.  The shell volumes are
    normalize_grv's.  A walker without samples gives NaN."""
    trip = np.asarray(counts["trip"], dtype=np.float64)
    pair = np.asarray(counts["pair"], dtype=np.float64)
    S = np.asarray(counts["samples"], dtype=np.float64) * (2.0 * window + 1.0)
    Nr, Na = pair.shape[-1], trip.shape[-1]
    if trip.shape[-2] != Nr * (Nr + 1) // 2:
        raise ValueError("trip must hold Nr*(Nr+1)/2 leg pairs")
    r = (np.arange(1, Nr + 1, dtype=np.float64) - 0.5) * rbin
    vol = unit_ball(dim) * ((r + 0.5 * rbin) ** dim - (r - 0.5 * rbin) ** dim)
    lo, hi = g3_pairs(Nr)
    m = np.where(lo == hi, 0.5, 1.0)
    w = g3_angle_weights(Na, dim)
    cosm = -1.0 + (np.arange(Na, dtype=np.float64) + 0.5) * (2.0 / float(Na))
    with np.errstate(divide="ignore", invalid="ignore"):
        g2 = pair / (S.reshape(S.shape + (1,)) * float(Np) * density * vol)
        g3 = trip / (S.reshape(S.shape + (1, 1)) * float(Np) * density ** 2 * (vol[lo] * vol[hi] * m)[:, None] * w)
    return {"r": r, "cos": cosm, "g2": g2, "g3": g3, "lo": lo, "hi": hi}


def bond_angle(trip, nshell):
    """P(cos theta) [.., Na] of the pairs of legs that both lie in the radial bins < nshell (trip: counts on the packed
    triangle, [.., Nr(Nr+1)/2, Na]), normalised to integrate to 1 over cos(theta) in [-1, 1]; all zero where there is no
    such triplet."""
    a = np.asarray(trip, dtype=np.float64)
    Nr, Na = g3_nr(a.shape[-2]), a.shape[-1]
    if not 1 <= int(nshell) <= Nr:
        raise ValueError("nshell must be 1..Nr")
    _, hi = g3_pairs(Nr)
    h = a[..., hi < int(nshell), :].sum(axis=-2)
    tot = h.sum(axis=-1, keepdims=True) * (2.0 / float(Na))
    return np.divide(h, tot, out=np.zeros_like(h), where=tot > 0)


def kirkwood_g3(g2, rbin, Na):
    """The Kirkwood superposition g(r) g(s) g(t) on normalize_g3's grid, [Nr(Nr+1)/2, Na] on the packed triangle, from one
    g2 [Nr]: r, s and cos(theta) at the bin mid-points, t = sqrt(r^2 + s^2 - 2 r s cos(theta)) the third side, g(t) by
    linear interpolation between the mid-points of g2 (its first value below the first mid-point, its last beyond the
    last), NaN where t >= rmax = Nr*rbin."""
    g = np.asarray(g2, dtype=np.float64)
    if g.ndim != 1:
        raise ValueError("kirkwood_g3 takes one g2 [Nr]")
    Nr = g.shape[0]
    r = (np.arange(Nr, dtype=np.float64) + 0.5) * rbin
    c = -1.0 + (np.arange(int(Na), dtype=np.float64) + 0.5) * (2.0 / float(Na))
    lo, hi = g3_pairs(Nr)
    t2 = (r[lo] ** 2 + r[hi] ** 2)[:, None] - 2.0 * (r[lo] * r[hi])[:, None] * c
    t = np.sqrt(np.maximum(t2, 0.0))
    gt = np.interp(t, r, g)
    return np.where(t < Nr * rbin, (g[lo] * g[hi])[:, None] * gt, np.nan)


def normalize_atm(raw, Np, nu=1.0):
    """raw: the dict of atm_read (T [W, 2 window + 1] raw sums, ntrip likewise, samples [W]) or one walker's slice of it.
    nu: the triple-dipole coupling (energy * length**9 in the run's units; 1: the bare geometric sum).
    Returns a dict: v3 [.., 2 window + 1] = nu*T/(samples*Np), the three-body energy per particle of every window slice,
    v3_mean [..] its mean over the window, and ntrip [.., 2 window + 1] the mean number of triplets within rc per slice.
    A walker without samples gives NaN."""
    T = np.asarray(raw["T"], dtype=np.float64)
    n = np.asarray(raw["ntrip"], dtype=np.float64)
    S = np.asarray(raw["samples"], dtype=np.float64)
    if T.shape != n.shape or T.shape[-1] % 2 == 0:
        raise ValueError("T and ntrip must be [.., 2 window + 1]")
    Sb = S.reshape(S.shape + (1,))
    with np.errstate(divide="ignore", invalid="ignore"):
        v3 = float(nu) * T / (Sb * float(Np))
        cnt = n / Sb
    return {"v3": v3, "v3_mean": v3.mean(axis=-1), "ntrip": cnt}


def pressure_atm(v3_per_particle, density, dim):
    """The three-body contribution to the pressure, P3 = 9 * density * (V3/N) / dim, of a periodic system: the
    Axilrod-Teller-Muto sum is homogeneous of degree -9 in the lengths, so its virial is 9 V3 (P3 = 9 nu <T>/(dim Volume)
    with V3/N as normalize_atm gives it).  Triplets with a side beyond rc are not in V3 and no tail correction is made."""
    return 9.0 * density * np.asarray(v3_per_particle, np.float64) / dim


def normalize_nk(sums, cworm, zconf, nobdm, Np, n=None, Lbox=None):
    """sums: the dict of nk_read (C [W, Nq], nopen [W]) or one walker's slice of it; cworm, nobdm: the run's CWorm and
    Nobdm; zconf: the diagonal configurations of the block ([W] or a scalar), the reference's NormalizeNr divisor.
    Returns a dict: nk [.., Nq] = C/(cworm*zconf*nobdm), the momentum distribution per stored vector (-k has the same
    value), nk0 [..] that of k = 0, n0 [..] = nk0/Np the condensate fraction, and, with the vectors n [Nq, dim]
    (nk_vectors) and Lbox given, k, nk_shell [.., n_shells] and mult from shell_average.  A block without diagonal
    configurations gives no finite value."""
    Cs = np.asarray(sums["C"], dtype=np.float64)
    no = np.asarray(sums["nopen"], dtype=np.float64)
    z = np.broadcast_to(np.asarray(zconf, dtype=np.float64), no.shape)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = float(cworm) * z * float(nobdm)
        nk = Cs / den.reshape(den.shape + (1,))
        nk0 = no / den
    out = {"nk": nk, "nk0": nk0, "n0": nk0 / float(Np)}
    if n is not None:
        out["k"], out["nk_shell"], out["mult"] = shell_average(n, Lbox, nk)
    return out


def normalize_nrvec(sums, cworm, zconf, nobdm, density, Lbox, dim):
    """sums: the dict of nk_read (H [W, nbin, ..dim times]) or one walker's slice of it.  Returns a dict: rho1 (same
    shape as H) = H/(cworm*zconf*nobdm*density*bin volume), the one-body density matrix over the density per Cartesian
    bin of the minimum-image cell in the reference's normalisation (1 at r -> 0), and the bin centres x (a list of dim
    arrays, x[k] along axis k of the box; array axis -1-k).  A block without diagonal configurations gives no finite value."""
    H = np.asarray(sums["H"], dtype=np.float64)
    nbin = H.shape[-1]
    L = np.asarray(Lbox, dtype=np.float64)[:dim]
    b = L / float(nbin)
    z = np.broadcast_to(np.asarray(zconf, dtype=np.float64), H.shape[:H.ndim - dim])
    with np.errstate(divide="ignore", invalid="ignore"):
        den = float(cworm) * z * float(nobdm) * float(density) * float(np.prod(b))
        rho1 = H / den.reshape(den.shape + (1,) * dim)
    x = [-0.5 * L[k] + (np.arange(nbin) + 0.5) * b[k] for k in range(dim)]
    return {"rho1": rho1, "x": x}


def nearest_neighbour_distance(sites, Lbox):
    """The shortest minimum-image distance between two of the lattice sites [nsite, dim] in the periodic box Lbox (every
    coordinate difference folded by its nearest multiple of the side); inf for a single site."""
    R = np.asarray(sites, dtype=np.float64)
    if R.ndim != 2:
        raise ValueError("sites must be [nsite, dim]")
    L = np.asarray(Lbox, dtype=np.float64)[:R.shape[1]]
    best = np.inf
    for s in range(R.shape[0] - 1):
        d = R[s + 1:] - R[s]
        d = d - L * np.rint(d / L)
        best = min(best, float(np.sqrt((d * d).sum(axis=1).min())))
    return best


def normalize_lat(raw, Np, nsite, a_nn, rmax):
    """raw: the dict of lat_read (mom [W, ns, 2 + dim], nassigned [W, ns], nlost, occ [W, ns, 4], hr [W, nbin],
    hx [W, dim, 2 nbin], hop1, hopw, samples [W]) or one walker's slice of it; a_nn: the sites' nearest-neighbour distance;
    rmax: the range of the histograms.  Returns a dict: u2 [.., ns], uk2 [.., ns, dim] and gamma_tau [.., ns] per window
    slice; over the window u2_mean, gamma, alpha2, vacant, multiple, hops_link, hops_window [..]; r [nbin] and
    rho_site [.., nbin]; x [2 nbin] and pu [.., dim, 2 nbin].  A walker without samples gives NaN."""
    mom = np.asarray(raw["mom"], dtype=np.float64)
    n = np.asarray(raw["nassigned"], dtype=np.float64)
    occ = np.asarray(raw["occ"], dtype=np.float64)
    hr = np.asarray(raw["hr"], dtype=np.float64)
    hx = np.asarray(raw["hx"], dtype=np.float64)
    S = np.asarray(raw["samples"], dtype=np.float64)
    dim, ns, nbin = mom.shape[-1] - 2, mom.shape[-2], hr.shape[-1]
    if dim not in (2, 3) or n.shape != mom.shape[:-1] or occ.shape != n.shape + (4,) or hx.shape[-2:] != (dim, 2 * nbin):
        raise ValueError("the arrays of lat_read do not fit each other")
    rbin = float(rmax) / nbin
    edges = np.arange(nbin + 1) * rbin
    shell = np.pi * np.diff(edges ** 2) if dim == 2 else 4.0 * np.pi / 3.0 * np.diff(edges ** 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        u2 = mom[..., 0] / n
        uk2 = mom[..., 2:] / n[..., None]
        ntot = n.sum(axis=-1)
        u2m = mom[..., 0].sum(axis=-1) / ntot
        u4m = mom[..., 1].sum(axis=-1) / ntot
        sites = S * ns * float(nsite)
        out = {"u2": u2, "uk2": uk2, "gamma_tau": np.sqrt(u2) / a_nn, "u2_mean": u2m, "gamma": np.sqrt(u2m) / a_nn,
               "alpha2": dim * u4m / ((dim + 2) * u2m * u2m) - 1.0,
               "vacant": occ[..., 0].sum(axis=-1) / sites, "multiple": (occ[..., 2] + occ[..., 3]).sum(axis=-1) / sites,
               "hops_link": (np.asarray(raw["hop1"], dtype=np.float64) / (S * Np * (ns - 1)) if ns > 1 else 0.0 * S),
               "hops_window": np.asarray(raw["hopw"], dtype=np.float64) / (S * Np),
               "r": 0.5 * (edges[1:] + edges[:-1]), "rho_site": hr / (sites[..., None] * shell),
               "x": -float(rmax) + (np.arange(2 * nbin) + 0.5) * rbin, "pu": hx / (ntot[..., None, None] * rbin)}
    return out


def normalize_sf(got, Np, dt, lam=0.5, window=None):
    """got: the dict of sf_read (C and D [W, Ntau+1, dim], samples [W], window) or one walker's slice of it; window: the
    window of sf_init where got does not carry it.  lam = hbar^2/2m; 1/2 is the run's own unit (a free link has variance
    dt per axis).  Returns a dict: tau [Ntau+1] = l dt; Dcm [.., Ntau+1, dim] = C / (samples n_pairs(l) Np);
    rhos [.., Ntau+1, dim] = Dcm / (2 lam tau_l), NaN at l = 0, and rhos_mean [.., Ntau+1], its mean over the axes;
    msd [.., Ntau+1, dim] = D / (samples n_pairs(l) Np); cross = Dcm - msd.  A walker without samples gives NaN."""
    Cs = np.asarray(got["C"], dtype=np.float64)
    Ds = np.asarray(got["D"], dtype=np.float64)
    S = np.asarray(got["samples"], dtype=np.float64)
    if window is None:
        window = got.get("window") if hasattr(got, "get") else None
    if window is None:
        raise ValueError("normalize_sf needs the window of sf_init (got['window'] or window=)")
    window = int(window)
    if Cs.ndim < 2 or Cs.shape != Ds.shape or S.shape != Cs.shape[:-2]:
        raise ValueError("the arrays of sf_read do not fit each other")
    nl = Cs.shape[-2]
    if nl > 2 * window + 1:
        raise ValueError("more lags than the window holds")
    n_pairs = 2.0 * window + 1.0 - np.arange(nl, dtype=np.float64)
    tau = np.arange(nl, dtype=np.float64) * float(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        norm = S[..., None, None] * n_pairs[:, None] * float(Np)
        Dcm = Cs / norm
        msd = Ds / norm
        rhos = Dcm / (2.0 * float(lam) * tau[:, None])
        rhos[..., 0, :] = np.nan
        return {"tau": tau, "Dcm": Dcm, "rhos": rhos, "rhos_mean": rhos.mean(axis=-1), "msd": msd, "cross": Dcm - msd}


def superfluid_fraction(tau, Dcm_k, tmin, lam=0.5):
    """The superfluid fraction along one axis from the diffusion of the centre of mass: the slope of the least-squares
    line (with an intercept: a crystal's plateau goes there) through Dcm_k [Ntau+1] over the lags with tau >= tmin,
    divided by 2 lam.  Returns (rho_s / rho, its standard error): the error is the fit's own, from the residuals with
    n - 2 degrees of freedom (NaN for two points), and knows nothing of the statistical error of Dcm."""
    t = np.asarray(tau, dtype=np.float64)
    y = np.asarray(Dcm_k, dtype=np.float64)
    if t.ndim != 1 or t.shape != y.shape:
        raise ValueError("tau and Dcm_k must be two vectors of one length")
    keep = t >= float(tmin)
    t, y = t[keep], y[keep]
    n = t.size
    if n < 2:
        raise ValueError("a slope needs two lags or more at tau >= tmin")
    tm, ym = t.mean(), y.mean()
    sxx = float(((t - tm) ** 2).sum())
    slope = float(((t - tm) * (y - ym)).sum()) / sxx
    res = y - (ym + slope * (t - tm))
    err = math.sqrt(float((res * res).sum()) / (n - 2) / sxx) if n > 2 else float("nan")
    return slope / (2.0 * float(lam)), err / (2.0 * float(lam))


def normalize_cl(got, Np, summed=False):
    """got: the dict of cl_read (nsize, nlarge, rg2 [W, Np], nbond, samples [W]) or one walker's slice of it; summed:
    add the walkers' sums first.  With S = samples (window slices) and s = 1..Np, returns a dict:
    s [Np]; n [.., Np] = nsize / S, the clusters of size s per sample; fraction [.., Np] = s n(s) / Np, the share of the
    particles that sit in clusters of size s; p_largest [.., Np] = nlarge / S; rg2 [.., Np] = rg2 / nsize, NaN where
    n(s) = 0; n_clusters [..] = sum_s n(s); smax [..] = sum_s s nlarge / (S Np), the mean largest cluster over Np;
    mean_size [..] = sum s^2 nsize / sum s nsize; bonds [..] = nbond / (S Np), the bonds per particle.  A walker without
    samples gives NaN."""
    ns = np.asarray(got["nsize"], dtype=np.float64)
    nl = np.asarray(got["nlarge"], dtype=np.float64)
    rg = np.asarray(got["rg2"], dtype=np.float64)
    nb = np.asarray(got["nbond"], dtype=np.float64)
    S = np.asarray(got["samples"], dtype=np.float64)
    if ns.ndim < 1 or ns.shape[-1] != int(Np) or nl.shape != ns.shape or rg.shape != ns.shape or \
            S.shape != ns.shape[:-1] or nb.shape != S.shape:
        raise ValueError("the arrays of cl_read do not fit each other or Np")
    if summed and ns.ndim > 1:
        ns, nl, rg, nb, S = ns.sum(axis=0), nl.sum(axis=0), rg.sum(axis=0), nb.sum(axis=0), S.sum(axis=0)
    s = np.arange(1, int(Np) + 1, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = ns / S[..., None]
        return {"s": s, "n": n, "fraction": s * n / float(Np), "p_largest": nl / S[..., None],
                "rg2": np.where(ns > 0, rg / ns, np.nan), "n_clusters": n.sum(axis=-1),
                "smax": (s * nl).sum(axis=-1) / (S * float(Np)),
                "mean_size": (s * s * ns).sum(axis=-1) / (s * ns).sum(axis=-1), "bonds": nb / (S * float(Np))}


def normalize_pc(got, Np, dim, summed=False):
    """got: the dict of pc_read (nwrap, mwrap, swrap [W, 8], nfin, rg2u [W, Np], samples [W], first, second, both, norig
    [W, ntau + 1]) or one walker's slice of it; summed: add the walkers' sums first.  With S = samples (window slices) and
    s = 1..Np, returns a dict:
    s [Np]; p_wrap [.., dim] = the share of the slices with a cluster that wraps along axis k; p_any [..] and p_all [..],
    along any axis and along all `dim` of them; p_inf [..] = sum_{mask != 0} mwrap / (Np S), the strength: the share of the
    particles in wrapping clusters; n_fin [.., Np] = nfin / (Np S), the finite clusters of size s per particle; mean_size
    [..] = sum s^2 nfin / sum s nfin over the finite clusters; rg2 [.., Np] = rg2u / nfin; persistence [.., ntau + 1] =
    both / first; jaccard [.., ntau + 1] = both / (first + second - both).  Elements with a zero denominator are NaN."""
    dim = int(dim)
    if dim not in (1, 2, 3):
        raise ValueError("dim is 1, 2 or 3")
    f = lambda k: np.asarray(got[k], dtype=np.float64)
    nw, mw, sw, nf, rg, S = f("nwrap"), f("mwrap"), f("swrap"), f("nfin"), f("rg2u"), f("samples")
    fi, se, bo = f("first"), f("second"), f("both")
    if nf.ndim < 1 or nf.shape[-1] != int(Np) or rg.shape != nf.shape or S.shape != nf.shape[:-1] or \
            any(a.shape != S.shape + (8,) for a in (nw, mw, sw)) or fi.ndim != nf.ndim or fi.shape[:-1] != S.shape or \
            se.shape != fi.shape or bo.shape != fi.shape:
        raise ValueError("the arrays of pc_read do not fit each other or Np")
    if summed and nf.ndim > 1:
        nw, mw, sw, nf, rg, S, fi, se, bo = (a.sum(axis=0) for a in (nw, mw, sw, nf, rg, S, fi, se, bo))
    s = np.arange(1, int(Np) + 1, dtype=np.float64)
    masks = np.arange(8)
    with np.errstate(divide="ignore", invalid="ignore"):
        nan_if = lambda num, den: np.where(den != 0, num / np.where(den != 0, den, 1.0), np.nan)
        p_wrap = np.stack([nan_if(sw[..., (masks >> k) & 1 == 1].sum(axis=-1), S) for k in range(dim)], axis=-1)
        return {"s": s, "p_wrap": p_wrap, "p_any": nan_if(sw[..., 1:].sum(axis=-1), S),
                "p_all": nan_if(sw[..., (1 << dim) - 1], S),
                "p_inf": nan_if(mw[..., 1:].sum(axis=-1), S * float(Np)),
                "n_fin": nan_if(nf, (S * float(Np))[..., None]),
                "mean_size": nan_if((s * s * nf).sum(axis=-1), (s * nf).sum(axis=-1)),
                "rg2": nan_if(rg, nf), "persistence": nan_if(bo, fi), "jaccard": nan_if(bo, fi + se - bo)}


def pressure_virial(kin_per_particle, w_per_particle, density, dim):
    """Virial pressure P = density/dim * (2*K/N - W/N) of a periodic system, with W/N = <sum_{i<j} r v'(r)>/N as
    normalize_tau's `w` gives it.  Pairs beyond rcut are not in W and no tail correction is made."""
    return density / dim * (2.0 * np.asarray(kin_per_particle, np.float64) - np.asarray(w_per_particle, np.float64))
