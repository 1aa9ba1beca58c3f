"""Normalisation of the accumulators that PigsContext.density_read (trapped systems, pigs_density_*) and
PigsContext.fqt_read (periodic systems, pigs_fqt_*) return.

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
