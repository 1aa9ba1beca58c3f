"""Bond-orientational order on the MI355X (pigs_bop_*, pigs_bop.hip) through the C ABI, against the numpy restatement in
tests/bop_numpy.py (which shares no formula with the kernel: bond x bond Legendre sums, no spherical harmonics).

Tolerances (include/pigs_hip.h has the definitions; `slices` = slices summed into the element):
  GN, sum n_i   exact equality: bonds and bins are comparisons in double on grv_numpy's arithmetic.
  H             for every k the cumulative count up to bin k lies between the cumulative numpy counts of q + 1e-9 and of
                q - 1e-9, and the sum is Np x slices: no particle is dropped, a bin edge may fall either way.
  S[1,3,4,5]    1e-12 x slices (every square is at most 1: a few thousand ulp).
  S[0,2]        sum over the slices of 1e-12 / max(Q_numpy, 1e-6): the root amplifies near Q = 0.
  G             GN_bin x (1e-12 + 2^-41): every c_ij carries half a quantum of the fixed-point sum.
Every check prints its largest error/bound ratio.

Shapes: Np = 2, 3, 64, 65, 256, 257, 300, 520 are the edges of a wave, of the 256 particles that the threads own at a
time, and of second rounds of one particle and of a few; each runs in 2D and 3D with a neighbour radius that leaves most
particles alone, one with about 12 (3D) or 6 (2D) neighbours, and half the shortest side, with W = 0, 2 and Nb.  The
restatement costs bonds^2 per slice.  So from Np = 256 on the 12-neighbour radius runs W = 2 and Nb with one walker
listed, and the half-box radius (35 000 bonds per slice and more: minutes of numpy per slice) is NOT compared with the
restatement at Np = 256, 257, 300 and 520.  In its place test_half_box_radius_counts_every_bond_at_large_np checks, at
exactly those Np, what is exact and cheap: sum n_i and GN against grv_numpy's arithmetic (a bond missed or taken twice by
the 64-partner masks, by a second round of owned particles or at the last partial mask shows there), the histogram
totals, and the invariants' range.  The harmonic sums over dense masks are compared up to Np = 65."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from bop_numpy import COORDINATION, LATTICES, Window, histogram
from conftest import ROOT
from pathintegralgroundstate_amd import SystemConfig

pytestmark = pytest.mark.gpu
DENSITY = {2: 0.25, 3: 0.365}
QUANTUM = 2.0 ** -40
DELTA = 1e-9
worst = {"ratio": 0.0}


def _status_codes():
    txt = open(os.path.join(ROOT, "include", "pigs_hip.h")).read()
    return {k: int(v) for k, v in re.findall(r"^\s*(PIGS_\w+)\s*=\s*(-?\d+)", txt, flags=re.M)}


ST = _status_codes()


def _cfg(dim, Np, Nb, **kw):
    return SystemConfig(dim=dim, Np=Np, Nb=Nb, density=DENSITY[dim], **kw)


def _random_paths(cfg, W, rng, scale=0.5):
    L = np.asarray(cfg.Lbox[:cfg.dim])
    return rng.uniform(-scale, scale, (W,) + tuple(cfg.path_shape)) * L


def _radius(dim, density, neighbours):
    """The radius of the ball that holds `neighbours` particles at this density."""
    return (neighbours / (np.pi * density)) ** 0.5 if dim == 2 else (3.0 * neighbours / (4.0 * np.pi * density)) ** (1.0 / 3.0)


def _check(got, exp, Np, Nh, window, what):
    """got: bop_read's dict; exp: Window.expected's.  Returns the largest error/bound ratio."""
    W = got["S"].shape[0]
    ns = 2 * window + 1
    assert np.array_equal(got["samples"], exp["samples"]), (what, got["samples"], exp["samples"])
    assert np.array_equal(got["GN"], exp["GN"]), what
    assert np.array_equal(got["S"][:, 6], exp["S"][:, 6]) and not got["S"][:, 7].any(), what
    ratio = 0.0
    for w in range(W):
        slices = int(exp["samples"][w]) * ns
        if slices == 0:
            assert not got["S"][w].any() and not got["H"][w].any() and not got["G"][w].any(), what
            continue
        err = np.abs(got["S"][w] - exp["S"][w])
        ratio = max(ratio, float(err[[1, 3, 4, 5]].max()) / (1e-12 * slices))
        for k, name in ((0, "Q4"), (2, "Q6")):
            ratio = max(ratio, float(err[k]) / sum(1e-12 / max(Q, 1e-6) for Q in exp[name][w]))
        for l, name in enumerate(("q4", "q6")):
            q = np.concatenate(exp[name][w])
            H = got["H"][w, l]
            assert H.sum() == Np * slices and H.min() >= 0, (what, name, H.sum())
            lo, hi = np.cumsum(histogram(q + DELTA, Nh)), np.cumsum(histogram(np.maximum(q - DELTA, 0.0), Nh))
            assert np.all(lo <= np.cumsum(H)) and np.all(np.cumsum(H) <= hi), (what, name)
        gerr = np.abs(got["G"][w] - exp["G"][w])
        bound = exp["GN"][w] * (1e-12 + 0.5 * QUANTUM)
        assert not np.any(gerr[bound == 0]), what
        if np.any(bound > 0):
            ratio = max(ratio, float((gerr[bound > 0] / bound[bound > 0]).max()))
    worst["ratio"] = max(worst["ratio"], ratio)
    print(f"{what}: error/bound {ratio:.3g} (largest so far {worst['ratio']:.3g})")
    assert ratio <= 1.0, what
    return ratio


def _run(ctx, cfg, win, rnb, window, Nh, Nr, what, walkers=None):
    rbin = cfg.rcut / float(np.float32(Nr)) if Nr else 0.0
    ctx.bop_init(rnb, window, Nh, Nr, rbin)
    ctx.bop_accumulate(walkers)
    got = ctx.bop_read()
    assert got["H"].shape == (ctx.n_walkers, 2, Nh) and got["G"].shape == got["GN"].shape == (ctx.n_walkers, Nr)
    exp = win.expected(range(ctx.n_walkers) if walkers is None else walkers, cfg.Nb, window, Nr, rbin)
    return _check(got, exp, cfg.Np, Nh, window, what)


# ---- 1. against the restatement on random in-box worldlines -----------------------------------------------------------
@pytest.mark.parametrize("Np", [2, 3, 64, 65, 256, 257, 300, 520])
@pytest.mark.parametrize("dim", [2, 3])
def test_matches_numpy_on_uploaded_worldlines(gpu_lib, dim, Np):
    W, Nb = 2, 4
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(1000 * dim + Np))
    half = 0.5 * min(cfg.Lbox[:dim])
    nfull = 12 if dim == 3 else 6
    full = _radius(dim, cfg.density, nfull)
    radii = [("sparse", min(_radius(dim, cfg.density, 0.3), half), (0, 2, Nb)),
             ("shell", min(full, half), (0, 2, Nb))]
    if Np <= 65:
        radii.append(("half", half, (0, 2)))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for name, rnb, windows in radii:
            win = Window(P, cfg.Lbox, cfg.rcut2, rnb)
            for window in windows:
                # (the restatement of a well-filled shell at Np >= 256 costs seconds per slice: one walker beyond W = 0)
                wl = [0] if name == "shell" and Np >= 256 and window > 0 else None
                for Nh, Nr in ((1, 0), (20, 1), (20, 50)):
                    _run(ctx, cfg, win, rnb, window, Nh, Nr, f"dim {dim} Np {Np} {name} rnb {rnb:.4g} W {window} Nh {Nh} Nr {Nr}",
                         walkers=wl)
            n = np.concatenate([win.slice(w, Nb).n for w in range(W)])
            print(f"dim {dim} Np {Np} {name}: mean coordination {n.mean():.3g}, {np.mean(n == 0):.0%} without neighbours")
            if name == "sparse" and Np >= 64:
                assert np.mean(n == 0) > 0.5                           # the radii do what they are here for
            if name == "shell" and Np >= 256:
                assert 0.7 * nfull < n.mean() < 1.3 * nfull


def _bond_and_pair_counts(X, cfg, rnb, Nr, rbin):
    """(sum n_i, GN [Nr]) of one slice from grv_numpy's arithmetic alone."""
    from grv_numpy import bin_radial, folded
    _, r2 = folded(X, cfg.Lbox)
    return 2 * int(np.count_nonzero((r2 > 0.0) & (r2 < rnb * rnb))), bin_radial(r2, cfg.rcut2, Nr, rbin)


@pytest.mark.parametrize("dim,Np", [(2, 256), (3, 256), (2, 257), (3, 257), (2, 300), (3, 300), (2, 520), (3, 520), (3, 3000)])
def test_half_box_radius_counts_every_bond_at_large_np(gpu_lib, dim, Np):
    """rnb = half the shortest side where the restatement is out of reach: every bond and pair counted exactly once.
    Np = 3000 in 3D (Nr = 0) holds its slice in 72 800 bytes of LDS, beyond what a kernel gets without a grant."""
    W, Nb, window, Nh = 2, 2, 1, 20
    Nr = 0 if Np == 3000 else 50
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(31 * dim + Np))
    rnb = 0.5 * min(cfg.Lbox[:dim])
    rbin = cfg.rcut / float(np.float32(Nr)) if Nr else 0.0
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.bop_init(rnb, window, Nh, Nr, rbin)
        ctx.bop_accumulate()
        got = ctx.bop_read()
    ns = 2 * window + 1
    for w in range(W):
        n, GN = 0, np.zeros(Nr, np.int64)
        for a in range(Nb - window, Nb + window + 1):
            c = _bond_and_pair_counts(P[w, a], cfg, rnb, Nr, rbin)
            n, GN = n + c[0], GN + (c[1] if Nr else 0)
        assert got["S"][w, 6] == n and n > 0.4 * ns * Np * (Np - 1), (w, got["S"][w, 6], n)
        assert np.array_equal(got["GN"][w], GN)
        assert np.array_equal(got["H"][w].sum(axis=1), [Np * ns] * 2)
        s = got["S"][w]
        assert np.all(s[:6] >= 0.0) and np.all(s[:6] <= ns * (1.0 + 1e-12)) and s[1] <= s[0] * (1 + 1e-12) and s[3] <= s[2] * (1 + 1e-12)
        assert s[0] <= s[4] * (1 + 1e-12) and s[2] <= s[5] * (1 + 1e-12)       # |mean of q_lm(i)| <= mean of |q_lm(i)|
        if Nr:
            assert np.all(np.abs(got["G"][w]) <= GN * (1.0 + 1e-12))           # |c_ij| <= 1


@pytest.mark.parametrize("dim", [2, 3])
def test_box_with_unequal_sides(gpu_lib, dim):
    Np, Nb, W = 65, 4, 2
    L = (Np / DENSITY[dim]) ** (1.0 / dim)
    cfg = _cfg(dim, Np, Nb, Lbox=[0.8 * L, 1.25 * L] if dim == 2 else [0.8 * L, 1.25 * L, L])
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(77 + dim))
    half = 0.5 * min(cfg.Lbox[:dim])
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for rnb in (min(_radius(dim, cfg.density, 12 if dim == 3 else 6), half), half):
            win = Window(P, cfg.Lbox, cfg.rcut2, rnb)
            _run(ctx, cfg, win, rnb, 2, 20, 50, f"unequal sides dim {dim} rnb {rnb:.4g}")
        # above half the shortest side, below half the longest: refused
        assert ctx.L.pigs_bop_init(ctx.h, half * (1.0 + 1e-12), 0, 20, 0, 0.0) == ST["PIGS_ERR_ARG"]


# ---- 2. perfect lattices through the ABI ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LATTICES))
def test_perfect_lattices_have_their_closed_forms(gpu_lib, name):
    build, rnb, Q4, Q6, tol = LATTICES[name]
    X, L = build()
    Np, dim = X.shape
    Nb, window, Nh, Nr, W = 2, 1, 20, 20, 2
    cfg = _cfg(dim, Np, Nb, Lbox=L[:dim])
    VT, WF = gpu_lib.build_tables(cfg)
    P = np.broadcast_to(X, (W, 2 * Nb + 1, Np, dim)).copy()
    ns = 2 * window + 1
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        _run(ctx, cfg, Window(P, cfg.Lbox, cfg.rcut2, rnb), rnb, window, Nh, Nr, f"lattice {name}")
        S = ctx.bop_read()
    for w in range(W):
        s, H = S["S"][w], S["H"][w]
        assert s[6] == COORDINATION[name] * Np * ns
        for k, Q in ((0, Q4), (2, Q6)):
            if Q is None:
                continue
            # the closed forms: the second moment to 1e-12 x slices (fcc: to the five digits known), the first through the root
            assert abs(s[k + 1] - ns * Q * Q) <= max(1e-12 * ns, ns * 2.0 * Q * tol), (name, k, s[k + 1] / ns, Q * Q)
            assert abs(s[k] - ns * Q) <= max(ns * 1e-12 / max(Q, 1e-6), ns * tol), (name, k, s[k] / ns, Q)
            assert abs(s[4 + k // 2] - ns * Q) <= max(ns * 1e-12 / max(Q, 1e-6), ns * tol)     # q_l(i) = Q_l for every i
            # every particle in the bin of Q_l (or, on an edge, its neighbour)
            b = min(int(Q * Nh), Nh - 1)
            assert H[k // 2][max(b - 1, 0):b + 2].sum() == Np * ns
        occ = S["GN"][w] > 0
        assert occ.any() and np.all(np.abs(S["G"][w][occ] / S["GN"][w][occ] - s[3] / ns) <= 1e-12 + 0.5 * QUANTUM)


# ---- 3. degenerate input ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,Np", [(2, 70), (3, 257)])
def test_degenerate_inputs_drop_out_as_in_numpy(gpu_lib, dim, Np):
    """Two coincident particles, a NaN and an Inf coordinate, a particle outside the box: walker 0 has them, walker 1 is
    clean and keeps its bits."""
    Nb, window, W, Nh, Nr = 3, 1, 2, 20, 30
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    clean = _random_paths(cfg, W, np.random.default_rng(5 * dim))
    P = clean.copy()
    L = np.asarray(cfg.Lbox[:dim])
    P[0, :, 1] = P[0, :, 0]
    P[0, Nb, 2, 0] = np.nan
    P[0, Nb - 1, 3, dim - 1] = np.inf
    P[0, Nb + 1, 4] = -np.inf
    P[0, :, 5] = 1.3 * L
    rnb = min(_radius(dim, cfg.density, 12 if dim == 3 else 6), 0.5 * L.min())
    rbin = cfg.rcut / float(np.float32(Nr))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(clean)
        ctx.bop_init(rnb, window, Nh, Nr, rbin)
        ctx.bop_accumulate()
        ref = ctx.bop_read(reset=True)
        ctx.upload_all(P)
        win = Window(P, cfg.Lbox, cfg.rcut2, rnb)
        _run(ctx, cfg, win, rnb, window, Nh, Nr, f"degenerate dim {dim}")
        got = ctx.bop_read()
    for k in ("S", "H", "G", "GN"):
        assert np.array_equal(got[k][1], ref[k][1]), k
        assert np.all(np.isfinite(got[k][0])), k
    assert got["S"][0, 6] != ref["S"][0, 6]
    s = win.slice(0, Nb)
    assert s.n[2] == 0 and np.isnan(s.r2).any()                        # the inputs do what they are here for


# ---- 4. bit-for-bit independence ------------------------------------------------------------------------------------
def _same(a, b, what):
    for k in ("S", "H", "G", "GN", "samples"):
        assert np.array_equal(a[k], b[k]), (what, k)


def test_bits_do_not_depend_on_the_list_the_split_or_the_context(gpu_lib):
    W, Nb, window, Nh, Nr = 300, 2, 1, 10, 8
    rng = np.random.default_rng(9)
    for dim, Np in ((2, 5), (3, 70)):
        cfg = _cfg(dim, Np, Nb)
        VT, WF = gpu_lib.build_tables(cfg)
        P = _random_paths(cfg, W, rng)
        rnb = 0.5 * min(cfg.Lbox[:dim])
        rbin = cfg.rcut / float(np.float32(Nr))
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
            ctx.upload_all(P)
            ctx.bop_init(rnb, window, Nh, Nr, rbin)
            ctx.bop_accumulate()                                       # 300 entries: two launches
            whole = ctx.bop_read(reset=True)
            assert whole["samples"].tolist() == [1] * W
            ctx.bop_accumulate(list(range(W - 1, -1, -1)))            # the other order, split elsewhere
            _same(ctx.bop_read(reset=True), whole, "reversed list")
            for lo in range(0, W, 100):
                ctx.bop_accumulate(list(range(lo, lo + 100)))
            _same(ctx.bop_read(reset=True), whole, "three lists")
            # a walker listed twice against two calls
            ctx.bop_accumulate([7, 3, 7, 299, 7])
            twice = ctx.bop_read(reset=True)
            for wl in ([7, 3], [7, 299], [7]):
                ctx.bop_accumulate(wl)
            _same(ctx.bop_read(reset=True), twice, "a walker listed three times")
            assert twice["samples"][[3, 7, 299]].tolist() == [1, 3, 1] and twice["samples"].sum() == 5
            assert np.array_equal(twice["H"][7], 3 * whole["H"][7]) and np.array_equal(twice["S"][3], whole["S"][3])
            # interleaved with other families
            ctx.grv_init(4, window)
            ctx.tau_init()
            ctx.bop_accumulate([1, 2])
            ctx.grv_accumulate()
            ctx.tau_accumulate()
            ctx.bop_accumulate([2])
            mixed = ctx.bop_read(reset=True)
            ctx.bop_accumulate([1, 2])
            ctx.bop_accumulate([2])
            _same(ctx.bop_read(reset=True), mixed, "interleaved grv and tau")
            # the restatement, on a few walkers
            win = Window(P[:3], cfg.Lbox, cfg.rcut2, rnb)
            exp = win.expected(range(3), Nb, window, Nr, rbin)
            _check({k: v[:3] for k, v in whole.items()}, exp, Np, Nh, window, f"300 walkers dim {dim}")
        # another context with one walker: the same worldline, the same bits
        with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as one:
            one.upload_all(P[5:6])
            one.bop_init(rnb, window, Nh, Nr, rbin)
            one.bop_accumulate()
            got = one.bop_read()
            for k in ("S", "H", "G", "GN", "samples"):
                assert np.array_equal(got[k][0], whole[k][5]), k


# ---- 5. reset mask, re-init and refusals -----------------------------------------------------------------------------
def test_reset_mask_and_reinit(gpu_lib):
    W, Nb, Np, dim = 4, 3, 40, 3
    cfg = _cfg(dim, Np, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    P = _random_paths(cfg, W, np.random.default_rng(4))
    rnb = 0.5 * min(cfg.Lbox[:dim])
    win = Window(P, cfg.Lbox, cfg.rcut2, rnb)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        _run(ctx, cfg, win, rnb, 1, 10, 6, "before the mask", walkers=[3, 1, 0])
        first = ctx.bop_read(reset=[0, 1, 0, 1])
        assert first["samples"].tolist() == [1, 1, 0, 1]
        after = ctx.bop_read()
        assert after["samples"].tolist() == [1, 0, 0, 0]
        for k in ("S", "H", "G", "GN"):
            assert np.array_equal(after[k][0], first[k][0]) and not after[k][1:].any(), k
        # a second init resizes and zeroes, also with a call in flight
        ctx.bop_accumulate()
        ctx.bop_init(rnb, 2, 7, 0)
        z = ctx.bop_read()
        assert z["H"].shape == (W, 2, 7) and z["G"].shape == (W, 0) and not z["S"].any() and not z["H"].any() and not z["samples"].any()
        ctx.bop_accumulate([2])
        _check(ctx.bop_read(), win.expected([2], Nb, 2, 0, 0.0), Np, 7, 2, "after re-init")
        ctx.bop_read(reset=True)
        assert not ctx.bop_read()["S"].any()
        # the defaults: the context's radial grid
        ctx.bop_init(rnb)
        assert ctx.bop_read()["G"].shape == (W, cfg.Nbin) and ctx.bop_read()["H"].shape == (W, 2, 50)


def test_status_codes(gpu_lib):
    W, Nb = 2, 3
    ARG, OK, UNS = ST["PIGS_ERR_ARG"], ST["PIGS_OK"], ST["PIGS_ERR_UNSUPPORTED"]
    assert len({ARG, OK, UNS}) == 3
    cfg = _cfg(2, 30, Nb)
    VT, WF = gpu_lib.build_tables(cfg)
    half = 0.5 * min(cfg.Lbox[:2])
    dbl, lng = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    d = np.zeros(4096).ctypes.data_as(dbl)
    l = np.zeros(4096, np.int64).ctypes.data_as(lng)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(_random_paths(cfg, W, np.random.default_rng(2)))
        init = lambda *a: ctx.L.pigs_bop_init(ctx.h, *a)
        with pytest.raises(gpu_lib.PigsError):
            ctx.bop_accumulate()
        with pytest.raises(gpu_lib.PigsError):
            ctx.bop_read()
        assert ctx.L.pigs_bop_accumulate(ctx.h, 1, None) == ARG and ctx.L.pigs_bop_read(ctx.h, d, l, d, l, l, None) == ARG
        for rnb in (0.0, -1.0, float("nan"), float("inf"), half * (1 + 1e-12)):
            assert init(rnb, 0, 10, 5, 0.1) == ARG, rnb
        for window, Nh, Nr, rbin in ((-1, 10, 5, 0.1), (Nb + 1, 10, 5, 0.1), (0, 0, 5, 0.1), (0, 4097, 5, 0.1), (0, 10, -1, 0.1),
                                     (0, 10, 5, 0.0), (0, 10, 5, -0.1), (0, 10, 5, float("nan")), (0, 10, 5, float("inf")),
                                     (0, 10, 2 ** 27, 0.1)):
            assert init(half, window, Nh, Nr, rbin) == ARG, (window, Nh, Nr, rbin)
            with pytest.raises(gpu_lib.PigsError):
                ctx.bop_init(half, window, Nh, Nr, rbin)
        assert ctx.L.pigs_bop_accumulate(ctx.h, 1, None) == ARG           # init stays undone
        # the limits themselves are accepted; rbin is ignored where Nr = 0
        assert init(half, Nb, 4096, 0, float("nan")) == OK
        ctx.bop_init(half, 0, 1, 1, 1e-300)
        for bad in ([2], [-1], [0, 2]):
            with pytest.raises(gpu_lib.PigsError):
                ctx.bop_accumulate(bad)
        assert ctx.L.pigs_bop_accumulate(ctx.h, -1, None) == ARG
        assert ctx.L.pigs_bop_read(ctx.h, None, l, d, l, l, None) == ARG and ctx.L.pigs_bop_read(ctx.h, d, l, None, l, l, None) == ARG
        assert ctx.L.pigs_bop_accumulate(ctx.h, W, None) == OK
        assert ctx.bop_read()["samples"].tolist() == [1] * W              # the refused lists added nothing
    # one slice's table has to fit the LDS: 128 Np + 16 Nr + 800 bytes in 3D
    big = _cfg(3, 1300, 1)
    VT, WF = gpu_lib.build_tables(big)
    with gpu_lib.PigsContext(big, VT, WF, n_walkers=1) as ctx:
        h = 0.5 * min(big.Lbox)
        assert ctx.L.pigs_bop_init(ctx.h, h, 0, 10, 100, 0.1) == ARG
        assert ctx.L.pigs_bop_init(ctx.h, h, 0, 10, 0, 0.0) == OK
    # trapped and 1D contexts: unsupported, a status of its own
    tcfg = SystemConfig(dim=2, Np=6, Nb=2, trap=True, a_ho=[1.0, 1.3], Nmax=2000, Rm=1.2, dt=0.01)
    for c in (tcfg, SystemConfig(dim=1, Np=8, Nb=2, density=0.2)):
        VT, WF = gpu_lib.build_tables(c)
        with gpu_lib.PigsContext(c, VT, WF, n_walkers=1) as ctx:
            assert ctx.L.pigs_bop_init(ctx.h, 0.1, 0, 10, 5, 0.1) == UNS
            assert ctx.L.pigs_bop_accumulate(ctx.h, 1, None) == ARG       # still before init
            with pytest.raises(gpu_lib.PigsError, match="periodic|2D"):
                ctx.bop_init(0.1)
            ctx.sync()                                                    # the context still works


# ---- 6. the front end -------------------------------------------------------------------------------------------------
RUNS = os.path.join(ROOT, "tests", "golden", "vpi_runs")
PRINT = 1.0000001e-9            # the files carry 10 significant digits


def _block_values(gpu_lib, cfg, steps, rnb, window, Nh, Nr, rbin):
    """One block through PigsContext.bop_* and normalize_bop: `steps` are the worldlines [1, M, Np, dim] after each of the
    block's (diagonal) steps.  (scalars [5], distributions [2 Nh] with q4's bins first, G6 [Nr] with empty bins as 0)."""
    from pathintegralgroundstate_amd.profiles import normalize_bop
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
        ctx.bop_init(rnb, window, Nh, Nr, rbin)
        for P in steps:
            ctx.upload_all(P)
            ctx.bop_accumulate()
        n = normalize_bop(ctx.bop_read(reset=True), cfg.Np, window)
    b = np.array([n[k][0] for k in ("Q4", "Q6", "q4", "q6", "coordination")])
    return b, np.concatenate([n["P4"][0], n["P6"][0]]), np.nan_to_num(n["G6"][0], nan=0.0)


def _compare_files(d, blocks, Nh, Nr, rbin, what):
    """bo_vpi.out, boh_vpi.out and g6_vpi.out in d against the block values (scalars, distributions, G6) of every
    block: means to one unit of the tenth printed digit, errors as the root of a difference of two moments."""
    nb = len(blocks)
    for f, k, shape in (("bo_vpi.out", 0, (1, 10)), ("boh_vpi.out", 1, (Nh, 5)), ("g6_vpi.out", 2, (Nr, 3))):
        x = np.stack([b[k] for b in blocks])
        mean = x.mean(axis=0)
        err = np.sqrt(np.maximum((x * x).mean(axis=0) - mean * mean, 0.0) / nb)
        tab = np.atleast_2d(np.loadtxt(os.path.join(d, f)))
        assert tab.shape == shape, (what, f, tab.shape)
        if k == 0:
            gm, ge = tab[0, 0::2], tab[0, 1::2]
        elif k == 1:
            assert np.allclose(tab[:, 0], (np.arange(Nh) + 0.5) / Nh, rtol=PRINT, atol=0)
            gm, ge = np.concatenate([tab[:, 1], tab[:, 3]]), np.concatenate([tab[:, 2], tab[:, 4]])
        else:
            assert np.allclose(tab[:, 0], (np.arange(Nr) + 0.5) * rbin, rtol=PRINT, atol=0)
            gm, ge = tab[:, 1], tab[:, 2]
        mtol = PRINT * np.abs(mean)
        assert np.all(np.abs(gm - mean) <= mtol), (what, f, np.abs(gm - mean).max())
        ok = np.abs(ge - err) <= np.sqrt(4.0 * np.abs(mean) * mtol) + PRINT * np.abs(err)
        assert np.all(ok | np.isnan(ge) & (err <= np.sqrt(4.0 * np.abs(mean) * mtol))), (what, f)
        assert mean.any(), (what, f)


@pytest.fixture(scope="module")
def exe(gpu_lib):
    import subprocess
    host = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
    subprocess.check_call(["make", "-s", "-C", host])
    return os.path.join(host, "pigs_vpi")


def test_front_end_2d_two_blocks_of_three_steps(gpu_lib, oracle, exe, tmp_path):
    """he4_cworm0 (2D, CWorm = 0: every step is a diagonal one) with the key on, against a replay of the run's chain
    (test_gpu_front_end_blocks.replay) through PigsContext.bop_* and normalize_bop."""
    from test_gpu_front_end_blocks import _input, _run as run_vpi, replay
    Nblock, Nstep, rnb, window, Nh, Nr = 2, 3, 2.5, 2, 10, 12
    txt, cfg = _input("he4_cworm0", Nblock, Nstep)
    plain, on = str(tmp_path / "plain"), str(tmp_path / "on")
    run_vpi(exe, txt, plain)
    out = run_vpi(exe, txt + f"&gpu\n bond_order = T, bo_rnb = {rnb}, bo_nhist = {Nh}, bo_nr = {Nr}, bo_window = {window}\n/\n", on)
    assert "Bond order" in out
    old = sorted(os.listdir(plain))
    assert sorted(os.listdir(on)) == sorted(old + ["bo_vpi.out", "boh_vpi.out", "g6_vpi.out"])
    for f in old:
        if f not in ("stdout.txt", "vpi.in"):
            assert open(os.path.join(plain, f), "rb").read() == open(os.path.join(on, f), "rb").read(), f
    rep = replay(gpu_lib, oracle, cfg, 1, Nblock, Nstep)
    final = np.fromfile(os.path.join(on, "worldlines_final.bin")).reshape(rep["final"].shape)
    assert np.array_equal(final, rep["final"]) and rep["diag"].all()         # the replay IS the run
    rbin = cfg.rcut / Nr
    blocks = [_block_values(gpu_lib, cfg, rep["snaps"][b * Nstep:(b + 1) * Nstep], rnb, window, Nh, Nr, rbin) for b in range(Nblock)]
    assert not np.array_equal(blocks[0][0], blocks[1][0])                    # the blocks differ: the errors have teeth
    _compare_files(on, blocks, Nh, Nr, rbin, "he4_cworm0")


def test_front_end_crystal_start(gpu_lib, exe, tmp_path):
    """he4_crystal (27 particles on a lattice, box and density from config_ini.in) with the key on and the defaults of
    bo_nhist, bo_nr and bo_window.  The replay helper starts chains from random configurations only, so this run is
    one block of one diagonal step (CWorm = 0): the sample is taken on the worldline that the run then dumps."""
    import shutil
    from test_gpu_front_end_blocks import _run as run_vpi
    src = os.path.join(RUNS, "he4_crystal")
    ini = open(os.path.join(src, "config_ini.in")).read().split("\n")
    Np, L, dens = int(ini[0]), [float(x) for x in ini[1].split()], float(ini[2])
    txt = open(os.path.join(src, "vpi.in")).read()
    txt = re.sub(r"Nstep\s*=\s*\d+", "Nstep = 1", re.sub(r"Nblock\s*=\s*\d+", "Nblock = 1", txt))
    txt, k = re.subn(r"CWorm = 0.5d0", "CWorm = 0.0d0", txt)
    assert k == 1
    cfg = SystemConfig.from_namelists(txt, Np=Np, density=dens, Lbox=L)
    rnb = 0.9 * cfg.rcut
    d = str(tmp_path)
    shutil.copy(os.path.join(src, "config_ini.in"), d)
    out = run_vpi(exe, txt + f"&gpu\n bond_order = T, bo_rnb = {rnb!r}\n/\n", d)
    assert "Bond order" in out
    P = np.fromfile(os.path.join(d, "worldlines_final.bin")).reshape((1,) + tuple(cfg.path_shape))
    blocks = [_block_values(gpu_lib, cfg, [P], rnb, 0, 50, cfg.Nbin, cfg.rbin)]
    _compare_files(d, blocks, 50, cfg.Nbin, cfg.rbin, "he4_crystal")
    # and a radius above half the side is refused with exit status 2, before any file is written
    import subprocess
    bad = tmp_path / "bad"
    os.makedirs(bad)
    shutil.copy(os.path.join(src, "config_ini.in"), bad)
    r = subprocess.run([exe], input=(txt + f"&gpu\n bond_order = T, bo_rnb = {1.01 * cfg.rcut!r}\n/\n").encode(), cwd=bad,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 2 and b"bo_rnb" in r.stdout and not os.path.exists(bad / "e_vpi.out")
