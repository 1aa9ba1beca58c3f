"""Every kernel and the front end in a periodic box whose sides differ (the reference reads one length per axis from
config_ini.in when crystal = T, vpi.f90:99-122: LboxHalf(k), qbin(k) per axis, rcut = min L_k / 2).

Boxes: [7.3, 4.1, 5.9] (the shortest side, which sets rcut = 2.05, is axis 1), 1.6 (2, 3, 4) (commensurate with a
lattice) and the 2D box [5, 8]: side ratios that are no permutation of one another, so an axis read in another's place
shows.  The density is always Np / prod(Lbox).  References, tolerances and helpers are those of the cubic tests
(test_gpu_parity.py, test_gpu_large_np.py, test_gpu_sampler_size.py, test_gpu_sqv/fqv/fqs/fqt/grv/tau.py, test_gpu_host.py);
only the box is new.  Every case prints its worst error / bound ratio."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import delta_s_tolerance, same_bits, term_scales
from pathintegralgroundstate_amd import SystemConfig
from pathintegralgroundstate_amd.profiles import normalize_fqs
from test_gpu_host import crystal_start, exe  # noqa: F401  (exe: the front end, built once)
from test_gpu_k1_pipe2_edges import n_cu  # noqa: F401
from test_gpu_sampler_size import check_against_driver, run_k6
import fqs_numpy
import fqt_numpy
import fqv_numpy
import grv_numpy
import sqv_numpy
import tau_numpy
import test_gpu_fqs
import test_gpu_fqt
import test_gpu_fqv
import test_gpu_grv
import test_gpu_sqv
import test_gpu_tau

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")
REL = 1e-10
BOX3, BOX2 = [7.3, 4.1, 5.9], [5.0, 8.0]
SHAPES = [dict(dim=3, Np=37, Lbox=BOX3), dict(dim=3, Np=300, Lbox=BOX3), dict(dim=2, Np=20, Lbox=BOX2)]
WINDOW_SHAPES = [SHAPES[0], SHAPES[2]]


def _id(kw):
    return "dim%d_Np%d" % (kw["dim"], kw["Np"])


def _systems(kw, Nb=4):
    from oracle.pyoracle import System
    kw = dict(kw, Nb=Nb, density=kw["Np"] / float(np.prod(kw["Lbox"])))
    S, cfg = System(**kw), SystemConfig(**kw)
    L = np.asarray(kw["Lbox"])
    assert S.rcut == cfg.rcut == 0.5 * L.min() and np.array_equal(S.Lbox[:S.dim], L) and list(cfg.Lbox[:S.dim]) == list(L)
    assert len(set(L.tolist())) == S.dim
    return S, cfg


def _random_paths(S, W, rng):
    return rng.uniform(-0.5, 0.5, (W, S.M, S.Np, S.dim)) * np.asarray(S.Lbox[:S.dim])


def _lattice_paths(S, W, rng):
    """Jittered lattice (finite energies: no pair near the table's head), the same number of cells along every axis, so
    the spacings differ like the sides and pairs sit on both sides of rcut."""
    d = S.dim
    g = int(np.ceil(S.Np ** (1.0 / d) - 1e-9))
    L = np.asarray(S.Lbox[:d])
    cell = (np.stack(np.meshgrid(*[np.arange(g)] * d, indexing="ij"), -1).reshape(-1, d)[:S.Np] + 0.5) / g - 0.5
    P = (cell * L)[None, None] + rng.normal(0, 0.06 * L.min() / g, (W, S.M, S.Np, d))
    P = np.where(P > L / 2, P - L, P)
    return np.where(P < -L / 2, P + L, P)


# ---- K1 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", SHAPES, ids=_id)
def test_k1_every_variant_vs_oracle(gpu_lib, oracle, n_cu, kw):
    """Delta S of every K1 variant (those of test_every_k1_variant_vs_golden and of
    test_k1_every_variant_vs_oracle_beyond_256, and the automatic choice) against oracle.delta_action_batch on
    16 x CUs + 37 items, so that pipe2 runs: worldlines random in the box; a fifth of the proposals and of the old
    positions up to 1.9 L_k from the origin on one axis (the reference folds once, per axis).  NaN and +-Inf patterns equal,
    helpers.delta_s_tolerance with term_scales, variants 12 and 13 the same bits."""
    S, cfg = _systems(kw)
    d, W = S.dim, 2
    L = np.asarray(S.Lbox[:d])
    VT, WF = oracle.tables(S)
    rng = np.random.default_rng(77 * S.Np + d)
    Paths = _random_paths(S, W, rng)
    n = 16 * n_cu + 37
    w = rng.integers(0, W, n).astype(np.int32)
    ip = rng.integers(1, S.Np + 1, n).astype(np.int32)
    ib = rng.integers(0, S.M, n).astype(np.int32)
    ib[::9] = 0
    ib[4::9] = 2 * S.Nb
    ip[1::11] = S.Np
    xold = Paths[w, ib, ip - 1].copy()
    xnew = xold + rng.normal(0, 0.3, xold.shape)
    xnew = np.where(xnew > L / 2, xnew - L, xnew)
    xnew = np.where(xnew < -L / 2, xnew + L, xnew)
    for x in (xnew, xold):
        far = np.flatnonzero(rng.uniform(size=n) < 0.2)
        ax = rng.integers(0, d, far.size)
        x[far, ax] = rng.uniform(-1.9, 1.9, far.size) * L[ax]
        assert (np.abs(x) > 0.5 * L).any(axis=1).sum() > n // 10
    assert {0, 2 * S.Nb} <= set(ib.tolist()) and (ib % 2 == 1).any() and ((ib % 2 == 0) & (ib > 0) & (ib < 2 * S.Nb)).any()
    want = oracle.delta_action_batch(S, WF, VT, Paths, w, ip, ib, xnew, xold)
    fin = np.isfinite(want)
    assert fin.mean() > 0.5, fin.mean()
    sv, sf, su = np.zeros(n), np.zeros(n), np.zeros(n)
    for k in range(W):
        m = w == k
        sv[m], sf[m], su[m] = term_scales(S, VT, WF, Paths[k], ip[m], ib[m], xnew[m], xold[m])
    tol = delta_s_tolerance(S, sv, sf, su)
    res = {}
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(Paths)
        for v in (1, 2, 7, 8, 12, 13, 14, 0):
            ctx.set_tuning("k1_variant", v)
            res[v] = ctx.delta_action_batch(w, ip, ib, xnew, xold)
    for v, got in res.items():
        err = np.abs(got - want)
        print(f"{_id(kw)} variant {v}: max err / tol = {np.max((err / tol)[fin]):.3f} over {int(fin.sum())} finite of {n} items")
    for v, got in res.items():
        assert np.array_equal(np.isnan(got), np.isnan(want)), v
        assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), v
        assert np.all(np.abs(got - want)[fin] <= tol[fin]), (v, np.max((np.abs(got - want) / tol)[fin]))
    assert same_bits(res[12], res[13]), int(np.sum(res[12].view(np.uint64) != res[13].view(np.uint64)))


# ---- K2 / K3, K4, K7 ------------------------------------------------------------------------------------------------------
def _close_rel(a, b, rel=REL):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.all(np.abs(a - b) <= rel * np.abs(b))


def _worst_rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.max(np.abs(a - b) / np.abs(b)))


# W = 2 for every shape; `lds` only where k_slice_energy_lds can run (Np <= 256, pigs_kernels.hip launch_slice_energy)
ESTIMATOR_CASES = [(kw, False) for kw in SHAPES] + [(kw, True) for kw in SHAPES if kw["Np"] <= 256]


@pytest.mark.parametrize("kw,many", ESTIMATOR_CASES, ids=[_id(kw) + ("-lds" if m else "-W2") for kw, m in ESTIMATOR_CASES])
def test_estimator_kernels_vs_oracle(gpu_lib, oracle, n_cu, kw, many):
    """potential_energy_slice (odd, even and end slices, with and without F2), therm_energy_batch, local_energy_batch at
    1e-10 and structure_batch (g(r) bit-identical, S(k) to 1e-12 (|S(k)| + Np)) against the oracle, as
    test_estimator_kernels_vs_oracle_beyond_256 and test_structure_estimators_vs_oracle assert.  `lds`: as many walkers as
    give 8 x CUs slices in one therm_energy_batch launch, the threshold of k_slice_energy_lds, as
    test_therm_energy_many_walkers_lds_table_kernel chooses it (the count of CUs is rocminfo's; the API does not report
    which form of K2 ran: that the LDS form ran is inferred from the launch rule, not observed; two walkers listed alone
    -- 2 M slices: the per-slice kernel -- are compared too)."""
    S, cfg = _systems(kw)
    W = -(-8 * n_cu // S.M) if many else 2
    VT, WF = oracle.tables(S)
    assert not many or (S.Np <= 256 and W * S.M >= 8 * n_cu > 2 * S.M)
    Paths = _lattice_paths(S, W, np.random.default_rng(5 * S.Np + S.dim + W))
    slices = (0, 1, 2, 2 * S.Nb - 1, 2 * S.Nb)
    some = sorted({0, 1, W // 2, W - 1})
    Nk = 20
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(Paths)
        te = ctx.therm_energy_batch()
        sub = ctx.therm_energy_batch(walkers=some[:2])
        pot = {(k, b, f): ctx.potential_energy_slice(k, b, f) for k in some for b in slices for f in (False, True)}
        le = {b: ctx.local_energy_batch(b) for b in (0, 2 * S.Nb)}
        st = ctx.structure_batch(S.Nb, S.Nbin, S.rbin, Nk)
    worst = 0.0
    inside = []
    for k in range(W):
        want = np.array(oracle.therm_energy(S, VT, Paths[k]))
        assert np.all(np.isfinite(want))
        worst = max(worst, _worst_rel([te[0][k], te[1][k], te[2][k]], want))
        assert _close_rel([te[0][k], te[1][k], te[2][k]], want), (k, te[0][k], want)
    for j, k in enumerate(some[:2]):
        assert _close_rel([sub[0][j], sub[1][j], sub[2][j]], oracle.therm_energy(S, VT, Paths[k])), k
    for k in some:
        for b in slices:
            p, f2 = oracle.potential_energy(S, VT, Paths[k][b], True)
            p0, _ = oracle.potential_energy(S, VT, Paths[k][b], False)
            assert np.isfinite(p) and np.isfinite(f2) and p0 == p
            worst = max(worst, _worst_rel(pot[k, b, True], [p, f2]))
            assert _close_rel(pot[k, b, True], [p, f2]), (k, b)
            assert _close_rel(pot[k, b, False][0], p), (k, b)
        for b in (0, 2 * S.Nb):
            want = np.array(oracle.local_energy(S, WF, VT, Paths[k][b]))
            assert np.all(np.isfinite(want))
            worst = max(worst, _worst_rel([le[b][0][k], le[b][1][k], le[b][2][k]], want))
            assert _close_rel([le[b][0][k], le[b][1][k], le[b][2][k]], want), (k, b)
        gr = oracle.pair_correlation(S, Paths[k][S.Nb])
        inside.append(gr.sum() / (S.Np * (S.Np - 1)))                  # PairCorrelation adds 2 per pair inside rcut
        assert same_bits(st[0][k], gr)
        want = oracle.structure_factor(S, Nk, Paths[k][S.Nb])
        bound = 1e-12 * (np.abs(want) + S.Np)
        worst_sk = float(np.max(np.abs(st[1][k] - want) / bound))
        assert np.all(np.abs(st[1][k] - want) <= bound), worst_sk
    print(f"{_id(kw)} W {W}: energies max rel err / 1e-10 = {worst / REL:.3e}; S(k) max err / bound = {worst_sk:.3e}; "
          f"pairs inside rcut {min(inside):.2f}..{max(inside):.2f}")
    assert 0.0 < min(inside) and max(inside) < 0.6                     # most pairs lie beyond the cutoff


# ---- K6 -------------------------------------------------------------------------------------------------------------------
K6_FORMS = [(None, 0, None), (256, 0, 0), (None, 1, None), (None, 0, 0), (None, 1, 0), (None, 0, 2)]
K6_RUNS = {"bis": ["ortho_bis_s1982", "ortho_bis_s1983"], "worm": ["ortho_worm_s7", "ortho_worm_s8"],
           "sta2d": ["ortho2d_sta_s1982", "ortho2d_sta_s1983"]}


@pytest.mark.parametrize("threads,split,cm", K6_FORMS)
@pytest.mark.parametrize("run", list(K6_RUNS))
def test_k6_unequal_sides(gpu_lib, oracle, run, threads, split, cm):
    """run_k6 / check_against_driver on the reference's chains in boxes with unequal sides, two walkers = two seeds: the
    forms of test_k6_config3_n256_161_beads and TranslateChain by two cooperating workgroups (pigs_cm.hip)."""
    names = K6_RUNS[run]
    r = run_k6(gpu_lib, oracle, names, threads, split, cm)
    cfg = r["cfg"]
    L = cfg.Lbox[:cfg.dim]
    assert len(set(L)) == cfg.dim and cfg.rcut == 0.5 * min(L) and cfg.density == cfg.Np / float(np.prod(L))
    for w in range(2):
        c = r["drv"][w]["counters"]
        assert c[0] > 0 and c[1] > 0 and c[2] > 0 and c[3] > 0          # accepted TranslateChain, head, tail, bisection / staging
        if run == "worm":
            assert c[5] >= 1 and c[7] >= 1 and c[13] >= 1 and r["drv"][w]["nrho_total"][:, 0].sum() > 0
    f = r["form"]
    print(f"{run} threads {threads} split {split} cm {cm}: sampler form {f}")
    assert r["counters"][:, 14].min() > 0                                # TranslateChain was attempted
    if cm is not None:
        assert f["cm_H"] == cm, f                                         # 2: the TranslateChain kernel; 0: the sweep kernel
    if threads:
        assert f["sweep_threads"] == threads, f
    assert f["stage_machine"] == (bool(split) and cfg.sampling == "bis"), f   # the stage machine runs the bisection moves only
    for w in range(2):
        worst, rel = check_against_driver(r, w)
        print(f"{run} walker {w}: worldline max |d| = {worst:.2e}, step energies max rel = {rel:.2e}")


# ---- the window estimators against their numpy restatements ---------------------------------------------------------------
def _window_case(gpu_lib, kw, seed, paths=_random_paths):
    S, cfg = _systems(kw)
    VT, WF = gpu_lib.build_tables(cfg)
    P = paths(S, 2, np.random.default_rng(seed * 1000 + S.Np))
    return S, cfg, VT, WF, P


def _nmaxes(dim):
    return (2, 3) if dim == 3 else (5, 6)          # 62, 171, 60 and 84 vectors: no multiple of a tile width


@pytest.mark.parametrize("kw", WINDOW_SHAPES, ids=_id)
def test_sqv_fqv_match_numpy(gpu_lib, kw):
    """pigs_sqv and pigs_fqv under the bounds of test_gpu_sqv.py / test_gpu_fqv.py; lag 0 of F(q,tau) is bitwise the vector
    S(q) of the same window."""
    S, cfg, VT, WF, P = _window_case(gpu_lib, kw, 1)
    W, Nb, dim = 2, S.Nb, S.dim
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for nmax, window, Ntau in zip(_nmaxes(dim), (4, 3), (8, 2)):
            ctx.sqv_init(nmax, window)
            n = ctx.sqv_vectors()
            assert np.array_equal(n, sqv_numpy.vectors(dim, nmax)) and len(n) % 32 != 0
            ctx.sqv_accumulate()
            sq = ctx.sqv_read()
            A, B, cnt = sqv_numpy.expected(P, range(W), Nb, window, n, cfg.Lbox)
            assert np.array_equal(sq["samples"], cnt)
            test_gpu_sqv._assert_close(sq["S"], A, B, f"sqv {_id(kw)} nmax {nmax} W {window}")
            ctx.fqv_init(nmax, Ntau, window)
            assert np.array_equal(ctx.fqv_vectors(), n)
            ctx.fqv_accumulate()
            fq = ctx.fqv_read()
            F, Bf, cntf = fqv_numpy.expected(P, range(W), Nb, window, Ntau, n, cfg.Lbox)
            assert fq["F"].shape == (W, Ntau + 1, n.shape[0]) and np.array_equal(fq["samples"], cntf)
            test_gpu_fqv._assert_close(fq["F"], F, Bf, f"fqv {_id(kw)} nmax {nmax} W {window} Ntau {Ntau}")
            assert same_bits(fq["F"][:, 0], sq["S"])


@pytest.mark.parametrize("kw", WINDOW_SHAPES, ids=_id)
def test_fqs_matches_numpy(gpu_lib, kw):
    """pigs_fqs under test_gpu_fqs.py's bounds; F_s(q, 0) = 1 and D(0) = 0 exactly."""
    S, cfg, VT, WF, P = _window_case(gpu_lib, kw, 2)
    W, Nb, dim = 2, S.Nb, S.dim
    assert S.Np * (2 * Nb + 1) <= 4000
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for nmax, window, Ntau in zip(_nmaxes(dim), (4, 3), (8, 2)):
            ctx.fqs_init(nmax, Ntau, window)
            n = ctx.fqs_vectors()
            assert np.array_equal(n, fqs_numpy.vectors(dim, nmax))
            ctx.fqs_accumulate()
            got = ctx.fqs_read()
            assert got["F"].shape == (W, Ntau + 1, n.shape[0]) and got["D"].shape == (W, Ntau + 1, 2)
            e = fqs_numpy.expected(P, range(W), Nb, window, Ntau, n, cfg.Lbox)
            test_gpu_fqs._assert_matches(got, e, f"fqs {_id(kw)} nmax {nmax} W {window} Ntau {Ntau}")
            Fs = normalize_fqs(got["F"], got["samples"], S.Np, window)
            assert np.all(np.abs(Fs[:, 0] - 1.0) <= 1e-12)
            assert not got["D"][:, 0].any()


@pytest.mark.parametrize("kw", WINDOW_SHAPES, ids=_id)
def test_fqt_matches_numpy(gpu_lib, kw):
    """pigs_fqt (qbin[k] per axis) under test_gpu_fqt.py's bound."""
    S, cfg, VT, WF, P = _window_case(gpu_lib, kw, 3)
    W, Nb, dim = 2, S.Nb, S.dim
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for Nk, window, Ntau in ((7, 4, 8), (13, 3, 2)):
            ctx.fqt_init(Nk, Ntau, window)
            ctx.fqt_accumulate()
            got = ctx.fqt_read()
            F, B, n = fqt_numpy.expected(P, range(W), Nb, window, Ntau, Nk, cfg.Lbox)
            assert got["F"].shape == (W, Ntau + 1, Nk, dim) and np.array_equal(got["samples"], n)
            test_gpu_fqt._assert_close(got["F"], F, B, f"fqt {_id(kw)} Nk {Nk} W {window} Ntau {Ntau}")


@pytest.mark.parametrize("kw", WINDOW_SHAPES, ids=_id)
def test_grv_matches_numpy(gpu_lib, kw):
    """pigs_grv (bin widths b[k] = L_k / Nbin per axis; radial part to rcut from the shortest side): every count equal,
    in every form; the vector grid totals pairs x slices minus what the bin rule excludes, by the reference's count."""
    S, cfg, VT, WF, P = _window_case(gpu_lib, kw, 4)
    W, Nb, dim = 2, S.Nb, S.dim
    pairs = S.Np * (S.Np - 1) // 2
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for Nbin, window in ((7, 3), (12, 4)):
            ref = grv_numpy.Window(P, Nb, window, cfg.Lbox, cfg.rcut2)
            for Nr in (50, 7):
                rbin = test_gpu_grv._rbin(cfg, Nr)
                V, R, cnt, dropped = ref.expected(range(W), Nbin, Nr, rbin)
                assert 0 < R.sum() < V.sum()                           # most pairs lie beyond the cutoff
                for form in test_gpu_grv._forms(gpu_lib, ctx, dim, Nbin, Nr, lambda: ctx.grv_init(Nbin, window, Nr, rbin)):
                    ctx.grv_accumulate()
                    got = ctx.grv_read()
                    assert got["vec"].sum() == W * (2 * window + 1) * pairs - dropped == V.sum(), (form, Nbin, window)
                    test_gpu_grv._check(got, V, R, cnt, f"grv {_id(kw)} Nbin {Nbin} W {window} Nr {Nr} form {form}")


@pytest.mark.parametrize("kw", WINDOW_SHAPES, ids=_id)
def test_tau_matches_numpy(gpu_lib, kw):
    """pigs_tau under test_gpu_tau.py's bound, 1e-12 x the sum of the terms' magnitudes, on random worldlines (no pair
    within three table cells of the NaN / -Inf head: asserted)."""
    S, cfg, VT, WF, P = _window_case(gpu_lib, kw, 5)
    W, Nb = 2, S.Nb
    lo, hi = tau_numpy.min_max_distance(P, cfg)
    assert lo > 3 * cfg.dr and hi > cfg.rcut, (lo, hi)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.tau_init()
        ctx.tau_accumulate()
        got = ctx.tau_read()
    Q, A, n = tau_numpy.expected(P, list(range(W)), VT, cfg)
    assert got["Q"].shape == (W, 2 * Nb + 1, 4) and np.array_equal(got["samples"], n)
    assert not got["Q"][:, :, 1].any() and not got["Q"][:, 2 * Nb, 3].any()
    test_gpu_tau._assert_close(got["Q"], Q, A, f"tau {_id(kw)}")


# ---- the front end --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", ["F", "T"])
def test_front_end_crystal_start_unequal_sides(exe, dev, tmp_path):
    """he4_crystal_ortho (a 2x3x4 lattice in a (2, 3, 4), box and density from config_ini.in) through pigs_vpi with both
    samplers, with the assertions of test_gpu_crystal_start_from_config_ini."""
    crystal_start(exe, dev, "he4_crystal_ortho", tmp_path)


PRINT = 1.0000001e-9            # the files carry 10 significant digits


def _rows(path):
    return [[float(t) for t in ln.split()] for ln in open(path) if ln.strip() and not ln.startswith("#")]


@pytest.mark.parametrize("ds", ["T", "F"])
def test_front_end_one_sample_equals_numpy_unequal_sides(gpu_lib, exe, tmp_path, ds):
    """One block of one step of he4_crystal_ortho (CWorm = 0, so the step is a diagonal one) with sq_vector, fq_vector,
    fq_self, gr_vector and tau_profile on: the single sample is taken on the worldline that the run then dumps, so numpy
    on worldlines_final.bin is the whole expectation, as in the test_front_end_one_sample_equals_numpy tests.  Bounds: each
    kernel's own, normalised, plus one unit of the last printed digit.  Box, Np and density are config_ini.in's (24
    particles at 0.45 in a (2, 3, 4)), not the namelist's (8 at 0.2): the shell files come from the front end's branch
    for unequal sides, the vector g(r) from one bin width per axis, the pressure from the file's density."""
    import re
    import shutil
    from pathintegralgroundstate_amd.profiles import (normalize_grv, normalize_msd, normalize_tau, pressure_virial,
                                                      shell_average)
    src = os.path.join(RUNS, "he4_crystal_ortho")
    ini = open(os.path.join(src, "config_ini.in")).read().split("\n")
    Np, L, dens = int(ini[0]), [float(x) for x in ini[1].split()], float(ini[2])
    txt = open(os.path.join(src, "vpi.in")).read()
    txt = re.sub(r"Nstep\s*=\s*\d+", "Nstep = 1", re.sub(r"Nblock\s*=\s*\d+", "Nblock = 1", txt))
    txt, k = re.subn(r"CWorm = 0.5d0", "CWorm = 0.0d0", txt)
    assert k == 1 and "crystal = T" in txt and "Np = 8" in txt and "density = 0.2d0" in txt
    cfg = SystemConfig.from_namelists(txt, Np=Np, density=dens, Lbox=L)
    assert Np == 24 and len(set(L)) == 3 and cfg.rcut == 0.5 * min(L) and abs(Np / np.prod(L) / dens - 1) < 1e-14
    dim, Nb, dt = cfg.dim, cfg.Nb, cfg.dt
    nmax, window, Ntau, nmax_s, Ng, gwin, twin = 3, 2, 3, 2, 7, 2, 2
    d = str(tmp_path)
    shutil.copy(os.path.join(src, "config_ini.in"), d)
    out = test_gpu_fqv._run(exe, txt + f"&gpu\n device_sampler = {ds}, sq_vector = T, sq_nmax = {nmax}, sq_window = {window}, "
                            f"fq_vector = T, fqv_nmax = {nmax}, fqv_ntau = {Ntau}, fq_self = T, fqs_nmax = {nmax_s}, "
                            f"fqs_ntau = {Ntau}, gr_vector = T, gr_nbin = {Ng}, gr_window = {gwin}, tau_profile = T, "
                            f"tau_window = {twin}\n/\n", d)
    for banner in ("Vector S(q)", "Vector F(q,tau)", "Self F_s(q,tau)", "Vector g(r)", "V(tau)"):
        assert banner in out, banner
    P = np.fromfile(os.path.join(d, "worldlines_final.bin")).reshape((1,) + tuple(cfg.path_shape))
    assert np.all(np.abs(P) <= 0.5 * np.asarray(L))
    qb = 2 * np.pi / np.asarray(L)
    what = f"front end, unequal sides, ds {ds}: "

    # ---- sqvec_vpi.out, sq_vpi.out
    n = sqv_numpy.vectors(dim, nmax)
    Nq = n.shape[0]
    qmod = np.sqrt(((n * qb) ** 2).sum(axis=1))
    A, B, _ = sqv_numpy.expected(P, [0], Nb, window, n, L)
    norm = (2 * window + 1) * Np
    tab = np.loadtxt(os.path.join(d, "sqvec_vpi.out"))
    assert tab.shape == (Nq, dim + 3) and np.array_equal(tab[:, :dim], n)
    assert np.allclose(tab[:, dim], qmod, rtol=PRINT, atol=0)
    want = A[0] / norm
    test_gpu_sqv._assert_close(tab[:, dim + 1], want, B[0] / norm + PRINT * np.abs(want), what + "sqvec_vpi.out")
    sh = np.loadtxt(os.path.join(d, "sq_vpi.out"))
    q, mean, mult = shell_average(n, L, tab[:, dim + 1])
    assert q.size < Nq and mult.max() > 2                                # shells of several vectors exist: (+-n_1, +-n_2, +-n_3)
    assert len(set((n.astype(int) ** 2).sum(1).tolist())) < q.size      # ... and they are not the cubic branch's
    assert sh.shape == (q.size, 4) and np.array_equal(sh[:, 3], mult) and int(mult.sum()) == 2 * Nq
    assert np.allclose(sh[:, 0], q, rtol=PRINT, atol=0)
    assert np.all(np.abs(sh[:, 1] - mean) <= 2 * PRINT * np.abs(mean))

    # ---- fqvec_vpi.out, fqsh_vpi.out (fqv_window left out: ceiling(fqv_ntau / 2) = 2)
    F, Bf, _ = fqv_numpy.expected(P, [0], Nb, window, Ntau, n, L)
    normf = (2 * window + 1 - np.arange(Ntau + 1))[:, None] * float(Np)
    tab = np.loadtxt(os.path.join(d, "fqvec_vpi.out"))
    assert tab.shape == ((Ntau + 1) * Nq, dim + 5)
    assert np.array_equal(tab[:, 0], np.repeat(np.arange(Ntau + 1), Nq))
    assert np.allclose(tab[:, 1], tab[:, 0] * dt, rtol=PRINT, atol=0)
    assert np.array_equal(tab[:, 2:2 + dim], np.tile(n, (Ntau + 1, 1)))
    assert np.allclose(tab[:, 2 + dim], np.tile(qmod, Ntau + 1), rtol=PRINT, atol=0)
    want = F[0] / normf
    got = tab[:, 3 + dim].reshape(Ntau + 1, Nq)
    test_gpu_fqv._assert_close(got, want, Bf[0] / normf + PRINT * np.abs(want), what + "fqvec_vpi.out")
    sh = np.loadtxt(os.path.join(d, "fqsh_vpi.out"))
    q, mean, mult = shell_average(n, L, got)
    assert sh.shape == ((Ntau + 1) * q.size, 6)
    assert np.array_equal(sh[:, 0], np.repeat(np.arange(Ntau + 1), q.size))
    assert np.allclose(sh[:, 2], np.tile(q, Ntau + 1), rtol=PRINT, atol=0)
    assert np.array_equal(sh[:, 5], np.tile(mult, Ntau + 1)) and int(mult.sum()) == 2 * Nq
    tol = PRINT * (np.abs(mean) + shell_average(n, L, np.abs(got))[1])
    assert np.all(np.abs(sh[:, 3].reshape(Ntau + 1, q.size) - mean) <= tol)

    # ---- fqself_vpi.out, fqssh_vpi.out, msd_vpi.out
    ns_ = fqs_numpy.vectors(dim, nmax_s)
    Nqs = ns_.shape[0]
    e = fqs_numpy.expected(P, [0], Nb, window, Ntau, ns_, L)
    norms = fqs_numpy.n_pairs(window, Ntau).astype(np.float64) * float(Np)
    tab = np.loadtxt(os.path.join(d, "fqself_vpi.out"))
    assert tab.shape == ((Ntau + 1) * Nqs, dim + 5)
    assert np.array_equal(tab[:, 2:2 + dim], np.tile(ns_, (Ntau + 1, 1)))
    want = e["F"][0] / norms[:, None]
    got = tab[:, 3 + dim].reshape(Ntau + 1, Nqs)
    test_gpu_fqs._assert_close(got, want, e["Fb"][0] / norms[:, None] + PRINT * np.abs(want), what + "fqself_vpi.out")
    assert np.all(np.abs(got[0] - 1.0) <= 1e-12 + PRINT)                # F_s(q, 0) = 1
    sh = np.loadtxt(os.path.join(d, "fqssh_vpi.out"))
    q, mean, mult = shell_average(ns_, L, got)
    assert sh.shape == ((Ntau + 1) * q.size, 6)
    assert np.allclose(sh[:, 2], np.tile(q, Ntau + 1), rtol=PRINT, atol=0)
    assert np.array_equal(sh[:, 5], np.tile(mult, Ntau + 1)) and int(mult.sum()) == 2 * Nqs
    tol = PRINT * (np.abs(mean) + shell_average(ns_, L, np.abs(got))[1])
    assert np.all(np.abs(sh[:, 3].reshape(Ntau + 1, q.size) - mean) <= tol)
    msd = np.loadtxt(os.path.join(d, "msd_vpi.out"))
    assert msd.shape == (Ntau + 1, 5) and np.array_equal(msd[:, 0], np.arange(Ntau + 1))
    wm, wa = normalize_msd(e["D"][0], 1, Np, window, dim)
    test_gpu_fqs._assert_close(msd[:, 2], wm, e["Db"][0, :, 0] / norms + PRINT * np.abs(wm), what + "msd_vpi.out")
    assert msd[0, 2] == 0.0 and np.all(msd[1:, 2] > 0)

    # ---- grvec_vpi.out, grw_vpi.out: integer counts, so the printed digits are the whole bound
    V, R, cnt, dropped = grv_numpy.expected(P, [0], Nb, gwin, L, cfg.rcut2, Ng, cfg.Nbin, cfg.rbin)
    assert dropped == 0 and V.sum() == (2 * gwin + 1) * Np * (Np - 1) // 2
    g = normalize_grv({"vec": V[0], "radial": R[0], "samples": cnt[0]}, Np, gwin, dens, L, cfg.rbin, dim)
    tab = np.loadtxt(os.path.join(d, "grvec_vpi.out"))
    assert tab.shape == (Ng ** dim, dim + 2)
    j = np.arange(Ng ** dim)
    for k in range(dim):
        wantx = g["x"][k][(j // Ng ** k) % Ng]                           # x fastest
        assert np.allclose(tab[:, k], wantx, rtol=PRINT, atol=PRINT * L[k]), k
    gv = g["g_vec"].ravel()
    assert gv.max() > 0 and np.all(np.abs(tab[:, dim] - gv) <= PRINT * np.abs(gv)), np.max(np.abs(tab[:, dim] - gv))
    gw = np.loadtxt(os.path.join(d, "grw_vpi.out"))
    assert gw.shape == (cfg.Nbin, 3) and np.allclose(gw[:, 0], g["r"], rtol=PRINT, atol=0)
    assert g["g_r"].max() > 0 and np.all(np.abs(gw[:, 1] - g["g_r"]) <= PRINT * np.abs(g["g_r"]))
    print(what + f"grvec_vpi.out {int(V.sum())} counts, grw_vpi.out {int(R.sum())} counts: equal to the printed digits")

    # ---- tau_vpi.out, press_vpi.out
    VT, _ = gpu_lib.build_tables(cfg)
    Q, Aq, _ = tau_numpy.expected(P, [0], VT, cfg)
    t = normalize_tau({"Q": Q[0], "samples": 1}, Np, dim, dt)
    rows = _rows(os.path.join(d, "tau_vpi.out"))
    M = 2 * Nb + 1
    assert len(rows) == M and [len(r) for r in rows] == [10] * (M - 1) + [8] and [r[0] for r in rows] == list(range(M))
    for col, key, a in ((2, "vpair", 0), (6, "w", 2)):
        gotc = np.array([r[col] for r in rows])
        bound = 1e-12 * Aq[0, :, a] / Np + PRINT * np.abs(t[key])
        err = np.abs(gotc - t[key])
        print(what + f"tau_vpi.out {key}: max err / bound = {np.max(err / bound):.3e}")
        assert np.all(err <= bound), key
    assert all(r[4] == 0.0 for r in rows)                                # Vext of a periodic system
    kl = np.array([r[8] for r in rows[:-1]])
    bound = 1e-12 * Aq[0, :M - 1, 3] / (2.0 * dt * dt * Np) + PRINT * np.abs(t["klink"]) + 4e-16 * dim / (2.0 * dt)
    assert np.all(np.abs(kl - t["klink"]) <= bound)
    pr = np.array(_rows(os.path.join(d, "press_vpi.out")))
    ev = np.loadtxt(os.path.join(d, "e_vpi.out")).reshape(-1, 4)
    assert pr.shape == (1, 4) and pr[0, 0] == 1.0 and pr[0, 2] == ev[0, 2]                # Kin/N as e_vpi.out has it
    wwin = t["w"][Nb - twin:Nb + twin + 1].mean()
    wb = 1e-12 * Aq[0, Nb - twin:Nb + twin + 1, 2].mean() / Np
    assert abs(pr[0, 1] - wwin) <= wb + PRINT * abs(wwin), (pr[0, 1], wwin)
    want = pressure_virial(pr[0, 2], wwin, dens, dim)                                    # the FILE's density, 0.45
    tolp = dens / dim * wb + 5.0000001e-10 * (abs(pr[0, 3]) + dens / dim * (2 * abs(pr[0, 2]) + abs(wwin)))
    assert abs(pr[0, 3] - want) <= tolp, (pr[0, 3], want)
    assert abs(pr[0, 3] - pressure_virial(pr[0, 2], wwin, 0.2, dim)) > 100 * tolp          # ... the namelist's would show

