"""The cluster and percolation files of the front end -- clus_vpi, clusblk_vpi, perc_vpi, percsz_vpi, clpers_vpi -- per
walker AND walker-averaged, with both keys in one run, on one and on two contexts, and behind the other keys, against an
expectation built without the product's normalisation code.

Method: test_gpu_front_end_blocks.py's.  The run's chains are replayed through the API; cl_numpy and pc_numpy give the raw
sums of every diagonal walker from the snapshots of every step; block_stats_numpy.norm_cl / norm_pc turn a block's sums
into block values and walker_stats / walker_average / average_stats into the files' columns: the means over the counted
blocks, the walker-averaged block values over the walkers that counted a block (the all-reduced block vector and its
counts), the blocks nobody counted left out.  <Rg^2>(s), C(l) and the Jaccard index are ratios of block means, and the mean
finite size of a block without finite clusters enters as 0.

Tolerances (test_gpu_front_end_blocks.py): columns made of integer sums: one unit of the tenth printed digit (PRINT);
Rg^2 columns: the restatements' 1e-12 * Sum|terms| carried through the block means, plus PRINT; error columns:
sqrt(4 |mean| mtol) + PRINT |err|, and where the expected error lies below that it may be NaN, in at most 1 % of a
file's rows."""
import os

import numpy as np
import pytest

import block_stats_numpy as bs
import cl_numpy as cn
import pc_numpy as pn
from test_gpu_front_end_blocks import (A_PLUS, B_BLOCKS, B_STEPS, B_WALKERS, PRINT, _blocks, _gpu_group, _input, _rows, _run, _same,
                                       _same_files, _suffixes, check_replay_is_the_run, exe, replay)  # noqa: F401 (exe: a fixture)

pytestmark = pytest.mark.gpu
WINDOW, NTAU = 2, 3
RC_FACTOR = 0.78                # of rcut in the worm run: chosen on the replay's snapshots, see scn
CL_FILES, PC_FILES = ["clus_vpi", "clusblk_vpi"], ["perc_vpi", "percsz_vpi", "clpers_vpi"]


def keys_text(rc, cl=True, pc=True):
    return ((f", clusters = T, cl_rc = {rc!r}, cl_window = {WINDOW}" if cl else "") +
            (f", percolation = T, pc_rc = {rc!r}, pc_window = {WINDOW}, pc_ntau = {NTAU}" if pc else ""))


def group(W, rc, cl=True, pc=True, shard=False):
    return (f"&gpu\n n_walkers = {W}, device_sampler = T" + (", device = 0, n_gpus = 2, same_device = T" if shard else "") +
            keys_text(rc, cl, pc) + "\n/\n")


def block_values(rep, rc):
    """The block values [W, Nblock, ...] of both families from the replay's snapshots, zeros where a walker had no sample,
    with the bound of the two Rg^2 sums; "counted" [W, Nblock]."""
    cfg, snaps, diag, W = rep["cfg"], rep["snaps"], rep["diag"], rep["W"]
    L = cfg.Lbox[:cfg.dim]
    steps = {}
    for t in range(snaps.shape[0]):
        ws = [int(w) for w in np.flatnonzero(diag[t])]                 # the diagonal walkers of the step, nobody else
        c = cn.Window(snaps[t], cfg.Nb, WINDOW, L, rc).expected(ws)
        p = pn.Window(snaps[t], cfg.Nb, WINDOW, L, rc, NTAU).expected(ws)
        assert np.array_equal(c["samples"], p["samples"])
        for k, v in list(c.items()) + [("pc_" + k, v) for k, v in p.items()]:
            steps.setdefault(k, []).append(v)
    raw = {k: _blocks(np.stack(v), rep) for k, v in steps.items()}
    S = raw["samples"]
    cnt = S > 0
    assert np.array_equal(S, (2 * WINDOW + 1) * _blocks(diag.astype(np.int64), rep))
    cl = bs.norm_cl(raw["nsize"], raw["nlarge"], raw["nbond"], raw["rg2"], S, cfg.Np)
    pc = bs.norm_pc(raw["pc_nwrap"], raw["pc_mwrap"], raw["pc_swrap"], raw["pc_nfin"], raw["pc_rg2u"], raw["pc_first"],
                    raw["pc_second"], raw["pc_both"], raw["pc_norig"], S, cfg.Np, cfg.dim)
    out = {"counted": cnt, "raw": raw}
    for fam, d in (("cl", cl), ("pc", pc)):
        for k, v in d.items():
            v = np.array(v, np.float64)
            v[~cnt] = 0.0
            out[f"{fam}_{k}"] = v
    out["cl_Gb"], out["pc_Gb"] = 1e-12 * out["cl_G"], 1e-12 * out["pc_G"]     # non-negative terms: Sum|terms| is the sum
    return out


def _stats(E, name, w):
    return bs.walker_stats(E[name], E["counted"], w) if w is not None else bs.average_stats(E[name], E["counted"])


def _columns(tag, got_m, got_e, wm, we, mb, n):
    """Means within PRINT |mean| + bound, errors within sqrt(4 |mean| mtol) + PRINT |err|; NaN error bars only where the
    expectation is ill-conditioned.  Returns the rows with a NaN."""
    mtol = PRINT * np.abs(wm) + mb
    dm = np.abs(got_m - wm)
    assert np.all(np.isfinite(got_m)) and np.all(dm <= mtol), (tag, "means", float(np.max(dm / np.maximum(mtol, 1e-300))))
    etol = np.sqrt(4.0 * np.abs(wm) * mtol) + PRINT * np.abs(we)
    nan = np.isnan(got_e)
    assert not np.any(nan & ~(we <= etol)), (tag, "NaN error bars where the expectation is well-conditioned")
    de = np.where(nan, 0.0, np.abs(got_e - we))
    assert np.all(got_e[~nan] >= 0) and np.all(de <= etol), (tag, "errors", float(np.max(de / np.maximum(etol, 1e-300))))
    print(f"{tag}: n = {n}, means worst {float(np.max(dm / np.maximum(mtol, 1e-300))):.3e}, errors worst "
          f"{float(np.max(de / np.maximum(etol, 1e-300))):.3e} of the bound")
    return nan, bool(np.any(we > etol))


def _table(path, cols):
    rows = _rows(path)
    return np.array(rows, np.float64).reshape(-1, cols)


def check_series_files(d, E, w, cfg, what):
    """clus_vpi, percsz_vpi and clpers_vpi: walker w's, or the walker-averaged ones with w = None."""
    suffix = f".w{w:04d}" if w is not None else ""
    Np = cfg.Np
    # ---- clus_vpi: s, then n(s), s n(s)/Np and P_largest(s) with errors, then <G> / <n> with the error of <G> over <n>
    (mn, en, n), (mf, ef, _), (mp, ep, _) = (_stats(E, k, w) for k in ("cl_n", "cl_fraction", "cl_p_largest"))
    mG, eG, _ = _stats(E, "cl_G", w)
    bG = bs.mean_bound(E["cl_Gb"], E["counted"], w)
    path = os.path.join(d, f"clus_vpi{suffix}.out")
    if n == 0:
        assert np.all(np.isnan(_table(path, 9)[:, 1:])), (what, path)
    else:
        seen = np.flatnonzero(mn > 0)
        t = _table(path, 9)
        assert t.shape == (seen.size, 9) and np.array_equal(t[:, 0], seen + 1.0), (what, path, t[:, 0], seen + 1)
        gm = np.stack([t[:, 1], t[:, 3], t[:, 5], t[:, 7]])
        ge = np.stack([t[:, 2], t[:, 4], t[:, 6], t[:, 8]])
        wm = np.stack([mn[seen], mf[seen], mp[seen], mG[seen] / mn[seen]])
        we = np.stack([en[seen], ef[seen], ep[seen], eG[seen] / mn[seen]])
        mb = np.stack([np.zeros(seen.size)] * 3 + [bG[seen] / mn[seen]])
        assert w is not None or (seen.size >= 3 and np.any(mG[seen] > 0))
        nan, teeth = _columns(f"{what} clus_vpi{suffix}", gm, ge, wm, we, mb, n)
        assert nan.any(axis=0).sum() <= 0.01 * seen.size and (teeth or n == 1)
    # ---- percsz_vpi: s, n_fin / Np with its error, <G> / (Np <n_fin / Np>) with the error of <G> over the same
    mnf, enf, n = _stats(E, "pc_nfin", w)
    mG, eG, _ = _stats(E, "pc_G", w)
    bG = bs.mean_bound(E["pc_Gb"], E["counted"], w)
    path = os.path.join(d, f"percsz_vpi{suffix}.out")
    if n > 0:
        seen = np.flatnonzero(mnf > 0)
        t = _table(path, 5)
        assert t.shape == (seen.size, 5) and np.array_equal(t[:, 0], seen + 1.0), (what, path, t[:, 0], seen + 1)
        den = mnf[seen] * Np
    if n > 0 and seen.size:
        nan, teeth = _columns(f"{what} percsz_vpi{suffix}", np.stack([t[:, 1], t[:, 3]]), np.stack([t[:, 2], t[:, 4]]),
                              np.stack([mnf[seen], mG[seen] / den]), np.stack([enf[seen], eG[seen] / den]),
                              np.stack([np.zeros(seen.size), bG[seen] / den]), n)
        assert nan.any(axis=0).sum() <= 0.01 * seen.size and (teeth or n == 1)
    # ---- clpers_vpi: l, tau, first, second and both per origin with errors, C = <both> / <first>, the Jaccard index
    m, e, n = _stats(E, "pc_pairs", w)
    path = os.path.join(d, f"clpers_vpi{suffix}.out")
    if n > 0:
        t = _table(path, 10)
        nl = NTAU + 1
        assert t.shape == (nl, 10) and t[:, 0].tolist() == list(range(nl)) and np.allclose(t[:, 1], np.arange(nl) * cfg.dt, rtol=PRINT, atol=0)
        nan, teeth = _columns(f"{what} clpers_vpi{suffix}", t[:, 2:8:2], t[:, 3:8:2], m, e, np.zeros(m.shape), n)
        assert nan.any(axis=1).sum() <= 0.01 * nl and (teeth or n == 1)
        C = bs.ratio_of_means(m[:, 2], m[:, 0])
        J = bs.ratio_of_means(m[:, 2], m[:, 0] + m[:, 1] - m[:, 2])
        assert np.all(np.abs(t[:, 8] - C) <= 3 * PRINT * C) and np.all(np.abs(t[:, 9] - J) <= 4 * PRINT * J), (what, path)
        assert C[0] == 1.0 and J[0] == 1.0 and np.all(C <= 1.0) and np.all(C > 0) and np.all(J <= C)


def check_block_files(d, E, w, what):
    """clusblk_vpi and perc_vpi: one row per counted block, every column made of integer sums."""
    cnt = E["counted"]
    suffix = f".w{w:04d}" if w is not None else ""
    for name, key, cols in (("clusblk_vpi", "cl_block", 5), ("perc_vpi", "pc_block", 8)):
        v, cb = (E[key][w], cnt[w]) if w is not None else bs.walker_average(E[key], cnt)
        path = os.path.join(d, f"{name}{suffix}.out")
        assert open(path).readline().startswith("# block")
        t = _table(path, cols)
        blocks = np.flatnonzero(cb)
        assert t[:, 0].tolist() == (blocks + 1).tolist(), (what, path, t[:, 0].tolist(), cb.tolist())
        assert np.all(np.abs(t[:, 1:] - v[blocks]) <= PRINT * np.abs(v[blocks])), (what, path)


def check_cluster_files(d, out, rep, E, what):
    check_replay_is_the_run(d, out, rep)
    for w in list(range(rep["W"])) + [None]:
        check_series_files(d, E, w, rep["cfg"], what)
        check_block_files(d, E, w, what)


# ---- (a), (c): the worm run with empty and partial blocks -----------------------------------------------------------------
@pytest.fixture(scope="module")
def scn(gpu_lib, oracle):
    txt, cfg = _input("he4_wormbusy_s7", B_BLOCKS, B_STEPS)
    assert not cfg.trap and cfg.Nb >= WINDOW and cfg.dim == 3
    rep = replay(gpu_lib, oracle, cfg, B_WALKERS, B_BLOCKS, B_STEPS)
    rc = float(np.floor(RC_FACTOR * cfg.rcut * 1e6) / 1e6)            # six decimals: the namelist and numpy read one double
    E = block_values(rep, rc)
    cnt, raw = E["counted"], E["raw"]
    S = raw["samples"] // (2 * WINDOW + 1)
    print("diagonal steps per (walker, block):", S.tolist())
    # what the scenario is for, on the restatement alone
    assert (S == 0).any() and ((S >= 1) & (S <= B_STEPS - 1)).any() and (~cnt.any(axis=0)).any() and (cnt.sum(axis=0) == 1).any()
    several = raw["pc_nfin"][..., 1:].sum(axis=-1)                     # finite clusters of several particles per (walker, block)
    print("finite clusters of several particles per (walker, block):", several.tolist())
    assert raw["nsize"][..., 0].sum() > 0 and raw["nbond"].sum() > 0, "no singles beside bonded particles"
    assert (cnt & (several > 0)).any() and (cnt & (several == 0)).any(), "no block with and one without finite several-particle clusters"
    assert raw["pc_swrap"][..., 1:].sum() > 0 and np.unique(E["pc_block"][..., 5][cnt]).size >= 3    # P_inf varies over the blocks
    assert (E["pc_block"][..., 6][cnt] == 0).any() and (E["pc_block"][..., 6][cnt] > 1).any()
    return txt, rep, rc, E


def test_worm_run_both_keys_one_and_two_contexts(exe, scn, tmp_path):
    """he4_wormbusy_s7, 8 blocks x 6 steps, four walkers, clusters = T and percolation = T together: the five files of every
    walker and the five walker-averaged ones against the replay, unsharded and with n_gpus = 2, same_device = T; the sharded
    run's files are the unsharded run's byte for byte; every file of the run without the two keys is unchanged; and each key
    alone writes the bytes it writes with the other key on."""
    txt, rep, rc, E = scn
    W = rep["W"]
    dirs = {k: str(tmp_path / k) for k in ("plain", "on", "two", "cl", "pc")}
    _run(exe, txt + group(W, rc, False, False), dirs["plain"])
    out = _run(exe, txt + group(W, rc), dirs["on"])
    assert "Clusters" in out and "Percolation" in out
    check_cluster_files(dirs["on"], out, rep, E, "one context:")
    old = sorted(os.listdir(dirs["plain"]))
    new = sorted(set(os.listdir(dirs["on"])) - set(old))
    assert new == sorted(f"{b}{s}.out" for b in CL_FILES + PC_FILES for s in _suffixes(W)), new
    for f in old:
        if f not in ("stdout.txt", "vpi.in"):
            assert _same(dirs["plain"], dirs["on"], f), f
    out2 = _run(exe, txt + group(W, rc, shard=True), dirs["two"])
    check_cluster_files(dirs["two"], out2, rep, E, "two contexts:")
    for f in new:
        assert _same(dirs["on"], dirs["two"], f), f
    _run(exe, txt + group(W, rc, pc=False), dirs["cl"])
    _run(exe, txt + group(W, rc, cl=False), dirs["pc"])
    for key, bases in (("cl", CL_FILES), ("pc", PC_FILES)):
        assert sorted(set(os.listdir(dirs[key])) - set(old)) == sorted(f"{b}{s}.out" for b in bases for s in _suffixes(W))
        for b in bases:
            for s in _suffixes(W):
                assert _same(dirs["on"], dirs[key], f"{b}{s}.out"), (key, b, s)


# ---- (b): behind the other keys ----------------------------------------------------------------------------------------------
def test_diagonal_run_behind_every_periodic_key(exe, tmp_path):
    """Scenario A+'s input (3D, 32 particles, three walkers) with every periodic diagonal key on, then with the two new keys
    behind them: the other families' files keep their bytes, and the new files are the bytes of a run with the two alone."""
    txt, cfg = _input("he4_bis_cworm0_s1982", 3, 4)
    W = 3
    rc = float(np.floor(0.7 * cfg.rcut * 1e6) / 1e6)
    old, both, alone = (str(tmp_path / k) for k in ("old", "both", "alone"))
    _run(exe, txt + _gpu_group(A_PLUS, W, "device_sampler = T, ", cfg), old)
    _run(exe, txt + _gpu_group(A_PLUS, W, "device_sampler = T, ", cfg).replace("\n/\n", keys_text(rc) + "\n/\n"), both)
    _run(exe, txt + group(W, rc), alone)
    _same_files(old, both, A_PLUS, W)
    for f in sorted(set(os.listdir(old))):
        if f not in ("stdout.txt", "vpi.in"):
            assert _same(old, both, f), f
    new = sorted(f"{b}{s}.out" for b in CL_FILES + PC_FILES for s in _suffixes(W))
    assert sorted(set(os.listdir(both)) - set(os.listdir(old))) == new
    for f in new:
        assert _same(both, alone, f), f
    t = _table(os.path.join(both, "clus_vpi.out"), 9)
    assert t.shape[0] >= 2 and np.all(np.isfinite(t[:, [1, 3, 5, 7]])) and t[:, 1].sum() > 0
