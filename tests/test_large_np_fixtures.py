"""The reference runs beyond 256 particles (tests/golden/vpi_runs/n257_*, n300_*, n520_*, trap3d_n260_*: more than four
64-partner passes per bead, so every kernel's second or third 256-partner trip): properties of the REFERENCE's runs that the
GPU tests of tests/test_gpu_large_np.py rely on, checked from the fixtures alone, and the driver's replay against the
reference program's own files."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from pathintegralgroundstate_amd import SystemConfig

RUNS = os.path.join(GOLDEN, "vpi_runs")
LARGE_NP_RUNS = ["n300_bis4_s1982", "n300_bis4_s1983", "n300_bis5_s1982", "n520_lstag20_s1982", "n257_sta_s1982",
                 "n300_worm_s4", "trap3d_n260_s1982"]
# acc_cm acc_head acc_tail acc_bd try_open acc_open try_close acc_close acc_cm_half acc_head_half acc_tail_half acc_bd_half
# try_swap acc_swap try_cm try_stag (tests/golden/ref_driver.py COUNTER_NAMES)
CM, HEAD, TAIL, BD, TRY_OPEN, ACC_OPEN, TRY_CLOSE, ACC_CLOSE = range(8)
TRY_SWAP, ACC_SWAP, TRY_CM, TRY_STAG = 12, 13, 14, 15


def _load(name):
    cfg = SystemConfig.from_namelists(open(os.path.join(RUNS, name, "vpi.in")).read())
    return cfg, dict(np.load(os.path.join(RUNS, name, "driver.npz")))


def test_the_shapes_are_the_ones_the_kernels_branch_on():
    """Passes of 64 partners and trips of 256 are what the kernels count in: 5 passes with a ragged last one (300), one
    particle in the fifth pass (257), 9 passes = a third trip (520), the stage machine's level count (Nlev = 5), task
    totals of Lstag = 20 items, a trap with a fifth pass."""
    shape = {n: _load(n)[0] for n in LARGE_NP_RUNS}
    passes = {n: -(-c.Np // 64) for n, c in shape.items()}
    assert passes == {"n300_bis4_s1982": 5, "n300_bis4_s1983": 5, "n300_bis5_s1982": 5, "n520_lstag20_s1982": 9,
                      "n257_sta_s1982": 5, "n300_worm_s4": 5, "trap3d_n260_s1982": 5}
    assert shape["n257_sta_s1982"].Np == 257 and shape["n257_sta_s1982"].sampling == "sta"
    assert shape["n300_bis4_s1982"].Nlev == 4 and shape["n300_bis5_s1982"].Nlev == 5
    assert 2 * shape["n300_bis5_s1982"].Nb >= 1 << 5                    # a 2^5-bead segment fits the chain
    c = shape["n520_lstag20_s1982"]
    assert c.Np == 520 and c.Lstag == 20 and c.Lstag <= c.Nb and c.CWorm == 0
    c = shape["n300_worm_s4"]
    assert c.Np == 300 and c.CWorm > 0 and c.swapping and c.Nobdm > 0 and c.Npw >= 1
    c = shape["trap3d_n260_s1982"]
    assert c.trap and c.dim == 3 and c.Np == 260 and c.Nlev <= 4
    for n in ("n300_bis4_s1982", "n300_bis4_s1983"):
        assert shape[n].Np == 300 and shape[n].dim == 3 and not shape[n].trap and shape[n].CWorm == 0
    for n, c in shape.items():
        assert 16 <= c.Nb <= 40, n


@pytest.mark.parametrize("name", LARGE_NP_RUNS)
def test_every_diagonal_mover_was_accepted_and_rejected(name):
    """A run in which a mover is always (or never) accepted cannot tell a wrong Delta S from a right one."""
    cfg, drv = _load(name)
    c = drv["counters"]
    assert 0 < c[CM] < c[TRY_CM], c
    for k in (HEAD, TAIL, BD):
        assert 0 < c[k] < c[TRY_STAG], (k, c)
    # every stored file stays below the largest fixture that existed before these runs (254 KB)
    for f in os.listdir(os.path.join(RUNS, name)):
        assert os.path.getsize(os.path.join(RUNS, name, f)) < 254 * 1024, f
    assert int(drv["bead_stride"]) == 8 and tuple(drv["Path_shape"]) == (cfg.M, cfg.Np, cfg.dim)


def test_the_worm_run_opens_closes_swaps_and_fills_the_obdm():
    cfg, drv = _load("n300_worm_s4")
    c = drv["counters"]
    assert c[ACC_OPEN] >= 1 and c[ACC_CLOSE] >= 1 and c[ACC_SWAP] >= 1, c
    assert c[ACC_OPEN] < c[TRY_OPEN] and c[ACC_CLOSE] < c[TRY_CLOSE] and c[ACC_SWAP] < c[TRY_SWAP], c
    assert np.all(c[8:12] >= 1), c                                      # every half-chain mover accepted at least once
    codes = drv["events"][:, 1].tolist()
    assert codes.count(1) == c[ACC_OPEN] and codes.count(2) == c[ACC_CLOSE] and codes.count(3) == c[ACC_SWAP]
    h = drv["nrho_total"]
    assert h.shape == (cfg.Nbin, cfg.Npw + 1) and h[:, 0].sum() > 0 and np.count_nonzero(h[:, 0]) > 1
    d = drv["steps"][:, 0]
    assert 0 < d.sum() < len(d)                                         # diagonal and off-diagonal steps both occur


@pytest.mark.parametrize("name", LARGE_NP_RUNS)
def test_driver_replay_equals_the_reference_programs_files(name):
    """The second half of ref_driver.validate_against_program (the first, the bit-identical final worldline, needs the
    program's checkpoint and is asserted when make_golden.py writes the run): the driver's 64-bit block energies are
    the digits the program printed.  Where the compiled reference is present the run is replayed afresh and must give
    driver.npz again, bit for bit."""
    import sys
    from oracle.pyoracle import Ref
    cfg, drv = _load(name)
    src = os.path.join(RUNS, name)
    for mine, f in ((drv["block_e"], "e_vpi.out"), (drv["block_t"], "et_vpi.out")):
        theirs = np.atleast_2d(np.loadtxt(os.path.join(src, f)))
        assert mine.shape[0] == theirs.shape[0] > 0, f
        assert np.array_equal(mine[:, 0], theirs[:, 0])
        assert np.all(np.abs(mine[:, 1:] - theirs[:, 1:4]) <= 0.6e-9 * np.abs(theirs[:, 1:4])), f
    assert np.array_equal(drv["ckpt_sha"][-1], drv["Path_sha256"]) and np.array_equal(drv["ckpt_counters"][-1], drv["counters"])
    if Ref.available():
        sys.path.insert(0, GOLDEN)
        try:
            import make_golden as mg
            import ref_driver as rd
        finally:
            sys.path.pop(0)
        kw = {k: v for k, v in mg.RUNS[name].items() if k != "big"}
        _, res = mg.drive_run(Ref(), kw)
        c = rd.compact(res, mg.BIG_STRIDE)
        for k in ("Path_sha256", "Path_sub", "counters", "events", "steps", "mt", "mti", "block_e", "block_t", "nrho_total",
                  "gr_total", "sk_total", "xend", "isopen"):
            a, b = np.asarray(c[k]), drv[k]
            assert a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), k
