"""The many-seed fixtures tests/golden/vpi_runs/*_walkers/walkers.npz (tests/golden/make_golden.py, WALKER_SETS) that
tests/test_gpu_sampler_occupancy.py holds every walker of a large device-sampler run to.  Here, without a GPU: their
first rows are the single-seed reference runs already pinned elsewhere, and the CPU twin of the front end (host-driven
sampler over tests/shim) reproduces far rows -- so row w is the reference's run of seed + w, the seed the front end
gives walker w."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
from helpers import (check_worldline_vs_driver, driver_blocks, read_hex_blocks, rng_sha256, walker_row,
                     walker_summed_structure)
from hostlib import build_cpu_host
from pathintegralgroundstate_amd import SystemConfig
from test_host_driver import run_pigs_vpi

RUNS = os.path.join(GOLDEN, "vpi_runs")
SETS = {"c3_n256_walkers": ("c3_n256_s1982", 1024), "c5_n256_dipolar_walkers": ("c5_n256_dipolar_s1982", 128)}


def _load(name):
    return dict(np.load(os.path.join(RUNS, name, "walkers.npz")))


def _driver(name):
    return dict(np.load(os.path.join(RUNS, name, "driver.npz")))


@pytest.mark.parametrize("name", list(SETS))
def test_walker_sets_are_complete(name):
    base, n = SETS[name]
    W = _load(name)
    assert open(os.path.join(RUNS, name, "vpi.in")).read() == open(os.path.join(RUNS, base, "vpi.in")).read()
    assert np.array_equal(W["seed"], 1982 + np.arange(n))
    for k in ("mti", "mt_sha256", "counters", "Path_sha256", "steps", "block_e", "block_t"):
        assert len(W[k]) == n, k
    assert len({bytes(s) for s in W["Path_sha256"]}) == n          # n different chains
    assert int(W["n_summed"]) == 128


@pytest.mark.parametrize("name,row,run", [("c3_n256_walkers", 0, "c3_n256_s1982"), ("c3_n256_walkers", 1, "c3_n256_s1983"),
                                          ("c5_n256_dipolar_walkers", 0, "c5_n256_dipolar_s1982")])
def test_first_rows_are_the_single_seed_runs(name, row, run):
    r, d = walker_row(_load(name), row), _driver(run)
    assert int(r["mti"]) == int(d["mti"]) and np.array_equal(r["mt_sha256"], rng_sha256(d["mt"]))
    for k in ("counters", "Path_sha256", "Path_shape", "block_e", "block_t"):
        assert np.array_equal(r[k], d[k]), k
    assert np.array_equal(r["steps"], d["steps"], equal_nan=True)
    assert str(r["potential"]) == str(d["potential"])
    assert np.array_equal(r["events"].reshape(-1, 3), d["events"].reshape(-1, 3))
    if "isopen" in r:                                              # the worm sector
        for k in ("isopen", "iworm", "xend", "nrho_total"):
            assert np.array_equal(r[k], d[k]), k


def test_summed_structure_normalisation_reproduces_the_program():
    """helpers.walker_summed_structure (what the GPU test expects in the walker-summed files) applied to one walker's
    raw histograms gives the reference PROGRAM's gr_vpi.out / sk_vpi.out of that run."""
    src = os.path.join(RUNS, "c3_n256_s1982")
    d = _driver("c3_n256_s1982")
    cfg = SystemConfig.from_namelists(open(os.path.join(src, "vpi.in")).read())
    gr, sk = walker_summed_structure(cfg, d["gr_total"], d["sk_total"], 1, int(d["steps"][:, 0].sum()))
    a, b = np.loadtxt(os.path.join(src, "gr_vpi.out")), np.loadtxt(os.path.join(src, "sk_vpi.out"))
    assert np.all(np.abs(a[:, 1] - gr) <= 1.01e-9 * np.abs(gr))           # ten printed digits
    assert np.all(np.abs(b[:, 1::3] - sk) <= 1.01e-9 * np.abs(sk))


@pytest.fixture(scope="module")
def exe():
    return build_cpu_host()[2]


def _rand_state(path):
    """host/pigs_rng.f90 mt_save: two unformatted sequential records (position; 624 words)."""
    b = np.fromfile(path, np.int32)
    assert b[0] == 4 and b[2] == 4 and b[3] == 4 * 624 and b[-1] == 4 * 624
    return int(b[1]), b[4:4 + 624].view(np.uint32)


PRINTED = [("CM movements", 0, 14), ("Staging movements", 3, 15), ("Head movements", 1, 15), ("Tail movements", 2, 15)]


@pytest.mark.parametrize("name,row", [("c3_n256_walkers", 127), ("c3_n256_walkers", 1023), ("c5_n256_dipolar_walkers", 127)])
def test_cpu_twin_reproduces_far_rows(exe, name, row, tmp_path):
    """The front end on the CPU twin, one walker with seed 1982 + row: final worldline (SHA-256) and generator state
    (position, words) bit for bit, block energies (e_vpi.hex) as tests/test_host_driver.py holds them; with the worm
    sector the final worm state of checkpoint.dat.  C3 runs one block: its printed acceptance percentages pin the
    counters (acceptances of 768 CM and 3 840 staging attempts are 0.13 and 0.026 points apart, printed to 0.01)."""
    W = _load(name)
    r = walker_row(W, row)
    seed = int(r["seed"])
    assert seed == 1982 + row
    txt = open(os.path.join(RUNS, name, "vpi.in")).read()
    txt, k = re.subn(r"seed = 1982\b", f"seed = {seed}", txt)
    assert k == 1
    run_pigs_vpi(exe, txt + f"&gpu\n n_walkers = 1, device = 0, potential = '{r['potential']}', checkpointing = T\n/\n",
                 str(tmp_path))
    shape = tuple(int(x) for x in r["Path_shape"])
    check_worldline_vs_driver(np.fromfile(tmp_path / "worldlines_final.bin").reshape(shape), r, None, tol=0.0)
    pos, words = _rand_state(tmp_path / "rand_state")
    assert pos == int(r["mti"]) and np.array_equal(rng_sha256(words), r["mt_sha256"])
    blocks, rows = read_hex_blocks(tmp_path / "e_vpi.hex")
    wb, wrows = driver_blocks(r)
    assert np.array_equal(blocks, wb)
    assert np.all(np.abs(rows - wrows) <= 1e-13 * np.abs(wrows)), np.max(np.abs(rows - wrows) / np.abs(wrows))
    if "isopen" in r:
        lines = open(tmp_path / "checkpoint.dat").read().split("\n")
        assert (lines[1].strip() == ".True.") == bool(r["isopen"])
        if r["isopen"]:
            assert int(lines[2]) == int(r["iworm"])
        M, Np = shape[0], shape[1]
        xend = np.array([[float(x) for x in ln.split()] for ln in lines[3 + M * Np + 2:3 + M * Np + 4]])
        assert np.array_equal(xend, r["xend"])
    else:
        out = open(tmp_path / "stdout.txt").read()
        c = r["counters"]
        for label, acc, tries in PRINTED:
            printed = float(re.search(label + r"\s*=\s*([-0-9.]+)", out).group(1))
            assert abs(printed - 100.0 * c[acc] / c[tries]) <= 0.0051, (label, printed, c[acc], c[tries])
