"""The superfluid key on a machine without a GPU: the Fortran normalisation and writers of the front end (pigs_estimators
normalize_sf / write_rhos / write_msdu over a block_series, through the host library's hook hs_sf_files) against
pathintegralgroundstate_amd.profiles.normalize_sf, and the front end's refusals on the CPU twin (the host built against
tests/shim, which does not provide pigs_sf_*)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from hostlib import build_cpu_host
from pathintegralgroundstate_amd import profiles

RUNS = os.path.join(GOLDEN, "vpi_runs")
PERIODIC = os.path.join(RUNS, "he4_cworm0", "vpi.in")               # 2D, periodic, no worm sector
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")
PRINT = 1.0000001e-9                                             # the files carry 10 significant digits
KEY = "&gpu\n superfluid = T, sf_ntau = 2\n/\n"


@pytest.fixture(scope="module")
def cpu_host():
    return build_cpu_host()


@pytest.fixture(scope="module")
def cpu_exe(cpu_host):
    return cpu_host[2]


def _run(exe, txt, wd):
    os.makedirs(wd, exist_ok=True)
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt)
    with open(os.path.join(wd, "vpi.in")) as fin:
        r = subprocess.run([exe], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=600)
    return r.returncode, r.stdout.decode(errors="replace")


def _short(txt):
    txt = re.sub(r"Nblock\s*=\s*\d+", "Nblock = 2", txt)
    return re.sub(r"Nstep\s*=\s*\d+", "Nstep = 3", txt)


def block_error(x):
    """The error of the mean of the front end's files: sqrt((<x^2> - <x>^2) / n) over the n blocks."""
    n = x.shape[0]
    a, a2 = x.sum(axis=0) / n, (x * x).sum(axis=0) / n
    return np.sqrt(np.maximum(a2 - a * a, 0.0) / n)


def check_files(fr, fm, blocks, dim, Ntau, dt, err_atol=0.0):
    """rhos_vpi.out and msdu_vpi.out against the block values `blocks`: a list of normalize_sf dicts of ONE walker."""
    Dcm = np.stack([b["Dcm"] for b in blocks])
    rhos = np.stack([b["rhos"] for b in blocks])
    rmean = np.stack([b["rhos_mean"] for b in blocks])
    msd = np.stack([b["msd"] for b in blocks])
    cross = np.stack([b["cross"] for b in blocks])
    tau = np.arange(Ntau + 1) * dt

    def same(tab, cols):
        for j, x in enumerate(cols):
            assert np.allclose(tab[:, 1 + 2 * j], x.mean(axis=0), rtol=PRINT, atol=PRINT * np.abs(x).max()), j
            # the error is a difference of two moments: to the scale of the values
            assert np.allclose(tab[:, 2 + 2 * j], block_error(x), rtol=1e-6, atol=1e-6 * np.abs(x).max() + err_atol), j

    if Ntau == 0:
        assert open(fr).read() == ""                                        # lag 0 has no line there
    else:
        r = np.loadtxt(fr, ndmin=2)
        assert r.shape == (Ntau, 1 + 2 * (2 * dim + 1))
        assert np.allclose(r[:, 0], tau[1:], rtol=PRINT, atol=0)
        same(r, [Dcm[:, 1:, k] for k in range(dim)] + [rhos[:, 1:, k] for k in range(dim)] + [rmean[:, 1:]])
    m = np.loadtxt(fm, ndmin=2)
    assert m.shape == (Ntau + 1, 1 + 2 * (2 * dim + 1))
    assert np.allclose(m[:, 0], tau, rtol=PRINT, atol=0)
    same(m, [msd[..., k] for k in range(dim)] + [msd.sum(axis=-1)] + [cross[..., k] for k in range(dim)])
    assert not np.any(m[0, 1:])


@pytest.mark.parametrize("dim,window,Ntau", [(2, 1, 2), (3, 3, 5), (1, 0, 0)])
def test_fortran_normalisation_and_writers_match_the_package(cpu_host, tmp_path, dim, window, Ntau):
    """Random sums of three blocks of one walker: both files against the means and the block errors of
    profiles.normalize_sf of every block."""
    H = C.CDLL(cpu_host[1])                                         # (not into the global scope: see test_atm_host.py)
    lp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    H.hs_sf_files.argtypes = [C.c_int] * 4 + [C.c_double] * 2 + [C.c_int, lp, dp, dp] + [C.c_char_p] * 2
    H.hs_sf_files.restype = None
    rng = np.random.default_rng(70 + dim)
    Np, dt, nb = 37, 0.0125, 3
    S = np.array([4, 1, 7], np.int64)
    lag = np.arange(Ntau + 1.0)[:, None]
    Cs = rng.uniform(0.5, 2.0, (nb, Ntau + 1, dim)) * lag * S[:, None, None] * Np
    Ds = rng.uniform(0.5, 2.0, (nb, Ntau + 1, dim)) * lag * S[:, None, None] * Np
    fr, fm = str(tmp_path / "rhos_vpi.out"), str(tmp_path / "msdu_vpi.out")
    H.hs_sf_files(dim, Np, Ntau, window, dt, 0.5, nb, S.ctypes.data_as(lp), Cs.ctypes.data_as(dp), Ds.ctypes.data_as(dp),
                  fr.encode(), fm.encode())
    blocks = [profiles.normalize_sf({"C": Cs[b], "D": Ds[b], "samples": S[b], "window": window}, Np, dt) for b in range(nb)]
    assert Ntau == 0 or all(np.all(b["rhos"][1:] > 0) for b in blocks)
    check_files(fr, fm, blocks, dim, Ntau, dt)


def test_cpu_twin_still_links_against_the_unchanged_shim(cpu_exe):
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout and b"pigs_sf" not in nm.stdout
    assert b"sf_window" in open(cpu_exe, "rb").read()                 # the front end knows the keys


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PERIODIC).read()) + KEY, str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "superfluid" in out and "backend" in out and all(s in out for s in ("pigs_sf_init", "_accumulate", "_read")), out
    assert not os.path.exists(tmp_path / "rhos_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + KEY, str(tmp_path))
    assert rc == 2
    assert "superfluid" in out and "periodic" in out and "pigs_sf" not in out, out
    assert not os.path.exists(tmp_path / "e_vpi.out")


@pytest.mark.parametrize("keys,word", [("sf_ntau = 3, sf_window = 1", "sf_ntau"), ("sf_ntau = -1", "sf_ntau"),
                                       ("sf_window = 1000", "sf_window"), ("sf_ntau = 1000", "sf_window")])
def test_out_of_range_lags_are_refused_for_their_value(cpu_exe, tmp_path, keys, word):
    """sf_ntau above 2 sf_window; a negative sf_ntau; a window beyond Nb, given or as the smallest that holds the lags."""
    rc, out = _run(cpu_exe, _short(open(PERIODIC).read()) + f"&gpu\n superfluid = T, {keys}\n/\n", str(tmp_path))
    assert rc == 2 and "superfluid" in out and word in out and "pigs_sf" not in out, out[-2000:]
    assert not os.path.exists(tmp_path / "e_vpi.out")
