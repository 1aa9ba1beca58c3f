"""The lattice key on a machine without a GPU: the Fortran normalisation and writers of the front end (pigs_estimators
normalize_lat / write_lind_block / write_lindtau / write_usite, through the host library's hook hs_lat_files) against
pathintegralgroundstate_amd.profiles.normalize_lat, and the front end's refusals on the CPU twin (the host built against
tests/shim, which does not provide pigs_lat_*)."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from hostlib import build_cpu_host
from pathintegralgroundstate_amd import profiles

RUNS = os.path.join(GOLDEN, "vpi_runs")
CRYSTAL = os.path.join(RUNS, "he4_crystal")                      # 3D, periodic, started from config_ini.in
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")
ONE_D = os.path.join(RUNS, "ho1d_n2", "vpi.in")                   # 1D (trapped as it stands)
PRINT = 1.0000001e-9                                             # the files carry 10 significant digits
KEY = "&gpu\n lattice = T\n/\n"


@pytest.fixture(scope="module")
def cpu_host():
    return build_cpu_host()


@pytest.fixture(scope="module")
def cpu_exe(cpu_host):
    return cpu_host[2]


def _run(exe, txt, wd, config=True):
    os.makedirs(wd, exist_ok=True)
    if config:
        shutil.copy(os.path.join(CRYSTAL, "config_ini.in"), wd)
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt)
    with open(os.path.join(wd, "vpi.in")) as fin:
        r = subprocess.run([exe], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=600)
    return r.returncode, r.stdout.decode(errors="replace")


def _short(txt):
    txt = re.sub(r"Nblock\s*=\s*\d+", "Nblock = 2", txt)
    return re.sub(r"Nstep\s*=\s*\d+", "Nstep = 3", txt)


@pytest.mark.parametrize("dim,window", [(2, 0), (3, 2)])
def test_fortran_normalisation_and_writers_match_the_package(cpu_host, tmp_path, dim, window):
    """Random sums of three blocks of one walker: lind_vpi.out per block against normalize_lat of every block;
    lindtau_vpi.out and usite_vpi.out against the means of the package's block values."""
    H = C.CDLL(cpu_host[1])                                         # (not into the global scope: see test_atm_host.py)
    lp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    H.hs_lat_files.argtypes = [C.c_int] * 5 + [C.c_double] * 3 + [C.c_int, lp, dp] + [lp] * 6 + [C.c_char_p] * 3
    H.hs_lat_files.restype = None
    rng = np.random.default_rng(60 + dim)
    Np, nsite, nbin, dt, ann, rmax, nb = 37, 38, 9, 0.0125, 3.1, 1.4, 3
    ns = 2 * window + 1
    S = np.array([4, 1, 7], np.int64)
    nass = (S[:, None] * Np - rng.integers(0, 3, (nb, ns))).astype(np.int64)
    mom = rng.uniform(0.5, 2.0, (nb, ns, 2 + dim)) * nass[..., None]
    mom[..., 0] = mom[..., 2:].sum(axis=-1)
    occ = rng.integers(0, 40, (nb, ns, 4)).astype(np.int64)
    hr = rng.integers(0, 1000, (nb, nbin)).astype(np.int64)
    hx = rng.integers(0, 1000, (nb, dim, 2 * nbin)).astype(np.int64)
    hop1, hopw = rng.integers(0, 50, nb).astype(np.int64), rng.integers(0, 9, nb).astype(np.int64)
    fl, ft, fu = (str(tmp_path / f) for f in ("lind_vpi.out", "lindtau_vpi.out", "usite_vpi.out"))
    H.hs_lat_files(dim, Np, nsite, window, nbin, dt, ann, rmax, nb, S.ctypes.data_as(lp), mom.ctypes.data_as(dp),
                   nass.ctypes.data_as(lp), occ.ctypes.data_as(lp), hr.ctypes.data_as(lp), hx.ctypes.data_as(lp),
                   hop1.ctypes.data_as(lp), hopw.ctypes.data_as(lp), fl.encode(), ft.encode(), fu.encode())
    raw = {"mom": mom, "nassigned": nass, "occ": occ, "hr": hr, "hx": hx, "hop1": hop1, "hopw": hopw, "samples": S}
    n = profiles.normalize_lat(raw, Np, nsite, ann, rmax)              # the blocks as the leading axis
    tab = np.loadtxt(fl, ndmin=2)
    assert open(fl).readline().startswith("#") and tab.shape == (nb, 8) and tab[:, 0].tolist() == [1.0, 2.0, 3.0]
    want = np.stack([n[k] for k in ("u2_mean", "gamma", "alpha2", "vacant", "multiple", "hops_link", "hops_window")], axis=1)
    assert np.all(want[:, :2] > 0) and (window == 0 or np.all(want[:, 5] > 0))
    # alpha_2 is a difference from 1: to the scale of its terms
    scale = np.abs(want)
    scale[:, 2] += 1.0
    assert np.all(np.abs(tab[:, 1:] - want) <= PRINT * scale), np.abs(tab[:, 1:] - want) / scale
    if window == 0:
        assert np.all(tab[:, 6] == 0.0)
    tau = np.loadtxt(ft, ndmin=2)
    assert tau.shape == (ns, 3 + dim)
    assert np.allclose(tau[:, 0], (np.arange(ns) - window) * dt, rtol=PRINT, atol=0)
    assert np.allclose(tau[:, 1], n["u2"].mean(axis=0), rtol=PRINT, atol=0)
    assert np.allclose(tau[:, 2:2 + dim], n["uk2"].mean(axis=0), rtol=PRINT, atol=0)
    assert np.allclose(tau[:, 2 + dim], n["gamma_tau"].mean(axis=0), rtol=PRINT, atol=0)
    us = np.loadtxt(fu, ndmin=2)
    assert us.shape == (nbin, 2 + 2 * dim)
    assert np.allclose(us[:, 0], n["r"], rtol=PRINT, atol=0) and np.allclose(us[:, 1], n["rho_site"].mean(axis=0), rtol=PRINT, atol=0)
    pu = n["pu"].mean(axis=0)
    for k in range(dim):
        assert np.allclose(us[:, 2 + 2 * k], pu[k, nbin - 1::-1], rtol=PRINT, atol=0)      # P(u_k = -r)
        assert np.allclose(us[:, 3 + 2 * k], pu[k, nbin:], rtol=PRINT, atol=0)            # P(u_k = +r)
    assert np.allclose(n["x"][nbin:], n["r"]) and np.allclose(n["x"][nbin - 1::-1], -n["r"])


def test_cpu_twin_still_links_against_the_unchanged_shim(cpu_exe):
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout and b"pigs_lat" not in nm.stdout
    assert b"lat_rmax" in open(cpu_exe, "rb").read()              # the front end knows the keys


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(os.path.join(CRYSTAL, "vpi.in")).read()) + KEY, str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "lattice" in out and "backend" in out and all(s in out for s in ("pigs_lat_init", "_accumulate", "_read")), out
    assert not os.path.exists(tmp_path / "lind_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_without_config_ini(cpu_exe, tmp_path):
    txt = _short(open(os.path.join(CRYSTAL, "vpi.in")).read())
    txt = re.sub(r"crystal\s*=\s*T", "crystal = F", txt)
    assert "crystal = F" in txt
    rc, out = _run(cpu_exe, txt + KEY, str(tmp_path), config=False)
    assert rc == 2, out[-2000:]
    assert "lattice" in out and "config_ini.in" in out and "pigs_lat" not in out, out
    assert not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + KEY, str(tmp_path))
    assert rc == 2
    assert "lattice" in out and "periodic" in out and "pigs_lat" not in out, out


def test_key_is_refused_in_one_dimension(cpu_exe, tmp_path):
    txt = open(ONE_D).read()
    assert re.search(r"dim\s*=\s*1\b", txt) and "trap = T" in txt
    rc, out = _run(cpu_exe, _short(txt.replace("trap = T", "trap = F")) + KEY, str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "lattice" in out and "dim = 2 or 3" in out and "pigs_lat" not in out, out
    assert not os.path.exists(tmp_path / "e_vpi.out")


def test_out_of_range_window_is_refused_for_its_value(cpu_exe, tmp_path):
    txt = _short(open(os.path.join(CRYSTAL, "vpi.in")).read())
    rc, out = _run(cpu_exe, txt + "&gpu\n lattice = T, lat_window = 1000\n/\n", str(tmp_path))
    assert rc == 2 and "lat_window" in out and "pigs_lat" not in out, out[-2000:]
