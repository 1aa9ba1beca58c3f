"""The momentum key on a machine without a GPU: the Fortran normalisation and writers of the front end (pigs_estimators
normalize_nk / normalize_nrvec / write_nkvec / write_n0_block, through the host library's hook hs_nk_files) against
pathintegralgroundstate_amd.profiles.normalize_nk / normalize_nrvec, and the front end's refusals on the CPU twin (the host
built against tests/shim, which does not provide pigs_nk_*)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from hostlib import build_cpu_host
from nk_numpy import half_space
from pathintegralgroundstate_amd import profiles

RUNS = os.path.join(GOLDEN, "vpi_runs")
WORM = os.path.join(RUNS, "he4_worm_s1982", "vpi.in")             # 3D, periodic, CWorm = 0.5
PBC = os.path.join(RUNS, "he4_cworm0", "vpi.in")                  # periodic, CWorm = 0
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")
PRINT = 1.0000001e-9                                             # the files carry 10 significant digits


def _key(extra=""):
    return f"&gpu\n momentum = T{extra}\n/\n"


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


def _hook(cpu_host):
    _, hostlib, _ = cpu_host
    H = C.CDLL(hostlib)                                           # (not into the global scope: see test_atm_host.py)
    lp, dp, ip = C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_int32)
    H.hs_nk_files.argtypes = [C.c_int, C.c_int, dp, C.c_double, C.c_double, C.c_int, C.c_int, ip, C.c_int, C.c_int, dp, dp,
                              lp, lp, dp, dp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]
    H.hs_nk_files.restype = None

    def call(dim, Np, Lbox, density, cworm, nobdm, n, nbin, zconf, Cs, nopen, Hc, files):
        nb, nq = Cs.shape
        L = np.ascontiguousarray(Lbox[:dim], np.float64)
        n32 = np.ascontiguousarray(n, np.int32)
        nk, rho1 = np.zeros(nq + 1), np.zeros(nbin ** dim)
        H.hs_nk_files(dim, Np, L.ctypes.data_as(dp), density, cworm, nobdm, nq, n32.ctypes.data_as(ip), nbin, nb,
                      zconf.ctypes.data_as(dp), Cs.ctypes.data_as(dp), nopen.ctypes.data_as(lp), Hc.ctypes.data_as(lp),
                      nk.ctypes.data_as(dp), rho1.ctypes.data_as(dp), *(f.encode() for f in files))
        return nk, rho1
    return call


@pytest.mark.parametrize("dim,nmax,nbin,L", [(2, 2, 3, [3.0, 4.5]), (3, 1, 2, [3.0, 4.5, 3.75]), (3, 2, 4, [4.0, 4.0, 4.0])])
def test_fortran_normalisation_and_writers_match_the_package(cpu_host, tmp_path, dim, nmax, nbin, L):
    """Random sums of three blocks of one walker: the last block's n(k) and rho1 from Fortran against normalize_nk /
    normalize_nrvec; the four files against numpy on the package's block values.  The n = 0 line of nkvec_vpi.out is
    n0 * Np."""
    call = _hook(cpu_host)
    rng = np.random.default_rng(60 + dim + nmax)
    Np, cworm, nobdm, nb = 16, 0.5, 4, 3
    density = Np / float(np.prod(L))
    n = half_space(dim, nmax)
    nq = len(n)
    nopen = np.array([40, 8, 120], np.int64)
    zconf = np.array([25.0, 31.0, 50.0])
    Cs = rng.uniform(-1.0, 1.0, (nb, nq)) * nopen[:, None]
    Hc = rng.integers(0, 20, (nb,) + (nbin,) * dim).astype(np.int64)
    files = [str(tmp_path / f) for f in ("nkvec_vpi.out", "nk_vpi.out", "n0_vpi.out", "nrvec_vpi.out")]
    nk, rho1 = call(dim, Np, L, density, cworm, nobdm, n, nbin, zconf, Cs, nopen, Hc, files)
    blocks = [profiles.normalize_nk({"C": Cs[b], "nopen": nopen[b]}, cworm, zconf[b], nobdm, Np, n=n, Lbox=L) for b in range(nb)]
    rhos = [profiles.normalize_nrvec({"H": Hc[b]}, cworm, zconf[b], nobdm, density, L, dim) for b in range(nb)]
    last = blocks[-1]
    assert np.allclose(nk[1:], last["nk"], rtol=1e-14, atol=0) and np.isclose(nk[0], last["nk0"], rtol=1e-14, atol=0)
    assert np.allclose(rho1, rhos[-1]["rho1"].ravel(), rtol=1e-14, atol=0)

    def stats(x):
        m = x.mean(axis=0)
        return m, np.sqrt(np.maximum((x * x).mean(axis=0) - m * m, 0.0) / nb)

    def close_err(got, err, m):
        return np.all(np.abs(got - err) <= np.sqrt(4.0 * np.abs(m) * PRINT * np.abs(m)) + PRINT * err)

    # nkvec_vpi.out: n = 0 first, then the stored vectors
    vec = np.loadtxt(files[0], ndmin=2)
    assert vec.shape == (nq + 1, dim + 3) and not vec[0, :dim + 1].any() and np.array_equal(vec[1:, :dim], n)
    kmod = np.sqrt(((2.0 * np.pi * n / np.asarray(L)) ** 2).sum(axis=1))
    assert np.allclose(vec[1:, dim], kmod, rtol=PRINT, atol=0)
    m, err = stats(np.stack([np.r_[b["nk0"], b["nk"]] for b in blocks]))
    assert np.allclose(vec[:, dim + 1], m, rtol=PRINT, atol=PRINT * np.abs(m).max()) and close_err(vec[:, dim + 2], err, m)
    n0m = np.mean([b["n0"] for b in blocks])
    assert abs(vec[0, dim + 1] - n0m * Np) <= PRINT * n0m * Np                # the n = 0 line is n0 * Np
    # nk_vpi.out: one line per |k| shell
    sh = np.loadtxt(files[1], ndmin=2)
    m, err = stats(np.stack([b["nk_shell"] for b in blocks]))
    assert sh.shape == (len(last["k"]), 4) and np.allclose(sh[:, 0], last["k"], rtol=PRINT, atol=0)
    assert np.allclose(sh[:, 1], m, rtol=PRINT, atol=PRINT * np.abs(m).max()) and np.array_equal(sh[:, 3], last["mult"])
    assert close_err(sh[:, 2], err, m)
    # n0_vpi.out: one line per block
    n0 = np.loadtxt(files[2], ndmin=2)
    assert open(files[2]).readline().startswith("#") and n0.shape == (nb, 3) and n0[:, 0].tolist() == [1.0, 2.0, 3.0]
    assert np.allclose(n0[:, 1], [b["n0"] for b in blocks], rtol=PRINT, atol=0)
    assert np.allclose(n0[:, 2], [b["nk0"] for b in blocks], rtol=PRINT, atol=0)
    assert np.allclose(n0[:, 1], nopen / (cworm * zconf * nobdm * Np), rtol=PRINT, atol=0)
    # nrvec_vpi.out: one line per bin, x fastest
    rv = np.loadtxt(files[3], ndmin=2)
    m, err = stats(np.stack([r["rho1"].ravel() for r in rhos]))
    assert rv.shape == (nbin ** dim, dim + 2) and np.allclose(rv[:, dim], m, rtol=PRINT, atol=0)
    assert close_err(rv[:, dim + 1], err, m)
    x = rhos[0]["x"]
    assert np.allclose(rv[:nbin, 0], x[0], rtol=PRINT, atol=0) and np.allclose(rv[::nbin, 1][:nbin], x[1], rtol=PRINT, atol=0)


def test_cpu_twin_still_links_against_the_unchanged_shim(cpu_exe):
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout and b"pigs_nk" not in nm.stdout
    assert b"nk_nbin" in open(cpu_exe, "rb").read()


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(WORM).read()) + _key(), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "momentum" in out and "backend" in out and all(s in out for s in ("pigs_nk_init", "_accumulate", "_add", "_read")), out
    assert not os.path.exists(tmp_path / "n0_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + _key(), str(tmp_path))
    assert rc == 2
    assert "momentum" in out and "periodic" in out and "pigs_nk" not in out, out


def test_key_is_refused_without_the_worm_sector(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "momentum" in out and "CWorm" in out and "pigs_nk" not in out, out
    assert not os.path.exists(tmp_path / "e_vpi.out")


@pytest.mark.parametrize("extra,word", [(", nk_nmax = 0", "nk_nmax"), (", nk_nmax = 17", "nk_nmax"), (", nk_nbin = 0", "nk_nbin"),
                                        (", nk_nbin = 129", "nk_nbin")])
def test_out_of_range_keys_are_refused(cpu_exe, tmp_path, extra, word):
    rc, out = _run(cpu_exe, _short(open(WORM).read()) + _key(extra), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "momentum" in out and word in out and "pigs_nk" not in out, out
    assert not os.path.exists(tmp_path / "e_vpi.out")


def test_limits_are_accepted_for_their_values(cpu_exe, tmp_path):
    for extra in ("", ", nk_nmax = 16, nk_nbin = 128", ", nk_nmax = 1, nk_nbin = 1"):
        rc, out = _run(cpu_exe, _short(open(WORM).read()) + _key(extra), str(tmp_path))
        assert rc == 2 and "pigs_nk" in out, out


def test_run_without_the_key_is_its_golden_files(cpu_exe, tmp_path):
    gold = os.path.join(RUNS, "he4_worm_s1982")
    rc, out = _run(cpu_exe, open(WORM).read() + "&gpu\n momentum = F, nk_nmax = 3, nk_nbin = 4\n/\n", str(tmp_path))
    assert rc == 0 and "Momentum" not in out, out[-2000:]
    assert not set(os.listdir(tmp_path)) & {"nkvec_vpi.out", "nk_vpi.out", "n0_vpi.out", "nrvec_vpi.out"}
    for f in ("e_vpi.out", "et_vpi.out", "gr_vpi.out", "sk_vpi.out", "nr_vpi.out"):
        assert open(tmp_path / f, "rb").read() == open(os.path.join(gold, f), "rb").read(), f
