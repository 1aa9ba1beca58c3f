"""The van Hove key on a machine without a GPU: the Fortran normalisation and writers of the front end
(pigs_estimators normalize_vh / write_vh, through the host library's hook hs_vh_files) against
pathintegralgroundstate_amd.profiles.normalize_vh, and the front end's refusals on the CPU twin (the host built against
tests/shim, which does not provide pigs_vh_*)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from hostlib import build_cpu_host

RUNS = os.path.join(GOLDEN, "vpi_runs")
PBC = os.path.join(RUNS, "he4_cworm0", "vpi.in")                  # 2D
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")
PRINT = 1.0000001e-9                                             # the files carry 10 significant digits


def _key(extra=""):
    return f"&gpu\n van_hove = T{extra}\n/\n"


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


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_fortran_normalisation_and_writers_match_the_package(cpu_host, tmp_path, dim):
    """Random counts of three blocks of one walker: the last block's G_s, G_d from Fortran against normalize_vh, and
    gd_vpi.out / gs_vpi.out (tau_l, r, mean, error over the blocks) against numpy on normalize_vh's block values."""
    from pathintegralgroundstate_amd.profiles import normalize_vh
    shim, hostlib, _ = cpu_host
    C.CDLL(shim, mode=C.RTLD_GLOBAL)
    H = C.CDLL(hostlib)
    lp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    H.hs_vh_files.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_double,
                              C.c_double, C.c_int, lp, lp, lp, dp, dp, C.c_char_p, C.c_char_p]
    H.hs_vh_files.restype = None
    rng = np.random.default_rng(40 + dim)
    Np, density, window, Ntau, Nr, rbin, Ns, sbin, dt, nb = 37, 0.365, 3, 4, 6, 0.37, 5, 0.083, 0.0125, 3
    S = np.array([4, 1, 7], np.int64)
    cself = rng.integers(0, 1000, (nb, Ntau + 1, Ns)).astype(np.int64)
    cdist = rng.integers(0, 100000, (nb, Ntau + 1, Nr)).astype(np.int64)
    gs, gd = np.zeros((Ntau + 1, Ns)), np.zeros((Ntau + 1, Nr))
    fd, fs = str(tmp_path / "gd_vpi.out"), str(tmp_path / "gs_vpi.out")
    H.hs_vh_files(dim, Np, density, window, Ntau, Nr, rbin, Ns, sbin, dt, nb, S.ctypes.data_as(lp), cself.ctypes.data_as(lp),
                  cdist.ctypes.data_as(lp), gs.ctypes.data_as(dp), gd.ctypes.data_as(dp), fd.encode(), fs.encode())
    blocks = [normalize_vh({"self": cself[b], "distinct": cdist[b], "samples": S[b]}, Np, window, density, rbin, sbin, dim, dt)
              for b in range(nb)]
    # the Fortran norm is a single-precision product of two small integers (exact); the rest is double
    assert np.allclose(gd, blocks[-1]["G_d"], rtol=1e-13, atol=0) and np.allclose(gs, blocks[-1]["G_s"], rtol=1e-13, atol=0)
    assert gd.min() > 0
    for f, key, rk, n in ((fd, "G_d", "r", Nr), (fs, "G_s", "rs", Ns)):
        tab = np.loadtxt(f)
        assert tab.shape == ((Ntau + 1) * n, 4), (f, tab.shape)
        x = np.stack([b[key] for b in blocks]).reshape(nb, -1)
        mean = x.mean(axis=0)
        err = np.sqrt(np.maximum((x * x).mean(axis=0) - mean * mean, 0.0) / nb)
        assert np.allclose(tab[:, 0], np.repeat(blocks[0]["tau"], n), rtol=PRINT, atol=0)
        assert np.allclose(tab[:, 1], np.tile(blocks[0][rk], Ntau + 1), rtol=PRINT, atol=0)
        assert np.allclose(tab[:, 2], mean, rtol=PRINT, atol=0)
        assert np.all(np.abs(tab[:, 3] - err) <= np.sqrt(4.0 * mean * PRINT * mean) + PRINT * err)


def test_cpu_twin_still_links_against_the_unchanged_shim(cpu_exe):
    """The front end names no pigs_vh_* symbol at link time: the shim does not define them and it still links."""
    assert os.path.exists(cpu_exe)
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout                     # nm lists the backend's symbols: the check has teeth
    assert b"pigs_vh" not in nm.stdout
    assert b"van_hove" in open(cpu_exe, "rb").read()            # the front end knows the key


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", vh_ntau = 2"), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "van_hove" in out and "backend" in out, out
    assert all(s in out for s in ("pigs_vh_init", "_accumulate", "_read")), out
    assert not os.path.exists(tmp_path / "gd_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + _key(), str(tmp_path))
    assert rc == 2
    assert "van_hove" in out and "periodic" in out and "pigs_vh" not in out, out


@pytest.mark.parametrize("extra,word", [(", vh_window = 1000", "vh_window"),                   # > Nb
                                        (", vh_ntau = 1000", "vh_window"),                     # its default window passes Nb
                                        (", vh_window = 1, vh_ntau = 3", "vh_ntau"),           # > 2 window
                                        (", vh_ntau = -1", "vh_ntau"),
                                        (", vh_nself = 0", "vh_nself"),
                                        (", vh_nself = -3", "vh_nself")])
def test_out_of_range_keys_are_refused(cpu_exe, tmp_path, extra, word):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "van_hove" in out and word in out and "pigs_vh" not in out, out        # refused for the values, not the backend
    assert not os.path.exists(tmp_path / "e_vpi.out")


def test_limits_are_accepted_for_their_values(cpu_exe, tmp_path):
    """vh_ntau = 2 vh_window and vh_nself = 1 pass the value checks (and are then refused for the backend)."""
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", vh_window = 1, vh_ntau = 2, vh_nself = 1"), str(tmp_path))
    assert rc == 2 and "pigs_vh" in out, out


def test_run_without_the_key_is_its_golden_files(cpu_exe, tmp_path):
    """The golden run itself, once plain and once with the key spelled out as off: both byte-identical to the golden files."""
    gold = os.path.join(RUNS, "he4_cworm0")
    txt = open(PBC).read()
    outs = []
    for name, extra in (("plain", ""), ("off", "&gpu\n van_hove = F, vh_ntau = 2, vh_nself = 9, vh_rself = 1.5\n/\n")):
        rc, out = _run(cpu_exe, txt + extra, str(tmp_path / name))
        assert rc == 0, out[-2000:]
        assert "Van Hove" not in out
        files = set(os.listdir(tmp_path / name))
        assert not files & {"gd_vpi.out", "gs_vpi.out"}
        for f in ("e_vpi.out", "et_vpi.out", "gr_vpi.out", "sk_vpi.out", "nr_vpi.out"):
            assert open(tmp_path / name / f, "rb").read() == open(os.path.join(gold, f), "rb").read(), (name, f)
        outs.append([ln for ln in out.splitlines() if "Time per block" not in ln and "host threads" not in ln])
    assert outs[0] == outs[1]
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "off"))
