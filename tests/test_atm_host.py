"""The three_body key on a machine without a GPU: the Fortran normalisation and writers of the front end (pigs_estimators
normalize_atm / write_v3_block / write_v3tau, through the host library's hook hs_atm_files) against
pathintegralgroundstate_amd.profiles.normalize_atm / pressure_atm, and the front end's refusals on the CPU twin (the host
built against tests/shim, which does not provide pigs_atm_*)."""
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
PBC = os.path.join(RUNS, "he4_cworm0", "vpi.in")                  # 2D, periodic
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")
ONE_D = os.path.join(RUNS, "ho1d_n2", "vpi.in")                   # 1D (trapped as it stands)
PRINT = 1.0000001e-9                                             # the files carry 10 significant digits


def _key(extra=""):
    return f"&gpu\n three_body = T{extra}\n/\n"


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
    # the host library finds the shim it was linked against by its run path.  The shim is NOT loaded into the global
    # scope: this file runs before the GPU tests of a whole-suite run, and the shim's pigs_* symbols would then take the
    # place of libpigs_hip.so's own in that library's internal calls.
    H = C.CDLL(hostlib)
    lp, dp = C.POINTER(C.c_int64), C.POINTER(C.c_double)
    H.hs_atm_files.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int, lp, dp, lp,
                               dp, dp, dp, C.c_char_p, C.c_char_p]
    H.hs_atm_files.restype = None

    def call(dim, Np, density, Nb, window, dt, nu, S, T, ntrip, fb, ft):
        nb, ns = len(S), 2 * window + 1
        assert T.shape == (nb, ns) and ntrip.shape == (nb, ns) and ntrip.dtype == np.int64 and T.dtype == np.float64
        v3, cnt, mean = np.zeros(ns), np.zeros(ns), C.c_double(0.0)
        H.hs_atm_files(dim, Np, density, Nb, window, dt, nu, nb, S.ctypes.data_as(lp), T.ctypes.data_as(dp),
                       ntrip.ctypes.data_as(lp), v3.ctypes.data_as(dp), cnt.ctypes.data_as(dp), C.byref(mean),
                       fb.encode(), ft.encode())
        return v3, cnt, mean.value
    return call


@pytest.mark.parametrize("dim,window,nu", [(2, 0, 1.0), (3, 3, 0.327), (3, 1, -2.5)])
def test_fortran_normalisation_and_writers_match_the_package(cpu_host, tmp_path, dim, window, nu):
    """Random sums of three blocks of one walker, of both signs: the last block's V3/N per slice, its window mean and the
    mean triplets from Fortran against normalize_atm; v3_vpi.out (block, V3/N, P3) against normalize_atm / pressure_atm per
    block; v3tau_vpi.out (a, tau, mean, error, triplets) against numpy on the package's block values."""
    call = _hook(cpu_host)
    rng = np.random.default_rng(50 + dim + window)
    Np, density, Nb, dt, nb = 37, 0.365, 5, 0.0125, 3
    ns = 2 * window + 1
    S = np.array([4, 1, 7], np.int64)
    T = rng.normal(0.0, 3.0, (nb, ns)) * np.array([1.0, 1e-3, 50.0])[:, None]
    ntrip = rng.integers(1, 100000, (nb, ns)).astype(np.int64)
    fb, ft = str(tmp_path / "v3_vpi.out"), str(tmp_path / "v3tau_vpi.out")
    v3, cnt, mean = call(dim, Np, density, Nb, window, dt, nu, S, T, ntrip, fb, ft)
    blocks = [profiles.normalize_atm({"T": T[b], "ntrip": ntrip[b], "samples": S[b]}, Np, nu) for b in range(nb)]
    last = blocks[-1]
    assert np.allclose(v3, last["v3"], rtol=1e-14, atol=0) and np.allclose(cnt, last["ntrip"], rtol=1e-14, atol=0)
    assert abs(mean - last["v3_mean"]) <= 1e-14 * np.abs(last["v3"]).sum()
    assert np.allclose(last["v3"], nu * T[-1] / (S[-1] * Np), rtol=1e-15) and (v3 * nu * T[-1] > 0).all()
    # v3_vpi.out: one line per block
    tab = np.loadtxt(fb, ndmin=2)
    assert tab.shape == (nb, 3) and tab[:, 0].tolist() == [1.0, 2.0, 3.0]
    assert open(fb).readline().startswith("#")
    vm = np.array([b["v3_mean"] for b in blocks])
    scale = np.array([np.abs(b["v3"]).mean() for b in blocks])            # the mean of terms of both signs: to their scale
    assert np.all(np.abs(tab[:, 1] - vm) <= PRINT * scale)
    assert np.allclose(tab[:, 2], profiles.pressure_atm(tab[:, 1], density, dim), rtol=PRINT, atol=0)
    assert np.all(np.abs(tab[:, 2] - 9.0 * density * vm / dim) <= 9.0 * density / dim * PRINT * scale)
    # v3tau_vpi.out: one line per window slice
    tau = np.loadtxt(ft, ndmin=2)
    assert tau.shape == (ns, 5)
    a = np.arange(Nb - window, Nb + window + 1)
    assert np.array_equal(tau[:, 0], a) and np.allclose(tau[:, 1], (a - Nb) * dt, rtol=PRINT, atol=0)
    x = np.stack([b["v3"] for b in blocks])
    m = x.mean(axis=0)
    err = np.sqrt(np.maximum((x * x).mean(axis=0) - m * m, 0.0) / nb)
    assert np.allclose(tau[:, 2], m, rtol=PRINT, atol=0)
    assert np.all(np.abs(tau[:, 3] - err) <= np.sqrt(4.0 * np.abs(m) * PRINT * np.abs(m)) + PRINT * err) and (err > 0).all()
    assert np.allclose(tau[:, 4], np.stack([b["ntrip"] for b in blocks]).mean(axis=0), rtol=PRINT, atol=0)
    # the window mean of the file's last block is the mean of the package's per-slice column
    assert abs(tab[-1, 1] - last["v3"].mean()) <= PRINT * scale[-1]


def test_normalize_atm_shapes_and_empty_walkers():
    raw = {"T": np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]]), "ntrip": np.array([[2, 4, 6], [0, 0, 0]]), "samples": np.array([2, 0])}
    n = profiles.normalize_atm(raw, 10, 3.0)
    assert n["v3"].shape == (2, 3) and n["v3_mean"].shape == (2,) and n["ntrip"].shape == (2, 3)
    assert np.allclose(n["v3"][0], 3.0 * np.array([1.0, 2.0, 3.0]) / 20.0) and np.isclose(n["v3_mean"][0], 0.3)
    assert n["ntrip"][0].tolist() == [1.0, 2.0, 3.0]
    assert np.isnan(n["v3"][1]).all() and np.isnan(n["v3_mean"][1]) and np.isnan(n["ntrip"][1]).all()   # no samples: NaN
    assert np.allclose(profiles.normalize_atm(raw, 10)["v3"][0] * 3.0, n["v3"][0], rtol=1e-15)     # nu left out: 1
    with pytest.raises(ValueError):
        profiles.normalize_atm({"T": np.zeros(4), "ntrip": np.zeros(4), "samples": np.array(1)}, 10)
    # P3 = 9 nu <T>/(dim Volume) = 9 density (V3/N)/dim
    assert profiles.pressure_atm(0.5, 0.2, 3) == 9.0 * 0.2 * 0.5 / 3 and profiles.pressure_atm(-1.0, 0.25, 2) == -1.125


def test_cpu_twin_still_links_against_the_unchanged_shim(cpu_exe):
    """The front end names no pigs_atm_* symbol at link time: the shim does not define them and it still links."""
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout and b"pigs_atm" not in nm.stdout
    assert b"atm_rc" in open(cpu_exe, "rb").read()             # the front end knows the keys


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", atm_nu = 0.5d0"), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "three_body" in out and "backend" in out and all(s in out for s in ("pigs_atm_init", "_accumulate", "_read")), out
    assert not os.path.exists(tmp_path / "v3_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + _key(), str(tmp_path))
    assert rc == 2
    assert "three_body" in out and "periodic" in out and "pigs_atm" not in out, out


def test_key_is_refused_in_one_dimension(cpu_exe, tmp_path):
    txt = open(ONE_D).read()
    assert re.search(r"dim\s*=\s*1\b", txt) and "trap = T" in txt
    rc, out = _run(cpu_exe, _short(txt.replace("trap = T", "trap = F")) + _key(), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "three_body" in out and "dim = 2 or 3" in out and "pigs_atm" not in out, out
    assert not os.path.exists(tmp_path / "e_vpi.out")


@pytest.mark.parametrize("extra,word", [(", atm_window = 1000", "atm_window"), (", atm_window = 7", "atm_window"),
                                        (", atm_rc = 1.d3", "atm_rc"), (", atm_rc = 3.0001d0", "atm_rc")])
def test_out_of_range_keys_are_refused(cpu_exe, tmp_path, extra, word):
    """he4_cworm0 has Nb = 6 and a square box of side 6 (Np = 9 at density 0.25): half a side is 3."""
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "three_body" in out and word in out and "pigs_atm" not in out, out      # refused for the values, not the backend
    assert not os.path.exists(tmp_path / "e_vpi.out")


def test_limits_and_defaults_are_accepted_for_their_values(cpu_exe, tmp_path):
    """atm_rc left out, zero, negative or at half the side, atm_window left out, negative or at Nb, atm_nu given or not: the
    value checks pass (and the run is then refused for the backend)."""
    for extra in ("", ", atm_rc = 0.d0, atm_window = 6", ", atm_rc = -1.d0, atm_window = -3", ", atm_rc = 3.d0, atm_nu = 2.d0"):
        rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
        assert rc == 2 and "pigs_atm" in out, out


def test_run_without_the_key_is_its_golden_files(cpu_exe, tmp_path):
    """The golden run with the key spelled out as off: byte-identical to the golden files."""
    gold = os.path.join(RUNS, "he4_cworm0")
    rc, out = _run(cpu_exe, open(PBC).read() + "&gpu\n three_body = F, atm_nu = 3.d0, atm_rc = 1.5, atm_window = 2\n/\n", str(tmp_path))
    assert rc == 0 and "Three-body" not in out, out[-2000:]
    assert not set(os.listdir(tmp_path)) & {"v3_vpi.out", "v3tau_vpi.out"}
    for f in ("e_vpi.out", "et_vpi.out", "gr_vpi.out", "sk_vpi.out", "nr_vpi.out"):
        assert open(tmp_path / f, "rb").read() == open(os.path.join(gold, f), "rb").read(), f
