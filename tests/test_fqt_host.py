"""Imaginary-time density correlations F(q,tau) on a machine without a GPU: the front end's refusals on the CPU twin (the
host built against tests/shim, which does not provide pigs_fqt_*), its unchanged runs without the key, and the package's
normalisation helper (pathintegralgroundstate_amd.profiles.normalize_fqt) on hand-made sums."""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from hostlib import build_cpu_host

RUNS = os.path.join(GOLDEN, "vpi_runs")
PBC = os.path.join(RUNS, "he4_cworm0", "vpi.in")
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")


def _key(extra=""):
    return f"&gpu\n fq_tau = T{extra}\n/\n"


@pytest.fixture(scope="module")
def cpu_exe():
    _, _, exe = build_cpu_host()
    return exe


def _run(exe, txt, wd):
    os.makedirs(wd, exist_ok=True)
    with open(os.path.join(wd, "vpi.in"), "w") as f:
        f.write(txt)
    with open(os.path.join(wd, "vpi.in")) as fin:
        r = subprocess.run([exe], stdin=fin, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, cwd=wd, timeout=600)
    return r.returncode, r.stdout.decode(errors="replace")


def _short(txt):
    """The fixture's input cut to two short blocks (the refusals never get that far; the unchanged run does)."""
    import re
    txt = re.sub(r"Nblock\s*=\s*\d+", "Nblock = 2", txt)
    return re.sub(r"Nstep\s*=\s*\d+", "Nstep = 3", txt)


def test_cpu_twin_still_links_against_the_unchanged_shim(cpu_exe):
    """The front end names no pigs_fqt_* symbol at link time: the shim does not define them and it still links."""
    assert os.path.exists(cpu_exe)
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout                     # nm lists the backend's symbols: the check has teeth
    assert b"pigs_fqt" not in nm.stdout
    # ... and the front end does know the key (the parent commit's namelist does not: it would run and write no file)
    assert b"fq_tau" in open(cpu_exe, "rb").read()


def test_periodic_run_without_the_key_is_unchanged(cpu_exe, tmp_path):
    """A regression guard, not a test of the feature: it also passes on a front end without the key (the &gpu read
    ignores its status, so an unknown `fq_tau = F` is dropped there).  It compares, within THIS binary, a run without
    the key against one with the key spelled out as off; it does not hold the bytes of any earlier build."""
    txt = _short(open(PBC).read())
    rc, out = _run(cpu_exe, txt, str(tmp_path / "plain"))
    assert rc == 0, out[-2000:]
    assert "F(q,tau)" not in out
    files = set(os.listdir(tmp_path / "plain"))
    assert {"e_vpi.out", "sk_vpi.out", "gr_vpi.out", "worldlines_final.bin"} <= files
    assert "fqt_vpi.out" not in files
    # the key spelled out as off: the same files, byte for byte, and the same report but for its timing lines
    rc, out2 = _run(cpu_exe, txt + "&gpu\n fq_tau = F, fq_ntau = 4\n/\n", str(tmp_path / "off"))
    assert rc == 0, out2[-2000:]
    assert set(os.listdir(tmp_path / "off")) == files
    for f in files - {"vpi.in"}:
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "off" / f, "rb").read(), f
    strip = lambda s: [ln for ln in s.splitlines() if "Time per block" not in ln and "host threads" not in ln]
    assert strip(out) == strip(out2)


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", fq_ntau = 4"), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "fq_tau" in out and "backend" in out and "pigs_fqt" in out, out
    assert not os.path.exists(tmp_path / "fqt_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + _key(), str(tmp_path))
    assert rc == 2
    assert "fq_tau" in out and "periodic" in out, out


@pytest.mark.parametrize("extra,word", [(", fq_ntau = 7, fq_window = 3", "fq_ntau"),      # Ntau > 2 W
                                        (", fq_ntau = -1", "fq_ntau"),
                                        (", fq_ntau = 2, fq_window = 1000", "fq_window"),   # W > Nb
                                        (", fq_ntau = 2000", "fq_window")])                 # default W = 1000 > Nb
def test_bad_lags_and_windows_are_refused(cpu_exe, tmp_path, extra, word):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "fq_tau" in out and word in out and "pigs_fqt" not in out, out      # refused for the values, not the backend


def test_normalisation_helper_on_hand_made_sums():
    from pathintegralgroundstate_amd.profiles import normalize_fqt
    Np, window, dt, Lbox = 5, 2, 0.25, [2.0, 4.0, 8.0]
    Ntau, Nk, dim = 3, 2, 3
    raw = np.zeros((2, Ntau + 1, Nk, dim))
    # walker 0: 3 samples; every pair product is 7, so every lag normalises to 7/Np
    for l in range(Ntau + 1):
        raw[0, l] = 3 * (2 * window + 1 - l) * 7.0
    raw[0, 2, 1, 2] = 3 * 3 * 10.0                     # lag 2 has 3 pairs
    F, q, tau = normalize_fqt({"F": raw, "samples": np.array([3, 0])}, Np, window, dt, Lbox)
    assert F.shape == raw.shape and q.shape == (Nk, dim) and tau.shape == (Ntau + 1,)
    want = np.full((Ntau + 1, Nk, dim), 7.0 / Np)
    want[2, 1, 2] = 10.0 / Np
    assert np.allclose(F[0], want, rtol=1e-15, atol=0.0)
    assert np.all(np.isnan(F[1]))                      # a walker without samples
    assert np.array_equal(tau, [0.0, 0.25, 0.5, 0.75])
    assert np.allclose(q, [[math.pi, math.pi / 2, math.pi / 4], [2 * math.pi, math.pi, math.pi / 2]], rtol=1e-15)
    # one walker's slice of the dict; n_pairs of lag 0 is 2*window + 1
    F1, _, _ = normalize_fqt({"F": raw[0], "samples": np.int64(3)}, Np, window, dt, Lbox)
    assert np.array_equal(F1, F[0])
    assert F1[0, 0, 0] == raw[0, 0, 0, 0] / (3 * 5 * Np)
    # dim 1, window 0: the S(k) normalisation sum/(samples*Np)
    F2, q2, tau2 = normalize_fqt({"F": np.array([[[[12.0]]]]), "samples": np.array([4])}, 3, 0, 0.1, [2.0])
    assert F2.shape == (1, 1, 1, 1) and F2[0, 0, 0, 0] == 1.0 and tau2.tolist() == [0.0] and q2[0, 0] == pytest.approx(math.pi)
    with pytest.raises(ValueError):
        normalize_fqt({"F": np.zeros((1, 4, 1, 1)), "samples": np.array([1])}, 3, 1, 0.1, [2.0])      # 4 lags, window 1
