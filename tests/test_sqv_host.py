"""The vector structure factor on a machine without a GPU: the front end's refusals on the CPU twin (the host built
against tests/shim, which does not provide pigs_sqv_*), its unchanged runs without the key, and the package's helpers
(pathintegralgroundstate_amd.profiles.normalize_sqv, shell_average) on hand-made sums."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from hostlib import build_cpu_host
from sqv_numpy import n_vectors, vectors

RUNS = os.path.join(GOLDEN, "vpi_runs")
PBC = os.path.join(RUNS, "he4_cworm0", "vpi.in")
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")


def _key(extra=""):
    return f"&gpu\n sq_vector = T{extra}\n/\n"


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
    txt = re.sub(r"Nblock\s*=\s*\d+", "Nblock = 2", txt)
    return re.sub(r"Nstep\s*=\s*\d+", "Nstep = 3", txt)


def test_cpu_twin_still_links_against_the_unchanged_shim(cpu_exe):
    """The front end names no pigs_sqv_* symbol at link time: the shim does not define them and it still links."""
    assert os.path.exists(cpu_exe)
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout                     # nm lists the backend's symbols: the check has teeth
    assert b"pigs_sqv" not in nm.stdout
    assert b"sq_vector" in open(cpu_exe, "rb").read()           # the front end knows the key


def test_periodic_run_without_the_key_is_unchanged(cpu_exe, tmp_path):
    """Within this binary: a run without the key against one with the key spelled out as off."""
    txt = _short(open(PBC).read())
    rc, out = _run(cpu_exe, txt, str(tmp_path / "plain"))
    assert rc == 0, out[-2000:]
    assert "Vector S(q)" not in out
    files = set(os.listdir(tmp_path / "plain"))
    assert {"e_vpi.out", "sk_vpi.out", "gr_vpi.out", "worldlines_final.bin"} <= files
    assert "sqvec_vpi.out" not in files and "sq_vpi.out" not in files
    rc, out2 = _run(cpu_exe, txt + "&gpu\n sq_vector = F, sq_nmax = 4, sq_window = 1\n/\n", str(tmp_path / "off"))
    assert rc == 0, out2[-2000:]
    assert set(os.listdir(tmp_path / "off")) == files
    for f in files - {"vpi.in"}:
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "off" / f, "rb").read(), f
    strip = lambda s: [ln for ln in s.splitlines() if "Time per block" not in ln and "host threads" not in ln]
    assert strip(out) == strip(out2)


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", sq_nmax = 4"), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "sq_vector" in out and "backend" in out and "pigs_sqv" in out, out
    assert not os.path.exists(tmp_path / "sqvec_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + _key(), str(tmp_path))
    assert rc == 2
    assert "sq_vector" in out and "periodic" in out, out


@pytest.mark.parametrize("extra,word", [(", sq_nmax = 0", "sq_nmax"),
                                        (", sq_nmax = 65", "sq_nmax"),            # the fixture is 2D: 64 is the limit
                                        (", sq_window = -1", "sq_window"),
                                        (", sq_window = 1000", "sq_window")])     # > Nb
def test_out_of_range_keys_are_refused(cpu_exe, tmp_path, extra, word):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "sq_vector" in out and word in out and "pigs_sqv" not in out, out      # refused for the values, not the backend
    assert not os.path.exists(tmp_path / "e_vpi.out")


def test_nmax_limit_depends_on_the_dimension(cpu_exe, tmp_path):
    """3D stops at 16: 17 is refused for its value; 2D takes 64 (and is then refused for the backend)."""
    txt3 = _short(open(os.path.join(RUNS, "he4_worm_s1982", "vpi.in")).read())
    rc, out = _run(cpu_exe, txt3 + _key(", sq_nmax = 17"), str(tmp_path / "a"))
    assert rc == 2 and "sq_nmax" in out and "pigs_sqv" not in out, out
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", sq_nmax = 64"), str(tmp_path / "b"))
    assert rc == 2 and "pigs_sqv" in out, out


def test_normalize_sqv_on_hand_made_sums():
    from pathintegralgroundstate_amd.profiles import normalize_sqv
    Np, window = 5, 2
    raw = np.array([[3 * 5 * Np * 1.5, 3 * 5 * Np * 0.25], [1.0, 2.0]])
    S = normalize_sqv(raw, np.array([3, 0]), Np, window)
    assert S.shape == raw.shape and S[0].tolist() == [1.5, 0.25]
    assert np.all(np.isnan(S[1]) | np.isinf(S[1]))                      # a walker without samples
    one = normalize_sqv(raw[0], 3, Np, window)
    assert one.tolist() == [1.5, 0.25]
    assert normalize_sqv(np.array([12.0]), np.int64(4), 3, 0)[0] == 1.0  # window 0: sum/(samples*Np)


def test_shell_average_cubic_box():
    """Cubic box, nmax = 2, 3D: 62 stored vectors in the shells sum n^2 = 1..6, 8, 9, 12 with the +-q multiplicities
    6, 12, 8, 6, 24, 24, 12, 24, 8, which sum to 5^3 - 1 = 124.  Shell 9 holds the 24 vectors of (2,2,1) type only: the
    six of (3,0,0) type that a full shell 9 would add lie outside |n_k| <= 2."""
    from pathintegralgroundstate_amd.profiles import shell_average
    n = vectors(3, 2)
    assert n.shape == (62, 3) == (n_vectors(3, 2), 3)
    L = [4.0, 4.0, 4.0]
    key = (n.astype(np.int64) ** 2).sum(axis=1)
    Sq = np.stack([key.astype(np.float64), 10.0 + n[:, 0] + 0.5 * n[:, 1] + 0.25 * n[:, 2]])
    q, mean, mult = shell_average(n, L, Sq)
    shells = [1, 2, 3, 4, 5, 6, 8, 9, 12]
    assert mult.tolist() == [6, 12, 8, 6, 24, 24, 12, 24, 8] and int(mult.sum()) == 124
    assert np.allclose(q, (2 * np.pi / 4.0) * np.sqrt(shells), rtol=1e-14)
    assert mean.shape == (2, 9) and np.allclose(mean[0], shells, rtol=1e-15)
    for j, s in enumerate(shells):                                      # the mean over the STORED vectors of the shell
        assert mean[1, j] == pytest.approx(Sq[1][key == s].mean(), rel=1e-15)
    q1, m1, c1 = shell_average(n, L, Sq[1])                             # one walker's row
    assert np.array_equal(m1, mean[1]) and np.array_equal(c1, mult)


def test_shell_average_non_cubic_box():
    """Box lengths with incommensurate squares: no two axes share a shell; only the sign variants (n1, +-n2, +-n3) do."""
    from pathintegralgroundstate_amd.profiles import shell_average
    n = vectors(3, 1)
    L = [2.0, 2.0 * np.sqrt(2.0), 2.0 * np.sqrt(3.0)]
    Sq = np.arange(13, dtype=np.float64)
    q, mean, mult = shell_average(n, L, Sq)
    # |n| patterns (a,b,c) in {0,1}^3 without 0: 7 shells; multiplicity 2^(number of non-zero components)
    assert q.size == 7 and sorted(mult.tolist()) == [2, 2, 2, 4, 4, 4, 8] and int(mult.sum()) == 26
    assert np.all(np.diff(q) > 0)
    qb = 2 * np.pi / np.asarray(L)
    axis = [np.flatnonzero((np.abs(n) == e).all(axis=1)) for e in np.eye(3, dtype=int)]
    assert all(a.size == 1 for a in axis)
    for k in range(3):                                                  # each axis vector sits alone in its shell
        j = int(np.argmin(np.abs(q - qb[k])))
        assert mult[j] == 2 and mean[j] == Sq[axis[k][0]] and q[j] == pytest.approx(qb[k], rel=1e-15)
    # 2D, a box with equal sides stored with one different bit is not cubic, but its shells still merge to 1e-12
    n2 = vectors(2, 1)
    q2, mean2, mult2 = shell_average(n2, [3.0, np.nextafter(3.0, 4.0)], np.array([1.0, 2.0, 3.0, 4.0]))
    assert mult2.tolist() == [4, 4] and mean2.tolist() == [2.0, 3.0]
