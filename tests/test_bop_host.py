"""The bond-orientational order key on a machine without a GPU: the front end's refusals on the CPU twin (the host built
against tests/shim, which does not provide pigs_bop_*) and its unchanged runs without the key."""
import os
import re
import subprocess

import pytest

from conftest import GOLDEN
from hostlib import build_cpu_host

RUNS = os.path.join(GOLDEN, "vpi_runs")
PBC = os.path.join(RUNS, "he4_cworm0", "vpi.in")                  # 2D, 9 particles at density 0.25: half side 3
TRAP = os.path.join(RUNS, "trap2d_bis_cworm0", "vpi.in")


def _key(extra=", bo_rnb = 2.0"):
    return f"&gpu\n bond_order = T{extra}\n/\n"


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
    """The front end names no pigs_bop_* symbol at link time: the shim does not define them and it still links."""
    assert os.path.exists(cpu_exe)
    nm = subprocess.run(["nm", "-u", cpu_exe], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True)
    assert b"pigs_ctx_create" in nm.stdout                     # nm lists the backend's symbols: the check has teeth
    assert b"pigs_bop" not in nm.stdout
    assert b"bond_order" in open(cpu_exe, "rb").read()          # the front end knows the key


def test_key_is_refused_by_a_backend_without_the_entry_points(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "bond_order" in out and "backend" in out, out
    assert all(s in out for s in ("pigs_bop_init", "_accumulate", "_read")), out
    assert not os.path.exists(tmp_path / "bo_vpi.out") and not os.path.exists(tmp_path / "e_vpi.out")


def test_key_is_refused_for_a_trapped_system(cpu_exe, tmp_path):
    rc, out = _run(cpu_exe, open(TRAP).read() + _key(), str(tmp_path))
    assert rc == 2
    assert "bond_order" in out and "periodic" in out and "pigs_bop" not in out, out


def test_key_is_refused_in_one_dimension(cpu_exe, tmp_path):
    txt, k = re.subn(r"dim\s*=\s*2", "dim = 1", _short(open(PBC).read()))
    assert k == 1
    rc, out = _run(cpu_exe, txt + _key(), str(tmp_path))
    assert rc == 2
    assert "bond_order" in out and "dim" in out and "pigs_bop" not in out, out


@pytest.mark.parametrize("extra,word", [("", "bo_rnb"),                                # missing
                                        (", bo_rnb = 0.0", "bo_rnb"),
                                        (", bo_rnb = -1.0", "bo_rnb"),
                                        (", bo_rnb = 3.001", "bo_rnb"),                 # above half the side
                                        (", bo_rnb = 2.0, bo_nhist = 0", "bo_nhist"),
                                        (", bo_rnb = 2.0, bo_nhist = 4097", "bo_nhist"),
                                        (", bo_rnb = 2.0, bo_nr = 8193", "bo_nr"),
                                        (", bo_rnb = 2.0, bo_window = -1", "bo_window"),
                                        (", bo_rnb = 2.0, bo_window = 1000", "bo_window")])   # > Nb
def test_out_of_range_keys_are_refused(cpu_exe, tmp_path, extra, word):
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(extra), str(tmp_path))
    assert rc == 2, out[-2000:]
    assert "bond_order" in out and word in out and "pigs_bop" not in out, out      # refused for the values, not the backend
    assert not os.path.exists(tmp_path / "e_vpi.out")


def test_radius_of_half_the_side_is_accepted_for_its_value(cpu_exe, tmp_path):
    """bo_rnb = half the side passes the value checks (and is then refused for the backend)."""
    rc, out = _run(cpu_exe, _short(open(PBC).read()) + _key(", bo_rnb = 3.0, bo_nr = 0, bo_nhist = 4096"), str(tmp_path))
    assert rc == 2 and "pigs_bop" in out, out


def test_run_without_the_key_is_its_golden_files(cpu_exe, tmp_path):
    """The golden run itself, once plain and once with the key spelled out as off: both byte-identical to the golden files."""
    gold = os.path.join(RUNS, "he4_cworm0")
    txt = open(PBC).read()
    outs = []
    for name, extra in (("plain", ""), ("off", "&gpu\n bond_order = F, bo_rnb = 2.0, bo_nhist = 9, bo_window = 1\n/\n")):
        rc, out = _run(cpu_exe, txt + extra, str(tmp_path / name))
        assert rc == 0, out[-2000:]
        assert "Bond order" not in out
        files = set(os.listdir(tmp_path / name))
        assert not files & {"bo_vpi.out", "boh_vpi.out", "g6_vpi.out"}
        for f in ("e_vpi.out", "et_vpi.out", "gr_vpi.out", "sk_vpi.out", "nr_vpi.out"):
            assert open(tmp_path / name / f, "rb").read() == open(os.path.join(gold, f), "rb").read(), (name, f)
        outs.append([ln for ln in out.splitlines() if "Time per block" not in ln and "host threads" not in ln])
    assert outs[0] == outs[1]
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "off"))
