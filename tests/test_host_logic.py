"""Host-side logic that needs no GPU: namelist front end, derived box / cutoff / grid values,
host table fill, and that the C-ABI library loads and exports every declared symbol."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden
from helpers import same_bits, ulp_diff
from pathintegralgroundstate_amd import SystemConfig, read_namelists

STOCK = """&system
 dim      = 3,          ! Dimensions
 Np       = 64,         ! Number of particles
 density  = 0.365d0,    ! Density
 trap     = F           ! T if the system is trapped, F otherwise
/
&samp
 resume   = F
 dt       = 5.00d-3,
 Nb       = 32,
 seed     = 1982,
 delta_cm = 0.12d0,
 CMFreq   = 1,
 sampling = 'bis',\t! Movement type
 Lstag    = 32,
 Nlev     = 4,
 Nstag    = 5,
 Nblock   = 400,
 Nstep    = 100,
 Nbin     = 100,
 Nk       = 50
/
&obdm
 swapping = T, CWorm = 0.5d0, Nobdm = 10, Npw = 0
/
&wavefun
 Nmax     = 10000, wf_table = T, v_table  = T
/
&jastrow
 Rm       = 1.20d0
/
"""


def test_namelists_stock_input():
    g = read_namelists(STOCK)
    assert g["system"] == {"crystal": False, "trap": False, "dim": 3, "np": 64, "density": 0.365}
    assert g["samp"]["sampling"] == "bis" and g["samp"]["nlev"] == 4 and g["samp"]["dt"] == 5e-3
    assert g["obdm"] == {"swapping": True, "cworm": 0.5, "nobdm": 10, "npw": 0}
    assert g["wavefun"] == {"nmax": 10000, "wf_table": True, "v_table": True}
    c = SystemConfig.from_namelists(STOCK)
    assert (c.dim, c.Np, c.Nb, c.M, c.Nmax) == (3, 64, 32, 65, 10000)
    assert c.path_shape == (65, 64, 3)


def test_namelist_defaults_and_trap():
    txt = "&system\n dim=1, Np=2, trap=T\n/\n&samp\n dt=1.d-2, Nb=10\n/\n&extpot\n a_ho = 1.5d0\n/\n&jastrow\n Rm=0.5\n/\n"
    c = SystemConfig.from_namelists(txt)
    assert c.trap and c.a_ho[0] == 1.5 and c.seed == 1982 and c.Lstag == 2 and c.Nlev == 1
    assert not c.swapping and c.CWorm == 0.0 and c.Nmax == 10000
    # vpi.f90:84-92: rcut = 10*(3*a)^(1/dim)
    assert c.rcut == 10.0 * (3.0 * 1.5)


@pytest.mark.parametrize("name", ["tables_he4_n64", "tables_he4_n256", "pbc2d_n16"])
def test_derived_quantities_match_reference(name):
    """Lbox, rcut, dr as the reference derives them (vpi.f90:112-128, vpi_mod.f90:94), bitwise."""
    d = load_golden(name)
    c = SystemConfig(dim=int(d["dim"]), Np=int(d["Np"]), Nb=int(d["Nb"]), density=float(d["density"]))
    assert c.Lbox[0] == d["Lbox"][0] and c.rcut == float(d["rcut"]) and c.dr == float(d["dr"])


def _header_symbols():
    txt = open(os.path.join(ROOT, "include", "pigs_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pigs_[a-z0-9_]+)\s*\(", txt)))


def test_abi_exports_every_declared_symbol():
    from pathintegralgroundstate_amd import api
    from pathintegralgroundstate_amd.build import build
    build()
    L = api.load_library()
    syms = _header_symbols()
    assert len(syms) >= 20
    assert sorted(api.ABI_SYMBOLS) == syms
    for s in syms:
        assert hasattr(L, s), f"libpigs_hip.so does not export {s}"
    assert L.pigs_abi_version() == 1


def test_host_table_fill_matches_reference_tables():
    from pathintegralgroundstate_amd import api
    from pathintegralgroundstate_amd.build import build
    build()
    for name in ("tables_he4_n64", "tables_he4_n256"):
        t = load_golden(name)
        c = SystemConfig(dim=3, Np=int(t["Np"]), Nb=int(t["Nb"]))
        VT, WF = api.build_tables(c)
        # table construction gets the looser bar of SURVEY §8c (<= 4 ulp); kernels are always
        # fed the reference's own tables in the parity tests
        assert np.nanmax(ulp_diff(VT, t["VTable"])) <= 4 and np.nanmax(ulp_diff(WF, t["LogWF"])) <= 4
        assert np.isnan(VT[1]) and WF[1] == -np.inf and VT[0] == VT[2]


def test_no_gpu_fails_loudly():
    """Without a device the product must raise -- never fall back to a CPU path."""
    from pathintegralgroundstate_amd import api
    from pathintegralgroundstate_amd.build import build
    build()
    if api.device_count() > 0:
        pytest.skip("a GPU is visible here")
    t = load_golden("tables_he4_n64")
    c = SystemConfig(dim=3, Np=64, Nb=40)
    with pytest.raises(api.PigsError, match="no HIP device|status -3|status -2"):
        api.PigsContext(c, t["VTable"], t["LogWF"], n_walkers=1)


def test_missing_library_fails_loudly(tmp_path):
    from pathintegralgroundstate_amd import api
    saved = api._lib
    api._lib = None
    try:
        with pytest.raises(api.PigsError, match="no CPU fallback"):
            api.load_library(str(tmp_path / "libpigs_hip.so"))
    finally:
        api._lib = saved


def test_product_never_imports_oracle():
    """The oracle is test infrastructure: nothing under the package may reference it."""
    pkg = os.path.join(ROOT, "pathintegralgroundstate_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".f90")):
                src = open(os.path.join(dp, f), errors="replace").read()
                assert "pyoracle" not in src and "pigs_oracle" not in src and "libvpiref" not in src, f


def test_lj_and_dipolar_table_fill():
    """Host table fill for the potentials of BASELINE configs 2 and 5 against the externally filled
    tables of the golden fixtures (numpy expressions of the same formulas: <= 4 ulp)."""
    from pathintegralgroundstate_amd import api
    from pathintegralgroundstate_amd.build import build
    build()
    c = SystemConfig(dim=3, Np=64, Nb=40)
    for kind in ("lj", "dipolar"):
        VT, WF = api.build_tables(c, potential=kind)
        want = load_golden(f"he4_n64_table_{kind}")["VTable"]
        fin = np.isfinite(want) & np.isfinite(VT)
        assert fin.sum() > 9990
        # (1/r^6 - 1) cancels at r = 1: compare on the scale of the two terms, not in ulps of the difference
        assert np.all(np.abs(VT[fin] - want[fin]) <= 1e-14 * (np.abs(want[fin]) + 22.0228))
        assert VT[0] == VT[2] and VT[c.Nmax + 1] == VT[c.Nmax]


def test_log_host_matches_this_machines_libm(tmp_path):
    """csrc/pigs_log_host.h (the device sampler's log) compiled for the CPU with the same fusions (g++ -mfma,
    -ffp-contract=off) against libm's log on 2e8 arguments of the sampler's domain: identical bits.  On the GPU the
    same source is checked by pigs_selftest_log (tests/test_gpu_parity.py)."""
    import subprocess
    from conftest import ROOT
    if "fma" not in open("/proc/cpuinfo").read():
        pytest.skip("this CPU has no FMA: glibc resolves log to another build")
    exe = str(tmp_path / "log_host_check")
    subprocess.check_call(["g++", "-O2", "-mfma", "-ffp-contract=off", "-fopenmp",
                           "-I" + os.path.join(ROOT, "pathintegralgroundstate_amd", "csrc"),
                           os.path.join(ROOT, "tests", "shim", "log_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe, "200"], capture_output=True, text=True, timeout=600)
    tested, bad, first = out.stdout.split()
    assert out.returncode == 0 and int(bad) == 0 and int(tested) >= 200000000, out.stdout


def _split_rule(sw, listed, cap, unique):
    """The launch split of the accumulator families, restated: (start, walkers) of every launch."""
    out, i0 = [], 0
    while i0 < len(sw):
        seen, m = set(), 0
        while i0 + m < len(sw) and m < cap and not (unique and listed and sw[i0 + m] in seen):
            seen.add(sw[i0 + m])
            m += 1
        out.append((i0, sw[i0:i0 + m]))
        i0 += m
    return out


def test_walker_split_matches_the_stated_rule(tmp_path):
    """csrc/pigs_walker_split.h (where every pigs_*_accumulate ends one launch and begins the next) compiled for the CPU
    against _split_rule: the same (start, count) sequence and the same list entries for random and built requests --
    lists left out, caps 1, 2, 3 and 256, lengths 0..700, repeats adjacent, separated and exactly at a cap boundary,
    with and without `unique`, all on ONE set of marks.  Once as built, once under -fsanitize=address,undefined."""
    import subprocess
    W = 700
    rng = np.random.default_rng(20261019)
    cases = []
    for cap in (1, 2, 3, 256):
        for unique in (0, 1):
            for n in (0, 1, cap - 1, cap, cap + 1, 2 * cap, 2 * cap + 1, 700):
                cases.append((cap, unique, 0, list(range(max(n, 0)))))              # the list left out
            base = list(range(10, 10 + 2 * cap + 2))
            for i, j in ((1, 0), (cap - 1, 0), (cap, 0), (cap, cap - 1), (cap + 1, cap), (cap + 1, 1), (2 * cap, cap),
                         (2 * cap, cap - 1), (2 * cap + 1, cap + 1)):
                sw = list(base)                                                     # walker sw[j] again at position i
                sw[i] = sw[j]
                cases.append((cap, unique, 1, sw))
            cases.append((cap, unique, 1, [5] * (cap + 3)))
            cases.append((cap, unique, 1, [5, 6] * (cap + 1)))
    for _ in range(3000):
        cap = int(rng.choice([1, 2, 3, 256]))
        n = int(rng.integers(0, 701))
        if rng.random() < 0.15:
            cases.append((cap, int(rng.integers(0, 2)), 0, list(range(n))))
        else:
            sw = rng.integers(0, int(rng.choice([1, 2, 3, 5, 40, 300, W])), n)
            if n and rng.random() < 0.5:                                            # runs of one walker
                sw = np.repeat(sw, rng.integers(1, 4, n))[:n]
            cases.append((cap, int(rng.integers(0, 2)), 1, [int(w) for w in sw]))
    text = "".join("%d %d %d %d %s\n" % (cap, u, l, len(sw), " ".join(map(str, sw))) for cap, u, l, sw in cases)
    want = [_split_rule(sw, bool(l), cap, bool(u)) for cap, u, l, sw in cases]
    assert any(len(b) < cap and a + len(b) < len(sw) for (cap, u, l, sw), ws in zip(cases, want) for a, b in ws)
    src = os.path.join(ROOT, "tests", "shim", "walker_split_check.cpp")
    inc = "-I" + os.path.join(ROOT, "pathintegralgroundstate_amd", "csrc")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("walker_split_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [inc, src, "-o", exe])
        out = subprocess.run([exe, str(W)], input=text, capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (name, out.returncode, out.stderr[-2000:])
        lines = out.stdout.split("\n")[:-1]
        assert len(lines) == len(cases)
        for (cap, u, l, sw), ws, line in zip(cases, want, lines):
            got = [[int(x) for x in part.split()] for part in line.split(";") if part.strip()]
            assert [(g[0], g[2:]) for g in got] == ws and all(g[1] == len(g) - 2 for g in got), (name, cap, u, l, sw)


def test_family_sizes_match_the_stated_rules(tmp_path):
    """csrc/pigs_family_sizes.h (the verdicts every pigs_*_init asks for) compiled for the CPU against the rules restated
    here, at their edges: the walkers a scratch budget holds one byte below, at and above k slots (k = 1, 2, 256, 257; W
    below and above the list's 256; less than one slot gives 1), the 2 GiB refusal at the last accepted and the first
    refused walker count (from exact integers: W x elements x 8 <= 2^31 is accepted) for 1, 3, 2^20 + 1 and 2^28
    elements per walker, a cut-off at the smallest half side of an unequal 1D..3D box, one ulp above it and at (1 + 4 eps)
    times it, without and with g3's tolerance, and nan, inf, 0 and a negative value, and the window and lag ranges at -1,
    0, the limit and the limit + 1.  Once as built, once under -fsanitize=address,undefined."""
    import math
    import subprocess
    eps = np.finfo(np.float64).eps
    cases, want = [], []
    for slot in (8, 24, 4096, 123457):
        for k in (1, 2, 256, 257):
            for budget in (k * slot - 1, k * slot, k * slot + 1):
                for W in (1, 3, 255, 256, 257, 1000):
                    cases.append("S %d 256 %d %d" % (W, budget, slot))
                    want.append(max(1, min(W, 256, budget // slot)))
        cases.append("S 64 256 %d %d" % (slot // 2, slot))
        want.append(1)
    assert {1, 2, 3, 255, 256} <= set(want) and 257 not in want
    for e in (1, 3, 2 ** 20 + 1, 2 ** 28):
        last = 2 ** 31 // (8 * e)                                   # the largest W with W e 8 <= 2^31
        assert last * e * 8 <= 2 ** 31 < (last + 1) * e * 8
        for W, refused in ((last, 0), (last + 1, 1), (1, 0), (2 * last + 1, 1)):
            cases.append("G %d %d" % (W, e))
            want.append(refused)
    for half in ((1.75,), (3.1, 2.3), (2.3, 3.1), (4.0, 5.5, 3.3), (3.3, 5.5, 4.0), (5.5, 3.3, 4.0), (0.1 * 3, 7.0, 7.0)):
        h = min(half)
        for tol in (0.0, 4.0 * eps):
            for r in (h, math.nextafter(h, math.inf), h * (1.0 + 4.0 * eps), 0.5 * h, 2.0 * h, math.nan, math.inf, 0.0, -h,
                      -math.inf):
                cases.append("C %d %s %s %s %s %s" % (len(half), *((float(x).hex() for x in (half + (1.0, 1.0))[:3])),
                                                      float(r).hex() if math.isfinite(r) else repr(r), float(tol).hex()))
                want.append(int(math.isfinite(r) and r > 0.0 and all(r <= x * (1.0 + tol) for x in half)))
            # at, one ulp above and 4 eps above the smallest half side: the tolerance decides the last two
            assert want[-10:-7] == ([1, 1, 1] if tol else [1, 0, 0]) and want[-7:] == [1, 0, 0, 0, 0, 0, 0]
    for Nb in (1, 3, 40):
        for window in (-1, 0, Nb, Nb + 1):
            cases.append("W %d %d" % (window, Nb))
            want.append(int(0 <= window <= Nb))
    for window in (0, 1, 7):
        for Ntau in (-1, 0, 2 * window, 2 * window + 1):
            cases.append("L %d %d" % (Ntau, window))
            want.append(int(0 <= Ntau <= 2 * window))
    src = os.path.join(ROOT, "tests", "shim", "family_sizes_check.cpp")
    inc = "-I" + os.path.join(ROOT, "pathintegralgroundstate_amd", "csrc")
    for name, flags in (("plain", ["-O2"]), ("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])):
        exe = str(tmp_path / ("family_sizes_" + name))
        subprocess.check_call(["g++", "-std=c++17", "-Wall"] + flags + [inc, src, "-o", exe])
        out = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (name, out.returncode, out.stderr[-2000:])
        got = [int(x) for x in out.stdout.split()]
        assert len(got) == len(cases)
        bad = [(c, w, g) for c, w, g in zip(cases, want, got) if w != g]
        assert not bad, (name, bad[:5])
