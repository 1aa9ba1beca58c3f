"""K6, the device-resident sampler, at the walker counts bench.py runs it at -- against the reference, walker by walker.

pigs_sampler_init and pigs_sampler_step pick the kernel form from the walker count W and the device's CU count: the
8-wave sweep kernel (table image in LDS) while every walker has a CU of its own, the 4-wave one (three workgroups per
CU) beyond; TranslateChain by H = min(4, CUs / W) cooperating workgroups per walker (pigs_cm.hip), which poll each other
across CUs; at 128 walkers the overlapped estimators (diagonal_estimators_begin / _end) on a second stream capped at
half the chip.  The parity tests of test_gpu_sampler_size.py run one or two walkers, a form no benchmark leg uses.

The reference answers are tests/golden/vpi_runs/*_walkers/walkers.npz (tests/golden/make_golden.py: one reference run
per seed; row w = walker w of a run with the input's seed).  Every walker is held to what check_against_driver asks of
one: generator position and words (SHA-256), all 16 counters, BIT-identical final worldline, the diagonal steps' V, Et,
Kt to 1e-10 and E, K to MIXED_TOL; with the worm sector the event log, worm state and OBDM histogram.  Every test also
asserts the form it meant to run (pigs_sampler_form), computed from the device's CU count."""
import gc
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from helpers import MIXED_TOL, block_energy_errors, driver_blocks, read_hex_blocks, sha256_of, walker_row, \
    walker_summed_structure
from test_gpu_sampler_size import _cfg, check_against_driver, run_k6

pytestmark = pytest.mark.gpu
RUNS = os.path.join(GOLDEN, "vpi_runs")
HOST = os.path.join(ROOT, "pathintegralgroundstate_amd", "host")
C3, C5 = "c3_n256_walkers", "c5_n256_dipolar_walkers"
_W = {}


def _walkers(name):
    if name not in _W:
        _W[name] = dict(np.load(os.path.join(RUNS, name, "walkers.npz")))
    return _W[name]


@pytest.fixture(scope="module")
def n_cu(gpu_lib):
    """CUs of the first GPU agent (rocminfo: read only)."""
    out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=120).stdout
    for agent in out.split("*******")[1:]:
        if re.search(r"Device Type:\s*GPU", agent):
            return int(re.search(r"Compute Unit:\s*(\d+)", agent).group(1))
    raise AssertionError("no GPU agent in rocminfo's output")


def expected_form(n_cu, W, cm_fits_one=True):
    """(sweep threads, H) that pigs_sampler_init / pigs_sampler_step pick for W walkers of a periodic input with even
    Nmax whose 8-wave form fits LDS: 512 threads up to one walker per CU, 256 beyond; H = CUs / W in 1..4 (0 where one
    workgroup per walker does not hold the worldline: 321 beads)."""
    H = min(4, max(1, n_cu // W))
    return (512 if W <= n_cu else 256), (H if H > 1 or cm_fits_one else 0)


def _run_and_check(gpu_lib, oracle, name, W, **kw):
    gc.collect()                                    # no other live context: it would lower H to 1 (pigs_capi.hip)
    rows = [walker_row(_walkers(name), w) for w in range(W)]
    r = run_k6(gpu_lib, oracle, [name], rows=rows, **kw)
    worst_rel = 0.0
    for w in range(W):
        try:
            _, rel = check_against_driver(r, w)
        except AssertionError as e:
            raise AssertionError(f"walker {w} of {W} (seed {rows[w]['seed']}): {e}") from e
        worst_rel = max(worst_rel, rel)
    return r, worst_rel


@pytest.mark.parametrize("W", [64, 128, 256, "n_cu+1", 1024])
def test_k6_config3_every_walker_at_benchmarked_occupancy(gpu_lib, oracle, n_cu, W):
    """C3 (N=256, 161 beads, 3 MC steps), default tuning.  At 128 walkers, bench.py's headline, the steps' energies come
    through the overlapped estimators queued behind the next step, and their g(r), S(k) summed over walkers and steps
    are held to the reference's sums."""
    W = n_cu + 1 if W == "n_cu+1" else W
    overlap = W == 128
    r, rel = _run_and_check(gpu_lib, oracle, C3, W, overlap=overlap)
    f = r["form"]
    threads, H = expected_form(n_cu, W)
    print(f"W={W} on {n_cu} CUs: form {f}; step energies max rel {rel:.2e}")
    assert (f["sweep_threads"], f["cm_H"], f["stage_machine"], f["cm_shared"]) == (threads, H, False, False), f
    if overlap:
        Wz = _walkers(C3)
        assert int(Wz["n_summed"]) == W
        gr, sk = Wz["gr_total"], Wz["sk_total"]
        assert np.all(np.abs(r["gr_sum"] - gr) <= 1e-9 * np.abs(gr)), np.max(np.abs(r["gr_sum"] - gr))
        assert np.all(np.abs(r["sk_sum"] - sk) <= 1e-8 * np.abs(sk)), np.max(np.abs(r["sk_sum"] - sk) / np.abs(sk))


def test_k6_config5_dipolar_every_walker_at_128(gpu_lib, oracle, n_cu):
    """C5 with the dipolar table (321 beads, worm sector, swaps, Npw = 2 OBDM), 128 walkers, default tuning: every
    walker's event log, worm state and OBDM histogram too.  TranslateChain by cooperating workgroups (321 beads do not
    fit one); the sweep kernel in the form the same input takes at one walker."""
    W = 128
    r, rel = _run_and_check(gpu_lib, oracle, C5, W)
    assert r["counters"][:, 5].sum() >= 1 and r["counters"][:, 13].sum() >= 1       # opens and swaps were accepted
    f = r["form"]
    threads, H = expected_form(n_cu, W, cm_fits_one=False)
    # the sweep form of 321 beads does not depend on W while W <= CUs: what a one-walker context of the input gets
    cfg = _cfg(C5)
    VT, WF = gpu_lib.build_tables(cfg, str(_walkers(C5)["potential"]))
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as one:
        one.sampler_init(CWorm=cfg.CWorm, swapping=cfg.swapping, Nobdm=cfg.Nobdm, Nbin=cfg.Nbin, Npw=cfg.Npw,
                         sampling=cfg.sampling)
        threads = one.sampler_form()["sweep_threads"]
    print(f"W={W} on {n_cu} CUs: form {f}; step energies max rel {rel:.2e}")
    assert threads in (256, 512)
    assert (f["sweep_threads"], f["cm_H"], f["stage_machine"], f["cm_shared"]) == (threads, H, False, False), f
    assert H >= 2


# ---- the front end at 128 walkers (bench.py's mc leg and its two-shard form) -------------------------------------------
@pytest.fixture(scope="module")
def exe(gpu_lib):
    subprocess.check_call(["make", "-s", "-C", HOST])
    return os.path.join(HOST, "pigs_vpi")


def _hex_rows_close(hexfile, drv, rel=1e-10, mixed=MIXED_TOL):
    blocks, rows = read_hex_blocks(hexfile)
    wb, wrows = driver_blocks(drv)
    assert np.array_equal(blocks, wb), (blocks, wb)
    em, er = block_energy_errors(rows, wrows)
    assert np.all(er <= rel), er.max()
    assert np.all(em <= mixed), em.max()


@pytest.mark.parametrize("n_gpus", [1, 2])
def test_front_end_config3_128_walkers_device_sampler(gpu_lib, exe, n_cu, n_gpus, tmp_path):
    """pigs_vpi, C3 with n_walkers = 128, device_sampler = T: one context (H = CUs / 128), or two shards of 64 walkers on
    this one device (n_gpus = 2, same_device = T: pigs_comm_init_all's shared TranslateChain, H = (CUs - 64) / 64).
    Every walker's final worldline (SHA-256) and block energies (e_vpi.wNNNN.hex); the walker-summed gr_vpi.out to 1e-9
    and sk_vpi.out to 1e-8 (device sin / cos are not libm's) against the reference's sums."""
    W = 128
    Wz = _walkers(C3)
    cfg = _cfg(C3)
    gpu = f" n_walkers = {W}, device = 0, device_sampler = T, checkpointing = F"
    if n_gpus == 2:
        gpu += ", n_gpus = 2, same_device = T"
    with open(tmp_path / "vpi.in", "w") as f:
        f.write(open(os.path.join(RUNS, C3, "vpi.in")).read() + f"&gpu\n{gpu}\n/\n")
    with open(tmp_path / "vpi.in") as fin, open(tmp_path / "stdout.txt", "w") as fo:
        p = subprocess.run([exe], stdin=fin, stdout=fo, stderr=subprocess.STDOUT, cwd=tmp_path, timeout=600)
    out = open(tmp_path / "stdout.txt").read()
    assert p.returncode == 0, out[-3000:]
    m = re.search(r"sampler form: sweep threads\s*(\d+), TranslateChain workgroups per walker\s*(-?\d+), "
                  r"stage machine\s*([TF]), shared\s*([TF])", out)
    assert m, out[-3000:]
    form = (int(m.group(1)), int(m.group(2)), m.group(3) == "T", m.group(4) == "T")
    shard = W // n_gpus
    H = min(4, n_cu // W) if n_gpus == 1 else min(4, (n_cu - shard) // shard)
    print(f"front end, {n_gpus} shard(s) of {shard} walkers on {n_cu} CUs: form {form}")
    assert form == (512, H, False, n_gpus == 2), form
    assert H >= 2
    shape = tuple(int(x) for x in Wz["Path_shape"])
    got = np.fromfile(tmp_path / "worldlines_final.bin").reshape((W,) + shape)
    for w in range(W):
        row = walker_row(Wz, w)
        assert np.array_equal(sha256_of(got[w]), row["Path_sha256"]), f"walker {w}: final worldline differs"
        try:
            _hex_rows_close(tmp_path / f"e_vpi.w{w:04d}.hex", row)
        except AssertionError as e:
            raise AssertionError(f"walker {w}: {e}") from e
    ngr = int(Wz["steps"][0, :, 0].sum())                  # diagonal steps per walker (CWorm = 0: every step)
    gr, sk = walker_summed_structure(cfg, Wz["gr_total"], Wz["sk_total"], W, ngr)
    a = np.loadtxt(tmp_path / "gr_vpi.out")
    assert np.all(np.abs(a[:, 1] - gr) <= 1e-9 * np.abs(gr) + 1.01e-9 * np.abs(gr)), np.max(np.abs(a[:, 1] - gr))
    b = np.loadtxt(tmp_path / "sk_vpi.out")[:, 1::3]       # (q, S, error) for every direction
    assert np.all(np.abs(b - sk) <= 1e-8 * np.abs(sk) + 1.01e-9 * np.abs(sk)), np.max(np.abs(b - sk))
