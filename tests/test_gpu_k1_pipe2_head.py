"""The head of K1's persistent kernel (pipe2, variant 12): a wave's static first record comes through the scalar unit,
the table image -- its odd last entry included -- goes to LDS by DMA behind it, and the first item's slice loads are
issued while the table chunks are still in flight.  Against the plain-grid twin (variant 13), bit for bit, where that
prologue can go wrong and the claim / edges tests do not reach:

  * table lengths that change a wave's chunk count.  nt = Nmax + 2 entries are staged as nt/2 16-byte pairs, 64 per wave
    and 1024 per round of the workgroup: nt/2 = 51 (only wave 0 stages anything; nt even and odd), exactly 1024 (even and
    odd nt: the odd entry sits right behind the last full chunk), 1025 (one pair into a second round), and an odd nt at
    nearly the default length.  Every value was accepted by SystemConfig, the oracle's System and both table builders;
  * a malformed static record in each field (walker, ip, ib; too high and negative), at a static item of wave 0 and of
    wave 15, through the staged entry (the batch entry rejects them on the host): NaN there, every other item keeps the
    bits of a clean run and of the twin;
  * a launch of exactly 16 CUs - 1 items forced to pipe2: one wave of the chip has no first item and must read nothing;
    the item arrays are device allocations of exactly n elements (made through the HIP runtime directly), so the record
    that wave must not read lies past the end of every one of them.

Np = 64, Nb = 4, 2 walkers as in test_gpu_k1_pipe2_claim.py, so a case takes a second or two.  The inputs' finite share
is checked against the CPU oracle without a GPU.
"""
import re
import subprocess

import numpy as np
import pytest

from helpers import same_bits

# Nmax: nt = Nmax + 2, pairs = nt // 2
NMAX = [100, 101, 2046, 2047, 2048, 9999]
CUS_MI355X = 256                                                   # for the oracle's check of the inputs
# a record's fields out of range, too high and negative (filled in with the system's sizes)
KINDS = [("w", "nW"), ("w", -1), ("ip", "Np+1"), ("ip", -3), ("ib", "M"), ("ib", -1)]


@pytest.fixture(scope="module")
def n_cu(gpu_lib):
    """CUs of the first GPU agent (rocminfo: read only)."""
    out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=120).stdout
    for agent in out.split("*******")[1:]:
        if re.search(r"Device Type:\s*GPU", agent):
            return int(re.search(r"Compute Unit:\s*(\d+)", agent).group(1))
    raise AssertionError("no GPU agent in rocminfo's output")


def _system(oracle, Nmax):
    from oracle.pyoracle import System
    from pathintegralgroundstate_amd import SystemConfig
    kw = dict(dim=3, Np=64, Nb=4, density=0.365, Nmax=Nmax)
    S, cfg = System(**kw), SystemConfig(**kw)
    VT, WF = oracle.tables(S)
    assert VT.size == Nmax + 2
    rng = np.random.default_rng(20)
    L = np.asarray(S.Lbox[:3])
    Ps = []
    for k in range(2):
        P, _ = oracle.init_path(S, 1982 + k)
        P = P + rng.normal(0, 0.1, P.shape)
        Ps.append(np.where(P > L / 2, P - L, np.where(P < -L / 2, P + L, P)))
    return S, cfg, VT, WF, np.stack(Ps)


@pytest.fixture(scope="module")
def systems(oracle):
    return {Nmax: _system(oracle, Nmax) for Nmax in NMAX + [10000]}


def _batch(S, Paths, n):
    rng = np.random.default_rng(7000 + n)
    w = rng.integers(0, Paths.shape[0], n).astype(np.int32)
    ip = rng.integers(1, S.Np + 1, n).astype(np.int32)
    ib = rng.integers(0, S.M, n).astype(np.int32)
    ib[::9] = 0                                                  # end, odd, even beads next to each other in every queue
    ib[4::9] = 2 * S.Nb
    ib[1::9] = 1
    ib[2::9] = 2
    xold = Paths[w, ib, ip - 1].copy()
    xnew = xold + rng.normal(0, 0.2, xold.shape)
    return w, ip, ib, xnew, xold


def _mismatches(a, b):
    return int(np.sum(a.view(np.uint64) != b.view(np.uint64)))


def _bad_places(wave, cus):
    """Six static items of one wave index, in six different workgroups (item = workgroup + wave * CUs)."""
    return np.array([wave * cus + (1 + 7 * g) % cus for g in range(6)])


def _bad_value(S, v):
    return {"nW": 2, "Np+1": S.Np + 1, "M": S.M}.get(v, v)


def test_inputs_keep_the_finite_share_above_one_half(oracle, systems):
    sizes = {Nmax: 17 * CUS_MI355X + 3 for Nmax in NMAX}
    sizes[10000] = 16 * CUS_MI355X - 1
    for Nmax, n in sizes.items():
        S, cfg, VT, WF, Paths = systems[Nmax]
        assert cfg.Nmax == Nmax and S.Nmax == Nmax
        w, ip, ib, xnew, xold = _batch(S, Paths, n)
        want = oracle.delta_action_batch(S, WF, VT, Paths, w, ip, ib, xnew, xold)
        print("Nmax", Nmax, "n", n, "finite", np.isfinite(want).mean())
        assert np.isfinite(want).mean() > 0.5, (Nmax, n, np.isfinite(want).mean())
    for wave in (0, 15):
        bad = _bad_places(wave, CUS_MI355X)
        assert len(set(bad.tolist())) == 6 and np.all(bad // CUS_MI355X == wave)


def _run(ctx, variant, entry, batch):
    ctx.set_tuning("k1_variant", variant)
    try:
        return getattr(ctx, entry)(*batch)
    finally:
        ctx.set_tuning("k1_variant", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("Nmax", NMAX)
def test_table_lengths_pipe2_equals_grid(gpu_lib, systems, n_cu, Nmax):
    S, cfg, VT, WF, Paths = systems[Nmax]
    n = 17 * n_cu + 3
    batch = _batch(S, Paths, n)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        ctx.upload_all(Paths)
        pipe2 = _run(ctx, 12, "delta_action_batch", batch)
        grid = _run(ctx, 13, "delta_action_batch", batch)
    print("Nmax", Nmax, "pairs", (Nmax + 2) // 2, "finite", np.isfinite(pipe2).mean(), "mismatches", _mismatches(pipe2, grid))
    assert same_bits(pipe2, grid), _mismatches(pipe2, grid)
    assert np.isfinite(pipe2).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("wave", [0, 15])
def test_malformed_static_records_give_nan_and_leave_neighbours_alone(gpu_lib, systems, n_cu, wave):
    S, cfg, VT, WF, Paths = systems[10000]
    n = 17 * n_cu + 3
    clean = _batch(S, Paths, n)
    w, ip, ib, xnew, xold = (a.copy() for a in clean)
    bad = _bad_places(wave, n_cu)
    for i, (field, v) in zip(bad, KINDS):
        {"w": w, "ip": ip, "ib": ib}[field][i] = _bad_value(S, v)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        ctx.upload_all(Paths)
        pipe2 = _run(ctx, 12, "delta_action_staged", (w, ip, ib, xnew, xold))
        grid = _run(ctx, 13, "delta_action_staged", (w, ip, ib, xnew, xold))
        ref = _run(ctx, 12, "delta_action_staged", clean)
    good = np.setdiff1d(np.arange(n), bad)
    print("wave", wave, "bad", bad, "finite", np.isfinite(ref[good]).mean(), "mismatches", _mismatches(pipe2[good], ref[good]))
    assert np.all(np.isnan(pipe2[bad]))
    assert np.isfinite(ref[good]).mean() > 0.5
    assert same_bits(pipe2[good], ref[good]), _mismatches(pipe2[good], ref[good])
    assert same_bits(pipe2, grid), _mismatches(pipe2, grid)


class _DeviceArrays:
    """Device allocations of exactly the arrays' sizes, through the HIP runtime the library itself is linked against
    (torch brings a runtime of its own, which finds no device once the library's has opened it)."""

    def __init__(self, arrays):
        import ctypes as C
        self.C, self.hip, self.ptrs = C, C.CDLL("libamdhip64.so"), []
        self.hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.hip.hipFree.argtypes = [C.c_void_p]
        for a in arrays:
            a = np.ascontiguousarray(a)
            p = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(p), a.nbytes) == 0
            self.ptrs.append(p)
            assert self.hip.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0          # host to device

    def download(self, k, like):
        out = np.empty_like(like)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptrs[k], out.nbytes, 2) == 0   # device to host
        return out

    def free(self):
        for p in self.ptrs:
            self.hip.hipFree(p)


@pytest.mark.gpu
def test_a_wave_without_a_first_item_reads_nothing(gpu_lib, systems, n_cu):
    S, cfg, VT, WF, Paths = systems[10000]
    n = 16 * n_cu - 1                                            # the last workgroup's wave 15 has no item
    batch = _batch(S, Paths, n)
    nan = np.full(n, np.nan)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        ctx.upload_all(Paths)
        d = _DeviceArrays(list(batch) + [nan, nan])              # exactly n (n * dim) elements each; two outputs
        try:
            outs = []
            for k, variant in enumerate((12, 13)):
                ctx.set_tuning("k1_variant", variant)
                try:
                    ctx.delta_action_batch_dev(n, *[p.value for p in d.ptrs[:5]], d.ptrs[5 + k].value)
                    ctx.sync()
                finally:
                    ctx.set_tuning("k1_variant", 0)
                outs.append(d.download(5 + k, nan))
        finally:
            d.free()
        host = _run(ctx, 13, "delta_action_batch", batch)
    pipe2, grid = outs
    print("n", n, "finite", np.isfinite(pipe2).mean(), "mismatches", _mismatches(pipe2, grid))
    assert same_bits(pipe2, grid), _mismatches(pipe2, grid)
    assert same_bits(pipe2, host), _mismatches(pipe2, host)
    assert np.isfinite(pipe2).mean() > 0.5
