"""K1's persistent kernel (pipe2, variant 12) and its item queue with the one-item claim-ahead: only a wave's first item
is static (k = wave), every further one is drawn from the workgroup's LDS counter at the top of the item before it, and a
draw past the end requests an empty record.  Forced at every launch size where that hand-over changes shape, against the
plain-grid twin (variant 13), which evaluates every item on its own with the same arithmetic, bit for bit:

  * 1, 15, 17 items: one or two workgroups, waves without any item, a wave whose static item is its only one;
  * 16 CUs: every wave gets exactly its static item, and the queue is drawn 16 times but empty;
  * 16 CUs + 1, 17 CUs: one wave of one / of every workgroup gets a second item;
  * 32 CUs + 1, 33 CUs + 7: two and three rounds, the last one partial.

Malformed records go through the staged entry (the batch entry rejects them on the host): a workgroup's first static item,
the very last item of the launch, and two consecutive queue positions of one workgroup each give NaN, and every other
item keeps the bits of a clean run.  The same claim / request / slice helpers serve both paths in the kernel.

Np = 64, Nb = 4, 2 walkers as in test_gpu_k1_pipe2_edges.py's smallest system, so a case takes a second or two; the bead
index cycles through end, odd and even beads.  The inputs' finite share is checked against the CPU oracle without a GPU.
"""
import re
import subprocess

import numpy as np
import pytest

from helpers import same_bits

# n = a * CUs + c
SIZES = [(0, 1), (0, 15), (0, 17), (16, 0), (16, 1), (17, 0), (32, 1), (33, 7)]
MALFORMED_AT = (33, 7)
CUS_MI355X = 256                                                   # for the oracle's check of the inputs


@pytest.fixture(scope="module")
def n_cu(gpu_lib):
    """CUs of the first GPU agent (rocminfo: read only)."""
    out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=120).stdout
    for agent in out.split("*******")[1:]:
        if re.search(r"Device Type:\s*GPU", agent):
            return int(re.search(r"Compute Unit:\s*(\d+)", agent).group(1))
    raise AssertionError("no GPU agent in rocminfo's output")


@pytest.fixture(scope="module")
def system(oracle):
    from oracle.pyoracle import System
    from pathintegralgroundstate_amd import SystemConfig
    kw = dict(dim=3, Np=64, Nb=4, density=0.365)
    S, cfg = System(**kw), SystemConfig(**kw)
    VT, WF = oracle.tables(S)
    rng = np.random.default_rng(20)
    L = np.asarray(S.Lbox[:3])
    Ps = []
    for k in range(2):
        P, _ = oracle.init_path(S, 1982 + k)
        P = P + rng.normal(0, 0.1, P.shape)
        Ps.append(np.where(P > L / 2, P - L, np.where(P < -L / 2, P + L, P)))
    return S, cfg, VT, WF, np.stack(Ps)


def _batch(S, Paths, n):
    rng = np.random.default_rng(1000 + n)
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


def _n(a, c, cus):
    return a * cus + c


def _bad_places(place, n, cus):
    if place == "first_static":
        return [min(5, cus - 1)]                                 # index < CUs: wave 0's static item of that workgroup
    if place == "last":
        return [n - 1]
    i = 16 * cus + 3                                             # queue positions 16 and 17 of workgroup 3
    return [i, i + cus]


def _mismatches(a, b):
    return int(np.sum(a.view(np.uint64) != b.view(np.uint64)))


def test_inputs_keep_the_finite_share_above_one_half(oracle, system):
    S, cfg, VT, WF, Paths = system
    for a, c in SIZES:
        n = _n(a, c, CUS_MI355X)
        w, ip, ib, xnew, xold = _batch(S, Paths, n)
        want = oracle.delta_action_batch(S, WF, VT, Paths, w, ip, ib, xnew, xold)
        assert np.isfinite(want).mean() > 0.5, (n, np.isfinite(want).mean())
        if n >= 9:
            assert {0, 1, 2, 2 * S.Nb} <= set(ib[:9].tolist())       # end, odd and even beads follow each other


@pytest.fixture(scope="module")
def ctx(gpu_lib, system):
    S, cfg, VT, WF, Paths = system
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as c:
        c.upload_all(Paths)
        yield c


def _run(ctx, variant, entry, batch):
    ctx.set_tuning("k1_variant", variant)
    try:
        return getattr(ctx, entry)(*batch)
    finally:
        ctx.set_tuning("k1_variant", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=["%dcu%+d" % s for s in SIZES])
def test_launch_sizes_pipe2_equals_grid(ctx, system, n_cu, size):
    S, cfg, VT, WF, Paths = system
    n = _n(*size, n_cu)
    batch = _batch(S, Paths, n)
    pipe2 = _run(ctx, 12, "delta_action_batch", batch)
    grid = _run(ctx, 13, "delta_action_batch", batch)
    print("n", n, "finite", np.isfinite(pipe2).mean(), "mismatches", _mismatches(pipe2, grid))
    assert same_bits(pipe2, grid), _mismatches(pipe2, grid)
    assert np.isfinite(pipe2).mean() > 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("place", ["first_static", "last", "two_consecutive_draws"])
def test_malformed_records_give_nan_and_leave_neighbours_alone(ctx, system, n_cu, place):
    S, cfg, VT, WF, Paths = system
    n = _n(*MALFORMED_AT, n_cu)
    clean = _batch(S, Paths, n)
    w, ip, ib, xnew, xold = (a.copy() for a in clean)
    bad = np.array(_bad_places(place, n, n_cu))
    kinds = {"first_static": [("ip", 0)], "last": [("ib", S.M)], "two_consecutive_draws": [("w", 2), ("ip", S.Np + 1)]}[place]
    for i, (field, v) in zip(bad, kinds):
        {"w": w, "ip": ip, "ib": ib}[field][i] = v
    pipe2 = _run(ctx, 12, "delta_action_staged", (w, ip, ib, xnew, xold))
    grid = _run(ctx, 13, "delta_action_staged", (w, ip, ib, xnew, xold))
    ref = _run(ctx, 12, "delta_action_staged", clean)
    good = np.setdiff1d(np.arange(n), bad)
    print("n", n, "bad", bad, "finite", np.isfinite(ref[good]).mean(), "mismatches", _mismatches(pipe2[good], ref[good]))
    assert np.all(np.isnan(pipe2[bad]))
    assert np.isfinite(ref[good]).mean() > 0.5
    assert same_bits(pipe2[good], ref[good]), _mismatches(pipe2[good], ref[good])
    assert same_bits(pipe2, grid), _mismatches(pipe2, grid)
