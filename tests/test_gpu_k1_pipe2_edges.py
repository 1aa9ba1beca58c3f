"""K1's persistent kernel (pipe2, variant 12) at the edges of its addressing and item queue, at pipe2 sizes (at least
16 items per CU unless a test says otherwise), against the plain-grid twin (variant 13), which evaluates every item on
its own with the same arithmetic:

  * launch sizes whose per-workgroup item count is not a multiple of 16, with waves that get 0, 1, 2 or 3 items;
  * Np = 130: NpPad = 136, so pass 2 is partly and pass 3 wholly beyond the padded rows, and the lanes there must get
    finite data without reading past a coordinate row (the last slice of the allocation among them);
  * malformed records in the middle of the queue give NaN and leave their neighbours' bits alone;
  * the moved particle's own row holds 1e300 (read as data it would give NaN) at a pipe2-sized launch.
"""
import re
import subprocess

import numpy as np
import pytest

from helpers import delta_s_tolerance, same_bits, term_scales

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def n_cu(gpu_lib):
    """CUs of the first GPU agent (rocminfo: read only)."""
    out = subprocess.run(["rocminfo"], capture_output=True, text=True, timeout=120).stdout
    for agent in out.split("*******")[1:]:
        if re.search(r"Device Type:\s*GPU", agent):
            return int(re.search(r"Compute Unit:\s*(\d+)", agent).group(1))
    raise AssertionError("no GPU agent in rocminfo's output")


def _system(oracle, Np, Nb, W, seed, density=0.365):
    from oracle.pyoracle import System
    from pathintegralgroundstate_amd import SystemConfig
    kw = dict(dim=3, Np=Np, Nb=Nb, density=density)
    S, cfg = System(**kw), SystemConfig(**kw)
    VT, WF = oracle.tables(S)
    rng = np.random.default_rng(seed)
    L = np.asarray(S.Lbox[:3])
    Ps = []
    for k in range(W):
        P, _ = oracle.init_path(S, 1982 + k)
        P = P + rng.normal(0, 0.1, P.shape)
        Ps.append(np.where(P > L / 2, P - L, np.where(P < -L / 2, P + L, P)))
    return S, cfg, VT, WF, np.stack(Ps), rng


def _batch(rng, S, Paths, n):
    W = Paths.shape[0]
    w = rng.integers(0, W, n).astype(np.int32)
    ip = rng.integers(1, S.Np + 1, n).astype(np.int32)
    ib = rng.integers(0, S.M, n).astype(np.int32)
    ib[::9] = 0
    ib[4::9] = 2 * S.Nb
    xold = Paths[w, ib, ip - 1].copy()
    xnew = xold + rng.normal(0, 0.2, xold.shape)
    return w, ip, ib, xnew, xold


def _variants(ctx, *batch):
    ctx.set_tuning("k1_variant", 12)
    pipe2 = ctx.delta_action_batch(*batch)
    ctx.set_tuning("k1_variant", 13)
    grid = ctx.delta_action_batch(*batch)
    ctx.set_tuning("k1_variant", 0)
    return pipe2, grid


def _mismatches(a, b):
    return int(np.sum(a.view(np.uint64) != b.view(np.uint64)))


@pytest.mark.parametrize("per_cu", [(9, 5), (17, 3), (37, 11), (48, -1)])
def test_queue_sizes_pipe2_equals_grid(gpu_lib, oracle, n_cu, per_cu):
    # n = a * CUs + c: workgroups of a or a + 1 items -- 9/10 (waves with 0 items), 17/18 (1 or 2), 37/38 (2 or 3),
    # 47/48 (the last workgroups one short of three full rounds)
    a, c = per_cu
    n = a * n_cu + c
    S, cfg, VT, WF, Paths, rng = _system(oracle, 128, 20, 3, n)
    batch = _batch(rng, S, Paths, n)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=3) as ctx:
        ctx.upload_all(Paths)
        pipe2, grid = _variants(ctx, *batch)
    assert same_bits(pipe2, grid), _mismatches(pipe2, grid)
    assert np.isfinite(pipe2).mean() > 0.5


def test_np130_padded_passes_pipe2_equals_grid_and_the_oracle(gpu_lib, oracle, n_cu):
    S, cfg, VT, WF, Paths, rng = _system(oracle, 130, 12, 2, 130)
    assert cfg.dim == 3
    n = 20 * n_cu + 3
    w, ip, ib, xnew, xold = _batch(rng, S, Paths, n)
    # the last slice of the allocation (walker 1, bead M - 1) and the highest rows as moved particles
    w[-40:] = 1
    ib[-40:] = S.M - 1
    ip[-20:] = np.arange(S.Np - 19, S.Np + 1)
    xold = Paths[w, ib, ip - 1].copy()
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        ctx.upload_all(Paths)
        pipe2, grid = _variants(ctx, w, ip, ib, xnew, xold)
    assert same_bits(pipe2, grid), _mismatches(pipe2, grid)
    sel = np.concatenate([np.arange(0, n, 97), np.arange(n - 40, n)])
    want = oracle.delta_action_batch(S, WF, VT, Paths, w[sel], ip[sel], ib[sel], xnew[sel], xold[sel])
    got = pipe2[sel]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    assert fin.mean() > 0.5
    sv, sf, su = np.zeros(len(sel)), np.zeros(len(sel)), np.zeros(len(sel))
    for k in range(2):
        m = w[sel] == k
        sv[m], sf[m], su[m] = term_scales(S, VT, WF, Paths[k], ip[sel][m], ib[sel][m], xnew[sel][m], xold[sel][m])
    tol = delta_s_tolerance(S, sv, sf, su)
    err = np.abs(got - want)[fin]
    assert np.all(err <= tol[fin]), (err.max(), np.max(err / tol[fin]))


def _staged(ctx, variant, *batch):
    """The staged entry (the batch entry rejects malformed records on the host before any launch; the staged one
    range-checks them in the kernel)."""
    ctx.set_tuning("k1_variant", variant)
    out = ctx.delta_action_staged(*batch)
    ctx.set_tuning("k1_variant", 0)
    return out


def test_malformed_items_mid_queue_give_nan_and_leave_neighbours_alone(gpu_lib, oracle, n_cu):
    S, cfg, VT, WF, Paths, rng = _system(oracle, 128, 20, 3, 7)
    n = 24 * n_cu + 5
    clean = _batch(rng, S, Paths, n)
    w, ip, ib, xnew, xold = (a.copy() for a in clean)
    bad = np.arange(n // 3, n, n // 11)[:10]                     # inside the queues, past the static first items
    kinds = [("w", 3), ("w", -1), ("ip", 0), ("ip", S.Np + 1), ("ib", S.M), ("ib", -1)]
    for i, (field, v) in zip(bad, kinds * 2):
        {"w": w, "ip": ip, "ib": ib}[field][i] = v
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=3) as ctx:
        ctx.upload_all(Paths)
        pipe2 = _staged(ctx, 12, w, ip, ib, xnew, xold)
        grid = _staged(ctx, 13, w, ip, ib, xnew, xold)
        ref = _staged(ctx, 12, *clean)
    assert np.all(np.isnan(pipe2[bad]))
    good = np.setdiff1d(np.arange(n), bad)
    assert np.isfinite(ref[good]).mean() > 0.5
    assert same_bits(pipe2[good], ref[good]), _mismatches(pipe2[good], ref[good])
    assert same_bits(pipe2, grid), _mismatches(pipe2, grid)


def test_moved_particles_row_is_never_read_at_pipe2_size(gpu_lib, oracle, n_cu):
    # one item per (walker, bead) slice, so that 1e300 in one item's own row is no other item's partner
    W = 128
    S, cfg, VT, WF, Paths, rng = _system(oracle, 64, 20, W, 3)
    n = 16 * n_cu + 9
    assert n <= W * S.M
    slot = rng.permutation(W * S.M)[:n]
    w, ib = (slot // S.M).astype(np.int32), (slot % S.M).astype(np.int32)
    ip = rng.integers(1, S.Np + 1, n).astype(np.int32)
    ip[:64] = np.arange(1, 65)                                   # every lane of pass 0 as the moved particle
    xold = Paths[w, ib, ip - 1].copy()
    xnew = xold + rng.normal(0, 0.2, xold.shape)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(Paths)
        ctx.set_tuning("k1_variant", 12)
        a = ctx.delta_action_batch(w, ip, ib, xnew, xold)
        ctx.commit_beads(w, ip, ib, np.full((n, 3), 1e300))
        b = ctx.delta_action_batch(w, ip, ib, xnew, xold)
        ctx.set_tuning("k1_variant", 13)
        g = ctx.delta_action_batch(w, ip, ib, xnew, xold)
        ctx.set_tuning("k1_variant", 0)
    assert np.isfinite(a).mean() > 0.5
    assert same_bits(a, b), _mismatches(a, b)
    assert same_bits(b, g), _mismatches(b, g)
