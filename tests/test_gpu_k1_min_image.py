"""K1's pipe arithmetic after the magnitude minimum image (even and end beads: m = min(|v|, L - |v|)):

  * partners placed at the fold's edges (L/2 +- k ulp, L, 1.5 L, 2 L +- ulp, in either sign and on every axis) for
    even, end and odd beads: the persistent kernel (pipe2, a launch of at least 16 x CUs items) equals the plain-grid
    twin (variant 13) bit for bit, and both stay within delta_s_tolerance of the oracle (the reference's two-compare
    fold) with the oracle's NaN pattern -- a pair the two sides counted differently at the cutoff would not;
  * launches of exactly 16 x CUs, 16 x CUs + 1 and 32 x CUs - 1 items, where some waves of the persistent kernel have
    only their first item: every item equals the same item evaluated alone, bit for bit.
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


def _ulps(x, k):
    for _ in range(abs(k)):
        x = np.nextafter(x, np.inf if k > 0 else 0.0)
    return x


def _edge_offsets(L, dim):
    """Separation vectors (moved particle minus partner) at the fold's edges; the other axes keep r well above dr."""
    h = 0.5 * L
    one = []
    for k in (-3, -1, 0, 1, 3):
        one.append((_ulps(h, k), 0.0))                   # on the cutoff sphere when rcut = L/2
    for c, side in ((L, 0.3 * h), (1.5 * L, 0.0), (_ulps(2 * L, 1), 0.2 * h), (_ulps(2 * L, -1), 0.2 * h),
                    (_ulps(1.5 * L, 1), 0.0), (_ulps(L, -1), 0.5 * h), (0.7 * h, 0.0), (0.4 * h, 0.3 * h)):
        one.append((c, side))
    offs = []
    for axis in range(dim):
        for sign in (1.0, -1.0):
            for c, side in one:
                v = np.zeros(dim)
                v[axis] = sign * c
                if dim > 1:
                    v[(axis + 1) % dim] = side
                offs.append(v)
    return np.array(offs)


def _edge_system(oracle, dim, seed):
    from oracle.pyoracle import System
    from pathintegralgroundstate_amd import SystemConfig
    kw = dict(dim=dim, Np=len(_edge_offsets(1.0, dim)) + 1, Nb=6, density=0.05 if dim == 3 else 0.2, dt=0.01)
    S, cfg = System(**kw), SystemConfig(**kw)
    L = np.asarray(S.Lbox[:dim])
    assert np.all(L == L[0]) and S.rcut == 0.5 * L[0]
    offs = _edge_offsets(float(L[0]), dim)
    VT, WF = oracle.tables(S)
    rng = np.random.default_rng(seed)
    W = 2
    # particle 0 sits at the origin on every slice; partner j at -offs[j-1] (exact: the separation from the origin IS
    # the edge value); the other walker rolls the partners so that the edges sit on different rows
    Paths = np.zeros((W, S.M, S.Np, dim))
    Paths[0, :, 1:] = -offs[None]
    Paths[1, :, 1:] = -np.roll(offs, 5, axis=0)[None]
    return S, cfg, VT, WF, Paths, rng


@pytest.mark.parametrize("dim", [3, 2])
def test_partners_at_the_fold_edges_pipe2_equals_grid_and_the_oracle(gpu_lib, oracle, n_cu, dim):
    S, cfg, VT, WF, Paths, rng = _edge_system(oracle, dim, 11 + dim)
    L = np.asarray(S.Lbox[:dim])
    h = 0.5 * L
    n = 16 * n_cu + 37
    w = rng.integers(0, 2, n).astype(np.int32)
    ip = np.ones(n, np.int32)                                     # particle 0 (1-based) moves: separations are the edges
    ib = rng.integers(0, S.M, n).astype(np.int32)
    ib[::5] = 0                                                   # end beads, odd and even beads all present
    ib[2::5] = 2 * S.Nb
    xold = np.zeros((n, dim))
    # proposals: at the origin (old and new distances at the edges), shifted by whole / half boxes, or by a few ulps
    kind = rng.integers(0, 5, n)
    xnew = np.zeros((n, dim))
    xnew[kind == 1] = L
    xnew[kind == 2] = -h
    xnew[kind == 3] = rng.uniform(-0.3, 0.3, ((kind == 3).sum(), dim)) * L
    xnew[kind == 4] = np.array([_ulps(float(h[0]), 1)] + [0.0] * (dim - 1))
    xold[kind == 4] = np.array([_ulps(float(L[0]), -2)] + [0.0] * (dim - 1))
    assert {0, 2 * S.Nb} <= set(ib.tolist()) and (ib % 2 == 1).any() and ((ib % 2 == 0) & (ib != 0) & (ib != 2 * S.Nb)).any()
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=2) as ctx:
        ctx.upload_all(Paths)
        ctx.set_tuning("k1_variant", 12)
        pipe2 = ctx.delta_action_batch(w, ip, ib, xnew, xold)
        ctx.set_tuning("k1_variant", 13)
        grid = ctx.delta_action_batch(w, ip, ib, xnew, xold)
        ctx.set_tuning("k1_variant", 0)
        auto = ctx.delta_action_batch(w, ip, ib, xnew, xold)
    assert same_bits(pipe2, grid), int(np.sum(pipe2.view(np.uint64) != grid.view(np.uint64)))
    assert same_bits(auto, pipe2)
    sel = np.arange(0, n, 7)
    want = oracle.delta_action_batch(S, WF, VT, Paths, w[sel], ip[sel], ib[sel], xnew[sel], xold[sel])
    got = pipe2[sel]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want))
    fin = np.isfinite(want)
    assert fin.sum() > len(sel) // 2
    sv, sf, su = np.zeros(len(sel)), np.zeros(len(sel)), np.zeros(len(sel))
    for k in range(2):
        m = w[sel] == k
        sv[m], sf[m], su[m] = term_scales(S, VT, WF, Paths[k], ip[sel][m], ib[sel][m], xnew[sel][m], xold[sel][m])
    tol = delta_s_tolerance(S, sv, sf, su)
    err = np.abs(got - want)[fin]
    assert np.all(err <= tol[fin]), (err.max(), np.max(err / tol[fin]))


@pytest.mark.parametrize("extra", ["16cu", "16cu+1", "32cu-1"])
def test_waves_with_only_their_first_item_match_items_alone(gpu_lib, oracle, n_cu, extra):
    from oracle.pyoracle import System
    from pathintegralgroundstate_amd import SystemConfig
    n = {"16cu": 16 * n_cu, "16cu+1": 16 * n_cu + 1, "32cu-1": 32 * n_cu - 1}[extra]
    kw = dict(dim=3, Np=128, Nb=20, density=0.365)
    S, cfg = System(**kw), SystemConfig(**kw)
    VT, WF = oracle.tables(S)
    rng = np.random.default_rng(n)
    W = 3
    L = np.asarray(S.Lbox[:3])
    Ps = []
    for k in range(W):
        P, _ = oracle.init_path(S, 1982 + k)
        P = P + rng.normal(0, 0.1, P.shape)
        Ps.append(np.where(P > L / 2, P - L, np.where(P < -L / 2, P + L, P)))
    Paths = np.stack(Ps)
    w = rng.integers(0, W, n).astype(np.int32)
    ip = rng.integers(1, S.Np + 1, n).astype(np.int32)
    ib = rng.integers(0, S.M, n).astype(np.int32)
    ib[::9] = 0
    ib[4::9] = 2 * S.Nb
    xold = Paths[w, ib, ip - 1].copy()
    xnew = xold + rng.normal(0, 0.2, xold.shape)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(Paths)
        big = ctx.delta_action_batch(w, ip, ib, xnew, xold)               # the library's choice: pipe2 at this size
        ctx.set_tuning("k1_variant", 12)
        forced = ctx.delta_action_batch(w, ip, ib, xnew, xold)
        ctx.set_tuning("k1_variant", 0)
        # every item of the last workgroups' waves (the ones with a single item) and a sample of the rest, one at a time
        sel = np.unique(np.concatenate([np.arange(max(0, n - 2 * n_cu), n), np.arange(0, n, 13)]))
        alone = np.array([ctx.delta_action_batch(w[i:i + 1], ip[i:i + 1], ib[i:i + 1], xnew[i:i + 1], xold[i:i + 1])[0]
                          for i in sel])
    assert same_bits(big, forced)
    assert same_bits(big[sel], alone), int(np.sum(big[sel].view(np.uint64) != alone.view(np.uint64)))
    assert np.isfinite(big).mean() > 0.5
