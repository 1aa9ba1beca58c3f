"""pigs_sf_* on the MI355X where tests/test_gpu_sf.py does not reach (pigs_sf.hip), through the C ABI:

  A. windows of more than kSfChunk = 32 links, where k_sf_links takes its chunk loop more than once: the wave sums of a
     chunk wait in LDS between two barriers, W_k is carried from chunk to chunk in a register, red[] is indexed by the
     link's place in the chunk and the scratch by its place in the window; with the register form (Np <= 256) and the
     form that reads its own U back (Np > 256);
  B. 0 < Ntau < 2 window, where k_sf_lags' decode of (slot, lag) from the block index and the stride Ntau + 1 of the
     accumulators differ from the two cases Ntau = 0 and Ntau = 2 window;
  C. a scratch that holds fewer walkers than are listed TOGETHER WITH walkers listed twice, down to one slot per launch:
     slot != walker, and the scratch of a slot is taken over by another walker in the next launch.

The expected sums come from tests/sf_numpy.py and the comparison is test_gpu_sf.py's _assert_same: nwrap and samples
equal, C with the restatement's bits, D within 1e-12 of the expected value per element, nothing masked.  What a case is
there for -- links beyond the first chunk that fold, a centre of mass that moves across the chunk's edge, a slot larger
than the budget -- is asserted on the expectation before the device is asked.

Largest |got - want| / bound of D seen on the MI355X: see DESIGN.md (the superfluid section)."""
import numpy as np
import pytest

import sf_numpy as sn
from helpers import same_bits
from test_gpu_sf import _assert_same, _cfg, _dyadic, _same
from test_host_logic import _split_rule

pytestmark = pytest.mark.gpu
CHUNK = 32                      # kSfChunk of pigs_sf.hip
LANES = 256                     # kSfThreads


def _single(ctx, Ntau, window, walkers=None):
    ctx.sf_init(Ntau, window)
    ctx.sf_accumulate(walkers)
    got = ctx.sf_read()
    assert got["window"] == window
    return got


# ---- A. windows longer than one chunk -----------------------------------------------------------------------------------
@pytest.mark.parametrize("Np", [3, 65, 256, 257])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_windows_around_and_beyond_one_chunk(gpu_lib, dim, Np):
    """Nb = 33, two walkers, one context; the windows 15 (30 links: under one chunk), 16 (32: exactly one), 17 (34: a second
    chunk of 2), 32 (64: two full chunks) and 33 (66: two full chunks and 2), every lag of each.  Windows below Nb begin
    off slice 0.  Np = 3: one partly filled wave; 65: two waves; 256: the last shape that keeps U in registers; 257: the
    first that reads it back."""
    Nb, W = 33, 2
    cfg = _cfg(dim, Np, Nb)
    L = cfg.Lbox[:dim]
    P = sn.random_walk(W, 2 * Nb + 1, Np, L, np.random.default_rng(1000 * dim + Np), 0.04)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        for window in (15, 16, 17, 32, 33):
            Ntau, links = 2 * window, 2 * window
            exp = sn.Window(P, Nb, window, L, Ntau).expected(range(W))
            assert exp["nwrap"].sum() > 0
            assert (links > CHUNK) == (window >= 17)
            if links > CHUNK:                                           # the second chunk matters, by the reference alone
                late, moved = 0, np.zeros(dim, bool)
                for w in range(W):
                    X = P[w, Nb - window:Nb + window + 1]
                    late += sn.fold(X[CHUNK + 1:] - X[CHUNK:-1], L)[1]
                    Wc = sn.unfold(X, L)[2]
                    moved |= Wc[CHUNK + 1] != Wc[CHUNK]
                assert late >= 1, "no link beyond the first chunk folds"
                assert moved.all(), "W stands still across the chunk's edge on some axis"
            got = _single(ctx, Ntau, window)
            _assert_same(got, exp, f"A dim {dim} Np {Np} window {window}")
            assert not np.any(got["C"][:, 0]) and not np.any(got["D"][:, 0]) and np.all(got["D"][:, 1:] > 0)
            assert got["samples"].tolist() == [1] * W


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_rigid_drift_over_two_chunks_is_exact(gpu_lib, dim):
    """The rigid drift of test_unfolding_beyond_half_the_box (dyadic sides, the 2^-16 grid, c = round(0.3 L 64) / 64 per
    link) over Nb = window = 17: 34 links, 35 lags, Np = 65.  Every term is a multiple of 2^-12 and every sum stays below
    2^53 of them, so C and D equal the closed form bit for bit, in the second chunk as in the first."""
    Np, Nb = 65, 17
    cfg = _dyadic(dim, Np, Nb)
    L = np.asarray(cfg.Lbox[:dim])
    c = np.round(0.3 * L * 64.0) / 64.0
    ns, Ntau = 2 * Nb + 1, 2 * Nb
    assert Ntau > CHUNK and np.all(2 * c > 0.5 * L) and np.all(c < 0.5 * L) and np.all(Ntau * c > 2 * L)
    c64 = [int(x) for x in c * 64.0]
    assert np.array_equal(np.asarray(c64) / 64.0, c)
    for k in range(dim):                                                # in units of 2^-12: integers, and the largest sums
        assert ns * (Np * Ntau * c64[k]) ** 2 < 2 ** 53 and Np * ns * (Ntau * c64[k]) ** 2 < 2 ** 53
    P = sn.drift(Np, ns, L, c, np.ones(Np), np.random.default_rng(dim))
    lags = np.arange(Ntau + 1.0)
    npairs = ns - lags
    wantC = npairs[:, None] * (Np * lags[:, None] * c) ** 2
    wantD = Np * npairs[:, None] * (lags[:, None] * c) ** 2
    for l in range(Ntau + 1):                                           # the closed form itself is exact: against integers
        for k in range(dim):
            assert wantC[l, k] * 4096.0 == (ns - l) * (Np * l * c64[k]) ** 2 and wantD[l, k] * 4096.0 == Np * (ns - l) * (l * c64[k]) ** 2
    exp = sn.Window(P, Nb, Nb, L, Ntau).expected([0])
    assert same_bits(exp["C"][0], wantC) and same_bits(exp["D"][0], wantD)
    X = P[0]
    assert sn.fold(X[CHUNK + 1:] - X[CHUNK:-1], L)[1] >= 1, "no link beyond the first chunk folds"
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=1) as ctx:
        ctx.upload_all(P)
        got = _single(ctx, Ntau, Nb)
    assert same_bits(got["C"][0], wantC), np.flatnonzero((got["C"][0] != wantC).any(axis=1))
    assert same_bits(got["D"][0], wantD), np.flatnonzero((got["D"][0] != wantD).any(axis=1))
    assert got["nwrap"].tolist() == exp["nwrap"].tolist() and got["samples"].tolist() == [1]


LONG_NP, LONG_NB, LONG_W = 1077, 20, 3


@pytest.fixture(scope="module")
def long_system(gpu_lib):
    """Np = 1077 in 3D (five particle rounds of the read-back form), Nb = window = 20 (40 links: two chunks), three walkers:
    one context for the long case of A and for C2."""
    cfg = _cfg(3, LONG_NP, LONG_NB)
    P = sn.random_walk(LONG_W, 2 * LONG_NB + 1, LONG_NP, cfg.Lbox, np.random.default_rng(1077020), 0.04)
    ref = sn.Window(P, LONG_NB, LONG_NB, cfg.Lbox, LONG_NB)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=LONG_W) as ctx:
        ctx.upload_all(P)
        yield dict(cfg=cfg, P=P, ref=ref, ctx=ctx)


def test_read_back_form_over_two_chunks_and_five_rounds(long_system):
    """window 20 with Ntau 20: the shape that DESIGN.md measures.  Np = 1077 > 256: every thread reads back the U that it
    wrote for the link before, over five rounds of particles and across the chunk's edge."""
    s = long_system
    cfg, P, ctx = s["cfg"], s["P"], s["ctx"]
    assert -(-LONG_NP // LANES) == 5 and 2 * LONG_NB > CHUNK
    exp = s["ref"].expected(range(LONG_W))
    late = sum(sn.fold(P[w, CHUNK + 1:] - P[w, CHUNK:-1], cfg.Lbox)[1] for w in range(LONG_W))
    moved = np.any([s["ref"].Wcm[w][CHUNK + 1] != s["ref"].Wcm[w][CHUNK] for w in range(LONG_W)], axis=0)
    assert late >= 1 and moved.all()
    ctx.set_tuning("sf_scratch_mib", 256)                               # the default, whatever ran before on this context
    got = _single(ctx, LONG_NB, LONG_NB)
    _assert_same(got, exp, "A Np 1077 window 20 Ntau 20")
    assert np.all(got["D"][:, 1:] > 0) and np.all(got["C"][:, 1:] > 0)


# ---- B. lags between 0 and 2 window -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,Np,Nb,window,Ntau", [(3, 65, 3, 3, 1), (3, 65, 3, 3, 3), (3, 65, 3, 3, 5), (3, 65, 3, 2, 1),
                                                   (2, 257, 17, 17, 17)])
def test_lags_between_none_and_all(gpu_lib, dim, Np, Nb, window, Ntau):
    """0 < Ntau < 2 window on three walkers.  One call with the list [2, 0] (slot != walker, and walker 1 stays zero), then
    one with every walker.  Every lag is computed independently of Ntau: a single call with Ntau lags has, bit for bit, the
    first Ntau + 1 lags of a single call with all 2 window of them.  The last case has rows of 35 slices for the lag kernel
    and two rounds of particles."""
    W = 3
    assert 0 < Ntau < 2 * window
    cfg = _cfg(dim, Np, Nb)
    L = cfg.Lbox[:dim]
    P = sn.random_walk(W, 2 * Nb + 1, Np, L, np.random.default_rng(100 * dim + 10 * window + Ntau), 0.04)
    ref = sn.Window(P, Nb, window, L, Ntau)
    exp = ref.expected([2, 0, 0, 1, 2])
    assert exp["samples"].tolist() == [2, 1, 2] and all(n > 0 for n in ref.nwrap)
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        ctx.sf_init(Ntau, window)
        ctx.sf_accumulate([2, 0])
        first = ctx.sf_read()
        ctx.sf_accumulate()
        got = ctx.sf_read()
        some = _single(ctx, Ntau, window)
        every = _single(ctx, 2 * window, window)
    what = f"B dim {dim} Np {Np} window {window} Ntau {Ntau}"
    _assert_same(first, ref.expected([2, 0]), what + " list [2, 0]")
    assert not np.any(first["C"][1]) and not np.any(first["D"][1]) and first["samples"].tolist() == [1, 0, 1]
    _assert_same(got, exp, what)
    assert got["C"].shape == (W, Ntau + 1, dim) and np.all(got["D"][:, 1:] > 0) and np.all(got["C"][:, 1:] > 0)
    _assert_same(some, ref.expected(range(W)), what + " single")
    _assert_same(every, sn.Window(P, Nb, window, L, 2 * window).expected(range(W)), what + " every lag")
    assert every["C"].shape == (W, 2 * window + 1, dim)
    for k in ("C", "D"):
        assert same_bits(some[k], every[k][:, :Ntau + 1]), (what, k, "depends on Ntau")
    _same(first, some, [2, 0], [2, 0])                                  # a listed walker has what it has in a call with all


# ---- C. the scratch cap together with repeated walkers, and one slot per launch -----------------------------------------
def test_scratch_cap_and_walkers_listed_twice(gpu_lib):
    """The system of test_scratch_budget_split (Np = 300, nine slices, 40 walkers; 1 MiB holds 15 slots) with a list of 40
    entries in which a launch ends before the cap (walker 3 at 3 and 7), ends where the no-list cut would fall (walker 14
    at 14 and 15) and ends inside what would have been the last launch (walker 33 at 33 and 38).  The launches are
    [0, 7), [7, 15), [15, 30), [30, 38), [38, 40): one is full, and from the second on slot != walker, each slot's scratch
    being taken over by another walker.  Every walker has count x the bits of ONE call at the default budget (2 x is
    exact), and the whole equals the restatement."""
    W, Np, Nb, CAP = 40, 300, 4, 15
    cfg = _cfg(3, Np, Nb)
    P = sn.random_walk(W, 2 * Nb + 1, Np, cfg.Lbox, np.random.default_rng(40), 0.04)
    assert (1 << 20) // (8 * 9 * 3 * 304) == CAP
    wl = list(range(W))
    wl[7], wl[15], wl[38] = wl[3], wl[14], wl[33]
    launches = _split_rule(wl, True, CAP, True)
    assert [(i0, i0 + len(ws)) for i0, ws in launches] == [(0, 7), (7, 15), (15, 30), (30, 38), (38, 40)]
    assert len(launches) > 3 and max(len(ws) for _, ws in launches) == CAP
    assert any(slot != w for _, ws in launches for slot, w in enumerate(ws))
    count = np.bincount(wl, minlength=W)
    assert count.max() == 2 and sorted(np.flatnonzero(count == 2)) == [3, 14, 33] and sorted(np.flatnonzero(count == 0)) == [7, 15, 38]
    VT, WF = gpu_lib.build_tables(cfg)
    with gpu_lib.PigsContext(cfg, VT, WF, n_walkers=W) as ctx:
        ctx.upload_all(P)
        once = _single(ctx, 2 * Nb, Nb)
        ctx.set_tuning("sf_scratch_mib", 1)
        got = _single(ctx, 2 * Nb, Nb, wl)
    ref = sn.Window(P, Nb, Nb, cfg.Lbox, 2 * Nb)
    _assert_same(once, ref.expected(range(W)), "C1 one call, default budget")
    for w in range(W):
        _same(got, once, w, w, int(count[w]))
    _assert_same(got, ref.expected(wl), "C1 capped, repeats")
    assert np.all(once["D"][:, 1:] > 0) and not np.any(got["D"][[7, 15, 38]])


def test_one_slot_per_launch(long_system):
    """Np = 1077, window 20: one slot of the scratch, 8 x 41 x 3 x NpPad bytes, is more than the smallest budget of 1 MiB, so
    pigs_sf_init keeps one slot and every launch takes one walker.  The list [2, 2, 0]: walker 2 has twice the bits of a
    single call, walker 0 once, walker 1 nothing, as under the default budget."""
    s = long_system
    cfg, ctx = s["cfg"], s["ctx"]
    M = 2 * LONG_NB + 1
    NpPad = ctx.stream_read(1)[0] / (8.0 * LONG_W * M * cfg.dim)        # the resident worldlines: [W][M][dim][NpPad] doubles
    assert NpPad == (LONG_NP + 7) // 8 * 8 == 1080
    assert 8 * M * cfg.dim * int(NpPad) > 1 << 20, "a slot fits the budget"
    wl = [2, 2, 0]
    try:
        ctx.set_tuning("sf_scratch_mib", 256)
        once = _single(ctx, LONG_NB, LONG_NB)
        roomy = _single(ctx, LONG_NB, LONG_NB, wl)
        ctx.set_tuning("sf_scratch_mib", 1)
        tight = _single(ctx, LONG_NB, LONG_NB, wl)
    finally:
        ctx.set_tuning("sf_scratch_mib", 256)
    _assert_same(once, s["ref"].expected(range(LONG_W)), "C2 one call, default budget")
    _assert_same(tight, s["ref"].expected(wl), "C2 one slot")
    _same(tight, roomy)
    for w, f in ((2, 2), (0, 1), (1, 0)):
        _same(tight, once, w, w, f)
    assert tight["samples"].tolist() == [1, 0, 2] and np.all(once["D"][:, 1:] > 0)
