"""GPU: the LD scores of an LD window's measured SNPs (k_ldscore.hip) against tests/ldscore_ref.py.

(i)  On the B11 / B21 the GPU itself returns for the same window with matrices requested: raw and l2 within 1e-12 relative -- a sum of
     at most 4 200 non-negative fp64 terms carries at most count 2^-53 = 5e-13 -- and mass[0] exactly.  A category with real-valued
     weights sums terms of both signs: its bound is 1e-12 of the same sum with the weights' absolute values.  Every case prints whether
     the bits are those of the replayed order.
(ii) On the CPU oracle's LD of the same genotypes: 4e-12 count absolute (the project's LD entries are within 1e-12 of the oracle's,
     |d r^2| <= 2 |r| d + d^2), times the largest absolute weight for a stratified row.
Then: the same bits alone / first / last in a job, from one-byte, 2-bit and resident rows, on one queue, with and without the matrices;
a monomorphic reference row reaches exactly the targets whose band holds it; every refusal; a job in which nobody asks keeps its bits."""
import ctypes as C

import numpy as np
import pytest

import ldscore_ref as lr
import oracle
from gauss_amd import _lib, hotpath
from gauss_amd import panel as panel_mod

pytestmark = pytest.mark.gpu

CHUNK = _lib.LDS_CHUNK
KEYS = ("lds_raw", "lds_l2", "lds_mass")
_cache = {}


def _panel(S, seed, n_samples, n_pop, span=200_000):
    """S SNPs with LD between neighbours: a row is, three times in four, its predecessor with a tenth of its genotypes redrawn.  Every
    row varies inside the first population (no LD entry is 0 / 0)."""
    key = (S, seed, n_samples, n_pop, span)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(seed)
    G = np.empty((S, n_samples), dtype=np.uint8)
    for k in range(S):
        if k and rng.random() < 0.75:
            G[k] = G[k - 1]
            flip = rng.random(n_samples) < 0.1
            G[k, flip] = rng.integers(0, 3, size=int(flip.sum()))
        else:
            G[k] = rng.binomial(2, rng.uniform(0.1, 0.9), size=n_samples)
    G[:, 0], G[:, 1] = 0, 2
    cuts = np.sort(rng.choice(np.arange(40, n_samples - 40, 40), size=n_pop - 1, replace=False)) if n_pop > 1 else []
    off = np.array([0, *cuts, n_samples], dtype=np.int32)
    w = rng.uniform(0.1, 0.6, size=n_pop)
    bp = np.sort(rng.integers(1, span, size=S)).astype(np.int32)
    out = _cache[key] = dict(G=np.ascontiguousarray(G), off=off, w=w, bp=bp)
    return out


def _window(M, U, seed, n_samples=300, n_pop=2):
    p = _panel(M + U, seed, n_samples, n_pop)
    rng = np.random.default_rng(seed + 1)
    mi = np.sort(rng.permutation(M + U)[:M])
    ui = np.setdiff1d(np.arange(M + U), mi)
    return p, mi, ui


def _annot(C_, T, seed):
    """binary and real-valued categories in turn; one all-zero category when there is room for it"""
    if not C_:
        return None
    rng = np.random.default_rng(seed)
    a = np.vstack([rng.integers(0, 2, size=T).astype(np.float64) if c % 2 == 0 else rng.normal(size=T) for c in range(C_)])
    if C_ > 2:
        a[2] = 0.0
    return a


def _check(got, mats, want_cpu, bm, bu, radius, n, annot, what):
    """got: lds_* of a window; mats: b11 / b21 the GPU returned for it; want_cpu: the oracle's matrices of the same rows, or None"""
    ref = lr.replay(mats["b11"], mats["b21"], bm, bu, radius, n, annot)
    mag = lr.plain(mats["b11"], mats["b21"], bm, bu, radius, n, None if annot is None else np.abs(annot))
    cnt = lr.count(bm, bu, radius)
    bits = all(np.array_equal(got["lds_" + k], ref[k], equal_nan=True) for k in ("raw", "l2", "mass"))
    err = {}
    for k in ("raw", "l2"):
        nan = np.isnan(ref[k])                             # (a NaN inside a band: the same targets, and the bound for all the others)
        assert np.array_equal(np.isnan(got["lds_" + k]), nan), (what, k)
        scale = np.maximum(np.abs(ref[k]), np.abs(mag[k]))
        gap = np.where(nan, 0.0, np.abs(got["lds_" + k] - ref[k]) / np.maximum(scale, 1e-300))
        err[k] = float(np.max(gap))
    print(f"REACHED ldscore {what}: M {len(bm)} U {len(bu)} radius {radius} C {0 if annot is None else len(annot)}  count <= {int(cnt.max())}  "
          f"raw {err['raw']:.2e} l2 {err['l2']:.2e} (bound 1e-12)  bits equal: {bits}")
    assert err["raw"] <= 1e-12 and err["l2"] <= 1e-12, (what, err)
    assert np.array_equal(got["lds_mass"][0], cnt), what
    if annot is not None:
        assert np.all(np.abs(got["lds_mass"][1:] - ref["mass"][1:]) <= 1e-12 * np.maximum(mag["mass"][1:], 1e-300)), what
    if want_cpu is not None:
        cpu = lr.plain(want_cpu["b11"], want_cpu["b21"], bm, bu, radius, n, annot)
        amax = np.ones(1) if annot is None else np.concatenate([[1.0], np.abs(annot).max(axis=1)])
        gap = np.abs(got["lds_raw"] - cpu["raw"])
        bound = 4e-12 * cnt[None, :] * amax[:, None]
        print(f"REACHED ldscore {what}: against the oracle's LD {float(gap.max()):.2e} (bound {float(bound.max()):.2e})")
        assert np.all(gap <= bound), (what, float(np.max(gap - bound)))
        # l2 = raw (1 + 1 / (n - 2)) - mass / (n - 2): raw's bound times that factor, and four roundings of the expression's terms
        f = 1.0 + 1.0 / (n - 2.0)
        gap2 = np.abs(got["lds_l2"] - cpu["l2"])
        bound2 = bound * f + 4 * 2.0 ** -52 * (np.abs(cpu["raw"]) * f + np.abs(cpu["mass"]) / (n - 2.0))
        print(f"REACHED ldscore {what}: l2 against the oracle's LD {float(gap2.max()):.2e} (bound {float(bound2.max()):.2e})")
        assert np.all(gap2 <= bound2), (what, float(np.max(gap2 - bound2)))
    return ref


RADII = (0, 17_000, 10 ** 7)          # one position; bands that end inside a chunk and inside a block of targets; the whole window
SHAPES = [(M, U) for M in (1, 63, 64, 65, 130) for U in (0, 1, CHUNK - 1, CHUNK, CHUNK + 1, 700)]


@pytest.mark.parametrize("M,U", SHAPES, ids=lambda v: str(v))
def test_shapes_radii_and_categories(ctx, M, U):
    """M on either side of a wave of targets, U on either side of a chunk; every radius with one of C = 0, 1, 32, the pairing turned from
    case to case so that the set covers every combination; pooled and weighted, one to three populations"""
    k = SHAPES.index((M, U))
    mode, n_pop, n_samples = k % 2, 1 + k % 3, (200, 300, 450, 600)[k % 4]
    p, mi, ui = _window(M, U, seed=100 + k, n_samples=n_samples, n_pop=n_pop)
    gm, gu = np.ascontiguousarray(p["G"][mi]), np.ascontiguousarray(p["G"][ui])
    bm, bu = p["bp"][mi], p["bp"][ui]
    w = p["w"] if mode else None
    n = float(n_samples)
    cpu = oracle.ld_blocks(mode, gm, gu, p["off"], w, 1.0, (0,))
    mats = None
    for ir, radius in enumerate(RADII):
        C_ = (0, 1, 32)[(ir + k) % 3]
        annot = _annot(C_, M + U, seed=k)
        got = hotpath.ld_window(mode, gm, gu, p["off"], w, ctx=ctx, ldscore=dict(radius=radius, bp_m=bm, bp_u=bu, n=n, annot=annot))
        assert got["status"] == 0 and got["lds_raw"].shape == (1 + C_, M)
        if mats is not None:
            assert np.array_equal(got["b11"], mats["b11"]) and np.array_equal(got["b21"], mats["b21"])
        mats = dict(b11=got["b11"], b21=got["b21"])
        _check(got, mats, cpu, bm, bu, radius, n, annot, f"mode {mode} P {n_pop} N {n_samples}")
    if radius >= 10 ** 7:
        assert np.all(got["lds_mass"][0] == M + U)


def _same(a, b, what):
    for key in KEYS:
        assert np.array_equal(a[key], b[key], equal_nan=True), (what, key)


def test_the_bits_do_not_depend_on_the_job_the_source_or_the_queue(ctx, monkeypatch):
    """One window alone, first and last in a job of windows of other sizes; its rows as bytes in host memory, as a resident one-byte
    store, as a resident 2-bit store; on a context with one queue; with and without the matrices coming back"""
    S = 900
    p = _panel(S, seed=77, n_samples=330, n_pop=3)
    G, bp = p["G"], p["bp"]
    rng = np.random.default_rng(3)

    def rows(lo, hi, M):
        idx = np.arange(lo, hi)
        mi = np.sort(rng.permutation(idx)[:M])
        return mi.astype(np.int32), np.setdiff1d(idx, mi).astype(np.int32)

    sets = [rows(100, 600, 130), rows(0, 90, 20), rows(500, 900, 65)]
    annot = _annot(3, 500, seed=9)

    def lds(k):
        mi, ui = sets[k]
        return dict(radius=25_000, bp_m=bp[mi], bp_u=bp[ui], n=330.0, annot=annot if k == 0 else None)

    def host(k, **more):
        mi, ui = sets[k]
        return dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=np.zeros(len(mi)), geno_m=np.ascontiguousarray(G[mi]),
                    geno_u=np.ascontiguousarray(G[ui]), lam=0.0, ldscore=lds(k), **more)

    def run(c, wins, on_device=False):
        job = hotpath.Job(wins, ctx=c, on_device=on_device)
        try:
            job.run()
            return job.fetch()
        finally:
            job.close()

    ref = run(ctx, [host(0)])[0]
    mi, ui = sets[0]
    _check(ref, ref, None, bp[mi], bp[ui], 25_000, 330.0, annot, "the window alone")
    _same(run(ctx, [host(0), host(1), host(2)])[0], ref, "first in a job")
    _same(run(ctx, [host(1), host(2), host(0)])[2], ref, "last in a job")
    bare = run(ctx, [host(1), host(0, want_matrices=False)])[1]
    assert bare["b11"] is None and bare["b21"] is None
    _same(bare, ref, "no matrices back")
    one = hotpath.ld_window(1, G[mi], G[ui], p["off"], p["w"], ctx=ctx, ldscore=lds(0), want_matrices=False)
    assert one["b11"] is None
    _same(one, ref, "the one-window call, no matrices back")

    rows2, src_off = panel_mod.pack2bit(G, p["off"])

    def resident(c):
        out = []
        for fmt, store_rows, src in ((0, G, None), (1, rows2, src_off)):
            store = hotpath.RowStore(store_rows, ctx=c)
            try:
                wins = []
                for k in (1, 0, 2):
                    a, b = sets[k]
                    packed = dict(fmt=fmt, rows_m=a, rows_u=b)
                    if src is not None:
                        packed["pop_src_off"] = src
                    wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=np.zeros(len(a)), lam=0.0, ldscore=lds(k),
                                     dev=(store.ptr, store.ptr, len(a), len(b), store.ld), packed=packed))
                out.append(run(c, wins, on_device=True)[1])
            finally:
                store.close()
        return out

    for name, got in zip(("resident one-byte rows", "resident 2-bit rows"), resident(ctx)):
        _same(got, ref, name)
        assert np.array_equal(got["b11"], ref["b11"]) and np.array_equal(got["b21"], ref["b21"]), name
    with monkeypatch.context() as m:                   # read when a context is made: one queue
        m.setenv("GAUSS_SIDE_STREAM", "0")
        c = hotpath.Context(0)
        try:
            _same(run(c, [host(1), host(0)])[1], ref, "one queue, host rows")
            for name, got in zip(("one queue, one-byte store", "one queue, 2-bit store"), resident(c)):
                _same(got, ref, name)
        finally:
            c.close()


def test_a_monomorphic_reference_row_reaches_only_the_bands_that_hold_it(ctx):
    """Pooled LD of a row without variance is 0 / 0.  The targets within the radius of it are NaN, exactly those; every other target has
    the value it has on the returned matrices, and the value of the window without that row"""
    M, U, radius = 130, 200, 9_000
    p, mi, ui = _window(M, U, seed=41, n_samples=260, n_pop=1)
    gm, gu = np.ascontiguousarray(p["G"][mi]), np.ascontiguousarray(p["G"][ui])
    bm, bu = p["bp"][mi], p["bp"][ui]
    dead = U // 2
    gu[dead, :] = 1
    hit = np.abs(bm.astype(np.int64) - int(bu[dead])) <= radius
    assert 0 < hit.sum() < M
    annot = np.zeros((1, M + U))                      # a zero weight does not hide it
    got = hotpath.ld_window(0, gm, gu, p["off"], None, ctx=ctx, ldscore=dict(radius=radius, bp_m=bm, bp_u=bu, n=260.0, annot=annot))
    assert np.all(np.isnan(got["b21"][dead]))
    for c in (0, 1):
        assert np.array_equal(np.isnan(got["lds_raw"][c]), hit), c
        assert np.array_equal(np.isnan(got["lds_l2"][c]), hit), c
    assert np.all(np.isfinite(got["lds_mass"]))
    _check(got, got, None, bm, bu, radius, 260.0, annot, "a monomorphic row")
    keep = np.arange(U) != dead
    less = hotpath.ld_window(0, gm, gu[keep], p["off"], None, ctx=ctx, ldscore=dict(radius=radius, bp_m=bm, bp_u=bu[keep], n=260.0))
    far = ~hit
    assert np.all(np.abs(got["lds_raw"][0][far] - less["lds_raw"][0][far]) <= 1e-12 * less["lds_raw"][0][far])
    assert np.array_equal(got["lds_mass"][0][far], less["lds_mass"][0][far])


def _refused(ctx, text, mode=0, lam=0.0, codings=1, kind=None, n_annot=None, **change):
    p, mi, ui = _window(20, 30, seed=5, n_samples=200, n_pop=1)
    gm, gu = np.ascontiguousarray(p["G"][mi]), np.ascontiguousarray(p["G"][ui])
    q = dict(radius=1000, bp_m=p["bp"][mi], bp_u=p["bp"][ui], n=200.0, annot=None)
    q.update(change)
    desc = hotpath.WindowDesc()
    win = hotpath._Win(desc, dict(mode=mode, geno_m=gm, geno_u=gu, pop_off=p["off"], z1=np.zeros(20), lam=lam, ld_codings=codings, ldscore=q), True)
    if n_annot is not None:                            # a count that disagrees with the weights passed
        desc.lds_n_annot = n_annot
    if kind is not None:                               # an imputation window that asks
        desc.kind = kind
        desc.z1 = win.z1.ctypes.data_as(C.POINTER(C.c_double))
        desc.out_z, desc.out_info = win.z.ctypes.data_as(C.POINTER(C.c_double)), win.info.ctypes.data_as(C.POINTER(C.c_double))
    rc = ctx.lib.gauss_impute_window(ctx.handle, C.byref(desc))
    msg = ctx.lib.gauss_last_error().decode()
    assert rc == -1, (text, rc, msg)                   # GAUSS_E_INVALID
    assert text in msg, (text, msg)


def test_every_refusal_is_invalid_with_its_message(ctx):
    bp = _window(20, 30, seed=5, n_samples=200, n_pop=1)
    p, mi, ui = bp
    down_m, down_u = p["bp"][mi].copy(), p["bp"][ui].copy()
    down_m[[3, 4]] = down_m[[4, 3]] + np.array([1, 0], dtype=np.int32)
    down_u[[7, 8]] = down_u[[8, 7]] + np.array([1, 0], dtype=np.int32)
    bad = np.zeros((2, 50))
    bad[1, 33] = np.inf
    _refused(ctx, "are for LD windows only (imputation window)", kind=_lib.WIN_IMPUTE)
    _refused(ctx, "a window with lambda = 0", lam=0.1)
    _refused(ctx, "take the additive coding only", codings=3)
    _refused(ctx, "lds_bp_m[4]", bp_m=down_m)
    _refused(ctx, "lds_bp_u[8]", bp_u=down_u)
    _refused(ctx, "lds_bp_m is NULL", bp_m=None)
    _refused(ctx, "lds_bp_u is NULL", bp_u=None)
    for n in (2.0, 1.0, np.nan, np.inf):
        _refused(ctx, "the sample size of the bias adjustment is finite and above 2", n=n)
    _refused(ctx, "the radius of an LD score is not negative", radius=-1)
    _refused(ctx, "LD scores take 0 .. 32 annotation categories", annot=np.zeros((33, 50)))
    _refused(ctx, "LD scores take 0 .. 32 annotation categories", n_annot=-1)
    _refused(ctx, "the categories' weights (lds_annot) are NULL", n_annot=2)
    _refused(ctx, "lds_annot[1][33]", annot=bad)


def test_more_chunks_than_a_grid_holds_are_refused(ctx):
    """The chunks are the y extent of ldscore_kernel's grid, 65 535 at the most: one target and 65 535 chunks of other rows make one
    too many.  Refused by the planner, before anything is allocated or launched"""
    U = 65534 * CHUNK + 1
    gm, gu = np.array([[0, 1, 2, 1, 0, 2, 1, 1]], dtype=np.uint8), np.ones((U, 8), dtype=np.uint8)
    desc = hotpath.WindowDesc()
    win = hotpath._Win(desc, dict(mode=0, geno_m=gm, geno_u=gu, pop_off=[0, 8], z1=np.zeros(1), lam=0.0,
                                  ldscore=dict(radius=10, bp_m=[5], bp_u=np.arange(U, dtype=np.int32), n=8.0), want_matrices=False), True)
    rc = ctx.lib.gauss_impute_window(ctx.handle, C.byref(desc))
    msg = ctx.lib.gauss_last_error().decode()
    assert rc == -1 and "1 + 4194177 rows make 65536 chunks of 64; a window takes at most 65535" in msg, (rc, msg)
    assert "lds_raw" in win.result() and np.all(np.isnan(win.result()["lds_raw"]))


def test_a_job_in_which_nobody_asks_keeps_its_bits(ctx):
    """An LD window and an imputation window: as they are, and beside an LD window that asks"""
    p, mi, ui = _window(70, 150, seed=12, n_samples=240, n_pop=2)
    gm, gu = np.ascontiguousarray(p["G"][mi]), np.ascontiguousarray(p["G"][ui])
    z1 = np.random.default_rng(1).normal(size=70)
    ld = dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=np.zeros(70), geno_m=gm, geno_u=gu, lam=0.0, ld_codings=1)
    imp = dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z1, geno_m=gm, geno_u=gu)
    ask = dict(ld, ldscore=dict(radius=20_000, bp_m=p["bp"][mi], bp_u=p["bp"][ui], n=240.0))
    del ask["ld_codings"]

    def run(wins):
        job = hotpath.Job(wins, ctx=ctx)
        try:
            job.run()
            return job.fetch()
        finally:
            job.close()

    plain = run([ld, imp])
    assert "lds_raw" not in plain[0]
    mixed = run([ld, imp, ask])
    for key in ("b11", "b21"):
        assert np.array_equal(mixed[0][key], plain[0][key]) and np.array_equal(mixed[2][key], plain[0][key]), key
    for key in ("z", "info"):
        assert np.array_equal(mixed[1][key], plain[1][key]), key
    assert mixed[1]["status"] == plain[1]["status"]
    _check(mixed[2], mixed[2], None, p["bp"][mi], p["bp"][ui], 20_000, 240.0, None, "beside an imputation window")
