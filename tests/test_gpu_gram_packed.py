"""The packed f32 Gram routine (k_gram.hip: two A rows per lane on items with 16-bit slabs) against the exact integers.

The integer reference is G.astype(int64) @ G.T: gauss_gram_counts (byte rows, f32 slabs, one A row per lane) is compared with
it directly, and the 2-bit rows of the same matrix -- the items that take the packed routine -- must then give B11, B21, z and
info with the bits of the byte-row job: every correlation is formed from those integers in one fixed order, so one count off
by one changes its bits."""
import numpy as np
import pytest

from gauss_amd import hotpath
from gauss_amd import panel as panel_mod
from helpers import small_panel

pytestmark = pytest.mark.gpu

KEYS = ("b11", "b21", "z", "info")


def _same(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)
    assert a["status"] == b["status"], what


def _rows(n_rows, sizes, kind, seed):
    """Genotype rows over populations of `sizes` samples: `kind` 'three' = every code 3 (each 448-sample stretch sums to the
    4032 the sub-flush bound allows), 'near' = code 3 with a sprinkle of other codes (sums stay next to the bound and the rows
    have a variance, so that a wrong count shows in a correlation), 'mixed' = codes 0..3 at random."""
    rng = np.random.default_rng(seed)
    n = int(np.sum(sizes))
    if kind == "three":
        return np.full((n_rows, n), 3, dtype=np.uint8)
    if kind == "near":
        G = np.full((n_rows, n), 3, dtype=np.uint8)
        hit = rng.random((n_rows, n)) < 0.02
        G[hit] = rng.integers(0, 3, size=int(hit.sum()))
        return G
    return rng.integers(0, 4, size=(n_rows, n)).astype(np.uint8)


def _packed_vs_bytes(ctx, G, sizes, M, mode, what):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    w = np.linspace(0.05, 0.3, len(sizes))
    z1 = np.random.default_rng(11).standard_normal(M)
    gm, gu = np.ascontiguousarray(G[:M]), np.ascontiguousarray(G[M:])
    cnt = hotpath.gram_counts(G, ctx=ctx)
    assert np.array_equal(cnt, G.astype(np.int64) @ G.astype(np.int64).T), what
    base = hotpath.impute_window(mode, gm, gu, off, w, z1, want_mats=True, ctx=ctx)
    rows2, _ = panel_mod.pack2bit(G, off)
    job = hotpath.Job([dict(mode=mode, geno_m=rows2[:M], geno_u=rows2[M:], pop_off=off, pop_wgt=w, z1=z1, packed=dict(fmt=1))],
                      ctx=ctx, want_mats=True)
    job.run()
    got = job.fetch()[0]
    job.close()
    _same(got, base, what)
    return got


# populations that sit on every boundary of the routine: a sub-flush interval (448 k +/- 1 samples), the longest 16-bit-slab
# segment (7168) and one sample more (a second segment of a single live unit)
SIZES = {
    "448k": [447, 448, 449, 895, 897, 1343, 1345],
    "7168": [7168],
    "7169": [7169],
    "7168+7169": [7168, 7169, 449],
}
# (measured rows M, all rows): the measured rows are the Gram's columns -- the last column tile holds 16, 32, 40 or 64 live
# columns: 1, 2, 3, 4 groups of 16 -- and the last tile of unmeasured rows holds 20 or 100: one or two live 32-row halves of
# its first wave row; every job has diagonal tiles (B11)
SHAPES = [(144, 144 + 148), (160, 160 + 228), (168, 168 + 20), (192, 192 + 100), (16, 16 + 40), (300, 300 + 33)]


@pytest.mark.parametrize("kind", ["three", "near", "mixed"])
@pytest.mark.parametrize("pops", sorted(SIZES))
def test_packed_items_match_the_integer_gram_on_boundary_populations(ctx, kind, pops):
    M, n_rows = SHAPES[sorted(SIZES).index(pops) % len(SHAPES)]
    G = _rows(n_rows, SIZES[pops], kind, seed=5)
    _packed_vs_bytes(ctx, G, SIZES[pops], M, 1, (kind, pops))


@pytest.mark.parametrize("shape", SHAPES)
def test_packed_items_match_the_integer_gram_on_every_wave_shape(ctx, shape):
    M, n_rows = shape
    sizes = [449, 7168, 30, 897]
    for kind, mode in (("near", 1), ("mixed", 0)):
        _packed_vs_bytes(ctx, _rows(n_rows, sizes, kind, seed=M), sizes, M, mode, (shape, kind))


def test_packed_form_and_unpacked_form_give_the_same_bits_in_every_launch_form(monkeypatch):
    """GAUSS_GRAM_PACKED=0 (one A row per lane, the form before) against the default: z, info, status, B11 and B21 bit for bit
    on a job queued with the chain behind one Gram launch, beside it in the merged launch, and beside it as two launches; own
    and shared measured rows.  The switch is read when a context is made: a new context per form."""
    p = small_panel(n_snp=2600, scale=0.05, seed=43)
    G = p["G"]
    rows2, src_off = panel_mod.pack2bit(G, p["off"])
    rng = np.random.default_rng(6)
    n = G.shape[0]
    measured = np.sort(np.concatenate([np.arange(12), 12 + rng.choice(n - 12, size=n // 3, replace=False)]))
    unmeasured = np.setdiff1d(np.arange(n), measured)
    z = rng.standard_normal(n)

    def run(packed, aside, merged, share):
        monkeypatch.setenv("GAUSS_GRAM_PACKED", "1" if packed else "0")
        monkeypatch.setenv("GAUSS_CHAIN_ASIDE", "2" if aside else "0")
        monkeypatch.setenv("GAUSS_CHAIN_MERGED", "2" if merged else "0")
        monkeypatch.setenv("GAUSS_SHARE_MEASURED", "1" if share else "0")
        c = hotpath.Context(0)
        try:
            store = hotpath.RowStore(rows2, ctx=c)
            wins = []
            for a, b in [(0, 131), (97, 340), (211, 760), (330, len(measured)), (500, 640)]:
                mi = measured[a:b]
                lo, hi = mi[len(mi) // 4], mi[3 * len(mi) // 4]
                ui = unmeasured[(unmeasured > lo) & (unmeasured < hi)]
                wins.append(dict(mode=1, pop_off=p["off"], pop_wgt=p["w"], z1=z[mi], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                                 packed=dict(fmt=1, rows_m=mi.astype(np.int32), rows_u=ui.astype(np.int32), pop_src_off=src_off)))
            job = hotpath.Job(wins, ctx=c, on_device=True, want_mats=True)
            job.run()
            out = job.fetch()
            stats = job.stats()
            job.close()
            store.close()
            return out, stats
        finally:
            c.close()

    for share in (False, True):
        for aside, merged in ((False, False), (True, True), (True, False)):
            old, s_old = run(False, aside, merged, share)
            new, s_new = run(True, aside, merged, share)
            for k, (x, y) in enumerate(zip(old, new)):
                _same(x, y, (share, aside, merged, k))
            # the MFMAs actually issued: a packed wave issues one per live B half where the unpacked one issues one per A half too
            assert 0.5 * s_old["executed_flops"] <= s_new["executed_flops"] < s_old["executed_flops"]
