"""GPU: the LD epilogue's per-population tables on both sides of their size gates (k_pack_epilogue.hip).

launch_epilogue keeps a tile's tables in LDS up to EPI_MAXP = 32 populations and reads them from global memory beyond;
epilogue_b11_lite_tile brings them through LDS in chunks of ELP = 16 populations; a 2-bit window's 16-bit slabs (slab16) stop at
32 populations.  Windows of P = 16, 17, 32, 33 and 64 populations -- 168 measured x 218 unmeasured SNPs: a full tile, a 16-column
edge and a half-live row tile -- are held to the oracle, and every source, Gram dtype and launch form must give one set of bits:
they are the same integer sums whatever staged them."""
import numpy as np
import pytest

import oracle
from gauss_amd import hotpath, panel, synth

pytestmark = pytest.mark.gpu

PS = [16, 17, 32, 33, 64]
M, U = 168, 218
FORMS = {
    "default": dict(),
    "i8": dict(GAUSS_GRAM_DTYPE="i8"),
    "behind": dict(GAUSS_CHAIN_ASIDE="0"),
    "merged": dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),      # the lite B11 epilogue under a merged launch
}
ENV_KEYS = sorted({k for s in FORMS.values() for k in s})
KEYS = ("b11", "b21", "z", "info", "status")

_PANEL, _WANT = {}, {}


def _panel(P):
    """P populations of 20..90 samples, M + U SNPs none of which is constant, weights, measured Z-scores; made once."""
    if P not in _PANEL:
        rng = np.random.default_rng(1000 + P)
        pops = [(f"P{k:02d}", int(rng.integers(20, 91)), ("EUR", "ASN", "AFR", "AMR")[k % 4]) for k in range(P)]
        bp = np.sort(rng.choice(np.arange(1, 900_000), size=M + U + 60, replace=False))
        G, _ = synth.synth_genotypes(bp, pops, seed=P)
        G = np.ascontiguousarray(G[G.min(1) != G.max(1)][:M + U])
        assert G.shape[0] == M + U
        off = synth.pop_offsets([q[1] for q in pops])
        rows2, src = panel.pack2bit(G, off)
        _PANEL[P] = dict(G=G, gm=np.ascontiguousarray(G[:M]), gu=np.ascontiguousarray(G[M:]), off=off, w=rng.uniform(0.0, 2.0 / P, size=P),
                         z1=rng.standard_normal(M), rows2=rows2, src=src)
    return _PANEL[P]


def _want(P, mode):
    if (P, mode) not in _WANT:
        p = _panel(P)
        _WANT[(P, mode)] = oracle.run_impute(mode, p["gm"], p["gu"], p["off"], p["w"] if mode else None, p["z1"], want_mats=True)
    return _WANT[(P, mode)]


def _host_window(P, mode):
    p = _panel(P)
    return dict(mode=mode, geno_m=p["gm"], geno_u=p["gu"], pop_off=p["off"], pop_wgt=p["w"] if mode else None, z1=p["z1"])


def _store_window(P, mode, store):
    p = _panel(P)
    return dict(mode=mode, pop_off=p["off"], pop_wgt=p["w"] if mode else None, z1=p["z1"], dev=(store.ptr, store.ptr, M, U, store.ld),
                packed=dict(fmt=1, rows_m=np.arange(M, dtype=np.int32), rows_u=np.arange(M, M + U, dtype=np.int32), pop_src_off=p["src"]))


def _job(windows, c, on_device):
    job = hotpath.Job(windows, ctx=c, on_device=on_device, want_mats=True)
    try:
        job.run()
        return [{k: np.array(r[k], copy=True) for k in KEYS} for r in job.fetch()]
    finally:
        job.close()


def _alone(P, c):
    """{(source, mode): result} of the P-population window, each in a job of its own: one-byte host rows, a resident 2-bit store."""
    out = {}
    store = hotpath.RowStore(_panel(P)["rows2"], ctx=c)
    try:
        for mode in (1, 0):
            out["host", mode] = _job([_host_window(P, mode)], c, False)[0]
            out["store", mode] = _job([_store_window(P, mode, store)], c, True)[0]
    finally:
        store.close()
    return out


def _bits(a, b, what):
    for k in KEYS:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, int(np.sum(~((a[k] == b[k]) | (np.isnan(a[k]) & np.isnan(b[k]))))))


_BASE = {}


def _base(P, ctx):
    """The session context's results: what every other form is compared with."""
    if P not in _BASE:
        _BASE[P] = _alone(P, ctx)
    return _BASE[P]


@pytest.mark.parametrize("P", PS)
def test_tables_against_the_oracle(ctx, P):
    got = _base(P, ctx)
    for mode in (1, 0):
        want = _want(P, mode)
        assert want["mpd"] == 0
        for source in ("host", "store"):
            g = got[source, mode]
            assert int(g["status"]) == 0
            for k in ("b11", "b21"):
                nan = np.isnan(want[k])
                assert np.array_equal(np.isnan(g[k]), nan), (source, mode, k)
                err = np.max(np.abs(g[k][~nan] - want[k][~nan]), initial=0.0)
                assert err <= 1e-12, (source, mode, k, float(err))
            assert np.isfinite(want["b21"]).mean() > 0.99
            for k in ("z", "info"):
                ok = ~np.isnan(want[k])
                assert np.array_equal(np.isnan(g[k]), ~ok), (source, mode, k)
                err = np.max(np.abs(g[k][ok] - want[k][ok]) / np.maximum(1.0, np.abs(want[k][ok])), initial=0.0)
                assert err <= 1e-8, (source, mode, k, float(err))
        # one-byte rows and the 2-bit store: the same integer sums on either side of the slab16 switch at P = 32 / 33
        _bits(got["store", mode], got["host", mode], (P, mode, "2-bit store vs one-byte rows"))


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form_gives_the_same_bits(ctx, monkeypatch, form):
    """A new context per launch form and Gram dtype (the switches are read when a context and its jobs are made): 1, 2, 3 and 4 table
    chunks of the lite B11 epilogue, and a partial last chunk."""
    base = {P: _base(P, ctx) for P in PS}
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    c = hotpath.Context(0)
    try:
        for P in PS:
            got = _alone(P, c)
            for key, r in got.items():
                _bits(r, base[P][key], (form, P) + key)
    finally:
        c.close()


@pytest.mark.parametrize("order", [(64, 5, 33), (33, 5, 64)])
def test_small_and_large_tables_in_one_job(ctx, order):
    """Windows past EPI_MAXP beside a 5-population one: the launch's LDS is sized by the cap of 32 while the small window stages
    its own 5 -- each window's outputs equal those of its own job."""
    for mode in (1, 0):
        alone = {P: _base(P, ctx)["host", mode] if P != 5 else _job([_host_window(5, mode)], ctx, False)[0] for P in order}
        want5 = _want(5, mode)
        assert np.max(np.abs(alone[5]["b21"] - want5["b21"])) <= 1e-12
        mixed = _job([_host_window(P, mode) for P in order], ctx, False)
        for P, r in zip(order, mixed):
            _bits(r, alone[P], (order, mode, P, "host rows"))
        stores = {P: hotpath.RowStore(_panel(P)["rows2"], ctx=ctx) for P in order}
        try:
            mixed2 = _job([_store_window(P, mode, stores[P]) for P in order], ctx, True)
        finally:
            for s in stores.values():
                s.close()
        for P, r in zip(order, mixed2):
            _bits(r, alone[P], (order, mode, P, "2-bit stores"))
