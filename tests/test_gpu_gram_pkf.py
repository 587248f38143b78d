"""The packed f32 Gram routine's sub-flush interval by the codes of the run (k_gram.hip: PK_F = 7 chunks when a 2-bit row of the
run holds a 3, PK_F_GENO = 15 when none does; the pack kernel tells the Gram launch of the same run).

Small 2-bit-store jobs whose populations sit on the new interval's boundaries are compared bit for bit -- B11, B21, z, info,
status: every correlation is formed from the integer counts in one fixed order, so one count off by one changes its bits --
against two references that know no interval: the same job under GAUSS_GRAM_PACKED=0 (one A row per lane) and on the int8
matrix cores (GAUSS_GRAM_DTYPE=i8).  The switches are read when a context is made: a new context per setting."""
import numpy as np
import pytest

from gauss_amd import hotpath
from gauss_amd import panel as panel_mod

pytestmark = pytest.mark.gpu

# 15 chunks -1 / 0 / +1 sample, 16 chunks, 30 and 31 chunks, and a population of about a hundred samples
SIZES = [959, 960, 961, 1024, 1920, 1984, 100]
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
N_ROWS, N_MEAS = 460, 200
SMALL = slice(int(OFF[-2]), int(OFF[-1]))          # the last population: where the all-2 rows get their variance
# rows of the store: the measured rows are the even ones below 400
MEASURED = np.arange(0, 2 * N_MEAS, 2)
UNMEASURED = np.setdiff1d(np.arange(N_ROWS), MEASURED)
# window A: 168 measured rows = a full column tile + 40 columns (three groups of 16: the 16-column edge), 218 unmeasured rows =
# a full row tile + 90 rows (the second wave row holds 26: one live 32-row half); window B shares measured rows 40..167 with it
# (160 = a full tile + 32 columns) and has 160 unmeasured rows; window C is window B's rows as an LD export under all three
# codings (the dominant and recessive blocks of unmeasured rows are recoded by the pack kernel)
WIN = [(0, 168, 0, 218, None), (40, 200, 100, 260, None), (40, 200, 100, 260, 7)]
ALL2_M, ALL2_U = MEASURED[[3, 50, 130, 167, 199]], UNMEASURED[[5, 101, 140, 217, 259]]

SETTINGS = {
    "unpacked": dict(GAUSS_GRAM_PACKED="0"),
    "i8": dict(GAUSS_GRAM_DTYPE="i8"),
    "default": dict(),
    "merged": dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),
    "pkf7": dict(GAUSS_GRAM_PKF="7"),
}
ENV_KEYS = sorted({k for s in SETTINGS.values() for k in s})


def _codes(kind):
    rng = np.random.default_rng(150)
    G = rng.integers(0, 3, size=(N_ROWS, int(OFF[-1]))).astype(np.uint8)
    # rows of all 2s in both operands (every product is 4: the worst case of the bound), random in the small population only
    for r in list(ALL2_M) + list(ALL2_U):
        keep = G[r, SMALL].copy()
        G[r] = 2
        G[r, SMALL] = keep
    if kind == "u3":
        G[ALL2_U[1], 959 + 17] = 3                 # one 3 in a single unmeasured row (windows A, B and C)
    elif kind == "m3":
        G[ALL2_M[1], 959 + 960 + 5] = 3            # one 3 in a single measured row
    elif kind == "threes":
        # rows of 3s against the rows of 2s: 6 * 960 > 4095 -- with these the long interval WOULD run one row's sum into the other's
        for r in (ALL2_U[2], ALL2_M[2]):
            keep = G[r, SMALL].copy()
            G[r] = 3
            G[r, SMALL] = keep
    else:
        assert kind == "clean"
    return G


_ROWS2 = {}


def _rows2(kind):
    if kind not in _ROWS2:
        _ROWS2[kind] = panel_mod.pack2bit(_codes(kind), OFF)
    return _ROWS2[kind]


def _windows(store, src_off, with_ld):
    w = np.linspace(0.05, 0.3, len(SIZES))
    z = np.random.default_rng(11).standard_normal(N_ROWS)
    wins = []
    for m0, m1, u0, u1, codings in WIN:
        if codings and not with_ld:
            continue
        mi, ui = MEASURED[m0:m1], UNMEASURED[u0:u1]
        d = dict(mode=1, pop_off=OFF, pop_wgt=w, z1=z[mi], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                 packed=dict(fmt=1, rows_m=mi.astype(np.int32), rows_u=ui.astype(np.int32), pop_src_off=src_off))
        if codings:
            d.update(ld_codings=codings, lam=0.0)
        wins.append(d)
    return wins


def _copy(res):
    return [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in res]


def _run_setting(monkeypatch, name, sequences):
    """Under one setting, in one new context: every entry of `sequences` is a list of store contents; a job is created on the
    first and run once per content (the store's rows change between the runs, the job stays).  Returns the runs' results."""
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SETTINGS[name].items():
        monkeypatch.setenv(k, v)
    c = hotpath.Context(0)
    out = []
    try:
        for seq in sequences:
            host = np.array(_rows2(seq[0])[0], copy=True)
            src_off = _rows2(seq[0])[1]
            store = hotpath.RowStore(host, ctx=c, reserve_only=True)
            assert store._host is host
            store.fill(0, N_ROWS)
            # (the forced merged launch form is for imputation windows: the LD export stays with the other settings)
            job = hotpath.Job(_windows(store, src_off, name != "merged"), ctx=c, on_device=True, want_mats=True)
            runs = []
            for i, kind in enumerate(seq):
                if i:
                    new = _rows2(kind)[0]
                    changed = np.flatnonzero((new != host).any(axis=1))
                    assert len(changed)
                    host[changed] = new[changed]
                    for r in changed:
                        store.fill(int(r), int(r) + 1)
                job.run()
                runs.append(_copy(job.fetch()))
            job.close()
            store.close()
            out.append(runs)
    finally:
        c.close()
    return out


KINDS = ["clean", "u3", "m3", "threes"]
_REF = {}


def _reference(monkeypatch):
    """The four store contents under the two settings that have no sub-flush interval; computed once."""
    if not _REF:
        for name in ("unpacked", "i8"):
            res = _run_setting(monkeypatch, name, [[k] for k in KINDS])
            _REF[name] = {k: r[0] for k, r in zip(KINDS, res)}
    return _REF


def _same(got, want, what):
    assert 2 <= len(got) <= len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert sorted(a) == sorted(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k], equal_nan=True), (what, i, k)
            else:
                assert a[k] == b[k], (what, i, k)


def test_the_two_references_agree_and_see_the_data(monkeypatch):
    ref = _reference(monkeypatch)
    for k in KINDS:
        _same(ref["i8"][k], ref["unpacked"][k], k)
        for r in ref["unpacked"][k][:2]:
            assert np.all(np.isfinite(r["z"])) and np.all(np.isfinite(r["b21"]))
    # a single 3 changes the results: the references are not blind to the rows the cases below touch
    for k in ("u3", "m3", "threes"):
        assert not np.array_equal(ref["unpacked"][k][0]["b21"], ref["unpacked"]["clean"][0]["b21"])
    # the recoded blocks of window C differ from its additive block
    b = ref["unpacked"]["clean"][2]["b21"]
    U = b.shape[0] // 3
    assert not np.array_equal(b[:U], b[U:2 * U]) and not np.array_equal(b[:U], b[2 * U:])


@pytest.mark.parametrize("setting", ["default", "merged", "pkf7"])
def test_every_store_content_gives_the_references_bits(monkeypatch, setting):
    """Codes <= 2 with rows of all 2s in both operands (the long interval, at its bound), one 3 in a single unmeasured row, one in
    a single measured row, and rows of 3s (the short interval must have been taken: 6 * 960 does not fit twelve bits)."""
    ref = _reference(monkeypatch)
    res = _run_setting(monkeypatch, setting, [[k] for k in KINDS])
    for k, r in zip(KINDS, res):
        _same(r[0], ref["unpacked"][k], (setting, k))
        _same(r[0], ref["i8"][k], (setting, k, "i8"))


@pytest.mark.parametrize("setting", ["default", "merged"])
def test_a_run_never_uses_another_runs_verdict(monkeypatch, setting):
    """One job, two runs, the store changes in between: a 3 (rows of 3s) that is gone in the second run, and the reverse."""
    ref = _reference(monkeypatch)
    seqs = [["threes", "clean"], ["clean", "threes"], ["u3", "clean", "m3", "threes"]]
    res = _run_setting(monkeypatch, setting, seqs)
    for seq, runs in zip(seqs, res):
        for k, r in zip(seq, runs):
            _same(r, ref["unpacked"][k], (setting, seq, k))
            _same(r, ref["i8"][k], (setting, seq, k, "i8"))
