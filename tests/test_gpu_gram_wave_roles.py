"""The Gram kernel's wave roles (k_gram_common.h: which block of a 128 x 128 tile each of a workgroup's four waves multiplies).

A tile whose live rows or live columns end in its first half gets a narrow layout from the planner -- four blocks of 64 x 32
(32 x 32 when both halves are empty and the item is not packed) instead of the four 64 x 64 quadrants, of which two or three would be empty.  The sums
and the slab addresses are the same, so everything a job returns must have the bits of the quadrant roles
(GAUSS_GRAM_ROTATE=0: the planner sets no layout); the int8 kernel keeps the quadrants and must give the same bits too.

No rotation of the roles over the wave index is tested because none is built: the hardware already starts every workgroup's
waves on another SIMD (tools/wave_simd_probe.py).

The first test needs no GPU: the role functions are compiled for the host, dumped for every layout and a grid of live
extents, and held against the mirror below, which is then checked to cover every live entry of the tile exactly once."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- mirror of k_gram_common.h ------------------------------------------------------------------------------------------
QUAD, NARROW_B, NARROW_A, NARROW_AB = 0, 1, 2, 3


def wave_role(wave, layout):
    """(r0, c0, rows, cols) of the wave's block."""
    if layout == NARROW_B:
        return (wave >> 1) * 64, (wave & 1) * 32, 64, 32
    if layout == NARROW_A:
        return 0, wave * 32, 64, 32
    if layout == NARROW_AB:
        return (wave >> 1) * 32, (wave & 1) * 32, 32, 32
    return (wave >> 1) * 64, (wave & 1) * 64, 64, 64


def tile_layout(rows_a, rows_b, packed):
    if rows_a <= 64 and rows_b <= 64:
        return NARROW_B if packed else NARROW_AB
    return NARROW_B if rows_b <= 64 else (NARROW_A if rows_a <= 64 else QUAD)


def wave_work(rows_a, rows_b, diag, packed, edge16, wave, layout):
    """(na, nb, nc, sk10): live 32-row halves of A and of B in the block, groups of 16 columns for the edge routine (0: none),
    and whether the block's lower-left 32 x 32 sub-block is left out (unpacked diagonal block)."""
    r0, c0, rows, cols = wave_role(wave, layout)
    clamp = lambda v, hi: max(0, min(hi, v))
    na = clamp((rows_a - r0 + 31) // 32, rows // 32)
    nb = clamp((rows_b - c0 + 31) // 32, cols // 32)
    nb16 = clamp((rows_b - c0 + 15) // 16, cols // 16)
    if diag and r0 >= c0 + cols:
        na = 0
    nc = nb16 if (edge16 and na > 0 and nb16 % 2 == 1) else 0
    return na, nb, nc, bool(diag and not packed and r0 == c0 and na == 2 and nb == 2)


EXTENTS = [1, 8, 16, 17, 31, 32, 33, 40, 48, 49, 63, 64, 65, 70, 80, 81, 96, 97, 112, 113, 127, 128]

DUMP = r"""
#include "k_gram_common.h"
#include <cstdio>
using namespace gauss;
int main()
{
    const int ext[] = {%s};
    for (int layout = 0; layout < 4; layout++)
        for (int w = 0; w < 4; w++) {
            const WaveRole ro = wave_role(w, layout);
            printf("R %%d %%d %%d %%d %%d %%d\n", layout, w, ro.r0, ro.c0, ro.rows, ro.cols);
        }
    for (int ra : ext)
        for (int rb : ext) {
            printf("L %%d %%d %%d %%d\n", ra, rb, tile_layout(ra, rb, false), tile_layout(ra, rb, true));
            for (int layout = 0; layout < 4; layout++)
                for (int f = 0; f < 8; f++)
                    for (int w = 0; w < 4; w++) {
                        const WaveWork x = wave_work(ra, rb, (f & 1) != 0, (f & 2) != 0, (f & 4) != 0, w, layout);
                        printf("W %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", ra, rb, layout, f, w, x.na, x.nb, x.nc, x.sk10 ? 1 : 0);
                    }
        }
    return 0;
}
"""


def test_the_role_functions_cover_every_live_entry_once_and_the_mirror_is_the_header(tmp_path):
    # 1. the mirror is what the header computes (the header's functions are plain constexpr C++: compiled for the host)
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    src = tmp_path / "role_dump.cpp"
    src.write_text(DUMP % ", ".join(str(e) for e in EXTENTS))
    exe = tmp_path / "role_dump"
    subprocess.check_call([hipcc, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                           "-I" + os.path.join(ROOT, "gauss_amd", "csrc"), "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    seen = {"R": 0, "L": 0, "W": 0}
    for line in subprocess.check_output([str(exe)]).decode().split("\n"):
        if not line:
            continue
        v = [int(x) for x in line[2:].split()]
        seen[line[0]] += 1
        if line[0] == "R":
            assert wave_role(v[1], v[0]) == tuple(v[2:]), line
        elif line[0] == "L":
            assert (tile_layout(v[0], v[1], False), tile_layout(v[0], v[1], True)) == (v[2], v[3]), line
        else:
            ra, rb, layout, f, w = v[:5]
            got = wave_work(ra, rb, bool(f & 1), bool(f & 2), bool(f & 4), w, layout)
            assert (got[0], got[1], got[2], int(got[3])) == tuple(v[5:]), line
    assert seen == {"R": 16, "L": len(EXTENTS) ** 2, "W": len(EXTENTS) ** 2 * 4 * 8 * 4}

    # 2. coverage: under the quadrant layout and under the layout the planner picks, the four waves' live blocks hold every
    # live (row, column) of the tile exactly once and nothing is held twice; a diagonal tile: every live entry on or above
    # the diagonal at least (blocks below it are mirrors and may be left out)
    for ra, rb in itertools.product(sorted(set(EXTENTS) | set(range(1, 129, 5))), repeat=2):
        for diag, packed, edge16 in itertools.product((False, True), repeat=3):
            if diag and ra != rb:
                continue
            for layout in {QUAD, tile_layout(ra, rb, packed)}:
                cover = np.zeros((128, 128), dtype=np.int8)
                for w in range(4):
                    r0, c0, _, _ = wave_role(w, layout)
                    na, nb, nc, sk10 = wave_work(ra, rb, diag, packed, edge16, w, layout)
                    if na == 0:
                        continue
                    wide = 16 * nc if nc else 32 * nb
                    cover[r0:r0 + 32 * na, c0:c0 + wide] += 1
                    if sk10:
                        cover[r0 + 32:r0 + 64, c0:c0 + 32] -= 1
                assert cover.max() <= 1, (ra, rb, layout, diag, packed, edge16)
                live = np.zeros((128, 128), dtype=bool)
                live[:ra, :rb] = True
                if diag:
                    live &= np.triu(np.ones((128, 128), dtype=bool))
                assert np.all(cover[live] == 1), (ra, rb, layout, diag, packed, edge16)
                # nothing is multiplied that lies wholly in the padding: a covered 16-column group holds a live column, a covered
                # 32-row half a live row
                rows_cov, cols_cov = np.flatnonzero(cover.any(axis=1)), np.flatnonzero(cover.any(axis=0))
                assert rows_cov.max() < -(-ra // 32) * 32 and cols_cov.max() < (-(-rb // 16) * 16 if edge16 else -(-rb // 32) * 32)
    # the planner's choice is the narrow one exactly when a half is empty
    for pk in (False, True):
        assert tile_layout(64, 64, pk) == (NARROW_B if pk else NARROW_AB) and tile_layout(65, 64, pk) == NARROW_B
        assert tile_layout(64, 65, pk) == NARROW_A and tile_layout(65, 65, pk) == QUAD


# ---- on the GPU ------------------------------------------------------------------------------------------------------------
SIZES = [70, 130, 200]
OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
N_STORE = 2 * 256 + 2 * 256 + 8
# (M, U): what the shape exercises
SHAPES = {
    (97, 40): "both edges light: B21's tiles and B11's are narrow both ways",
    (130, 70): "second column tile with 2 live columns (one group of 16); rows 65..70 in the second row block",
    (176, 200): "second column tile with 48 live columns (three groups of 16); a diagonal B11 tile with an idle wave",
    (64, 64): "exactly half-empty both ways: two full 64 x 32 blocks (packed items)",
    (256, 256): "full tiles: no layout anywhere",
}
SETTINGS = {
    "narrow": dict(),
    "quadrants": dict(GAUSS_GRAM_ROTATE="0"),
    "narrow merged": dict(GAUSS_CHAIN_ASIDE="2", GAUSS_CHAIN_MERGED="2"),
    "i8": dict(GAUSS_GRAM_DTYPE="i8"),
}
ENV_KEYS = sorted({k for s in SETTINGS.values() for k in s})

_PANEL = {}


def _panel():
    if not _PANEL:
        from gauss_amd import panel as panel_mod
        rng = np.random.default_rng(2026)
        G = rng.integers(0, 3, size=(N_STORE, int(OFF[-1]))).astype(np.uint8)
        rows2, src_off = panel_mod.pack2bit(G, OFF)
        _PANEL.update(G=G, rows2=rows2, src_off=src_off, z=rng.standard_normal(N_STORE), w=np.array([0.2, 0.3, 0.5]))
    return _PANEL


def _rows(shape):
    """Two windows that share their M measured rows (the job-wide measured tiles then have the window's own edge) and take
    different unmeasured rows."""
    M, U = shape
    measured = np.arange(0, 2 * M, 2)
    rest = np.setdiff1d(np.arange(N_STORE), measured)
    return [(measured, rest[:U]), (measured, rest[U // 2 + 3:U // 2 + 3 + U])]


_WANT = {}


def _oracle(shape):
    if shape not in _WANT:
        import oracle
        p = _panel()
        _WANT[shape] = [oracle.run_impute(1, np.ascontiguousarray(p["G"][mi]), np.ascontiguousarray(p["G"][ui]), OFF, p["w"], p["z"][mi], want_mats=True)
                        for mi, ui in _rows(shape)]
    return _WANT[shape]


def _run(monkeypatch, capfd, setting, shape):
    from gauss_amd import hotpath
    p = _panel()
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("GAUSS_PLAN_FILL", "1")
    c = hotpath.Context(0)
    try:
        store = hotpath.RowStore(p["rows2"], ctx=c)
        wins = [dict(mode=1, pop_off=OFF, pop_wgt=p["w"], z1=p["z"][mi], dev=(store.ptr, store.ptr, len(mi), len(ui), store.ld),
                     packed=dict(fmt=1, rows_m=mi.astype(np.int32), rows_u=ui.astype(np.int32), pop_src_off=p["src_off"])) for mi, ui in _rows(shape)]
        capfd.readouterr()
        job = hotpath.Job(wins, ctx=c, on_device=True, want_mats=True)
        fill = [l for l in capfd.readouterr().err.split("\n") if l.startswith("[fill]")]
        job.run()
        out = [{k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in r.items()} for r in job.fetch()]
        job.close()
        store.close()
    finally:
        c.close()
    # items with a narrow layout, as the planner counted them (B11's and B21's lines)
    narrow = sum(int(l.split(" narrow)")[0].split()[-1]) for l in fill)
    return out, narrow


def _same(got, want, what):
    assert len(got) == len(want) == 2
    for i, (a, b) in enumerate(zip(got, want)):
        assert sorted(a) == sorted(b)
        for k in a:
            if isinstance(a[k], np.ndarray):
                assert np.array_equal(a[k], b[k], equal_nan=True), (what, i, k)
            else:
                assert a[k] == b[k], (what, i, k)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_narrow_layouts_give_the_quadrant_roles_bits(monkeypatch, capfd, shape):
    """z, info, status, B11 and B21 of a two-window job on the 2-bit store: the planner's layouts against GAUSS_GRAM_ROTATE=0
    bit for bit, in the default launch form and in the forced merged one (counted items), and the int8 kernel against both;
    both forms against the CPU oracle at the suite's usual bounds."""
    M, U = shape
    base, n0 = _run(monkeypatch, capfd, "quadrants", shape)
    assert n0 == 0
    for r in base:
        assert r["status"] == 0 and np.all(np.isfinite(r["z"])) and np.all(np.isfinite(r["info"]))
    for setting in ("narrow", "narrow merged"):
        got, n = _run(monkeypatch, capfd, setting, shape)
        # the layouts were on where the shape has a half-empty tile, and only there
        assert (n > 0) == (0 < M % 128 <= 64 or 0 < U % 128 <= 64), (shape, setting, n)
        _same(got, base, (shape, setting))
    i8, n8 = _run(monkeypatch, capfd, "i8", shape)
    assert n8 == 0
    _same(i8, base, (shape, "i8"))
    for r, want in zip(base, _oracle(shape)):
        assert np.max(np.abs(r["b11"] - want["b11"])) <= 1e-12
        assert np.max(np.abs(r["b21"] - want["b21"])) <= 1e-12
        assert np.max(np.abs(r["info"] - want["info"]) / np.abs(want["info"])) <= 1e-8
        assert np.max(np.abs(r["z"] - want["z"]) / np.maximum(1.0, np.abs(want["z"]))) <= 1e-8
