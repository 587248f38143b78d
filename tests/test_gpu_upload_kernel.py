"""GPU: where a row store's bytes land when its chunks travel by the copy kernel (k_misc.hip: h2d_copy_kernel through
gauss_store.cpp: upload_rows(..., by_kernel = true)), at a size whose launches run the kernel's unrolled loop.

launch_h2d_copy gives a launch min(512, ceil(n16 / 256)) workgroups of 256 lanes, each lane moving 16-byte words a grid stride
apart, UN = 4 of them per turn of the unrolled loop and one per turn of the tail loop: the unrolled loop runs only in a launch of
more than 3 * 512 * 256 words (6 MB), which of all callers only a row store's 32 MB chunks are.  The store here is one full chunk
and a last one of 8 MB and a bit; every row is random and no two are alike, so a word that landed anywhere but in its place changes
some LD entry of its row."""
import numpy as np
import pytest

import oracle
from gauss_amd import _lib, hotpath

pytestmark = pytest.mark.gpu

N_ROWS, LD = 2563, 16389                     # 42 005 007 bytes of one-byte codes
CHUNK = 32 << 20                             # UPLOAD_CHUNK (gauss_job.h)
UN, STRIDE = 4, 512 * 256                    # h2d_copy_kernel's unroll, and its grid stride in words at 512 workgroups
LD_TOL = 1e-12


def _chunks(total):
    """(offset, length, words of the 16-byte body, offset at which every lane has left the unrolled loop) of every chunk."""
    out = []
    for off in range(0, total, CHUNK):
        n = min(CHUNK, total - off)
        n16 = n // 16
        assert (n16 + 255) // 256 >= 512                     # the launch has its 512 workgroups: the stride is STRIDE
        # lane i's unrolled turns end at the first i + 4 k STRIDE with i + (4 k + 3) STRIDE >= n16; when the words left over by
        # whole turns of the grid are at most 3 STRIDE, that is the same k for every lane: the tail loop moves all the rest
        turns = n16 // (UN * STRIDE)
        assert n16 - turns * UN * STRIDE <= (UN - 1) * STRIDE
        out.append((off, n, n16, off + 16 * turns * UN * STRIDE))
    return out


@pytest.fixture(scope="module")
def rows():
    G = np.random.default_rng(20261).integers(0, 3, size=(N_ROWS, LD), dtype=np.uint8)
    G.setflags(write=False)
    return G


def _ld_of(store, ctx):
    return hotpath.ld_matrix_rows(store, np.arange(N_ROWS, dtype=np.int32), np.array([0, LD], dtype=np.int32), None,
                                  hotpath.MODE_POOLED, 1.0, fmt=_lib.GENO_U8, ctx=ctx)


def test_rows_land_in_place_by_copy_kernel_and_by_dma(ctx, rows, monkeypatch):
    total = rows.nbytes
    assert total == N_ROWS * LD and 40 << 20 <= total <= 48 << 20 and total % 16 != 0
    assert np.all(rows.min(1) != rows.max(1)) and len(np.unique(rows[:, :64], axis=0)) == N_ROWS
    chunks = _chunks(total)
    assert [c[1] for c in chunks] == [CHUNK, total - CHUNK] and chunks[1][1] >= 8 << 20
    for off, n, n16, handover in chunks:
        assert n16 > (UN - 1) * STRIDE                        # some lane's first unrolled turn is inside the body: the loop runs
        assert off < handover <= off + 16 * n16
    assert chunks[0][3] == CHUNK and CHUNK < chunks[1][3] < total - 16

    ld = {}
    sync = hotpath.RowStore(rows, ctx=ctx)
    try:
        ld["sync"] = _ld_of(sync, ctx)
    finally:
        sync.close()
    for name, flag in (("dma", "0"), ("kernel", "1")):
        monkeypatch.setenv("GAUSS_UPLOAD_BY_KERNEL", flag)      # read when the upload starts
        st = hotpath.RowStore(rows, ctx=ctx, asynchronous=True)
        try:
            assert st._host is rows or np.shares_memory(st._host, rows)     # alive until wait(0) has returned
            st.wait(0)
            ld[name] = _ld_of(st, ctx)
        finally:
            st.close()
    monkeypatch.delenv("GAUSS_UPLOAD_BY_KERNEL")

    for name in ("dma", "kernel"):
        bad = ld[name] != ld["sync"]
        assert not bad.any(), (name, int(bad.sum()), np.flatnonzero(bad.any(1))[:8])
    assert np.isfinite(ld["sync"]).all()

    # the oracle on 64 rows: the ends, the rows around the chunk boundary and around every hand-over to the tail loop, random ones
    pick = {0, N_ROWS - 1}
    for off, n, n16, handover in chunks:
        for b in (off, handover, off + 16 * n16):
            for r in ((b - 1) // LD - 1, (b - 1) // LD, b // LD, b // LD + 1):
                if 0 <= r < N_ROWS:
                    pick.add(int(r))
    assert {CHUNK // LD - 1, CHUNK // LD, CHUNK // LD + 1} <= pick and len(pick) < 40
    rng = np.random.default_rng(5)
    while len(pick) < 64:
        pick.add(int(rng.integers(0, N_ROWS)))
    pick = np.array(sorted(pick))
    want = oracle.ld_pooled(np.ascontiguousarray(rows[pick]), np.array([0, LD], dtype=np.int32), 1.0)
    for name, m in ld.items():
        got = m[np.ix_(pick, pick)]
        assert np.max(np.abs(got - want)) <= LD_TOL, (name, float(np.max(np.abs(got - want))))
        assert np.all(np.diag(m) == 1.0)
