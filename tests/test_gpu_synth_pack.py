"""The two kernels every benchmark figure stands on (k_misc.hip): synth_kernel, which writes the byte panel in HBM, and
pack2bit_kernel, which turns it into the resident 2-bit row store the timed jobs read.

The packer is compared bit for bit with panel.pack2bit on the same bytes.  The generator is compared cell by cell with its
fp64 restatement (tests/synth_ref.py; tests/test_synth_ref.py checks that one against the model): a cell may differ only
where a latent value lies within DELTA = 1e-3 of its threshold -- the kernel's float32 recurrence with __logf / __sincosf
stays well inside that (about 1e-4 at rho <= 0.99: a hundred steps of float32 roundoff and intrinsic error) -- and the inputs
are chosen so that at most 1 % of the cells are that close.  A wrong key, rho index or population lookup flips thousands of
cells.  Device buffers are prefilled with 0xA5 so that a byte written outside the panel shows."""
import ctypes as C

import numpy as np
import pytest

import synth_ref
from gauss_amd import hotpath
from gauss_amd import panel as panel_mod
from helpers import small_panel

pytestmark = pytest.mark.gpu

FILL = 0xA5
E_INVALID = -1
_ip = C.POINTER(C.c_int32)
_fp = C.POINTER(C.c_float)


class _Buf:
    """A device buffer of bytes from the HIP runtime the library itself is bound to.  (bench.py takes its buffers from torch,
    which it starts BEFORE the library, so that both share torch's runtime.  In this suite the session's context comes first;
    torch then maps a second copy of the runtime, and that copy finds no device.  The runtime's functions are therefore
    looked up through libgauss_hip.so's own handle, which searches the library's dependencies: whichever copy it is bound
    to, never the other.)"""
    _hip = None

    @classmethod
    def hip(cls):
        if cls._hip is None:
            h = hotpath._lib.load()
            h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
            h.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
            h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            h.hipFree.argtypes = [C.c_void_p]
            h.hipDeviceSynchronize.argtypes = []
            cls._hip = h
        return cls._hip

    def __init__(self, shape):
        self.shape = tuple(int(x) for x in shape)
        self.nbytes = int(np.prod(self.shape))
        p = C.c_void_p()
        assert self.hip().hipMalloc(C.byref(p), self.nbytes) == 0
        self.ptr = p.value

    def data_ptr(self):
        return self.ptr

    def fill(self, byte):
        assert self.hip().hipMemset(self.ptr, byte, self.nbytes) == 0
        assert self.hip().hipDeviceSynchronize() == 0       # the library works on streams of its own
        return self

    def put(self, a):
        a = np.ascontiguousarray(a, dtype=np.uint8)
        assert a.shape == self.shape
        assert self.hip().hipMemcpy(self.ptr, a.ctypes.data, self.nbytes, 1) == 0       # hipMemcpyHostToDevice
        assert self.hip().hipDeviceSynchronize() == 0
        return self

    def host(self):
        out = np.empty(self.shape, dtype=np.uint8)
        assert self.hip().hipDeviceSynchronize() == 0
        assert self.hip().hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0     # hipMemcpyDeviceToHost
        return out

    def __del__(self):
        if getattr(self, "ptr", None):
            self._hip.hipFree(self.ptr)
            self.ptr = None


def _filled(shape):
    return _Buf(shape).fill(FILL)


def _upload(a):
    return _Buf(np.shape(a)).put(a)


def _off(sizes):
    return synth_ref.pop_offsets(sizes)


def _pack_rc(ctx, d_in, ld_in, d_out, ld_out, n_snp, off, n_pop=None):
    return ctx.lib.gauss_pack2bit_device(ctx.handle, d_in, ld_in, d_out, ld_out, n_snp,
                                         None if off is None else off.ctypes.data_as(_ip), len(off) - 1 if n_pop is None else n_pop)


def _synth_rc(ctx, d_out, n_snp, ld, off, thr, rho, seed, n_pop=None):
    return ctx.lib.gauss_synth_device(ctx.handle, d_out, n_snp, ld, None if off is None else off.ctypes.data_as(_ip),
                                      len(off) - 1 if n_pop is None else n_pop, None if thr is None else thr.ctypes.data_as(_fp),
                                      None if rho is None else rho.ctypes.data_as(_fp), C.c_uint64(seed))


def _synth(ctx, n_snp, ld, off, thr, rho, seed, extra_rows=3):
    """The device generator's panel as a host array (n_snp + extra_rows, ld), the buffer prefilled with FILL."""
    out = _filled((n_snp + extra_rows, ld))
    thr = np.ascontiguousarray(thr, dtype=np.float32)
    rho = np.ascontiguousarray(rho, dtype=np.float32)
    hotpath.check(_synth_rc(ctx, out.data_ptr(), n_snp, ld, off, thr, rho, seed))
    return out.host()


# ------------------------------------------------------------------------------------------
# pack2bit_kernel
# ------------------------------------------------------------------------------------------
PACK_SIZES = {
    "edges": [1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257],      # around 4 samples a byte and 64 samples a block unit
    "one": [1],
    "seam": [1000, 70, 1029],             # blocks of 256 + 32 + 272 bytes: grid.y = 3, the first block ends ON byte 256, the
                                          # third lies across byte 512
    "straddle": [1030, 70, 1001],         # blocks of 272 + 32 + 256 bytes: the first lies across byte 256
}
ACROSS = {"seam": 512, "straddle": 256}   # a 256-byte seam of grid.y inside a block of the list
N_ROWS, EXTRA_ROWS, PAD_IN = 37, 3, 29


def _codes(kind, n_rows, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "ascii":
        return (rng.integers(0, 3, size=(n_rows, n)) + ord("0")).astype(np.uint8)
    return rng.integers(0, 4, size=(n_rows, n)).astype(np.uint8)


def _device_pack(ctx, G, off, ld_out, ld_in=None):
    """Rows G uploaded with stride ld_in (stride padding 0xFF: its low bits are 3) and packed on the device into a buffer
    of n_rows + EXTRA_ROWS rows prefilled with FILL; returns the whole buffer."""
    n_rows, n = G.shape
    ld_in = n + PAD_IN if ld_in is None else ld_in
    src = np.full((n_rows, ld_in), 0xFF, dtype=np.uint8)
    src[:, :n] = G
    d_in = _upload(src)
    d_out = _filled((n_rows + EXTRA_ROWS, ld_out))
    hotpath.check(_pack_rc(ctx, d_in.data_ptr(), ld_in, d_out.data_ptr(), ld_out, n_rows, off))
    return d_out.host()


@pytest.mark.parametrize("extra_out", [0, 48])
@pytest.mark.parametrize("kind", ["codes", "ascii"])
@pytest.mark.parametrize("pops", sorted(PACK_SIZES))
def test_device_packer_matches_host_packer_bit_for_bit(ctx, pops, kind, extra_out):
    sizes = PACK_SIZES[pops]
    off = _off(sizes)
    G = _codes(kind, N_ROWS, int(off[-1]), seed=len(sizes) + extra_out)
    want, src_off = panel_mod.pack2bit(G, off)
    total = want.shape[1]
    assert total == sum((m + 63) // 64 * 16 for m in sizes)
    if pops in ACROSS:
        assert any(a < ACROSS[pops] < b for a, b in zip(src_off, list(src_off[1:]) + [total]))
    got = _device_pack(ctx, G, off, total + extra_out)
    assert np.array_equal(got[:N_ROWS, :total], want)
    assert not got[:N_ROWS, total:].any()                       # bytes past the blocks are zero
    assert np.all(got[N_ROWS:] == FILL)                         # rows past n_snp are not touched
    codes = G & 3 if kind == "codes" else G - ord("0")
    assert np.array_equal(panel_mod.unpack2bit(got[:N_ROWS], sizes), codes)


def test_device_packer_with_the_tightest_input_stride(ctx):
    """ld_in == N: the last sample of a row is followed by the first of the next."""
    sizes = [5, 130, 3]
    off = _off(sizes)
    G = _codes("codes", N_ROWS, int(off[-1]), seed=3)
    want, _ = panel_mod.pack2bit(G, off)
    got = _device_pack(ctx, G, off, want.shape[1], ld_in=int(off[-1]))
    assert np.array_equal(got[:N_ROWS], want) and np.all(got[N_ROWS:] == FILL)


def test_job_over_device_packed_store_has_the_bits_of_host_packed_rows(ctx):
    p = small_panel(n_snp=130, scale=0.02, seed=17)
    G, off = p["G"][:110], p["off"]
    assert G.shape[0] == 110
    rng = np.random.default_rng(5)
    idx = rng.permutation(110)
    mi, ui = np.sort(idx[:70]).astype(np.int32), np.sort(idx[70:]).astype(np.int32)
    z1 = rng.standard_normal(70) * 2.0
    rows2, _ = panel_mod.pack2bit(G, off)
    ld2 = rows2.shape[1]

    def run(ptr):
        job = hotpath.Job([dict(mode=1, pop_off=off, pop_wgt=p["w"], z1=z1, dev=(ptr, ptr, 70, 40, ld2),
                                packed=dict(fmt=1, rows_m=mi, rows_u=ui))], ctx=ctx, on_device=True, want_mats=True)
        job.run()
        out = job.fetch()[0]
        job.close()
        return out

    ld_in = int(off[-1]) + PAD_IN
    src = np.full((110, ld_in), 0xFF, dtype=np.uint8)
    src[:, :off[-1]] = G
    d_in = _upload(src)
    d_store = _filled((110, ld2))
    hotpath.check(_pack_rc(ctx, d_in.data_ptr(), ld_in, d_store.data_ptr(), ld2, 110, off))
    assert np.array_equal(d_store.host(), rows2)
    got = run(d_store.data_ptr())
    store = hotpath.RowStore(rows2, ctx=ctx)
    want = run(store.ptr)
    store.close()
    assert np.all(np.isfinite(want["z"])) and np.ptp(want["z"]) > 0
    for k in ("z", "info", "b11", "b21"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert got["status"] == want["status"]


# ------------------------------------------------------------------------------------------
# synth_kernel
# ------------------------------------------------------------------------------------------
LD = 1024 + 64


@pytest.fixture(scope="module")
def exact(ctx):
    """The committed inputs (three populations, N = 1000, S = 48), the device panel and the fp64 reference, made once."""
    a = synth_ref.exact_inputs()
    a["N"] = int(a["off"][-1])
    a["buf"] = _synth(ctx, a["S"], LD, a["off"], a["thr"], a["rho"], a["seed"])
    a["G"], a["z0"], a["z1"], a["t"] = synth_ref.synth(a["S"], a["off"], a["thr"], a["rho"], a["seed"])
    a["buf"].setflags(write=False)
    a["G"].setflags(write=False)
    return a


def test_generator_matches_the_fp64_reference_away_from_the_thresholds(exact):
    S, N = exact["S"], exact["N"]
    got, want = exact["buf"][:S, :N], exact["G"]
    assert got.max() <= 2
    m = synth_ref.margin(exact["z0"], exact["z1"], exact["t"])
    near = m <= synth_ref.DELTA
    # a condition on the inputs (tests/test_synth_ref.py checks it without a GPU): few cells are next to a threshold
    assert near.mean() <= 0.01
    differ = got != want
    worst = float(m[differ].max()) if differ.any() else 0.0
    print(f"synth_kernel vs fp64: {int(differ.sum())} of {differ.size} cells differ, largest reference distance to a threshold "
          f"among them {worst:.3e}; {int(near.sum())} cells within {synth_ref.DELTA}")
    assert not (differ & ~near).any(), (int((differ & ~near).sum()), worst)
    # "zero or a handful": a cell can differ only if the kernel's error exceeds its margin.  With the error at most 1e-4 (the
    # estimate the comparison rests on) the model expects 48 000 cells * 2 latent values * 2e-4 * phi(thr) <= 0.4 -> at most 8
    # such cells, and 8 + 5 sqrt(8) < 24.
    assert differ.sum() <= 24


def test_generator_leaves_stride_padding_and_rows_past_n_snp_alone(exact):
    S, N = exact["S"], exact["N"]
    assert np.all(exact["buf"][:S, N:] == FILL)
    assert np.all(exact["buf"][S:] == FILL)


def test_generator_takes_each_sample_s_threshold_from_its_own_population(ctx, exact):
    """Thresholds of +-30 (every latent value below / none below), alternating by population and, per SNP, in the opposite
    phase: every byte is 0 or 2 by the population of its column, whatever the random numbers -- columns pop_off[k] - 1 and
    pop_off[k] included."""
    S, off, N = exact["S"], exact["off"], exact["N"]
    P = len(off) - 1
    sign = (-1.0) ** (np.arange(S)[:, None] + np.arange(P)[None, :])
    thr = (30.0 * sign).astype(np.float32)
    got = _synth(ctx, S, LD, off, thr, exact["rho"], exact["seed"])[:S, :N]
    want = np.repeat(np.where(sign > 0, 2, 0).astype(np.uint8), np.diff(off), axis=1)
    assert want[0, 299] == 2 and want[0, 300] == 0 and want[1, 299] == 0 and want[0, 556] == 0 and want[0, 557] == 2
    assert np.array_equal(got, want)


def test_generator_output_depends_only_on_seed_snp_and_sample(ctx, exact):
    S, off, N, thr, rho, seed = (exact[k] for k in ("S", "off", "N", "thr", "rho", "seed"))
    base = exact["buf"][:S, :N]
    # fewer SNPs: the first rows of the longer run; nothing written behind them
    short = _synth(ctx, 24, LD, off, thr[:24], rho[:24], seed)
    assert np.array_equal(short[:24, :N], base[:24]) and np.all(short[24:] == FILL) and np.all(short[:24, N:] == FILL)
    # another stride (the tightest one): the same bytes
    tight = _synth(ctx, S, N, off, thr, rho, seed)
    assert np.array_equal(tight[:S], base) and np.all(tight[S:] == FILL)
    # the same call again: the same bytes
    again = _synth(ctx, S, LD, off, thr, rho, seed)
    assert np.array_equal(again, exact["buf"])
    # another seed: another panel.  Two independent panels agree in a cell with probability sum_g P(g)^2 < 0.9 unless the
    # allele is rare; over these frequencies (0.02 .. 0.98) far more than 10 % of the cells differ
    other = _synth(ctx, S, LD, off, thr, rho, seed + 1)[:S, :N]
    assert (other != base).mean() > 0.10


def test_generator_with_equal_thresholds_ignores_the_population_split(ctx, exact):
    S, N, rho, seed = (exact[k] for k in ("S", "N", "rho", "seed"))
    t = exact["thr"][:, :1]
    panels = []
    for sizes in ([300, 257, 443], [1000], [1, 998, 1], [256, 256, 256, 232]):
        thr = np.ascontiguousarray(np.repeat(t, len(sizes), axis=1))
        panels.append(_synth(ctx, S, LD, _off(sizes), thr, rho, seed)[:S, :N])
    for g in panels[1:]:
        assert np.array_equal(g, panels[0])


def test_generator_repeats_the_latent_values_where_rho_is_one(ctx, exact):
    """rho[17] == 1: SNP 17 has the latent values of SNP 16, so with SNP 16's thresholds it has SNP 16's bytes."""
    S, off, N, rho, seed = (exact[k] for k in ("S", "off", "N", "rho", "seed"))
    assert rho[17] == 1.0
    thr = exact["thr"].copy()
    thr[17] = thr[16]
    got = _synth(ctx, S, LD, off, thr, rho, seed)[:S, :N]
    assert np.array_equal(got[17], got[16]) and np.array_equal(got[16], exact["buf"][16, :N])
    assert (got[18] != got[17]).any()


def test_generator_statistics_in_the_bench_regime(ctx):
    """rho 0.993 .. 0.9999, as between neighbouring SNPs of the benchmark's chromosome: the error of the float32 recurrence
    decays more slowly here, so the cell-by-cell rule is not applied; the panel must still have the model's frequencies
    (5 binomial standard errors) and the reference's LD between neighbours."""
    a = synth_ref.bench_regime_inputs()
    S, off = a["S"], a["off"]
    N = int(off[-1])
    got = _synth(ctx, S, N + 64, off, a["thr"], a["rho"], a["seed"])[:S, :N]
    assert got.max() <= 2
    za, zh = synth_ref.frequency_excess(got, off, a["thr"])
    want, _, _, _ = synth_ref.synth(S, off, a["thr"], a["rho"], a["seed"])
    r_got, r_want = synth_ref.adjacent_correlation(got, off), synth_ref.adjacent_correlation(want, off)
    print(f"bench regime: allele frequency within {np.max(np.abs(za)):.2f} se, heterozygotes within {np.max(np.abs(zh)):.2f} se, "
          f"adjacent-SNP correlation within {np.max(np.abs(r_got - r_want)):.2e} of the reference's, "
          f"{int((got != want).sum())} of {got.size} cells differ")
    assert np.max(np.abs(za)) <= 5.0
    assert np.max(np.abs(zh)) <= 5.0
    assert np.max(np.abs(r_got - r_want)) <= 0.03


# ------------------------------------------------------------------------------------------
# arguments that would put a kernel outside the caller's buffers are refused on the host
# ------------------------------------------------------------------------------------------
def _refused(ctx, rc, buf, word=None):
    assert rc == E_INVALID, rc
    msg = ctx.lib.gauss_last_error().decode()
    assert msg and (word is None or word in msg), msg
    assert np.all(buf.host() == FILL)                   # nothing was cleared or launched


def test_synth_device_refuses_bad_arguments(ctx):
    off = _off([30, 50, 20])
    S = 8
    thr = np.zeros((S, 3), dtype=np.float32)
    rho = np.full(S, 0.5, dtype=np.float32)
    buf = _filled((S + 1, 128))
    p = buf.data_ptr()
    _refused(ctx, _synth_rc(ctx, p, S, 99, off, thr, rho, 1), buf, "ld")                    # ld < N: rows would overlap and overrun
    _refused(ctx, _synth_rc(ctx, p, S, 0, off, thr, rho, 1), buf, "ld")
    _refused(ctx, _synth_rc(ctx, p, S, 128, np.array([0, 50, 30, 100], dtype=np.int32), thr, rho, 1), buf, "pop_off")
    _refused(ctx, _synth_rc(ctx, p, S, 128, np.array([-4, 30, 80, 100], dtype=np.int32), thr, rho, 1), buf, "pop_off")
    _refused(ctx, _synth_rc(ctx, None, S, 128, off, thr, rho, 1), buf)
    _refused(ctx, _synth_rc(ctx, p, S, 128, None, thr, rho, 1, n_pop=3), buf)
    _refused(ctx, _synth_rc(ctx, p, S, 128, off, None, rho, 1), buf)
    _refused(ctx, _synth_rc(ctx, p, S, 128, off, thr, None, 1), buf)
    _refused(ctx, _synth_rc(ctx, p, 0, 128, off, thr, rho, 1), buf)
    _refused(ctx, _synth_rc(ctx, p, S, 128, off, thr, rho, 1, n_pop=0), buf)
    assert ctx.lib.gauss_synth_device(None, p, S, 128, off.ctypes.data_as(_ip), 3, thr.ctypes.data_as(_fp), rho.ctypes.data_as(_fp),
                                      C.c_uint64(1)) == E_INVALID
    # and the same buffer takes a valid call: ld == N is the shortest stride there is
    hotpath.check(_synth_rc(ctx, p, S, 100, off, thr, rho, 1))
    flat = buf.host().reshape(-1)
    assert flat[:S * 100].max() <= 2 and np.all(flat[S * 100:] == FILL)


def test_pack2bit_device_refuses_bad_arguments(ctx):
    off = _off([30, 50, 20])                             # blocks of 16 bytes each: 48 in all
    S = 8
    d_in = _upload(np.ones((S, 100), dtype=np.uint8))
    buf = _filled((S + 1, 64))
    pi, po = d_in.data_ptr(), buf.data_ptr()
    _refused(ctx, _pack_rc(ctx, pi, 99, po, 48, S, off), buf, "ld_in")                      # ld_in < N: reads past the input
    _refused(ctx, _pack_rc(ctx, pi, 100, po, 56, S, off), buf, "ld_out")                    # not a multiple of 16
    _refused(ctx, _pack_rc(ctx, pi, 100, po, 32, S, off), buf, "ld_out")                    # below the block total
    _refused(ctx, _pack_rc(ctx, pi, 100, po, 0, S, off), buf, "ld_out")
    _refused(ctx, _pack_rc(ctx, pi, 100, po, 48, S, np.array([0, 50, 30, 100], dtype=np.int32)), buf, "pop_off")
    _refused(ctx, _pack_rc(ctx, pi, 100, po, 48, S, np.array([-4, 30, 80, 100], dtype=np.int32)), buf, "pop_off")
    _refused(ctx, _pack_rc(ctx, None, 100, po, 48, S, off), buf)
    _refused(ctx, _pack_rc(ctx, pi, 100, None, 48, S, off), buf)
    _refused(ctx, _pack_rc(ctx, pi, 100, po, 48, S, None, n_pop=3), buf)
    _refused(ctx, _pack_rc(ctx, pi, 100, po, 48, 0, off), buf)
    _refused(ctx, _pack_rc(ctx, pi, 100, po, 48, S, off, n_pop=0), buf)
    assert ctx.lib.gauss_pack2bit_device(None, pi, 100, po, 48, S, off.ctypes.data_as(_ip), 3) == E_INVALID
    hotpath.check(_pack_rc(ctx, pi, 100, po, 48, S, off))
    want, _ = panel_mod.pack2bit(np.ones((S, 100), dtype=np.uint8), off)
    flat = buf.host().reshape(-1)
    assert np.array_equal(flat[:S * 48].reshape(S, 48), want) and np.all(flat[S * 48:] == FILL)
