"""CPU: what the LD-only functions of hotpath hand to the library, pinned argument by argument -- the C symbol, every scalar, where
every pointer points (an input, a returned buffer, a returned scalar) and what comes back -- against a record made before their
source arguments became one object (tests/golden/hotpath_ld_calls.json).  The functions need neither the library nor a GPU to
marshal a call: the context here is a stub whose `lib` records (symbol, arguments) and returns 0."""
import ctypes as C
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hotpath_ld_calls.json")
HANDLE, DEV_PTR, STORE_PTR = 0x5EED, 0x7E0000001000, 0x7E0000A02000
S, N, T, G = 6, 8, 2, 2                 # SNPs; samples, in populations of 5 and 3; traits; genes of 3 SNPs
# every input is contiguous and of its final dtype: no conversion copies it, so a pointer into it is "this input + offset"
INPUTS = dict(
    geno=(np.arange(S * N).reshape(S, N) * 7 % 3).astype(np.uint8),
    geno2=(np.arange(S * 32).reshape(S, 32) * 11 % 251).astype(np.uint8),          # 2-bit rows: two blocks of 16 bytes
    pop_off=np.array([0, 5, N], dtype=np.int32), pop_wgt=np.array([0.75, 0.5]), pop_src_off=np.array([0, 16], dtype=np.int32),
    rows=np.array([4, 1, 5, 0, 3, 2], dtype=np.int32), bp=np.arange(S, dtype=np.int32) * 100 + 7,
    key=np.linspace(1.0, 30.0, S), key2=np.linspace(1.0, 30.0, T * S).reshape(T, S),
    z=np.linspace(-2.0, 3.0, S), z2=np.linspace(-2.0, 3.0, T * S).reshape(T, S),
    gene_off=np.array([0, 3, S], dtype=np.int32), pop_group=np.array([0, 0], dtype=np.int32),
    draw_pop=np.array([1, 0, 0, 1, 0], dtype=np.int32), draw_sample=np.array([2, 4, 0, 1, 3], dtype=np.int32),
    bp_short=np.arange(S - 1, dtype=np.int32), z_short=np.linspace(0.0, 1.0, S - 1), z3d=np.zeros((1, T, S)),
    draw_short=np.array([1, 0], dtype=np.int32),
)
U8, BIT2 = 0, 1                         # GAUSS_GENO_U8, GAUSS_GENO_2BIT


class _Arg(str):
    """the name of an input, of the store stub or of the raw pair in a case's argument list"""


def _i(name):
    return _Arg(name)


# the source forms of a `_rows` function: (store, rows, fmt, pop_src_off)
FORMS = {
    "u8_all": (_i("geno"), None, U8, None),
    "u8_rows": (_i("geno"), _i("rows"), U8, None),
    "2bit": (_i("geno2"), _i("rows"), BIT2, _i("pop_src_off")),
    "store": (_i("STORE"), _i("rows"), BIT2, None),
    "raw": (_i("RAW"), _i("rows"), BIT2, _i("pop_src_off")),
}
PO, PW = _i("pop_off"), _i("pop_wgt")


def _cases():
    """name -> (function, positional arguments, keyword arguments)"""
    c = {}
    # the byte-matrix forms: once with defaults, once with every argument given by position
    c["ld_matrix"] = ("ld_matrix", [_i("geno"), PO], {})
    c["ld_matrix_all"] = ("ld_matrix", [_i("geno"), PO, PW, 0, 1.25], {})
    c["ld_clump"] = ("ld_clump", [_i("geno"), PO, _i("bp"), _i("key")], {})
    c["ld_clump_all"] = ("ld_clump", [_i("geno"), PO, _i("bp"), _i("key2"), PW, 0, 1234, 0.25, 9.5, 3.5], {})
    c["ld_split"] = ("ld_split", [_i("geno"), PO, _i("bp")], {})
    c["ld_split_all"] = ("ld_split", [_i("geno"), PO, _i("bp"), PW, 0, 1234, 0.03, 2, 4, 3, 0.4], {})
    c["ld_hess"] = ("ld_hess", [_i("geno"), PO, _i("z")], {})
    c["ld_hess_all"] = ("ld_hess", [_i("geno"), PO, _i("z2"), PW, 0, 5, 1e-3, False], {})
    c["ld_hess_vectors"] = ("ld_hess", [_i("geno"), PO, _i("z2"), PW, 0, 5, 1e-3, True], {})
    c["gene_ld_batch"] = ("gene_ld_batch", [_i("geno"), PO, _i("gene_off")], {})
    c["gene_ld_batch_all"] = ("gene_ld_batch", [_i("geno"), PO, _i("gene_off"), PW, 1, 1.25], {})
    c["gene_sumchi2"] = ("gene_sumchi2", [_i("geno"), PO, _i("gene_off"), _i("z")], {})
    c["gene_sumchi2_all"] = ("gene_sumchi2", [_i("geno"), PO, _i("gene_off"), _i("z2"), PW, 0, 0.8], {})
    c["ld_per_pop"] = ("ld_per_pop", [_i("geno"), PO], {})
    c["zmix_normal_eq"] = ("zmix_normal_eq", [_i("geno"), PO, _i("z")], {})
    c["zmix_normal_eq_groups"] = ("zmix_normal_eq", [_i("geno"), PO, _i("z"), _i("pop_group")], {})
    # the row forms, every argument by position, over the source forms; rows=None where the function takes it
    for form, (store, rows, fmt, so) in FORMS.items():
        if rows is not None:
            c[f"ld_matrix_rows.{form}"] = ("ld_matrix_rows", [store, rows, PO, PW, 0, 1.25, fmt, so], {})
            c[f"gene_ld_batch_rows.{form}"] = ("gene_ld_batch_rows", [store, rows, PO, _i("gene_off"), PW, 1, 1.25, fmt, so], {})
        c[f"ld_clump_rows.{form}"] = ("ld_clump_rows", [store, rows, PO, _i("bp"), _i("key2"), PW, 0, 1234, 0.25, 9.5, 3.5, fmt, so], {})
        c[f"ld_split_rows.{form}"] = ("ld_split_rows", [store, rows, PO, _i("bp"), PW, 0, 1234, 0.03, 2, 4, 3, 0.4, fmt, so], {})
        c[f"ld_hess_rows.{form}"] = ("ld_hess_rows", [store, rows, PO, _i("z2"), PW, 0, 5, 1e-3, False, fmt, so], {})
        c[f"ld_hess_rows_vectors.{form}"] = ("ld_hess_rows", [store, rows, PO, _i("z"), PW, 1, 5, 1e-3, True, fmt, so], {})
        c[f"ld_resampled.{form}"] = ("ld_resampled", [store, rows, PO, _i("draw_pop"), _i("draw_sample"), 7, 1.25, fmt, so], {})
        c[f"gene_sumchi2_rows.{form}"] = ("gene_sumchi2_rows", [store, rows, PO, _i("gene_off"), _i("z2"), PW, 0, 0.8, fmt, so], {})
    # the row forms with their defaults (a 2-bit store, weighted, no source offsets)
    c["ld_matrix_rows"] = ("ld_matrix_rows", [_i("geno2"), _i("rows"), PO], {})
    c["ld_clump_rows"] = ("ld_clump_rows", [_i("geno2"), _i("rows"), PO, _i("bp"), _i("key")], {})
    c["ld_split_rows"] = ("ld_split_rows", [_i("geno2"), _i("rows"), PO, _i("bp")], {})
    c["ld_hess_rows"] = ("ld_hess_rows", [_i("geno2"), _i("rows"), PO, _i("z")], {})
    c["ld_resampled"] = ("ld_resampled", [_i("geno2"), _i("rows"), PO, _i("draw_pop"), _i("draw_sample"), 7], {})
    c["gene_ld_batch_rows"] = ("gene_ld_batch_rows", [_i("geno2"), _i("rows"), PO, _i("gene_off")], {})
    c["gene_sumchi2_rows"] = ("gene_sumchi2_rows", [_i("geno2"), _i("rows"), PO, _i("gene_off"), _i("z")], {})
    # what each raises for a bad shape, in both members of a pair
    c["error_clump_bp"] = ("ld_clump", [_i("geno"), PO, _i("bp_short"), _i("key")], {})
    c["error_clump_key"] = ("ld_clump", [_i("geno"), PO, _i("bp"), _i("z_short")], {})
    c["error_clump_key_3d"] = ("ld_clump_rows", [_i("geno"), _i("rows"), PO, _i("bp"), _i("z3d")], dict(fmt=U8))
    c["error_clump_rows_bp"] = ("ld_clump_rows", [_i("geno"), None, PO, _i("bp_short"), _i("key")], dict(fmt=U8))
    c["error_split_bp"] = ("ld_split", [_i("geno"), PO, _i("bp_short")], {})
    c["error_split_rows_bp"] = ("ld_split_rows", [_i("geno2"), _i("rows"), PO, _i("bp_short")], {})
    c["error_hess_z"] = ("ld_hess", [_i("geno"), PO, _i("z_short")], {})
    c["error_hess_rows_z_3d"] = ("ld_hess_rows", [_i("STORE"), _i("rows"), PO, _i("z3d")], {})
    c["error_resampled_draws"] = ("ld_resampled", [_i("geno2"), _i("rows"), PO, _i("draw_pop"), _i("draw_short"), 7], {})
    c["error_sumchi2_z"] = ("gene_sumchi2", [_i("geno"), PO, _i("gene_off"), _i("z_short")], {})
    c["error_sumchi2_rows_z_3d"] = ("gene_sumchi2_rows", [_i("RAW"), _i("rows"), PO, _i("gene_off"), _i("z3d")], {})
    c["error_ld_matrix_rows_no_rows"] = ("ld_matrix_rows", [_i("geno"), None, PO], dict(fmt=U8))
    c["error_gene_ld_batch_rows_no_rows"] = ("gene_ld_batch_rows", [_i("geno"), None, PO, _i("gene_off")], dict(fmt=U8))
    c["error_zmix_z"] = ("zmix_normal_eq", [_i("geno"), PO, _i("z_short")], {})
    return c


CASES = _cases()
SYMBOLS = {"gauss_ld", "gauss_ld_rows", "gauss_ld_clump_rows", "gauss_ld_split_rows", "gauss_ld_hess_rows", "gauss_ld_resampled_rows",
           "gauss_gene_ld_batch", "gauss_gene_ld_batch_rows", "gauss_gene_sumchi2", "gauss_gene_sumchi2_rows", "gauss_ld_per_pop",
           "gauss_zmix_normal_eq"}


def _scalar(v):
    """ints as they are, floats by repr (NaN and the last bit included)"""
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    raise TypeError(f"not a scalar: {type(v)}")


class _Lib:
    """Every attribute is a C entry point that records its call and returns 0.  poke: {argument index: value} written through
    those pointer arguments, as the library would write a result."""

    def __init__(self, poke=()):
        self.calls, self.poke = [], dict(poke)

    def __getattr__(self, symbol):
        def call(*args):
            self.calls.append((symbol, args))
            for k, v in self.poke.items():
                a = args[k]
                if isinstance(a, C._Pointer):
                    a[0] = type(a[0])(v)
                else:                                   # C.byref(x)
                    a._obj.value = type(a._obj.value)(v)
            return 0
        return call


class _Ctx:
    def __init__(self, poke=()):
        self.lib, self.handle = _Lib(poke), HANDLE


def _address(a):
    """the address a pointer argument holds; None for an argument that is no pointer object"""
    if isinstance(a, C._Pointer):
        return C.cast(a, C.c_void_p).value or 0
    if type(a).__name__ == "CArgObject":               # C.byref(x)
        return C.addressof(a._obj)
    return None


def _root(a):
    while isinstance(a.base, np.ndarray):
        a = a.base
    return a


def _flat(res, prefix=""):
    """the returned value as {path: leaf}: a dict by its keys, a list or tuple by [index]"""
    if isinstance(res, dict):
        items = [(str(k), v) for k, v in res.items()]
    elif isinstance(res, (list, tuple)):
        items = [(f"[{k}]", v) for k, v in enumerate(res)]
    else:
        return {prefix.rstrip("."): res}
    out = {}
    for k, v in items:
        out.update(_flat(v, prefix + k + "."))
    return out


def _inside(arrays, addr):
    """(name, byte offset) of the array that holds the address"""
    for name, a in arrays.items():
        lo = _root(a).ctypes.data
        if lo <= addr < lo + max(_root(a).nbytes, 1):
            return name, addr - a.ctypes.data
    return None


def _value(v):
    if v is None:
        return None
    if not isinstance(v, np.ndarray):
        return _scalar(v)
    flat = v.reshape(-1)
    body = dict(all=_scalar(flat[0])) if flat.size > 1 and all(_scalar(x) == _scalar(flat[0]) for x in flat) else [_scalar(x) for x in flat]
    return dict(s=list(v.shape), t=v.dtype.str, v=body)


def _run(fn, args, kwargs, poke=()):
    from gauss_amd import hotpath
    store = hotpath.RowStore.__new__(hotpath.RowStore)           # a resident store without a device: its pointer and its stride
    store.ptr, store.ld = STORE_PTR, 48
    special = dict(STORE=store, RAW=(DEV_PTR, 64))
    ctx = _Ctx(poke)
    real = [special[a] if a in special else INPUTS[a] if isinstance(a, _Arg) else a for a in args]
    try:
        res = getattr(hotpath, fn)(*real, **kwargs, ctx=ctx)
    finally:
        store.ptr = None
    assert len(ctx.lib.calls) == 1, f"{fn} made {len(ctx.lib.calls)} library calls"
    return ctx.lib.calls[0], res


def record(fn, args, kwargs):
    """One case as plain data: the symbol; per argument a scalar, "NULL", ["in", input, offset(, dtype, shape of the array handed
    over)], ["ret", path, offset] or ["ret_scalar", path]; and what is returned.  A scalar that the library returns through a pointer
    into memory the caller never sees (n_pos, yty, ...) is found by a second run whose stub writes a marker there."""
    try:
        (symbol, cargs), res = _run(fn, args, kwargs)
    except (ValueError, TypeError) as ex:
        return dict(error=[type(ex).__name__, str(ex)])
    flat = _flat(res)
    returned = {k: v for k, v in flat.items() if isinstance(v, np.ndarray)}
    out, lost = [], {}
    for k, a in enumerate(cargs):
        addr = _address(a)
        if addr is None and isinstance(a, int) and _inside(INPUTS, a):          # a raw address (matrix.ctypes.data)
            addr = a
        if a is None or addr == 0:
            out.append("NULL")
        elif addr is None:
            out.append(_scalar(a))
        elif _inside(INPUTS, addr):
            rec = ["in", *_inside(INPUTS, addr)]
            arr = getattr(a, "_arr", None)
            out.append(rec + [arr.dtype.str, list(arr.shape)] if isinstance(arr, np.ndarray) else rec)
        elif _inside(returned, addr):
            out.append(["ret", *_inside(returned, addr)])
        else:
            lost[k] = 7001 + k
            out.append(None)
    if lost:
        _, res2 = _run(fn, args, kwargs, lost)
        flat2 = _flat(res2)
        for k, marker in lost.items():
            hits = [p for p, v in flat2.items() if not isinstance(v, np.ndarray) and v is not None and v == marker]
            assert len(hits) == 1, f"{fn}: argument {k} of {symbol} points at nothing the caller gave or gets ({hits})"
            out[k] = ["ret_scalar", hits[0]]
    return dict(symbol=symbol, args=out, ret={p: _value(v) for p, v in flat.items()})


def dump(fixture, path):
    """sorted keys, one case per line"""
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(fixture[k], sort_keys=True, separators=(",", ":"))
                                    for k in sorted(fixture)) + "\n}\n")


def record_all(path=GOLDEN):
    """The recorder: run once, before the functions change."""
    dump({name: record(*case) for name, case in CASES.items()}, path)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_call_is_what_it_was(golden, name):
    """The symbol, every argument and the returned value of the case are the recorded ones exactly"""
    got = json.loads(json.dumps(record(*CASES[name])))          # (tuples become lists, as in the fixture)
    want = golden[name]
    for part in want:
        assert got.get(part) == want[part], (name, part)
    assert got == want


def test_the_cases_cover_what_they_claim(golden):
    """Every C symbol of the LD-only calls, every source form of every row function, and every ValueError for a bad shape"""
    assert {rec["symbol"] for rec in golden.values() if "symbol" in rec} == SYMBOLS
    assert all(("error" in rec) == name.startswith("error_") for name, rec in golden.items())
    for fn in ("ld_clump_rows", "ld_split_rows", "ld_hess_rows", "ld_hess_rows_vectors", "ld_resampled", "gene_sumchi2_rows"):
        assert {f"{fn}.{form}" for form in FORMS} <= set(golden), fn
    for fn in ("ld_matrix_rows", "gene_ld_batch_rows"):
        assert {f"{fn}.{form}" for form in FORMS if form != "u8_all"} <= set(golden), fn
    errors = [golden[k]["error"] for k in golden if k.startswith("error_")]
    assert all(kind == ("TypeError" if name.endswith("_no_rows") else "ValueError") for name, (kind, _) in
               ((k, golden[k]["error"]) for k in golden if k.startswith("error_")))
    for text in ("bp has shape (5,) and key (6,)", "and key (5,)", "and key (1, 2, 6)", "bp has shape (5,): expected (6,)",
                 "z_traits has shape (1, 5)", "z_traits has shape (1, 2, 6)", "draw_pop has 5 entries, draw_sample 2",
                 "z has shape (5,): expected (6,) or (T, 6)", "z has shape (1, 2, 6)", "z has shape (5,), expected (6,)", "has no len()"):
        assert any(text in msg for _, msg in errors), text
    # no pointer of any call is left unexplained, and every input array is handed over somewhere
    seen = set()
    for rec in golden.values():
        for a in rec.get("args", ()):
            assert a is not None
            if isinstance(a, list) and a[0] == "in":
                seen.add(a[1])
    assert seen == set(INPUTS) - {"bp_short", "z_short", "z3d", "draw_short"}

