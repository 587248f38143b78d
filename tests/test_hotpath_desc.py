"""CPU: what hotpath._Win builds, pinned field by field -- the window descriptor it fills, the buffers behind the descriptor's
pointers, and what result() makes of them -- against snapshots recorded before the constructor was taken apart
(tests/golden/hotpath_desc.json); the whole descriptor mirror against the header; and the roles Job gives the windows of a group.
_Win needs neither the library nor a GPU: it fills a ctypes struct."""
import copy
import ctypes as C
import json
import os

import numpy as np
import pytest

from helpers import desc_layout

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hotpath_desc.json")
M, U, N = 5, 7, 8
T = M + U
# the descriptor's pointers that the library reads: their record holds the contents, not the fill
INPUTS = {"pop_off", "pop_wgt", "z1", "z_more", "miss_more", "slct_forced", "xs_from_lead", "prs_s", "prs_lam", "lds_bp_m", "lds_bp_u",
          "lds_annot", "rows_m", "rows_u", "pop_src_off"}
VARIANTS = {"base": (False, False), "mats": (True, False), "dev": (False, True), "dev_mats": (True, True)}     # (want_mats, dev=)


def _scalar(v):
    """ints as they are, floats by repr (NaN and the last bit included)"""
    if isinstance(v, (bool, np.bool_)):
        return bool(v)
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    raise TypeError(f"not a scalar: {type(v)}")


def _root(a):
    while isinstance(a.base, np.ndarray):
        a = a.base
    return a


def _arrays(obj, found):
    """Every numpy array reachable from obj through attributes (of the window object itself), dicts, lists and tuples; a view
    counts as the array that owns its memory."""
    if isinstance(obj, np.ndarray):
        found[id(_root(obj))] = _root(obj)
    elif isinstance(obj, dict):
        for v in obj.values():
            _arrays(v, found)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            _arrays(v, found)
    return found


def _owner(arrays, addr):
    for a in arrays:
        lo = a.ctypes.data
        if lo <= addr < lo + max(a.nbytes, 1):
            return a
    return None


def _flat(res, prefix=""):
    """result() with its nested dicts (slct_raw, cs_raw) as dotted keys"""
    out = {}
    for k, v in res.items():
        if isinstance(v, dict):
            out.update(_flat(v, prefix + k + "."))
        else:
            out[prefix + k] = v
    return out


def _pointers(desc, win):
    """name -> (address, owning array or None) of every non-null pointer of the descriptor"""
    arrays = list(_arrays(vars(win), {}).values())
    out = {}
    for name, ctype in type(desc)._fields_:
        v = getattr(desc, name)
        if ctype is C.c_void_p:
            addr = v
        elif isinstance(v, C._Pointer):
            addr = C.cast(v, C.c_void_p).value
        else:
            continue
        if addr:
            out[name] = (addr, _owner(arrays, addr))
    return out


def snapshot(desc, win):
    """The descriptor as plain data: a scalar field is its value, a null pointer is left out, a pointer is the array of the window
    that owns the address -- the offset into it, its shape, dtype and first element (an input: its contents) and the result() keys
    that are that memory.  No attribute name of the window object appears: those are free to change."""
    ptrs = _pointers(desc, win)
    res = {k: v for k, v in _flat(win.result()).items() if isinstance(v, np.ndarray)}
    snap = {}
    for name, ctype in type(desc)._fields_:
        if name in ptrs:
            addr, a = ptrs[name]
            if a is None:                # a raw device address (dev=): nothing of the window owns it
                assert ctype is C.c_void_p, f"{name} points at memory the window does not keep alive"
                snap[name] = dict(raw=addr)
                continue
            rec = dict(o=addr - a.ctypes.data, s=list(a.shape), t=a.dtype.str, k=sorted(k for k, v in res.items() if _root(v) is a))
            if name in INPUTS:
                rec["v"] = [_scalar(x) for x in a.reshape(-1)]
            elif a.size:
                rec["f"] = _scalar(a.reshape(-1)[0])
            snap[name] = rec
        elif ctype is not C.c_void_p and not isinstance(getattr(desc, name), C._Pointer):
            snap[name] = _scalar(getattr(desc, name))
    return snap


def fake_fetch(desc, win):
    """What a fetch would do, without the library: index + 1 through every out_* pointer over its whole buffer (2 signals selected,
    1 study fitted, so that result() has something to trim)."""
    for name, (_, a) in _pointers(desc, win).items():
        if name.startswith("out_"):
            a.reshape(-1)[:] = {"out_slct_n": 2, "out_xs_n": 1}.get(name, np.arange(1, a.size + 1).astype(a.dtype))


def _value(v):
    if isinstance(v, dict):
        return {k: _value(x) for k, x in v.items()}
    if v is None:
        return None
    if not isinstance(v, np.ndarray):
        return _scalar(v)
    flat = v.reshape(-1)
    if flat.size > 2 and np.array_equal(flat, np.arange(1, flat.size + 1).astype(v.dtype)):
        body = "ramp"
    elif flat.size > 2 and all(_scalar(x) == _scalar(flat[0]) for x in flat):
        body = dict(all=_scalar(flat[0]))
    else:
        body = [_scalar(x) for x in flat]
    return dict(s=list(v.shape), t=v.dtype.str, v=body)


def _inputs(dev, extra):
    gm = (np.arange(M * N, dtype=np.uint8).reshape(M, N) * 7 % 3).astype(np.uint8)
    gu = (np.arange(U * N, dtype=np.uint8).reshape(U, N) * 5 % 3).astype(np.uint8)
    w = dict(mode=0, pop_off=[0, N], pop_wgt=None, z1=np.linspace(-2.0, 2.0, M), lam=0.1, min_abs_eig=1e-5)
    w.update(dev=(0x10000, 0x20000, M, U, 16)) if dev else w.update(geno_m=gm, geno_u=gu)
    w.update(copy.deepcopy(extra))
    return w


def record(make, case, want_mats, dev):
    """One case through make(desc, window, want_mats, xs) (hotpath._Win's signature): the snapshot, then result() after the
    fake fetch; a ValueError is recorded by its message."""
    from gauss_amd import _lib
    extra = dict(case)
    xs = extra.pop("xs", None)
    desc = _lib.WindowDesc()
    try:
        win = make(desc, _inputs(dev, extra), want_mats, xs)
    except ValueError as ex:
        return dict(error=str(ex))
    snap = snapshot(desc, win)
    fake_fetch(desc, win)
    return dict(desc=snap, result=_value(win.result()))


def _delta(base, rec):
    """What a variant's record changes in the base variant's (the fixture holds the base in full and the other three as this)"""
    if "error" in rec or "error" in base:
        return rec
    out = {}
    for part in ("desc", "result"):
        out[part] = {k: v for k, v in rec[part].items() if k not in base[part] or base[part][k] != v}
        out[part + "_gone"] = sorted(k for k in base[part] if k not in rec[part])
    return out


def _count(res):
    return sum(_count(v) if isinstance(v, dict) and set(v) != {"s", "t", "v"} else 1 for v in res.values())


def record_case(make, case):
    """-> (the fixture's entry of the case, the number of descriptor fields and result entries it compares)"""
    recs = {name: record(make, case, *how) for name, how in VARIANTS.items()}
    n_fields = sum(len(r.get("desc", ())) + _count(r.get("result", {})) + ("error" in r) for r in recs.values())
    return dict({name: _delta(recs["base"], r) for name, r in recs.items() if name != "base"}, base=recs["base"]), n_fields


def _z(rows, cols=M):
    return (np.arange(rows * cols, dtype=np.float64).reshape(rows, cols) - 3.0) / 4.0


def _mask(rows=3):
    m = np.zeros((rows, M), dtype=np.int64)
    m[0, 1] = m[-1, 0] = m[-1, 4] = 1
    return m


_SUSIE_ALL = dict(L=4, coverage=0.9, prior_var=16.0, tol=1e-3, max_sweeps=50, min_abs_corr=0.25, estimate_var=False, measured_only=True,
                  want_alpha=True, want_lbf=True)
_BP = dict(radius=1000, bp_m=np.arange(M) * 100, bp_u=np.arange(U) * 70 + 5, n=8.0)
# sizes that could be confused differ: M 5, U 7, T 12, N 8; slct max 3; L 4 (6 in a group); traits 2; groups of 2, 3, 4; grid 2 x 3
CASES = {
    "plain": dict(),
    "weighted": dict(mode=1, pop_off=[0, 3, N], pop_wgt=[0.75, 0.5], lam=0.25, min_abs_eig=1e-4),
    "loo": dict(loo=True),
    "slct": dict(slct=dict(max=3)),
    "slct_options": dict(slct=dict(max=3, chi2_stop=3.5, collin=0.8)),
    "slct_default_max": dict(slct=dict()),
    "slct_unmeasured": dict(slct=dict(max=3, unmeasured=True)),
    "slct_cs": dict(slct=dict(max=3, cs=dict())),
    "slct_cs_unmeasured": dict(slct=dict(max=3, collin=0.8, unmeasured=True, cs=dict(coverage=0.5, prior_var=9.0))),
    "slct_forced": dict(slct=dict(max=3, forced=[4, 1])),
    "slct_min_var_frac": dict(slct=dict(max=3, min_var_frac=0.125, min_var_frac_u=0.25, unmeasured=True)),
    "slct_min_var_frac_cs": dict(slct=dict(max=3, min_var_frac=0.125, min_var_frac_u=0.25, cs=dict())),
    "slct_negative_max": dict(slct=dict(max=-2, unmeasured=True, cs=dict())),
    "susie_defaults": dict(susie=dict()),
    "susie_options": dict(susie=_SUSIE_ALL),
    "susie_traits_coloc": dict(z_more=_z(3), susie=dict(L=4, traits=2, coloc=dict())),
    "susie_traits_coloc_options": dict(z_more=_z(3), susie=dict(_SUSIE_ALL, traits=2, coloc=dict(p1=1e-3, p2=2e-3, p12=1e-6))),
    "susie_traits_alone": dict(z_more=_z(3), susie=dict(L=4, traits=1)),
    "susie_coloc_alone": dict(susie=dict(L=4, coloc=dict())),
    "susie_traits_above_max": dict(z_more=_z(3), susie=dict(L=4, traits=9, coloc=dict())),
    "susie_traits_negative": dict(susie=dict(L=4, traits=-1)),
    "susie_L_above_max": dict(susie=dict(L=40, want_alpha=True)),
    "susie_L_negative": dict(susie=dict(L=-1)),
    "leader_of_2": dict(susie=dict(L=6, group=2, want_mu=True), xs=("leader", 2)),
    "leader_of_4": dict(susie=dict(L=6, group=2, want_mu=True), xs=("leader", 4)),
    "leader_of_6": dict(susie=dict(L=6, group=2, want_mu=True), xs=("leader", 6)),
    "leader_plain": dict(susie=dict(_SUSIE_ALL, L=6, group=7), xs=("leader", 3)),
    "leader_traits_coloc": dict(z_more=_z(3), susie=dict(L=6, group=1, traits=2, coloc=dict()), xs=("leader", 3)),
    "leader_from_lead": dict(susie=dict(L=6, group=2, from_lead=list(range(T))), xs=("leader", 2)),
    "group_without_a_role": dict(susie=dict(L=6, group=5, want_mu=True)),
    "peer_map": dict(susie=dict(_SUSIE_ALL, L=6, group=2, traits=1, from_lead=[0, 1, -1, 7, 2, 3, 4, 5, 6, -1, 8, 9]), xs=("peer", 3)),
    "peer_no_map": dict(susie=dict(group=2, coloc=dict(), want_mu=True), xs=("peer", 2)),
    "z_more": dict(z_more=_z(3)),
    "z_more_no_rows": dict(z_more=_z(0)),
    "z_more_miss": dict(z_more=_z(3), miss_more=_mask()),
    "z_more_miss_nothing": dict(z_more=_z(3), miss_more=np.zeros((3, M))),
    "prs_defaults": dict(prs=dict()),
    "prs_grid": dict(prs=dict(n=1000.0, s=[0.5, 1.0], lam=[0.1, 0.01, 0.001], tol=1e-3, max_sweeps=20)),
    "prs_grid_above_max": dict(prs=dict(n=50.0, s=np.linspace(0.1, 0.9, 9), lam=np.linspace(0.5, 0.01, 33))),
    "ld_1": dict(ld_codings=1),
    "ld_3": dict(ld_codings=3),
    "ld_7": dict(ld_codings=7),
    "ld_0": dict(ld_codings=0),
    "ld_with_riders": dict(ld_codings=1, loo=True, slct=dict(max=3)),
    "ldscore": dict(ldscore=_BP),
    "ldscore_empty": dict(ldscore=dict()),
    "ldscore_annot": dict(ldscore=dict(_BP, annot=_z(2, T))),
    "ldscore_annot_one_row": dict(ldscore=dict(_BP, annot=_z(1, T)[0])),
    "ldscore_annot_above_max": dict(ldscore=dict(_BP, annot=_z(33, T))),
    "ldscore_no_matrices": dict(ldscore=_BP, want_matrices=False),
    "ldscore_codings_3": dict(ldscore=_BP, ld_codings=3),
    "qcat": dict(qcat=(1, 3, 0.01)),
    "qcat_with_riders": dict(qcat=(1, 3, 0.01), loo=True, prs=dict(s=[0.5], lam=[0.1])),
    "packed": dict(packed=dict(fmt=1, rows_m=[9, 2, 4, 6, 8], rows_u=[1, 3, 5, 7, 10, 11, 12], pop_src_off=[0, N])),
    "packed_rows": dict(packed=dict(fmt=1, rows_m=[9, 2, 4], rows_u=[1, 3, 5, 7])),
    "packed_no_rows_u": dict(packed=dict(fmt=1, rows_m=[9, 2, 4]), loo=True, slct=dict(max=3, unmeasured=True)),
    "packed_format_only": dict(packed=dict()),
    "packed_ld": dict(packed=dict(fmt=1, rows_m=[9, 2, 4], rows_u=np.zeros(0, np.int32)), ld_codings=1),
    "loo_slct_traits_prs": dict(loo=True, slct=dict(max=3, unmeasured=True, cs=dict()), z_more=_z(3), miss_more=_mask(),
                                prs=dict(s=[0.5, 1.0], lam=[0.1, 0.01, 0.001])),
    "everything": dict(loo=True, slct=dict(max=3, forced=[2], unmeasured=True, cs=dict()), z_more=_z(3), susie=dict(_SUSIE_ALL, traits=2, coloc=dict()),
                       prs=dict(), unknown_key="ignored"),
    "error_row_stride": dict(geno_u=np.zeros((U, 2 * N), dtype=np.uint8)),
    "error_z_more_columns": dict(z_more=_z(3, M - 1)),
    "error_z_more_1d": dict(z_more=_z(1)[0]),
    "error_miss_more_without_z_more": dict(miss_more=_mask()),
    "error_miss_more_rows": dict(z_more=_z(3), miss_more=_mask(2)),
    "error_prs_no_s": dict(prs=dict(s=[])),
    "error_no_matrices_without_ldscore": dict(want_matrices=False),
    "error_no_matrices_ld": dict(ld_codings=1, want_matrices=False),
}


def dump(fixture, path):
    """sorted keys, one case per line"""
    with open(path, "w") as fh:
        fh.write("{\n" + ",\n".join(json.dumps(k) + ": " + json.dumps(fixture[k], sort_keys=True, separators=(",", ":"))
                                    for k in sorted(fixture)) + "\n}\n")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_fixture_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("name", sorted(CASES))
def test_win_builds_what_it_built(golden, name):
    """The descriptor, the buffers and result() of the case, in its four variants, are the recorded ones exactly"""
    from gauss_amd import hotpath
    got, _ = record_case(hotpath._Win, CASES[name])
    got = json.loads(json.dumps(got))                    # (tuples become lists, as in the fixture)
    want = golden[name]
    for variant in want:
        for part in want[variant]:
            assert got[variant][part] == want[variant][part], (name, variant, part)
    assert got == want


def test_the_cases_cover_what_they_claim(golden):
    """Every ValueError of the constructor, and every field of the descriptor set by some case"""
    errors = [golden[k]["base"]["error"] for k in golden if k.startswith("error_")]
    for text in ("must share a row stride", "z_more must be [T, 5]", "miss_more must be [", "prs_n_s = 0", "want_matrices=False is for an LD window"):
        assert any(text in e for e in errors), text
    assert not any("error" in golden[k]["base"] for k in golden if not k.startswith("error_"))
    assert "error" not in golden["error_row_stride"]["dev"]                  # (raw addresses have no stride to compare)
    from gauss_amd import _lib
    seen = set()
    for rec in golden.values():
        for variant in rec.values():
            seen.update(k for k, v in variant.get("desc", {}).items() if v not in (0, "0.0"))
    assert seen == {f[0] for f in _lib.WindowDesc._fields_}


def test_descriptor_mirror_has_the_size_and_every_offset_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    size, offs, _ = desc_layout(["lambda" if n == "lambda_" else n for n in names])        # (lambda is a keyword in Python)
    assert C.sizeof(_lib.WindowDesc) == size
    assert [getattr(_lib.WindowDesc, n).offset for n in names] == offs
    assert offs == sorted(offs) and len(set(offs)) == len(offs)


def test_job_gives_each_window_of_a_group_its_role():
    from gauss_amd import hotpath
    g = lambda group, **kw: dict(mode=0, susie=dict(L=3, group=group, **kw))
    wins = [dict(mode=0), g(1), g(2), dict(mode=0, susie=dict(L=3)), g(1, from_lead=[1, 0]), dict(mode=1, susie=None), g(2), g(1),
            g(3), g(3), g(3), g(3), dict(mode=0, susie=dict(L=3, group=0)), g(9)]
    before = copy.deepcopy(wins)
    roles = hotpath._xs_roles(wins)
    assert roles == [None, ("leader", 3), ("leader", 2), None, ("peer", 3), None, ("peer", 2), ("peer", 3),
                     ("leader", 4), ("peer", 4), ("peer", 4), ("peer", 4), None, ("leader", 1)]
    assert repr(wins) == repr(before)                    # the caller's dicts are as they came: no private key is written into them
    assert hotpath._xs_roles([]) == []
