"""CPU: the definition of the leave-one-out values (closed form against brute-force deletion through the oracle) and the
plumbing a GPU-less machine can check -- the C ABI's window descriptor and its ctypes mirror, the host entry points."""
import ctypes
import os
import re

import numpy as np
import pytest

import oracle
from helpers import desc_layout, relerr, small_panel, split_window
from loo_ref import loo_by_deletion, loo_closed_form, window_b11

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Z_TOL = 1e-8        # the project's bar for z / info against the oracle (tests/test_gpu_parity.py)


def _zerr(got, want):
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


@pytest.mark.parametrize("lam", [0.1, 1e-3])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", [40, 60, 300])
def test_closed_form_equals_deletion(M, mode, lam):
    """The rank-one downdate is the reference's answer for the deleted SNP: every i of the window, both LD modes (the weighted
    oracle forms its LD row by row in Python: at M = 300 every tenth SNP is deleted there, 30 oracle calls instead of 300)."""
    p = small_panel(n_snp=M + 60, scale=0.02, seed=11 + M)
    gm, _, z1 = split_window(dict(G=p["G"][: M + 30]), M)
    w = p["w"] if mode else None
    b11 = window_b11(mode, gm, p["off"], w, lam)
    assert np.linalg.eigvalsh(b11).min() > 1e-5          # MakePosDef stays silent, on B11 and so on every principal submatrix
    cf = loo_closed_form(b11, z1)
    idx = np.arange(0, M, 10) if (mode == 1 and M >= 300) else np.arange(M)
    dl = loo_by_deletion(mode, gm, p["off"], w, z1, lam=lam, idx=idx)
    assert dl["mpd"] == 0
    assert relerr(cf["info"][idx], dl["info"]) <= Z_TOL
    assert _zerr(cf["z"][idx], dl["z"]) <= Z_TOL
    assert _zerr(cf["t"][idx], dl["t"]) <= Z_TOL
    assert cf["info"].min() > 1e-3                       # nothing here is ill-conditioned


def test_deletion_through_the_loop_literal_oracle_agrees():
    p = small_panel(n_snp=80, scale=0.02, seed=5)
    gm, _, z1 = split_window(dict(G=p["G"][:70]), 40)
    for mode in (0, 1):
        w = p["w"] if mode else None
        cf = loo_closed_form(window_b11(mode, gm, p["off"], w, 0.1), z1)
        dl = loo_by_deletion(mode, gm, p["off"], w, z1, run_impute=oracle.run_impute)
        assert relerr(cf["info"], dl["info"]) <= Z_TOL and _zerr(cf["z"], dl["z"]) <= Z_TOL and _zerr(cf["t"], dl["t"]) <= Z_TOL


def test_one_measured_snp():
    cf = loo_closed_form(np.array([[1.1]]), np.array([2.0]))
    assert cf["info"][0] == 0.0 and np.isnan(cf["z"][0]) and abs(cf["t"][0] - 2.0 / np.sqrt(1.1)) <= 1e-15


def test_host_header_declares_and_api_binds_the_two_calls():
    from gauss_amd import api
    src = open(os.path.join(ROOT, "include", "gauss_host.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("gauss_host_dist_loo", "gauss_host_distmix_loo"):
        assert re.search(r"\bint\s+%s\s*\(" % name, src), name
        assert name in api.HOST_SYMBOLS
    assert callable(api.dist_loo) and callable(api.distmix_loo)
    h = api.load_host()                                   # builds on a GPU-less machine too; the symbols must be exported
    assert h.gauss_host_dist_loo.argtypes == h.gauss_host_dist.argtypes
    assert h.gauss_host_distmix_loo.argtypes == h.gauss_host_distmix.argtypes


def test_window_descriptor_mirror_has_the_size_and_the_fields_of_the_header():
    from gauss_amd import _lib
    names = [f[0] for f in _lib.WindowDesc._fields_]
    assert names[-3:] == ["out_loo_z", "out_loo_info", "out_loo_t"]
    size, (off_z, off_t), _ = desc_layout(["out_loo_z", "out_loo_t"])
    assert ctypes.sizeof(_lib.WindowDesc) == size
    assert _lib.WindowDesc.out_loo_z.offset == off_z and _lib.WindowDesc.out_loo_t.offset == off_t


def test_zero_initialised_descriptor_asks_for_nothing():
    from gauss_amd import _lib
    d = _lib.WindowDesc()
    assert not d.out_loo_z and not d.out_loo_info and not d.out_loo_t
