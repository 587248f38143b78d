"""CPU suite: the host data layer of afmix() / cpw2() (gauss_host_popwgt_inputs) against a Python restatement of the reference's
steps 1-4 (ReadInputAf, ReadReferenceIndexAll, the measured list, the interval-major layout), on a text and a packed panel."""
import math
import os

import numpy as np
import pytest

from gauss_amd import api, panel

from popwgt_ref import build_x, make_panel, measured_list, pops_table, read_study

P = 6


@pytest.fixture(scope="module")
def setup(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("popwgt_host"))
    pn = make_panel(d, 400, pops_table(P), seed=3)
    packed = os.path.join(d, "pw_packed.bin")
    assert api.pack_panel(pn["paths"]["index.gz"], pn["paths"]["data.gz"], pn["paths"]["desc.txt"], packed) == 400
    rng = np.random.default_rng(9)
    rows = []
    for i in rng.choice(400, 300, replace=False):           # unsorted: the study lists SNPs in random order
        rsid, c, bp, a1, a2 = pn["snps"][i]
        af = float(rng.uniform(0.01, 0.99))
        if rng.random() < 0.2:
            a1, a2 = a2, a1                                   # swapped alleles: the panel's order is adopted, af -> 1 - af
        rows.append((f"st{i}", c, bp, a1, a2, af))
    for k in range(12):                                       # absent from the panel
        rows.append((f"abs{k}", 7, 3 + k, "A", "C", float(rng.uniform(0.1, 0.9))))
    rows = [rows[k] for k in rng.permutation(len(rows))]
    rep = next(r for r in rows if r[0].startswith("st"))
    rows.append((rep[0], *rep[1:5], 0.123456))               # a repeated key: the later row wins
    rsid, c, bp, a1, a2 = pn["snps"][int(rng.choice(400))]
    other = [b for b in "ACGT" if b not in (a1, a2)]
    rows.append(("other", c, bp, other[0], other[1], 0.4))   # same position, different alleles: not measured
    study = os.path.join(d, "study_af.txt")
    panel.write_study_af(study, *[[r[k] for r in rows] for k in range(6)])
    return dict(pn=pn, packed=packed, study=study, dir=d)


def _files(s, packed):
    p = s["pn"]["paths"]
    return (s["study"], p["index.gz"], s["packed"] if packed else p["data.gz"], p["desc.txt"])


@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("kind", [api.KIND_AFMIX, api.KIND_CPW2])
def test_inputs_match_the_restatement(setup, packed, kind, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    interval = 7
    df, x, off = api.popwgt_inputs(kind, *_files(setup, packed), interval=interval)
    want = measured_list(read_study(setup["study"]), setup["pn"]["snps"])
    assert len(want) > 250
    assert list(df["rsid"]) == [w[0] for w in want]
    assert list(df["bp"]) == [w[2] for w in want]
    assert list(df["a1"]) == [w[3] for w in want] and list(df["a2"]) == [w[4] for w in want]
    # the flipped 1 - af1 and the repeated key's later row, bit for bit
    assert np.array_equal(np.asarray(df["af1study"]), np.array([w[5] for w in want]))
    assert any(w[5] in (0.123456, 1 - 0.123456) for w in want)
    wx, woff = build_x(want, setup["pn"]["af"], interval, cpw2=(kind == api.KIND_CPW2))
    assert np.array_equal(off, woff)
    assert x.shape == wx.shape and x.tobytes() == wx.tobytes()


def test_text_and_packed_panels_give_the_same_bytes(setup, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    t = api.popwgt_inputs(api.KIND_CPW2, *_files(setup, False), interval=13)
    p = api.popwgt_inputs(api.KIND_CPW2, *_files(setup, True), interval=13)
    assert t[0].equals(p[0])
    assert t[1].tobytes() == p[1].tobytes() and np.array_equal(t[2], p[2])


def test_cpw2_transform_is_asin_sqrt_bit_for_bit(setup, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    _, xa, off = api.popwgt_inputs(api.KIND_AFMIX, *_files(setup, True), interval=5)
    _, xc, _ = api.popwgt_inputs(api.KIND_CPW2, *_files(setup, True), interval=5)
    want = np.array([[math.asin(math.sqrt(v)) for v in row] for row in xa])
    assert xc.tobytes() == want.tobytes()


def test_default_interval_is_1000(setup, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    with pytest.raises(api.GaussError, match=r"interval = 1000"):
        api.popwgt_inputs(api.KIND_AFMIX, *_files(setup, True), interval=None)
    with pytest.raises(api.GaussError, match=r"interval = 1000"):
        api.popwgt_inputs(api.KIND_AFMIX, *_files(setup, True), interval=0)


def test_fewer_measured_snps_than_interval_is_refused(setup, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    S = len(measured_list(read_study(setup["study"]), setup["pn"]["snps"]))
    with pytest.raises(api.GaussError, match=rf"{S} measured SNPs and interval = {S + 1}"):
        api.popwgt_inputs(api.KIND_AFMIX, *_files(setup, False), interval=S + 1)
    df, x, off = api.popwgt_inputs(api.KIND_AFMIX, *_files(setup, False), interval=S)
    assert len(df) == S and np.array_equal(np.diff(off), np.ones(S))


@pytest.mark.parametrize("packed", [False, True])
def test_both_orientations_in_the_study_are_refused(setup, packed, tmp_path, monkeypatch):
    monkeypatch.setenv("GAUSS_AUTO_PACK", "0")
    rsid, c, bp, a1, a2 = setup["pn"]["snps"][10]
    _, c2, bp2, b1, b2 = setup["pn"]["snps"][11]
    study = str(tmp_path / "dup.txt")
    panel.write_study_af(study, ["x", "y", "z"], [c, c, c2], [bp, bp, bp2], [a1, a2, b1], [a2, a1, b2], [0.2, 0.8, 0.5])
    p = setup["pn"]["paths"]
    files = (study, p["index.gz"], setup["packed"] if packed else p["data.gz"], p["desc.txt"])
    with pytest.raises(api.GaussError, match="ERROR: input file contains duplicates"):
        api.popwgt_inputs(api.KIND_AFMIX, *files, interval=1)
