"""The two restatements of the fuse's hit handling in tests/fuse_model.py against each other, the refusals, and the properties the
scenes were engineered for.  No GPU and no part of the library."""
import numpy as np
import pytest

import fuse_model as fm

_cache = {}


def scene(name):
    if name not in _cache:
        _cache[name] = fm.make_scene(**fm.SCENES[name])
    return _cache[name]


def _same(a, b, sc):
    for key in ("slots", "valid", "found", "code", "refresh_sel", "result"):
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key


@pytest.mark.parametrize("form", ["rows", "by_row"])
@pytest.mark.parametrize("name", sorted(fm.SCENES))
def test_the_array_form_and_the_objects_agree(name, form):
    """slots, validity, found counters, codes, d_refresh_sel and d_result of the header's array form equal what the MapPoint / KeyFrame
    objects are left with, with an explicit row list and with entry j = row j; the scene holds what it was built for"""
    sc = scene(name) if form == "rows" else fm.by_row(scene(name))
    a, b = fm.apply(sc), fm.apply_objects(sc)
    print(name, form, "d_result", a["result"].tolist(), "codes", np.bincount(a["code"], minlength=8).tolist())
    _same(a, b, sc)
    fm.check_scene(sc, a)
    assert (a["slots"] != sc["slots"]).any() and (a["valid"] != sc["valid"]).any() and (a["found"] != sc["found"]).any()


@pytest.mark.parametrize("name", sorted(fm.SCENES))
def test_without_the_counters_and_with_a_spoilt_csr(name):
    """d_found / d_visible absent changes nothing else; unusable CSR entries and broken offsets of rows without an observation only
    add to d_result[7]; the fresh CSR has no list the undone rule would catch"""
    sc = scene(name)
    a = fm.apply(sc)
    b = fm.apply(dict(sc, found=None, visible=None))
    assert b["found"] is None and all(np.array_equal(a[k], b[k]) for k in ("slots", "valid", "code", "refresh_sel", "result"))
    csr = fm.fresh_csr(sc)
    c = fm.apply(sc, csr)
    _same(a, c, sc)
    spoilt, junk = fm.spoil_csr(sc, csr, 5)
    d = fm.apply(sc, spoilt)
    assert junk > 20 and d["result"][fm.R_DROPPED] == a["result"][fm.R_DROPPED] + junk
    assert all(np.array_equal(a[k], d[k]) for k in ("slots", "valid", "found", "code", "refresh_sel")) and np.array_equal(a["result"][:7], d["result"][:7])


def test_a_list_over_1024_entries_leaves_the_replace_undone():
    sc = scene("small")
    j = sc["expect"]["occupant_loses"][0][0]
    p = int(sc["rows"][j])
    off, kf, kp = fm.long_csr(fm.fresh_csr(sc), p)                       # row p's list: its own entries and 1025 unusable ones
    assert off[p + 1] - off[p] > fm.LONG and fm.lists_of_rows_kept(fm.fresh_csr(sc), (off, kf, kp), p)
    a, b = fm.apply(sc), fm.apply(sc, (off, kf, kp))
    assert a["code"][j] == fm.OCCUPANT_REPLACED and b["code"][j] == fm.UNDONE and b["refresh_sel"][j] == -1 and b["valid"][p]
    assert b["result"][fm.R_MATCHES] == a["result"][fm.R_MATCHES] and b["result"][fm.R_OCCUPANT_REPLACED] == a["result"][fm.R_OCCUPANT_REPLACED] - 1
    assert b["result"][fm.R_DROPPED] == a["result"][fm.R_DROPPED] + 1 + 1025


@pytest.mark.parametrize("name", sorted(fm.SCENES))
def test_the_refusals_are_found_on_the_arrays_as_passed(name):
    sc = scene(name)
    assert fm.refusal(sc) == 0
    for want, bad_scene in fm.refusal_scenes(sc).items():
        out = fm.apply(bad_scene)
        assert out["result"].tolist() == [0, want, 0, 0, 0, 0, 0, 0] and out["code"] is None and out["refresh_sel"] is None
        assert np.array_equal(out["slots"], bad_scene["slots"]) and np.array_equal(out["valid"], bad_scene["valid"])
        assert np.array_equal(out["found"], bad_scene["found"])
    both = dict(fm.refusal_scenes(sc)[2], rows=fm.refusal_scenes(sc)[1]["rows"])
    assert fm.refusal(both) == 1                                         # a row twice wins
