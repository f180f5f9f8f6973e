"""orbm_triangulate_matches{,_device} without a GPU: exports, the argument checks that run before any device call, and the sanity of
the numpy model (tests/triangulation_model.py) the GPU tests compare with: its float32 and float64 runs on the seeded clouds."""
import ctypes as C

import numpy as np
import pytest

import triangulation_model as tm

# (fisheye, matches, seed, baseline in m, mismatched octaves, column margin): the clouds of both test files.  The baselines are
# wide enough that only the N_FAR far points and wrong pairings come near the parallax limit: the GPU test excludes every match a
# 1e-4 relative move of a threshold re-decides, and 0.99998 * (1 + 1e-4) > 1 re-decides every parallax rejection.
CLOUDS = [(False, 8000, 21, 2.5, False, 40), (False, 8000, 22, 4.0, False, 40), (True, 8000, 24, 4.0, False, 150),
          (False, 8000, 25, 3.0, True, 40), (True, 8000, 26, 4.0, True, 150)]
FLIP_CAP = 0.005
HANDFUL = 5


@pytest.fixture(scope="module")
def mlib():
    import __graft_entry__ as g
    g.build()
    from monoorbslam3_amd import matcher
    return matcher._mlib(), matcher


ARGS = ("h", "cam", "scale", "scale_w", "scale_h", "R1", "t1", "R2", "t2", "kps1", "n1", "kps2", "desc2", "n2", "matches12", "sigma2",
        "n_levels", "max_sf", "cos", "chi2", "ratio", "n_points", "cap", "points", "valid", "normals", "mind", "maxd", "desc", "obs", "mp1",
        "mp2", "has1", "has2", "code", "result")


def _call(L, matcher, device, **over):
    """one call with valid arguments (fake, never dereferenced pointers) except for `over`"""
    a = {k: 0x1000 for k in ARGS}
    a.update(h=None, cam=matcher.ProjCamera.make((460.0, 460.0, 376.0, 240.0), (0.0, 752.0, 0.0, 480.0)), scale=None, scale_w=0, scale_h=0,
             n1=100, n2=120, sigma2=(C.c_float * 16)(*([1.0] * 16)), n_levels=8, max_sf=3.58, cos=0.99998, chi2=5.991, ratio=1.8, cap=500)
    a.update(over)
    vals = [a[k] for k in ARGS]
    vals[1] = C.byref(a["cam"]) if a["cam"] is not None else None
    vals[15] = C.cast(a["sigma2"], C.c_void_p) if a["sigma2"] is not None else None
    if device:
        return L.orbm_triangulate_matches_device(*vals, None)
    return L.orbm_triangulate_matches(*vals)


@pytest.mark.parametrize("device", [True, False])
def test_bad_arguments_are_rejected_before_any_device_call(mlib, device):
    L, matcher = mlib
    fish = matcher.ProjCamera.make((300.0, 300.0, 376.0, 240.0, 0.0, 0.0, 0.0, 0.0), (0.0, 752.0, 0.0, 480.0))
    bad_cam = matcher.ProjCamera.make((460.0, 460.0, 376.0, 240.0), (0.0, 752.0, 0.0, 480.0))
    bad_cam.model = 2
    cases = [dict(cam=None), dict(cam=bad_cam), dict(cam=fish), dict(cam=fish, scale=0x1000, scale_w=0, scale_h=480), dict(n1=-1), dict(n2=-1),
             dict(cap=-1), dict(n_levels=0), dict(n_levels=17), dict(sigma2=None), dict(desc2=0x1001), dict(desc=0x1002)]
    cases += [{k: None} for k in ("R1", "t1", "R2", "t2", "kps1", "kps2", "desc2", "matches12", "n_points", "points", "valid", "normals", "mind",
                                  "maxd", "desc", "obs", "mp1", "mp2", "has1", "has2", "result")]
    for over in cases:
        assert _call(L, matcher, device, **over) == -1, over
        assert L.orbx_last_error()


def test_valid_calls_fail_loudly_without_a_gpu(mlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    L, matcher = mlib
    for device in (True, False):
        assert _call(L, matcher, device) == -2 and b"no HIP device" in L.orbx_last_error()
        assert _call(L, matcher, device, n1=0, n2=0, code=None) == -2


def test_header_declares_both_entry_points(mlib):
    """test_abi.test_every_declared_symbol_is_exported then checks that the library exports them"""
    from test_abi import _declared
    assert {"orbm_triangulate_matches_device", "orbm_triangulate_matches"} <= set(_declared("orbm.h"))
    L, matcher = mlib
    assert L.orbm_triangulate_matches_device and L.orbm_triangulate_matches
    assert hasattr(matcher.ORBMatcher, "TriangulateMatchesDevice") and hasattr(matcher.ORBMatcher, "TriangulateMatches")


@pytest.mark.parametrize("fisheye,n,seed,baseline,mismatched,margin", CLOUDS)
def test_float32_model_against_float64(fisheye, n, seed, baseline, mismatched, margin):
    """The float32 and the float64 run agree on the gate code of all but 0.5 % of the matches, every gate rejects at least a
    handful in the float64 run -- the re-projection test of either key frame, and scale consistency on the clouds with
    mismatched octaves --, and the accepted points of both runs lie within 1e-4 of the distance to the current key frame of each
    other.  (The depth test of key frame 2 never fires alone on these clouds: a point behind camera 2 is behind camera 1 too.)"""
    cloud = tm.make_cloud(fisheye, n, seed, baseline, mismatched, margin)
    e32, e64 = tm.run_model(cloud), tm.run_model(cloud, np.float64)
    matched = e64["code"] >= 0
    assert matched.sum() == n and np.array_equal(e32["code"] >= 0, matched)
    flips = (e32["code"] != e64["code"]).sum()
    res = e64["result"]
    by_view = lambda g, v: int(((e64["all_code"] == g) & (e64["view"] == v)).sum())  # noqa: E731
    print("%s baseline %.1f mismatched %d: float64 result %s, float32 result %s, flips %d of %d; re-projection %d / %d, depth %d / %d" % (
        "fisheye" if fisheye else "pinhole", baseline, mismatched, res.tolist(), e32["result"].tolist(), flips, n, by_view(tm.REPROJ, 1),
        by_view(tm.REPROJ, 2), by_view(tm.NEGATIVE, 1), by_view(tm.NEGATIVE, 2)))
    assert flips <= FLIP_CAP * n
    # what the GPU test leaves out of its comparison stays under the same cap
    band = tm.threshold_band(cloud, e64, 0) | tm.threshold_band(cloud, e64, 1) | tm.threshold_band(cloud, e64, 2)
    print("re-decided by a 1e-4 relative move of a threshold: %d" % band.sum())
    assert (band | (e32["code"] != e64["code"])).sum() <= FLIP_CAP * n
    assert res[0] + res[2:].sum() == n and res[1] == 0
    assert res[0] >= 0.3 * n
    for g in (tm.ILLEGAL, tm.PARALLAX, tm.NEGATIVE, tm.REPROJ):
        assert res[g] >= HANDFUL, g
    # key frame 2's test only sees what key frame 1's let pass: it bites where the two octaves, hence the two bounds, differ
    assert by_view(tm.REPROJ, 1) >= HANDFUL and by_view(tm.REPROJ, 2) >= (HANDFUL if mismatched else 1)
    assert res[tm.ILLEGAL] == tm.N_NONFINITE
    if mismatched:
        assert res[tm.SCALE] >= HANDFUL
    # rows in ascending feature order, one per accepted match, behind n_points
    assert np.array_equal(e64["feat1"], np.flatnonzero(e64["code"] == 0))
    assert np.array_equal(e64["index"][e64["feat1"]], cloud["n_points"] + np.arange(res[0]))
    both = (e32["code"] == 0) & (e64["code"] == 0)
    r32, r64 = e32["index"][both] - cloud["n_points"], e64["index"][both] - cloud["n_points"]
    rel = np.linalg.norm(e32["points"][r32].astype(np.float64) - e64["points"][r64], axis=1) / e64["dist2"][r64]
    print("accepted points: largest |Pw32 - Pw64| / dist2 = %.3e" % rel.max())
    assert rel.max() < 1e-4
    assert (e64["min_dist"] < e64["dist2"]).all() and (e64["dist2"] < e64["max_dist"]).all()
    nn = np.linalg.norm(e64["normals"], axis=1)               # the mean of two unit vectors: cos(parallax / 2)
    assert (nn <= 1 + 1e-12).all() and (nn > 0.7).all()
