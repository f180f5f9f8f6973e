"""orbm_two_view_pose{,_device} and orbm_two_view_decide without a GPU: the header's declarations, the exports and the wrappers; the
refusals that come before any device call; the decision rules against the model's over an exhaustive grid of edge counts; and the
conditions that the scenes of tests/test_two_view_pose_gpu.py have to meet, asserted on the numpy model (tests/two_view_pose_model.py)
alone."""
import ctypes as C
import itertools

import numpy as np
import pytest

import two_view_pose_model as pm
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, built, declared, device_present, exported, flat, returns

NAMES = {"orbm_two_view_pose_device", "orbm_two_view_pose", "orbm_two_view_decide"}


@pytest.fixture(scope="module")
def matcher():
    return built("matcher")


def test_header_declares_the_entry_points_the_library_exports_them_and_the_wrappers_bind(matcher):
    assert NAMES <= declared("orbm_", "orbm.h")
    exported(NAMES)
    L = matcher._mlib()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert callable(matcher.ORBMatcher.TwoViewPoseDevice) and callable(matcher.ORBMatcher.TwoViewPose) and callable(matcher.two_view_decide)
    text = flat("include/orbm.h")
    # the two places where the reference is not followed literally, and the order of the hypotheses, are said where a caller reads them
    assert "push_backs the eight computed hypotheses BEHIND them" in text
    assert "the isfinite gate of :636 drops the match" in text
    assert "compare hypotheses by nearest (R, t), never by index" in text
    design = flat("DESIGN.md")
    assert "orbm_two_view_pose_device" in design and "never by index" in design


ARGS = ("h", "fx", "fy", "cx", "cy", "kps1", "n1", "kps2", "n2", "matches12", "pairs", "H", "F", "inl_H", "inl_F", "ransac_result", "family", "sigma",
        "min_parallax", "R21", "t21", "points3D", "triangulated", "matches12_out", "hyp_R", "hyp_t", "hyp_good", "hyp_parallax", "hyp_code", "result")
REQUIRED = ("kps1", "kps2", "matches12", "pairs", "H", "F", "inl_H", "inl_F", "ransac_result", "R21", "t21", "points3D", "triangulated",
            "matches12_out", "hyp_R", "hyp_t", "hyp_good", "hyp_parallax", "result")


def _call(L, device, **over):
    """one call with valid arguments (the fake pointer, never dereferenced: abi_checks' rule) except for `over`"""
    a = {k: P for k in ARGS}
    a.update(h=None, fx=460.0, fy=460.0, cx=376.0, cy=240.0, n1=100, n2=120, family=-1, sigma=1.0, min_parallax=1.0)
    a.update(over)
    vals = [a[k] for k in ARGS]
    return L.orbm_two_view_pose_device(*vals, None) if device else L.orbm_two_view_pose(*vals)


def _named(device):
    def call(L, **over):
        return _call(L, device, **over)
    call.__name__ = "orbm_two_view_pose" + ("_device" if device else "")
    return call


@pytest.mark.parametrize("device", [True, False])
def test_the_refusals_come_before_any_device_call(matcher, device):
    L = matcher._mlib()
    call = _named(device)
    inf, nan = float("inf"), float("nan")
    cases = [dict(n1=0), dict(n2=0), dict(n1=-1), dict(n2=-5), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=nan), dict(fx=0.0), dict(fx=-460.0),
             dict(fx=inf), dict(fx=nan), dict(fy=0.0), dict(fy=-1.0), dict(fy=inf), dict(fy=nan), dict(family=-2), dict(family=2)]
    cases += [{k: None} for k in REQUIRED]
    for over in cases:
        returns(E_ARG, call, L, **over)
    # more key points than the RANSAC ahead of it takes; an argument error wins over the limit
    returns(E_UNSUPPORTED, call, L, n1=65537)
    returns(E_UNSUPPORTED, call, L, n2=65537)
    returns(E_ARG, call, L, n1=65537, family=3)
    # the optional one may be NULL, the limits themselves are allowed: such a call passes every check
    for over in (dict(), dict(hyp_code=None), dict(family=0), dict(family=1), dict(n1=1, n2=1), dict(n1=65536, n2=65536), dict(min_parallax=0.0)):
        returns(E_NO_DEVICE, call, L, **over)


def test_the_decide_function_refuses_what_it_cannot_decide(matcher):
    L = matcher._mlib()
    g, p = np.zeros(8, np.int32), np.zeros(8, np.float32)
    w, mg, why = C.c_int32(7), C.c_int32(7), C.c_int32(7)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    ok = (0, vp(g), vp(p), 10, 1.0, C.byref(w), C.byref(mg), C.byref(why))
    for k, bad in ((0, -1), (0, 2), (1, None), (2, None), (3, -1), (5, None), (6, None), (7, None)):
        args = list(ok)
        args[k] = bad
        returns(E_ARG, L.orbm_two_view_decide, *args)
    assert (w.value, mg.value, why.value) == (7, 7, 7)


def test_every_wrapper_fails_loudly_without_a_gpu(matcher):
    if device_present():
        pytest.skip("needs a machine without a GPU")
    from monoorbslam3_amd import _lib
    with pytest.raises(_lib.OrbxError) as e:
        matcher.ORBMatcher()                     # the handle itself
    assert e.value.code == E_NO_DEVICE

    class NoHandle:                              # the wrappers behind a handle that could not exist
        _L, _h = matcher._mlib(), None

    class Fake:
        def data_ptr(self):
            return P

    m = matcher.ORBMatcher(handle=NoHandle())
    names = [k for k in REQUIRED] + ["hyp_code"]
    returns(E_NO_DEVICE, m.TwoViewPoseDevice, {k: Fake() for k in names}, 100, 120, pm.K4)
    sc = pm.make_scene(n=33, seed=5, t=pm.T_WIDE)
    from monoorbslam3_amd.extractor import KP_DTYPE
    k1, k2 = np.zeros(len(sc["xy1"]), KP_DTYPE), np.zeros(len(sc["xy2"]), KP_DTYPE)
    ransac = dict(pairs=sc["pairs"], H=sc["H"], F=sc["F"], inl_H=sc["inl_H"], inl_F=sc["inl_F"], result=sc["ransac_result"])
    returns(E_NO_DEVICE, m.TwoViewPose, k1, k2, sc["matches12"], ransac, pm.K4)


def _edge_counts(n_inlier):
    """nGood values around minGood of either family, 0.7 and 0.75 of a maximum, and the ends"""
    mg = {min(int(np.floor(0.6 * n_inlier)), 100), min(int(np.rint(0.6 * n_inlier)), 100)}
    out = {0, 1, n_inlier}
    for m in mg:
        out |= {m - 1, m, m + 1}
    return sorted(v for v in out if 0 <= v <= max(n_inlier, 1))


def test_min_good_over_every_inlier_count(matcher):
    """every nInlier in 0..200: minGood of both families is the model's, cvRound (to nearest, ties to even, of the DOUBLE product) for H and
    cvFloor for F.  An exact tie 0.6 * n = k + 0.5 would need 6 n = 10 k + 5, even = odd: no inlier count reaches one, so the whole range
    is what holds the rounding (the two families differ wherever the fraction of 0.6 * n is 0.6 or 0.8)."""
    differ = 0
    for n in range(201):
        for fam in (0, 1):
            assert matcher.two_view_decide(fam, [0] * 8, [0.0] * 8, n) == pm.decide(fam, [0] * 8, [0.0] * 8, n), (n, fam)
        h, f = matcher.two_view_decide(1, [0] * 8, [0.0] * 8, n)[1], matcher.two_view_decide(0, [0] * 8, [0.0] * 8, n)[1]
        assert h == min(int(np.rint(0.6 * n)), 100) and f == min(int(np.floor(0.6 * n)), 100)
        differ += h != f
    assert differ > 50


def test_decide_equals_the_models_decision_over_the_edge_grid(matcher):
    """both families: equal maxima in every position, counts around 0.7 * max, 0.75 * best and minGood, a parallax exactly at, just below
    and just above min_parallax"""
    one = np.float32(1.0)
    pars = [float(np.nextafter(one, np.float32(0))), 1.0, float(np.nextafter(one, np.float32(2))), 0.0]
    checked = 0
    for n_inlier in (0, 1, 5, 15, 50, 51, 85, 166, 167, 200):
        for mx in sorted(set(_edge_counts(n_inlier)) | {10, 20, 100, 101}):
            if mx < 0:
                continue
            near = sorted({0, int(np.floor(0.7 * mx)), int(np.floor(0.7 * mx)) + 1, int(np.floor(0.75 * mx)), int(np.ceil(0.75 * mx)),
                           max(int(np.ceil(0.75 * mx)) - 1, 0), mx - 1 if mx else 0, mx})
            # F: the maximum in every position, a second value in every other position
            for pos, other in itertools.product(range(4), near):
                for pos2 in range(4):
                    g = [0, 0, 0, 0]
                    g[pos2] = other
                    g[pos] = mx
                    for pw, po in itertools.product(pars, (0.0, 5.0)):
                        p = [po] * 4
                        p[pos] = pw
                        got = matcher.two_view_decide(0, g + [0] * 4, p + [0.0] * 4, n_inlier)
                        assert got == pm.decide(0, g + [0] * 4, p + [0.0] * 4, n_inlier), (0, g, p, n_inlier, got)
                        checked += 1
            # H: the best in every position, the second best in every other one, a third equal to the second
            for pos, pos2 in itertools.product(range(8), range(8)):
                for other in near:
                    g = [0] * 8
                    g[pos2] = other
                    g[(pos2 + 3) % 8] = other
                    g[pos] = mx
                    for pw in pars:
                        p = [5.0] * 8
                        p[pos] = pw
                        got = matcher.two_view_decide(1, g, p, n_inlier)
                        assert got == pm.decide(1, g, p, n_inlier), (1, g, p, n_inlier, got)
                        checked += 1
    print("decisions compared:", checked)
    # the first maximum wins in both families, the parallax test is strict for F and not for H
    assert matcher.two_view_decide(0, [9, 0, 9, 0], [5.0, 0, 5.0, 0], 10)[2] == 3          # two at the maximum: no clear winner
    assert matcher.two_view_decide(0, [0, 9, 0, 0], [0, 1.0, 0, 0], 10) == (-1, 6, 4)
    assert matcher.two_view_decide(1, [0, 9, 0, 0, 0, 0, 0, 0], [0, 1.0, 0, 0, 0, 0, 0, 0], 10) == (1, 6, 0)
    assert matcher.two_view_decide(1, [9, 9, 0, 0, 0, 0, 0, 0], [5.0] * 8, 10)[2] == 3     # the second best equals the best


@pytest.mark.parametrize("name", list(pm.SCENES))
def test_the_scenes_meet_their_conditions_on_the_model(name):
    """n1 != n2 and holes in matches12; the status intended; the decision does not change anywhere inside the band; the banded matches
    of every hypothesis are at most 2 % of the scene's inliers and never more than 4; the float32 model decides as the float64 one."""
    sc, m64, m32 = pm.scene_models(name)
    intended = pm.SCENES[name][1]
    assert len(sc["xy1"]) != len(sc["xy2"]) and (sc["matches12"] < 0).any()
    nb = [int(pm.banded(c, m64["th2"]).sum()) for c in m64["checks"]]
    print("%s: status %d, winner %d, nInlier %d, minGood %d, good %s, parallax %s, banded %s" % (
        name, m64["status"], m64["winner"], m64["n_inlier"], m64["min_good"], m64["good"], np.round(m64["parallax"], 3).tolist(), nb))
    assert intended is None or m64["status"] == intended
    assert m32["status"] == m64["status"]
    if m64["winner"] >= 0:
        k, er, et = pm.nearest(*m32["hyps"][m32["winner"]], m64["hyps"])
        assert k == m64["winner"]
    assert pm.decision_stable(m64)
    for b in nb:
        assert b <= 0.02 * m64["n_inlier"] and b <= 4, (name, nb, m64["n_inlier"])


def test_the_scenes_cover_what_the_issue_asks_for():
    models = {name: pm.scene_models(name) for name in pm.SCENES}
    assert {sc["n_matches"] for sc, _, _ in models.values()} >= {8, 9, 63, 64, 65, 300}
    assert {m64["status"] for _, m64, _ in models.values()} == {0, 2, 3, 4}            # status 1 is the RANSAC's refusal: the GPU test's
    assert {m64["family"] for _, m64, _ in models.values()} == {0, 1}
    winners = {m64["good"][m64["winner"]] for _, m64, _ in models.values() if m64["winner"] >= 0}
    assert winners >= {50, 51, 52}
    zero = [m64 for sc, m64, _ in models.values() if not sc["inl_F"].any() and not sc["inl_H"].any()]
    assert zero and all(m["good"] == [0] * 8 and not np.any(m["parallax"]) for m in zero)
