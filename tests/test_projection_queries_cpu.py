"""The query builders (orbm_project_{frame,frustum,fuse}_device, orbba_pose_drop_outliers_device) without a GPU: exports, the
argument checks that run before any device call, and the sanity of the numpy float32 model (tests/projection_model.py) the GPU
tests compare with, judged against the same formulas in float64 on the same seeded clouds."""
import ctypes as C

import numpy as np
import pytest

import projection_model as pm

CLOUDS = [(pm.FRAME, False, 5000, 11), (pm.FRAME, True, 4000, 12), (pm.FRUSTUM, False, 8000, 13), (pm.FRUSTUM, True, 6000, 14),
          (pm.FUSE, False, 6000, 15), (pm.FUSE, True, 3000, 16)]
EXCLUDED_CAP = 0.005


@pytest.fixture(scope="module")
def mlib():
    import __graft_entry__ as g
    g.build()
    from monoorbslam3_amd import matcher
    return matcher._mlib(), matcher


def _call(L, matcher, form, **over):
    """one builder call with valid arguments (fake, never dereferenced device pointers) except for `over`"""
    a = dict(h=None, cam=matcher.ProjCamera.make((460.0, 460.0, 376.0, 240.0), (0.0, 752.0, 0.0, 480.0)), R=0x1000, t=0x1000, points=0x1000,
             valid=0x1000, kps1=0x1000, normals=0x1000, mind=0x1000, maxd=0x1000, nq=100, frame_mp=0x1000, n2=50,
             sf=(C.c_float * 16)(*([1.0] * 16)), n_levels=8, log_sf=0.18, th=3.0, xy=0x1000, radius=0x1000, level=0x1000, angle=0x1000,
             ok=0x1000, vcos=None, result=0x1000)
    a.update(over)
    cam = C.byref(a["cam"]) if a["cam"] is not None else None
    sf = C.cast(a["sf"], C.c_void_p) if a["sf"] is not None else None
    if form == pm.FRAME:
        return L.orbm_project_frame_device(a["h"], cam, a["R"], a["t"], a["points"], a["valid"], a["kps1"], a["nq"], a["th"], a["xy"],
                                           a["radius"], a["level"], a["angle"], a["ok"], a["result"], None)
    if form == pm.FRUSTUM:
        return L.orbm_project_frustum_device(a["h"], cam, a["R"], a["t"], a["points"], a["valid"], a["normals"], a["mind"], a["maxd"],
                                             a["nq"], a["frame_mp"], a["n2"], sf, a["n_levels"], a["log_sf"], a["th"], 0.5, a["xy"],
                                             a["radius"], a["level"], a["ok"], a["vcos"], a["result"], None)
    return L.orbm_project_fuse_device(a["h"], cam, a["R"], a["t"], a["points"], a["valid"], a["normals"], a["mind"], a["maxd"], a["nq"],
                                      sf, a["n_levels"], a["log_sf"], a["th"], a["xy"], a["radius"], a["level"], a["ok"], a["result"], None)


@pytest.mark.parametrize("form", [pm.FRAME, pm.FRUSTUM, pm.FUSE])
def test_bad_arguments_are_rejected_before_any_device_call(mlib, form):
    L, matcher = mlib
    E_ARG = -1
    bad_cam = matcher.ProjCamera.make((460.0, 460.0, 376.0, 240.0), (0.0, 752.0, 0.0, 480.0))
    bad_cam.model = 2
    cases = [dict(nq=-1), dict(cam=bad_cam), dict(cam=None), dict(R=None), dict(t=None), dict(points=None), dict(valid=None), dict(xy=None),
             dict(radius=None), dict(level=None), dict(ok=None), dict(result=None)]
    if form == pm.FRAME:
        cases += [dict(kps1=None), dict(angle=None)]
    else:
        cases += [dict(n_levels=17), dict(n_levels=0), dict(sf=None), dict(normals=None), dict(mind=None), dict(maxd=None)]
    if form == pm.FRUSTUM:
        cases += [dict(frame_mp=None), dict(n2=-1)]
    for over in cases:
        assert _call(L, matcher, form, **over) == E_ARG, over
        assert L.orbx_last_error()
    # the ABI struct is the header's: int32 + 12 floats
    assert C.sizeof(matcher.ProjCamera) == 52


def test_drop_outliers_arguments(mlib):
    L, _ = mlib
    fn = L.orbba_pose_drop_outliers_device
    fn.restype, fn.argtypes = C.c_int, [C.c_int] + [C.c_void_p] * 5
    assert fn(-1, 0x1000, 0x1000, 0x1000, 0x1000, None) == -1
    for k in range(4):
        ptrs = [0x1000] * 4
        ptrs[k] = None
        assert fn(10, *ptrs, None) == -1, k


def test_valid_calls_fail_loudly_without_a_gpu(mlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    L, matcher = mlib
    for form in (pm.FRAME, pm.FRUSTUM, pm.FUSE):
        assert _call(L, matcher, form) == -2 and b"no HIP device" in L.orbx_last_error()
    fn = L.orbba_pose_drop_outliers_device
    fn.restype, fn.argtypes = C.c_int, [C.c_int] + [C.c_void_p] * 5
    assert fn(10, 0x1000, 0x1000, 0x1000, 0x1000, None) == -2


def test_headers_declare_the_four_entry_points():
    """test_abi.test_every_declared_symbol_is_exported then checks that the library exports them"""
    from test_abi import _declared
    assert {"orbm_project_frame_device", "orbm_project_frustum_device", "orbm_project_fuse_device"} <= set(_declared("orbm.h"))
    assert "orbba_pose_drop_outliers_device" in _declared("orbba.h")


@pytest.mark.parametrize("form,fisheye,n,seed", CLOUDS)
def test_float32_model_against_float64(form, fisheye, n, seed):
    """Every gate decision of the float32 model equals the float64 evaluation's except within the stated distances of a
    threshold (projection_model.TOL_*); the level agrees except where x = log(max_dist / dist) / log_scale_factor is within 1e-4 of
    an integer; the excluded points are at most 0.5 % of the cloud.  Expected share of the level exclusion for distances spread over
    a decade: 2e-4 x the unclamped fraction, about 0.02 %; the N_ON_BOUND candidates on the image bounds add 12 / n."""
    cloud = pm.make_cloud(form, fisheye, n, seed)
    e32, e64 = pm.run_model(cloud), pm.run_model(cloud, np.float64)
    near = pm.near_threshold(form, cloud, e64)
    res = e32["result"]
    print("%s %s n=%d result %s on-bound %d" % (form, "fisheye" if fisheye else "pinhole", n, res.tolist(), cloud["on_bound"].sum()))
    # the cloud exercises every gate: each rejects at least 2 %, at least 30 % pass
    n_gates = {pm.FRAME: 3, pm.FRUSTUM: 6, pm.FUSE: 5}[form]
    assert res[0] >= 0.30 * n and (res[1:1 + n_gates] >= 0.02 * n).all() and res[:1 + n_gates].sum() == n
    which = cloud["on_bound_which"][cloud["on_bound"][:pm.N_ON_BOUND]]
    assert (which % 2 == 0).any() and (which % 2 == 1).any(), "no point exactly on a lower and on an upper image bound"
    if form == pm.FRUSTUM:
        fm = cloud["frame_mp"]
        assert ((fm >= n) | (fm < -1)).sum() >= 20 and ((fm >= 0) & (fm < n)).sum() >= 0.05 * n
        assert res[7] == res[3:7].sum()
    gate_near = near["depth"] | near["image"] | near.get("dist", False) | near.get("angle", False)
    differs = e32["code"] != e64["code"]
    assert not (differs & ~gate_near).any(), "a gate decision flips away from every threshold"
    excluded = gate_near.copy()
    both = (e32["code"] == 0) & (e64["code"] == 0)
    assert np.abs(e32["q_xy"][both] - e64["q_xy"][both]).max() < pm.TOL_PIXEL
    if form != pm.FRAME:
        lv = both & (e32["q_level"] != e64["q_level"])
        assert not (lv & ~near["level"]).any() and (np.abs(e32["q_level"] - e64["q_level"])[both] <= 1).all()
        excluded |= near["level"]
        same = both & ~lv
        if form == pm.FRUSTUM:
            excluded |= near["radius_class"]
            same &= ~near["radius_class"]
            assert np.abs(e32["view_cos"][both] - e64["view_cos"][both]).max() < pm.TOL_COS
        assert np.allclose(e32["q_radius"][same], e64["q_radius"][same], rtol=1e-6, atol=0)
        unclamped = ((e64["x_level"] > 0) & (e64["x_level"] < pm.N_LEVELS - 1)).mean()
        print("level exclusion %.4f %% (expected about %.4f %%)" % (100 * near["level"].mean(), 100 * 2 * pm.TOL_LEVEL * unclamped))
    share = excluded.mean()
    print("excluded %d of %d = %.3f %%; decisions that differ: %d" % (excluded.sum(), n, 100 * share, differs.sum()))
    assert share <= EXCLUDED_CAP
