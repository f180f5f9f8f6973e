"""orbm_refresh_points_device / orbm_scene_median_depth_device without a GPU: exports, the argument checks that run before any
device call, and the sanity of the numpy model (tests/refresh_model.py) the GPU tests compare with: its float32 run against its
float64 run on the seeded scenes, its medoid against the reference's loops, its median against a sort."""
import ctypes as C

import numpy as np
import pytest

import refresh_model as rm
from test_abi import _defines

SCENES = [(41, 12), (42, 3), (43, 40)]   # (seed, key frames)
U = 2.0 ** -24                           # unit roundoff of float


@pytest.fixture(scope="module")
def mlib():
    import __graft_entry__ as g
    g.build()
    from monoorbslam3_amd import matcher
    return matcher._mlib(), matcher


R_ARGS = ("h", "kf", "sel", "n_sel", "points", "valid", "cap", "normals", "mind", "maxd", "desc", "obs_off", "obs_kf", "obs_kp", "n_obs",
          "ref_kf", "max_sf", "kf_self", "covis", "result")
KF_FIELDS = ("d_pose_R", "d_pose_t", "d_bad", "d_kps", "d_desc", "d_n")
M_ARGS = ("h", "n_kf", "R", "t", "slots", "n", "stride", "points", "cap", "cur", "median", "count", "baseline")


def _refresh(L, matcher, kf_over=None, **over):
    """one call with valid arguments (fake, never dereferenced pointers) except for `over`"""
    kf = matcher.KfTable(20, *([0x1000] * 6))
    for k, v in (kf_over or {}).items():
        setattr(kf, k, v)
    a = {k: 0x1000 for k in R_ARGS}
    a.update(h=None, kf=C.byref(kf), n_sel=100, cap=500, n_obs=3000, max_sf=3.58, kf_self=3)
    a.update(over)
    return L.orbm_refresh_points_device(*[a[k] for k in R_ARGS], None)


def _median(L, **over):
    a = {k: 0x1000 for k in M_ARGS}
    a.update(h=None, n_kf=20, stride=2000, cap=500, cur=19)
    a.update(over)
    return L.orbm_scene_median_depth_device(*[a[k] for k in M_ARGS], None)


def test_bad_arguments_are_rejected_before_any_device_call(mlib):
    L, matcher = mlib
    cases = [dict(kf=None), dict(n_sel=-1), dict(cap=-1), dict(n_obs=-1), dict(desc=0x1002), dict(kf_over=dict(n_kf=-1)),
             dict(kf_over=dict(d_desc=0x1004)), dict(kf_over=dict(d_kps=0x1001))]
    cases += [{k: None} for k in ("sel", "points", "valid", "normals", "mind", "maxd", "desc", "obs_off", "obs_kf", "obs_kp", "ref_kf", "result")]
    cases += [dict(kf_over={k: None}) for k in KF_FIELDS]
    for over in cases:
        assert _refresh(L, matcher, **over) == -1, over
        assert L.orbx_last_error()
    cases = [dict(n_kf=-1), dict(stride=-1), dict(cap=-1), dict(cur=20), dict(cur=21)]
    cases += [{k: None} for k in ("R", "t", "slots", "n", "points", "median", "count")]
    for over in cases:
        assert _median(L, **over) == -1, over
        assert L.orbx_last_error()
    # the limit on stride: stated in the header, at least ORBV_MAX_FEATURES, refused above it
    limit = _defines("orbm.h", "ORBM_MEDIAN_MAX_")["stride"]
    assert limit >= 8192
    assert _median(L, stride=limit + 1) == -4 and b"ORBM_MEDIAN_MAX_STRIDE" in L.orbx_last_error()


def test_valid_calls_fail_loudly_without_a_gpu(mlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    L, matcher = mlib
    assert _refresh(L, matcher) == -2 and b"no HIP device" in L.orbx_last_error()
    assert _refresh(L, matcher, n_sel=0, sel=None, covis=None) == -2
    limit = _defines("orbm.h", "ORBM_MEDIAN_MAX_")["stride"]
    assert _median(L) == -2 and b"no HIP device" in L.orbx_last_error()
    assert _median(L, stride=limit, cur=-1, baseline=None) == -2 and _median(L, n_kf=0, cur=-1) == -2


def test_header_declares_both_entry_points(mlib):
    """test_abi.test_every_declared_symbol_is_exported then checks that the library exports them"""
    from test_abi import _declared
    assert {"orbm_refresh_points_device", "orbm_scene_median_depth_device"} <= set(_declared("orbm.h"))
    L, matcher = mlib
    assert L.orbm_refresh_points_device and L.orbm_scene_median_depth_device
    assert hasattr(matcher.ORBMatcher, "RefreshPointsDevice") and hasattr(matcher.ORBMatcher, "SceneMedianDepthDevice")
    assert C.sizeof(matcher.KfTable) == 56 and matcher.KfTable.d_pose_R.offset == 8 and matcher.KfTable.d_n.offset == 48


@pytest.mark.parametrize("seed,n_kf", SCENES)
def test_float32_model_against_float64(seed, n_kf):
    """A sanity check of the yardstick, not a tolerance for the kernel (which must equal the float32 model bit for bit).
    With u = 2^-24 and a = the largest sum_i |R_ik t_i| / |Pw - O_k| of a row (`amp`): the camera centre carries 3 roundings of terms
    of size <= sum_i |R_ik t_i|, so v = Pw - O is off by (3 a + 1) u relative to its length; the norm adds 2.5 u, the division 1 u: a
    unit direction is off by at most (3 a + 4.5) u per component.  The ordered sum of n terms of size <= 1 rounds partial sums of
    size <= j: sum_j j u = n (n + 1) / 2 u, divided by n: (n + 1) / 2 u; the division adds u.  Normal: (n / 2 + 3 a + 7) u.
    Distances, relatively: (3 a + 1 + 2.5) u for dist, three more operations: (3 a + 7) u."""
    sc = rm.make_scene(seed, n_kf=n_kf)
    sel = rm.make_selection(sc, seed)
    m32, m64 = rm.refresh(sc, sel, sc["n_rows"], kf_self=1), rm.refresh(sc, sel, sc["n_rows"], kf_self=1, D=np.float64)
    assert np.array_equal(m32["result"], m64["result"]) and np.array_equal(m32["covis"], m64["covis"])
    assert np.array_equal(m32["touched"], m64["touched"]) and np.array_equal(m32["desc"], m64["desc"])
    res = m32["result"]
    print("seed %d: result %s" % (seed, res.tolist()))
    assert res[rm.DONE] > 200 and res[rm.INVALID] > 5 and res[rm.NONE] >= 2 and res[rm.LONG] >= 2 and res[rm.DROPPED] >= 8
    assert res[rm.ALL_BAD] >= 1 and res[rm.REF_UNSEEN] >= 1 and res[rm.REF_MISSING] >= 2
    t = np.flatnonzero(m32["touched"])
    n, a = m32["n"][t].astype(np.float64), m32["amp"][t]
    assert (n == 1024).sum() == 2 and n.max() == 1024 and (m32["n"] == 1025).sum() == 2   # both sides of the longest list
    assert set(rm.LENGTHS) - {0, 1025, 1027} <= set((sc["obs_off"][1:] - sc["obs_off"][:-1])[t].tolist())
    err_n = np.abs(m32["normals"][t].astype(np.float64) - m64["normals"][t]).max(axis=1)
    bound_n = (n / 2 + 3 * a + 7) * U
    err_d = np.maximum(np.abs(m32["max_dist"][t] / m64["max_dist"][t] - 1), np.abs(m32["min_dist"][t] / m64["min_dist"][t] - 1))
    bound_d = (3 * a + 7) * U
    print("normals: largest error %.3e, largest error / bound %.3f (bounds %.2e .. %.2e); distance ranges: %.3e, %.3f" % (
        err_n.max(), (err_n / bound_n).max(), bound_n.min(), bound_n.max(), err_d.max(), (err_d / bound_d).max()))
    assert (err_n <= bound_n).all() and (err_d <= bound_d).all()
    # untouched rows keep every field
    rest = ~m32["touched"]
    for key in ("normals", "min_dist", "max_dist", "desc"):
        assert np.array_equal(m32[key][rest], sc[key][rest]), key


def test_medoid_of_the_model_is_the_reference_loop():
    rng = np.random.RandomState(7)
    pool = rng.randint(0, 256, (5, 32)).astype(np.uint8)
    for n in list(range(1, 12)) + [16, 17]:
        for trial in range(6):
            rows = pool[rng.randint(0, 5, n)] if trial % 2 else rng.randint(0, 256, (n, 32)).astype(np.uint8)
            assert rm.medoid(rows) == rm.medoid_brute(rows), (n, trial)
    far = np.stack([np.zeros(32, np.uint8), np.full(32, 255, np.uint8)])
    assert rm.medoid(far) == 0 and rm.medoid_brute(far) == 0


def test_median_of_the_model_is_the_sorted_element():
    rng = np.random.RandomState(8)
    for n in (1, 2, 3, 8, 9, 500):
        pts = rng.uniform(-5, 5, (n + 4, 3)).astype(np.float32)
        slots = np.concatenate([rng.permutation(n), [-1, n + 4, n + 100]]).astype(np.int32)[None, :]
        R, t = rm._rodrigues(np.array([0.1, -0.2, 0.05])).reshape(1, 9), np.array([[0.3, -0.1, 0.4]])
        med, cnt, base = rm.median_depth(R, t, slots, np.array([n + 3]), n + 3, pts, n + 4, cur=0)
        R32, t32 = R.reshape(3, 3).astype(np.float32), t[0].astype(np.float32)
        z = ((R32[2, 0] * pts[:n, 0] + R32[2, 1] * pts[:n, 1]) + R32[2, 2] * pts[:n, 2]) + t32[2]
        assert cnt[0] == n and med[0] == np.sort(z)[n // 2] and base[0] == 0
        m64, _, _ = rm.median_depth(R, t, slots, np.array([n + 3]), n + 3, pts, n + 4, D=np.float64)
        assert abs(m64[0] - med[0]) <= 8 * U * np.abs(pts).sum(axis=1).max()
    med, cnt, _ = rm.median_depth(R, t, slots, np.array([0]), 5, pts, 4)
    assert np.isnan(med[0]) and cnt[0] == 0
