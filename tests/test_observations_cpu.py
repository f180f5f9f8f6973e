"""orbm_build_observations_device / orbm_cull_keyframes_device without a GPU: the array model the GPU tests compare with against an
independent object-style restatement of the reference (tests/observations_model.py) on every seeded scene, the exports and the
Python wrappers, and the argument checks that run before any device call."""
import ctypes as C

import numpy as np
import pytest

import observations_model as om
from test_abi import _declared, _defines

CULL_SEEDS = (21, 22, 23)
CULL_KEYS = ("bad", "slots", "valid", "ref_kf", "code", "num_mp", "num_redundant", "result")


@pytest.fixture(scope="module")
def mlib():
    import __graft_entry__ as g
    g.build()
    from monoorbslam3_amd import matcher
    return matcher._mlib(), matcher


@pytest.mark.parametrize("name", sorted(om.BUILD_SCENES))
def test_build_model_equals_the_object_restatement(name):
    kw = om.BUILD_SCENES[name]
    sc = om.make_build_scene(**kw)
    args = (sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"])
    a, b = om.build(*args, 1 << 30), om.build_objects(*args, 1 << 30)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.tobytes() == y.tobytes()
    off, kf, kp, res = a
    print("%s: d_result %s" % (name, res.tolist()))
    lengths = off[1:] - off[:-1]
    assert lengths[:len(kw["lengths"])].tolist() == list(kw["lengths"])
    assert res[om.SKIP_INVALID] > 0 and res[om.SKIP_BAD_KF] > 0 and res[om.TWICE] == 1 and res[om.LONGEST] == lengths.max() >= max(kw["lengths"])
    assert (sc["n"] > sc["stride"]).any() and (sc["slots"] == -1).any() and (sc["slots"] >= sc["cap_points"]).any() and (sc["slots"] < -1).any()
    key = kf.astype(np.int64) * om.MAX_STRIDE + kp                       # every list ascending in (k, i)
    inner = np.ones(len(key), bool)
    inner[off[:-1][lengths > 0]] = False
    assert (np.diff(key)[inner[1:]] > 0).all()
    if name == "long":
        assert set(lengths.tolist()) >= {0, 1, 2, 3, 4, 63, 64, 65, 1024, 1025} and res[om.N_LONG] == 1
    # overflow: the same counts, empty lists
    o, p = om.build(*args, len(kf) - 1), om.build_objects(*args, len(kf) - 1)
    assert o[3][om.OVERFLOW] == 1 and o[3][om.NOBS] == len(kf) and not o[0].any() and len(o[1]) == 0
    for x, y in zip(o, p):
        assert x.tobytes() == y.tobytes()


@pytest.mark.parametrize("seed", CULL_SEEDS)
def test_cull_model_equals_the_object_restatement(seed):
    sc = om.make_cull_scene(seed)
    off, kf, kp, _ = om.build(sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"], 1 << 30)
    trace = []
    out, obj = om.cull(sc, off, kf, kp, trace=trace), om.cull_objects(sc)
    print("seed %d: d_result %s, d_code %s" % (seed, out["result"].tolist(), out["code"].tolist()))
    for key in CULL_KEYS:
        assert out[key].dtype == obj[key].dtype and out[key].tobytes() == obj[key].tobytes(), key
    om.check_cull_scene(sc, out, trace)
    # the doctrine: the CSR rebuilt from the culled slots is what the objects are left with
    off2, kf2, kp2, _ = om.build(sc["n"], out["bad"], out["slots"], sc["stride"], out["valid"], sc["cap_points"], 1 << 30)
    assert om.lists_of(off2, kf2, kp2) == obj["lists"]


@pytest.mark.parametrize("th_obs", [3, 2])
def test_small_cull_model_equals_the_object_restatement(th_obs):
    sc = om.make_small_cull_scene(5)
    off, kf, kp, _ = om.build(sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"], 1 << 30)
    out, obj = om.cull(sc, off, kf, kp, th_obs=th_obs), om.cull_objects(sc, th_obs=th_obs)
    for key in CULL_KEYS:
        assert out[key].tobytes() == obj[key].tobytes(), key
    assert out["code"].tolist() == [-1, 0 if th_obs == 3 else 3, -1]


B_ARGS = ("h", "n_kf", "n", "bad", "slots", "stride", "valid", "cap", "cap_obs", "obs_off", "obs_kf", "obs_kp", "result")
C_ARGS = ("h", "kf", "bad", "slots", "stride", "valid", "cap", "obs_off", "obs_kf", "obs_kp", "n_obs", "ref_kf", "recent", "ts", "n_recent",
          "first_kf", "th_obs", "ratio", "gap", "code", "num_mp", "num_red", "result")


def _build(L, **over):
    """one call with valid arguments (fake, never dereferenced pointers) except for `over`"""
    a = {k: 0x1000 for k in B_ARGS}
    a.update(h=None, n_kf=25, stride=2000, cap=5000, cap_obs=40000)
    a.update(over)
    return L.orbm_build_observations_device(*[a[k] for k in B_ARGS], None)


def _cull(L, matcher, kf_over=None, recent_list=None, **over):
    kf = matcher.KfTable(25, *([0x1000] * 6))
    for k, v in (kf_over or {}).items():
        setattr(kf, k, v)
    rec = np.array(list(range(10)) if recent_list is None else recent_list, np.int32)
    ts = np.arange(max(len(rec), 1), dtype=np.float64)
    a = {k: 0x1000 for k in C_ARGS}
    a.update(h=None, kf=C.byref(kf), stride=2000, cap=5000, n_obs=40000, recent=rec.ctypes.data, ts=ts.ctypes.data, n_recent=len(rec),
             first_kf=-1, th_obs=3, ratio=0.9, gap=1.5)
    a.update(over)
    return L.orbm_cull_keyframes_device(*[a[k] for k in C_ARGS], None)


def test_header_declares_both_entry_points_and_the_wrappers_exist(mlib):
    """test_abi.test_every_declared_symbol_is_exported then checks that the library exports them"""
    L, matcher = mlib
    assert {"orbm_build_observations_device", "orbm_cull_keyframes_device"} <= set(_declared("orbm.h"))
    assert L.orbm_build_observations_device.argtypes is not None and len(L.orbm_build_observations_device.argtypes) == 14
    assert len(L.orbm_cull_keyframes_device.argtypes) == 24
    assert L.orbm_cull_keyframes_device.argtypes[17] is C.c_double and L.orbm_cull_keyframes_device.argtypes[18] is C.c_double
    assert hasattr(matcher.ORBMatcher, "BuildObservationsDevice") and hasattr(matcher.ORBMatcher, "CullKeyFramesDevice")
    header = open(_header_path()).read()
    assert "Observations built and key frames culled on the device" in header
    for text in ("int orbm_build_observations_device(orbm_t *h, int n_kf, const int32_t *d_n, const uint8_t *d_bad, const int32_t *d_slots, int stride,",
                 "int orbm_cull_keyframes_device(orbm_t *h, const orbm_kf_table *kf, uint8_t *d_bad, int32_t *d_slots, int stride, uint8_t *d_valid,"):
        assert text in header


def _header_path():
    import os
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "orbm.h")


def test_bad_arguments_are_rejected_before_any_device_call(mlib):
    L, matcher = mlib
    cases = [dict(n_kf=-1), dict(stride=-1), dict(cap=-1), dict(cap_obs=-1)]
    cases += [{k: None} for k in ("n", "bad", "slots", "valid", "obs_off", "obs_kf", "obs_kp", "result")]
    for over in cases:
        assert _build(L, **over) == -1, over
        assert L.orbx_last_error()
    stride_limit = _defines("orbm.h", "ORBM_MEDIAN_MAX_")["stride"]
    assert stride_limit == om.MAX_STRIDE
    for over, text in ((dict(stride=stride_limit + 1), b"ORBM_MEDIAN_MAX_STRIDE"), (dict(n_kf=om.MAX_KF + 1), b"262143"),
                       (dict(cap=om.MAX_POINTS + 1), b"524288")):
        assert _build(L, **over) == -4 and text in L.orbx_last_error(), over
    cases = [dict(kf=None), dict(stride=-1), dict(cap=-1), dict(n_obs=-1), dict(n_recent=-1), dict(th_obs=-1), dict(first_kf=-2), dict(first_kf=25),
             dict(kf_over=dict(n_kf=-1)), dict(kf_over=dict(d_kps=0x1001)), dict(kf_over=dict(d_kps=None)), dict(kf_over=dict(d_n=None)),
             dict(recent_list=[0, 1, 25, 3]), dict(recent_list=[0, -1, 2])]
    cases += [{k: None} for k in ("bad", "slots", "valid", "obs_off", "obs_kf", "obs_kp", "ref_kf", "recent", "ts", "code", "num_mp", "num_red",
                                  "result")]
    for over in cases:
        assert _cull(L, matcher, **over) == -1, over
        assert L.orbx_last_error()
    for over, text in ((dict(recent_list=list(range(25)) + list(range(8))), b"32 recent"), (dict(stride=stride_limit + 1), b"ORBM_MEDIAN_MAX_STRIDE"),
                       (dict(cap=om.MAX_POINTS + 1), b"524288")):
        assert _cull(L, matcher, **over) == -4 and text in L.orbx_last_error(), over


def test_valid_calls_fail_loudly_without_a_gpu(mlib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    L, matcher = mlib
    assert _build(L) == -2 and b"no HIP device" in L.orbx_last_error()
    assert _build(L, n_kf=0, n=None, bad=None, slots=None) == -2
    assert _build(L, stride=om.MAX_STRIDE, n_kf=om.MAX_KF, cap=om.MAX_POINTS) == -2
    assert _cull(L, matcher) == -2 and b"no HIP device" in L.orbx_last_error()
    assert _cull(L, matcher, recent_list=list(range(25)) + list(range(7)), first_kf=24) == -2
    assert _cull(L, matcher, recent_list=[], code=None, num_mp=None, num_red=None) == -2
