"""The declarations of include/orbm.h, "The inertial local BA window on the device-resident map": names exported and mirrored in Python,
the limits equal to the visual-window module's, every argument error reported before the device is looked for, the limits, and
ORBX_E_NO_DEVICE without a GPU.  No GPU."""
import ctypes as C
import re

import pytest

import inertial_window_model as wm
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, built, declared, flat, header, returns

NAMES = ("orbm_inertial_window_problem_device", "orbm_inertial_window_velocity_prior_device")
POINTERS = ("slots", "valid", "points", "obs_off", "obs_kf", "obs_kp", "window", "kf_imu", "work", "ba_points", "point_row", "edge_off", "edge_state",
            "edge_point", "edge_z", "edge_inv_sigma2", "edge_kf", "edge_kp", "state_kf", "init_jobs", "fixed", "inertial_edges", "prior_jobs",
            "recover_jobs", "bias_ids", "prior_info_jobs", "result")


@pytest.fixture(scope="module")
def mlib():
    matcher = built("matcher")
    return matcher._mlib(), matcher


def test_the_header_declares_the_entry_points_and_the_library_exports_them(mlib):
    L, matcher = mlib
    names = declared("orbm_", "orbm.h")
    for name in NAMES:
        assert name in names, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.argtypes[0] is C.c_void_p and fn.restype is C.c_int, name
    assert len(L.orbm_inertial_window_problem_device.argtypes) == 41 and len(L.orbm_inertial_window_velocity_prior_device.argtypes) == 9
    for method in ("InertialWindowProblemDevice", "InertialWindowVelocityPriorDevice"):
        assert callable(getattr(matcher.ORBMatcher, method)), method
    assert callable(matcher.inertial_window_problem_device) and callable(matcher.inertial_window_velocity_prior_device)


def test_the_limits_equal_the_visual_window_modules_and_the_flags_the_inertial_modules(mlib):
    """orbm.h does not include the headers whose calls take its outputs, so it names its limits itself: they must be those"""
    _, matcher = mlib
    from monoorbslam3_amd import imu, vw
    defines = dict(re.findall(r"#define (ORBM_IW_[A-Z_]+) (\d+)", header("orbm.h")))
    assert defines == {"ORBM_IW_MAX_SOLVE": "32", "ORBM_IW_MAX_FIXED_DEFAULT": "150"}
    assert int(defines["ORBM_IW_MAX_SOLVE"]) == vw.MAX_SOLVE_STATES == matcher.IW_MAX_SOLVE == wm.MAX_SOLVE
    assert int(defines["ORBM_IW_MAX_FIXED_DEFAULT"]) == matcher.IW_MAX_FIXED_DEFAULT == wm.MAX_FIXED_DEFAULT == 150   # Optimize.cpp:1095
    assert wm.MAX_OBS == vw.MAX_OBS == 256 and "more than 256 kept edges" in flat("include/orbm.h")
    assert wm.FIX_ALL == imu.FIX_POSE | imu.FIX_VELO | imu.FIX_GYRO | imu.FIX_ACC and wm.EDGE_WALKS == imu.EDGE_WALKS
    assert wm.PRIOR_ALL == imu.PRIOR_VELO | imu.PRIOR_GYRO | imu.PRIOR_ACC | imu.PRIOR_ACC_GYRO_INFO and wm.RECOVER_POSE == imu.RECOVER_POSE


def test_the_three_not_built_sentences_point_to_the_section():
    """the visual-window header, DESIGN.md and INTEGRATION.md said that assembling the window from the device-resident map was not built"""
    for path in ("include/orbvw.h", "DESIGN.md", "INTEGRATION.md", "README.md"):
        txt = flat(path)
        assert "orbm_inertial_window_problem_device" in txt, path
        assert "Not here either: assembling this problem from the device-resident map" not in txt, path


def _kf(matcher, **over):
    a = dict(n_kf=8, pose_R=P, pose_t=P, bad=P, kps=P, desc=P, n=P)
    a.update(over)
    return matcher.KfTable(a["n_kf"], a["pose_R"], a["pose_t"], a["bad"], a["kps"], a["desc"], a["n"])


def _problem(L, matcher, kf="default", **over):
    a = dict({k: P for k in POINTERS}, stride=96, cap_points=200, n_obs=900, n_window=3, n_src=10, cap_bank=11, n_priors=9, max_fixed=150,
             cap_states=20, cap_local_points=300, cap_edges=2000)
    a.update(over)
    table = _kf(matcher) if kf == "default" else kf
    return L.orbm_inertial_window_problem_device(
        None, C.byref(table) if table is not None else None, a["slots"], a["stride"], a["valid"], a["points"], a["cap_points"], a["obs_off"], a["obs_kf"],
        a["obs_kp"], a["n_obs"], a["window"], a["n_window"], a["kf_imu"], a["n_src"], a["cap_bank"], a["n_priors"], a["max_fixed"], a["cap_states"],
        a["cap_local_points"], a["cap_edges"], a["work"], a["ba_points"], a["point_row"], a["edge_off"], a["edge_state"], a["edge_point"], a["edge_z"],
        a["edge_inv_sigma2"], a["edge_kf"], a["edge_kp"], a["state_kf"], a["init_jobs"], a["fixed"], a["inertial_edges"], a["prior_jobs"],
        a["recover_jobs"], a["bias_ids"], a["prior_info_jobs"], a["result"], None)


def _velocity(L, **over):
    a = dict(priors=P, n_priors=9, src=P, n_src=10, recover_jobs=P, prior_jobs=P, result=P)
    a.update(over)
    return L.orbm_inertial_window_velocity_prior_device(None, a["priors"], a["n_priors"], a["src"], a["n_src"], a["recover_jobs"], a["prior_jobs"],
                                                        a["result"], None)


def test_the_entry_points_check_their_arguments_before_any_device_call(mlib):
    """every ORBX_E_ARG and ORBX_E_UNSUPPORTED case of the section, returned with a NULL handle and fake pointers: before the device is
    asked for; an argument error wins over a limit; without a device a valid call fails with ORBX_E_NO_DEVICE"""
    L, matcher = mlib

    def problem(**over):
        return _problem(L, matcher, **over)

    def velocity(**over):
        return _velocity(L, **over)

    for key in POINTERS:
        returns(E_ARG, problem, **{key: None})
    returns(E_ARG, problem, kf=None)
    for field in ("bad", "kps", "n"):
        returns(E_ARG, problem, kf=_kf(matcher, **{field: None}), what=field)
    returns(E_ARG, problem, kf=_kf(matcher, n_kf=-1)), returns(E_ARG, problem, kf=_kf(matcher, kps=P + 4))
    for key in ("stride", "cap_points", "n_obs", "n_src", "cap_bank", "n_priors"):
        returns(E_ARG, problem, **{key: -1})
    for key in ("n_window", "max_fixed", "cap_states", "cap_local_points", "cap_edges"):
        returns(E_ARG, problem, **{key: 0}), returns(E_ARG, problem, **{key: -3})
    returns(E_ARG, problem, n_window=33, cap_edges=0), returns(E_ARG, problem, stride=8193, work=None)   # the argument error first
    returns(E_UNSUPPORTED, problem, n_window=33), returns(E_UNSUPPORTED, problem, stride=8193), returns(E_UNSUPPORTED, problem, cap_points=524289)
    for key in ("priors", "src", "recover_jobs", "prior_jobs", "result"):
        returns(E_ARG, velocity, **{key: None})
    returns(E_ARG, velocity, n_priors=-1), returns(E_ARG, velocity, n_src=-1)
    returns(E_NO_DEVICE, problem), returns(E_NO_DEVICE, problem, n_window=32, stride=8192, cap_points=524288)
    returns(E_NO_DEVICE, problem, n_window=1, max_fixed=1), returns(E_NO_DEVICE, problem, kf=_kf(matcher, pose_R=None, pose_t=None, desc=None))
    returns(E_NO_DEVICE, velocity), returns(E_NO_DEVICE, velocity, n_priors=0, n_src=0)
