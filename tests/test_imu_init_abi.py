"""The ABI of the IMU initialisation's steps and of the map rescale without a GPU: every orbii_* name include/orbii.h declares, and
orbm_apply_scale_rotation_device, is exported by the built library and bound by its Python mirror; the #defines equal the mirror's and the
model's; bad arguments are refused before the device is looked for, in the documented order (ORBX_E_ARG, then ORBX_E_UNSUPPORTED, then
ORBX_E_NO_DEVICE); the places that said "not built" name what is built now."""
import ctypes as C
import re

import pytest

import imu_init_model as mm
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, built, declared, exported, exported_and_mirrored, flat, header, returns, stripped

ENTRY_POINTS = ["orbii_prior_device", "orbii_graph_init_device", "orbii_linearize_device", "orbii_damp_device", "orbii_oplus_device", "orbii_recover_device"]


@pytest.fixture(scope="module")
def ii():
    return built("imu_init")


def test_every_declared_entry_point_is_exported_and_mirrored(ii):
    from monoorbslam3_amd import imu, matcher
    names = declared("orbii_", "orbii.h")
    assert names == set(ENTRY_POINTS), sorted(names)
    exported_and_mirrored(ii, "orbii_", names, sigs_equal=True)
    assert ii.Calib is imu.Calib and C.sizeof(ii.Graph) == 64 and C.sizeof(ii.Bias) == 24
    assert '#include "orbi.h"' in stripped("orbii.h")
    assert "orbm_apply_scale_rotation_device" in declared("orbm_", "orbm.h")
    exported(["orbm_apply_scale_rotation_device"])
    fn = matcher._mlib().orbm_apply_scale_rotation_device
    assert len(fn.argtypes) == 20 and fn.restype is C.c_int and callable(matcher.ORBMatcher.ApplyScaleRotationDevice) and callable(matcher.apply_scale_rotation_device)


def test_the_defines_equal_the_mirrors_and_the_models(ii):
    defines = dict(re.findall(r"#define (ORBII_[A-Z_]+) (\d+)", header("orbii.h")))
    assert defines == {"ORBII_MAX_KF": "157", "ORBII_EDGE_WORK": "240", "ORBII_KIND_GS": "0", "ORBII_KIND_G": "1", "ORBII_SHARED_BG": "0",
                       "ORBII_SHARED_BA": "3", "ORBII_SHARED_RWG": "6", "ORBII_SHARED_SCALE": "15", "ORBII_SUMMARY": "10"}
    for name, value in defines.items():
        assert int(value) == getattr(ii, name[len("ORBII_"):]) == getattr(mm, name[len("ORBII_"):]), name
    for n_kf in (2, 3, 17, 66, 157):
        assert ii.system_size(n_kf) == mm.system_size(n_kf) == 15 * -(-(9 + 3 * n_kf) // 15)
    assert ii.system_size(157) == 480 and ii.system_size(2) == 15 and ii.system_size(17) == 60
    from monoorbslam3_amd import vw
    assert ii.system_size(ii.MAX_KF) == 15 * vw.MAX_SOLVE_STATES      # the ordered Cholesky takes exactly this much


def _graph(ii, n_kf=6, **over):
    a = dict(v=P, shared=P, iter=P, Rwb=P, twb=P, Oc=P, Pcb=P)
    a.update(over)
    return ii.Graph(a["v"], a["shared"], a["iter"], a["Rwb"], a["twb"], a["Oc"], a["Pcb"], n_kf, 0)


def _calls(ii):
    """name -> (call(**over) with valid fake arguments, its pointer arguments, whether it takes a graph / kind / mode)"""
    from monoorbslam3_amd import imu
    L = ii._L()
    cal, ib = imu.Calib.make([1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0], [1] * 6, [1] * 6), ii.Bias.make([0] * 6)

    def prior(**o):
        a = dict(pose_R=P, pose_t=P, n_pose=9, state=P, n_src=9, bank=P, cap=9, priors=P, n_priors=9, jobs=P, n=6, Rwg=P, result=P)
        a.update(o)
        return L.orbii_prior_device(a["pose_R"], a["pose_t"], a["n_pose"], a["state"], a["n_src"], a["bank"], a["cap"], a["priors"], a["n_priors"], a["jobs"], a["n"],
                                    a["Rwg"], a["result"], None)

    def init(**o):
        a = dict(graph=_graph(ii), pose_R=P, pose_t=P, n_pose=9, state=P, n_src=9, jobs=P, Rwg=None, result=P)
        a.update(o)
        return L.orbii_graph_init_device(a["graph"], cal, a["pose_R"], a["pose_t"], a["n_pose"], a["state"], a["n_src"], a["jobs"], ib, a["Rwg"], 1.0, a["result"], None)

    def linearize(**o):
        a = dict(graph=_graph(ii), bank=P, cap=9, edges=P, info=P, kind=0, mode=0, work=P, err=P, chi2=P, chi2_prior=P, total=P, H=P, b=P, flt=None, result=P)
        a.update(o)
        return L.orbii_linearize_device(a["graph"], a["bank"], a["cap"], 9.8, a["edges"], a["info"], ib, 1e6, 1e12, a["kind"], a["mode"], a["work"], a["err"], a["chi2"],
                                        a["chi2_prior"], a["total"], a["H"], a["b"], a["flt"], a["result"], None)

    def damp(**o):
        a = dict(n_kf=6, kind=0, H=P, b=P, lam=P, S=P, rhs=P, out=P, result=P)
        a.update(o)
        return L.orbii_damp_device(a["n_kf"], a["kind"], a["H"], a["b"], a["lam"], a["S"], a["rhs"], a["out"], a["result"], None)

    def oplus(**o):
        a = dict(graph=_graph(ii), kind=0, dx=P, result=P)
        a.update(o)
        return L.orbii_oplus_device(a["graph"], a["kind"], a["dx"], a["result"], None)

    def recover(**o):
        a = dict(graph=_graph(ii), jobs=P, state=P, n_src=9, priors=P, n_priors=9, bias=P, summary=P, result=P)
        a.update(o)
        return L.orbii_recover_device(a["graph"], a["jobs"], a["state"], a["n_src"], a["priors"], a["n_priors"], a["bias"], a["summary"], a["result"], None)

    return dict(prior=(prior, ("pose_R", "pose_t", "state", "bank", "priors", "jobs", "Rwg", "result"), ("n_pose", "n_src", "cap", "n_priors")),
                init=(init, ("pose_R", "pose_t", "state", "jobs", "result"), ("n_pose", "n_src")),
                linearize=(linearize, ("bank", "edges", "info", "work", "err", "chi2", "chi2_prior", "total", "H", "b", "result"), ("cap",)),
                damp=(damp, ("H", "b", "lam", "S", "rhs", "out", "result"), ()), oplus=(oplus, ("dx", "result"), ()),
                recover=(recover, ("jobs", "state", "priors", "bias", "summary", "result"), ("n_src", "n_priors")))


def test_bad_arguments_are_refused_before_the_device_in_the_documented_order(ii):
    """null pointers, n_kf 1 and 158, kind 2, mode 2; an argument error wins over the limit; without a device a valid call fails with
    ORBX_E_NO_DEVICE"""
    calls = _calls(ii)
    for name, (call, pointers, counts) in calls.items():
        for key in pointers:
            returns(E_ARG, call, **{key: None})
        for key in counts:
            returns(E_ARG, call, **{key: 0}), returns(E_ARG, call, **{key: -1})
        small, large = (dict(n=1), dict(n=158)) if name == "prior" else (dict(n_kf=1), dict(n_kf=158)) if name == "damp" else (dict(graph=_graph(ii, 1)), dict(graph=_graph(ii, 158)))
        returns(E_ARG, call, **small), returns(E_UNSUPPORTED, call, **large)
        returns(E_ARG, call, **dict(large, **{pointers[0]: None}))                            # the argument error first
        if name not in ("prior", "damp"):
            for field in ("v", "shared", "iter", "Rwb", "twb", "Oc", "Pcb"):
                returns(E_ARG, call, graph=_graph(ii, 6, **{field: None}), what=(name, field))
        if name in ("linearize", "damp", "oplus"):
            returns(E_ARG, call, kind=2), returns(E_ARG, call, kind=-1), returns(E_ARG, call, kind=2, **large)
        returns(E_NO_DEVICE, call)
    lin = calls["linearize"][0]
    returns(E_ARG, lin, mode=2), returns(E_ARG, lin, mode=-1), returns(E_ARG, lin, mode=0, H=None)
    # mode 1 takes no H and no b: still the device that is missing, not an argument (with a device: tests/test_imu_init_gpu.py)
    returns(E_NO_DEVICE, lin, mode=1, H=None, b=None), returns(E_NO_DEVICE, calls["init"][0], Rwg=P), returns(E_NO_DEVICE, calls["prior"][0], n=157)


def test_the_rescale_checks_its_arguments_before_any_device_call(ii):
    from monoorbslam3_amd import imu, matcher
    L = matcher._mlib()
    cal = imu.Calib.make([1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0], [1] * 6, [1] * 6)

    def call(**o):
        a = dict(calib=C.addressof(cal), n_kf=6, pose_R=P, pose_t=P, bad=P, kf_imu=P, state=P, n_src=9, priors=P, n_priors=9, points=P, valid=P, n_points=P,
                 cap_points=100, summary=P, result=P)
        a.update(o)
        return L.orbm_apply_scale_rotation_device(None, a["calib"], a["n_kf"], a["pose_R"], a["pose_t"], a["bad"], a["kf_imu"], a["state"], a["n_src"], a["priors"],
                                                  a["n_priors"], a["points"], a["valid"], a["n_points"], a["cap_points"], a["summary"], 1, 0.1, a["result"], None)

    for key in ("calib", "pose_R", "pose_t", "bad", "kf_imu", "state", "priors", "points", "valid", "n_points", "summary", "result"):
        returns(E_ARG, call, **{key: None})
    for key in ("n_kf", "n_src", "n_priors", "cap_points"):
        returns(E_ARG, call, **{key: -1})
    returns(E_UNSUPPORTED, call, cap_points=524289), returns(E_ARG, call, cap_points=524289, summary=None)
    returns(E_NO_DEVICE, call), returns(E_NO_DEVICE, call, n_kf=0, pose_R=None, bad=None), returns(E_NO_DEVICE, call, cap_points=0, points=None, valid=None)


def test_the_not_built_sentences_name_what_is_built():
    """DESIGN.md said three times that the IMU initialisation was not built; it names the new calls now and records what is still open"""
    design = flat("DESIGN.md")
    for name in ENTRY_POINTS + ["orbm_apply_scale_rotation_device"]:
        assert name in design, name
    for gone in ("the gravity direction of `initializeIMU` [is] not built", "`applyScaleRotation` … not built"):
        assert gone not in design
    for still_open in ("fullInertialOptimize", "gravityOptimize"):
        assert still_open in design
    for path in ("INTEGRATION.md", "README.md"):
        assert "orbii_linearize_device" in flat(path) and "orbm_apply_scale_rotation_device" in flat(path), path
    assert "orbvw_solve_device" in flat("INTEGRATION.md") and "IMU initialisation as a chain on one stream" in flat("INTEGRATION.md")
    for name in ("orbii.h",):                                   # the header describes the solve's layout without naming the call
        assert "orbvw" not in header(name) and "orbvi" not in header(name)
