"""The BA entry points (include/orbba.h) without a GPU.  The host index builder that orbba_linearize, orbba_optimize and
orbba_local_bundle_adjustment share (csrc/orbba_problem.h), compiled alone by tests/cpp/ba_index.cpp with the host compiler, against a
numpy restatement; and the eight entry points through ctypes: a NULL argument, bad sizes and malformed content are reported before
the device is looked for, with the texts the GPU tests match on, and without a GPU a valid call fails with ORBX_E_NO_DEVICE."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from abi_checks import E_ARG, E_NO_DEVICE, P, ROOT, built, declared, returns

OK = 0
RANGE, ORDER, TWICE, ALL_FIXED = ("edge index out of range", "edges must be grouped by point",
                                  "a point is observed twice by the same key frame", "every pose is fixed: nothing to optimise")

# 3 poses, one fixed; 5 points; 9 edges, grouped by point, no pose twice at a point; point 3 is seen by the fixed pose alone
FIXED = [0, 1, 0]
EDGE_POSE = [2, 0, 1, 0, 1, 2, 0, 1, 0]
EDGE_POINT = [0, 0, 1, 1, 2, 2, 2, 3, 4]
VALID = {
    "3_poses_5_points_9_edges": (FIXED, 5, EDGE_POSE, EDGE_POINT),
    "1_pose_1_point": ([0], 1, [0], [0]),
}


def _edit(seq, **at):
    out = list(seq)
    for k, v in at.items():
        out[int(k[1:])] = v
    return out


# the five malformed variants of the first problem -> the text that has to come back
MALFORMED = {
    "out_of_range": ((FIXED, 5, _edit(EDGE_POSE, e4=3), EDGE_POINT), RANGE),
    "unordered": ((FIXED, 5, EDGE_POSE, _edit(EDGE_POINT, e5=1)), ORDER),
    "observed_twice": ((FIXED, 5, _edit(EDGE_POSE, e6=2), EDGE_POINT), TWICE),       # pose 2 at point 2 by edges 5 and 6
    "all_fixed": (([1, 1, 1], 5, EDGE_POSE, EDGE_POINT), ALL_FIXED),
    # edge 3 breaks the order, edge 6 has no such point: the first offending edge decides, whatever the order of the checks per edge
    "two_faults": ((FIXED, 5, EDGE_POSE, _edit(EDGE_POINT, e3=0, e6=5)), ORDER),
}


@pytest.fixture(scope="module")
def ba_index(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ba_index") / "ba_index")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "monoorbslam3_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "ba_index.cpp"), "-o", exe])

    def run(lm, fixed, n_points, ep, el):
        text = " ".join(str(int(v)) for v in [lm, len(fixed), n_points, len(ep)] + list(fixed) + list(ep) + list(el))
        lines = subprocess.run([exe], input=text, text=True, capture_output=True, check=True).stdout.splitlines()
        out = dict(status=int(lines[0].split()[1]), message=lines[1][len("message "):])
        for ln in lines[2:]:
            name, *vals = ln.split()
            out[name] = np.array(vals, np.int64)
        return out
    return run


def _restated(lm, fixed, n_points, ep, el):
    """the six arrays as numpy says them"""
    fixed, ep, el = np.asarray(fixed, bool), np.asarray(ep, np.int64), np.asarray(el, np.int64)
    out = dict(pose_off=np.concatenate([[0], np.cumsum(np.bincount(ep, minlength=len(fixed)))]),
               pose_edges=np.argsort(ep, kind="stable"), point_off=np.searchsorted(el, np.arange(n_points + 1)),
               free_pose=np.zeros(0, np.int64), pose_slot=np.zeros(0, np.int64), edge_of=np.zeros(0, np.int64))
    if lm:
        out["free_pose"] = np.flatnonzero(~fixed)
        out["pose_slot"] = np.where(fixed, -1, np.cumsum(~fixed) - 1)
        table = np.full((len(out["free_pose"]), n_points), -1, np.int64)
        free_edges = np.flatnonzero(~fixed[ep])
        table[out["pose_slot"][ep[free_edges]], el[free_edges]] = free_edges
        out["edge_of"] = table.ravel()
    return out


@pytest.mark.parametrize("lm", [0, 1])
@pytest.mark.parametrize("name", sorted(VALID))
def test_the_index_builder_equals_the_numpy_restatement(ba_index, name, lm):
    got, want = ba_index(lm, *VALID[name]), _restated(lm, *VALID[name])
    assert (got["status"], got["message"]) == (OK, "")
    for k, v in want.items():
        assert np.array_equal(got[k], v), (k, got[k], v)
    if name.startswith("3_poses") and lm:
        assert (got["edge_of"] >= 0).sum() == 6 and len(got["edge_of"]) == 10    # the fixed pose's edges 2, 4 and 7 have no cell


def test_the_index_builder_on_a_problem_without_edges(ba_index):
    """orbba_linearize's: empty ranges everywhere; the LM entry points refuse it by its sizes"""
    got, want = ba_index(0, FIXED, 5, [], []), _restated(0, FIXED, 5, [], [])
    assert (got["status"], got["message"]) == (OK, "")
    for k, v in want.items():
        assert np.array_equal(got[k], v), k
    assert not got["pose_off"].any() and not got["point_off"].any() and len(got["pose_edges"]) == 0
    refused = ba_index(1, FIXED, 5, [], [])
    assert (refused["status"], refused["message"]) == (E_ARG, "bad sizes")


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_the_index_builder_refuses_malformed_content(ba_index, name):
    problem, text = MALFORMED[name]
    got = ba_index(1, *problem)
    assert (got["status"], got["message"]) == (E_ARG, text)
    # orbba_linearize takes fixed poses and repeated observations as they are: only the range and the order are its business
    base = ba_index(0, *problem)
    if text in (RANGE, ORDER):
        assert (base["status"], base["message"]) == (E_ARG, text)
    else:
        assert base["status"] == OK and np.array_equal(base["pose_edges"], np.argsort(np.asarray(problem[2]), kind="stable"))


# ----------------------------------------------------------------------------------------------------------------- the C ABI
@pytest.fixture(scope="module")
def ba():
    return built("ba")


def _host_problem(ba, fixed, n_points, ep, el, keep):
    """an orbba_problem on host arrays (`keep` holds them)"""
    n_poses, n_edges = len(fixed), len(ep)
    arrays = [np.tile(np.eye(3).reshape(9), (n_poses, 1)), np.zeros((n_poses, 3)), np.asarray(fixed, np.uint8), np.ones((n_points, 3)),
              np.asarray(ep, np.int32), np.asarray(el, np.int32), np.zeros((max(n_edges, 1), 2)), np.ones(max(n_edges, 1))]
    keep.extend(arrays)
    return ba._Problem(500.0, 500.0, 320.0, 240.0, ba.HUBER_MONO, n_poses, n_points, n_edges, *[a.ctypes.data for a in arrays], 0,
                       (C.c_double * 4)(0, 0, 0, 0))


def _host_calls(ba, prob):
    """the three host-pointer entry points on one problem, every output NULL (any of them may be)"""
    L = ba._L()
    lin, opt, res = ba._Result(), ba._LmOptions(max_iterations=1), ba._LmResult()
    return dict(orbba_linearize=lambda: L.orbba_linearize(C.byref(prob), C.byref(lin), -1),
                orbba_optimize=lambda: L.orbba_optimize(C.byref(prob), C.byref(opt), C.byref(res), -1),
                orbba_local_bundle_adjustment=lambda: L.orbba_local_bundle_adjustment(C.byref(prob), C.byref(res), None, -1))


def _device_calls(ba, **over):
    """the five entry points that take device pointers and a pose batch on host pointers, with valid arguments (the fake device address)
    except for `over`"""
    L = ba._L()
    p = P
    a = dict(n_poses=3, n_points=5, n_edges=9, n_frames=1, n2=4, nq=4, pose_R=p, out_R=p, chi2=p, outlier=p, edge_off=p, frame_mp=p, inlier=p)
    a.update(over)
    tail = (0, (C.c_double * 4)(0, 0, 0, 0))
    prob = ba._Problem(500.0, 500.0, 320.0, 240.0, ba.HUBER_MONO, a["n_poses"], a["n_points"], a["n_edges"], a["pose_R"], p, p, p, p, p, p, p, *tail)
    res = ba._LmResult(a["out_R"], p, p, a["chi2"])
    pose = ba._PoseProblem(500.0, 500.0, 320.0, 240.0, ba.HUBER_MONO, a["n_frames"], 0, 0, a["edge_off"], a["pose_R"], p, p, p, p, *tail)
    pose_res = ba._PoseResult(a["out_R"], p, a["inlier"], p, a["chi2"], 0.0)
    off = (C.c_int32 * 2)(0, 0)                                      # the host form reads its offsets: one frame without edges
    host_pose = ba._PoseProblem(500.0, 500.0, 320.0, 240.0, ba.HUBER_MONO, a["n_frames"], 0, 0, C.addressof(off) if a["edge_off"] else None,
                                a["pose_R"], p, None, None, None, *tail)
    return dict(
        orbba_local_bundle_adjustment_device=lambda: L.orbba_local_bundle_adjustment_device(C.byref(prob), C.byref(res), a["outlier"], None),
        orbba_pose_optimize_batch_device=lambda: L.orbba_pose_optimize_batch_device(C.byref(pose), C.byref(pose_res), None),
        orbba_pose_edges_device=lambda: L.orbba_pose_edges_device(a["n2"], a["nq"], a["frame_mp"], p, p, a["edge_off"], p, p, p, None, None),
        orbba_pose_drop_outliers_device=lambda: L.orbba_pose_drop_outliers_device(a["n2"], a["edge_off"], p, a["inlier"], a["frame_mp"], None),
        orbba_pose_optimize_batch=lambda: (L.orbba_pose_optimize_batch(C.byref(host_pose), C.byref(pose_res), -1), off)[0])


HOST_NAMES = ("orbba_linearize", "orbba_optimize", "orbba_local_bundle_adjustment")
DEVICE_NAMES = ("orbba_local_bundle_adjustment_device", "orbba_pose_optimize_batch_device", "orbba_pose_edges_device",
                "orbba_pose_drop_outliers_device", "orbba_pose_optimize_batch")


def test_the_eight_entry_points_are_declared_and_bound(ba):
    names = declared("orbba_", "orbba.h")
    assert names == set(HOST_NAMES) | set(DEVICE_NAMES) | {"orbba_set_variant"}
    L = ba._L()
    for name in names:
        assert getattr(L, name).argtypes is not None, name


def test_argument_errors_are_reported_before_the_device_is_looked_for(ba):
    L = ba._L()
    keep = []
    good = _host_problem(ba, *VALID["3_poses_5_points_9_edges"], keep)
    lin, opt, res = ba._Result(), ba._LmOptions(max_iterations=1), ba._LmResult()
    # a NULL struct
    for fn, *args in ((L.orbba_linearize, None, C.byref(lin), -1), (L.orbba_linearize, C.byref(good), None, -1),
                      (L.orbba_optimize, None, C.byref(opt), C.byref(res), -1), (L.orbba_optimize, C.byref(good), None, C.byref(res), -1),
                      (L.orbba_optimize, C.byref(good), C.byref(opt), None, -1), (L.orbba_local_bundle_adjustment, None, C.byref(res), None, -1),
                      (L.orbba_local_bundle_adjustment, C.byref(good), None, None, -1), (L.orbba_local_bundle_adjustment_device, None, C.byref(res), P, None),
                      (L.orbba_local_bundle_adjustment_device, C.byref(good), None, P, None), (L.orbba_pose_optimize_batch, None, None, -1),
                      (L.orbba_pose_optimize_batch_device, None, None, None)):
        assert returns(E_ARG, fn, *args) == "null argument"
    # sizes and arrays of the host-pointer problem
    for field, value, text, names in [("n_poses", 0, "bad sizes", HOST_NAMES), ("n_points", 0, "bad sizes", HOST_NAMES),
                                      ("n_edges", -1, "bad sizes", HOST_NAMES), ("n_edges", 0, "bad sizes", HOST_NAMES[1:]),
                                      ("pose_R", None, "null input array", HOST_NAMES), ("pose_fixed", None, "null input array", HOST_NAMES),
                                      ("points", None, "null input array", HOST_NAMES), ("edge_pose", None, "null input array", HOST_NAMES),
                                      ("edge_inv_sigma2", None, "null input array", HOST_NAMES)]:
        bad = _host_problem(ba, *VALID["3_poses_5_points_9_edges"], keep)
        setattr(bad, field, value)
        calls = _host_calls(ba, bad)
        for name in names:
            assert returns(E_ARG, calls[name], what=(field, name)) == text
    opt_bad = ba._LmOptions(max_iterations=-1)
    assert returns(E_ARG, L.orbba_optimize, C.byref(good), C.byref(opt_bad), C.byref(res), -1) == "negative iteration count"
    # malformed content
    for case, (problem, text) in MALFORMED.items():
        calls = _host_calls(ba, _host_problem(ba, *problem, keep))
        for name in HOST_NAMES[1:] + (HOST_NAMES[:1] if text in (RANGE, ORDER) else ()):
            assert returns(E_ARG, calls[name], what=(case, name)) == text
    # the device-pointer entry points and the pose batch
    lba, pob = "null array (every pointer is device memory here, chi2 and outlier included)", "null array (every pointer is device memory here, chi2 included)"
    for over, name, text in [(dict(n_poses=0), "orbba_local_bundle_adjustment_device", "bad sizes"),
                             (dict(n_edges=0), "orbba_local_bundle_adjustment_device", "bad sizes"),
                             (dict(pose_R=None), "orbba_local_bundle_adjustment_device", lba), (dict(out_R=None), "orbba_local_bundle_adjustment_device", lba),
                             (dict(chi2=None), "orbba_local_bundle_adjustment_device", lba), (dict(outlier=None), "orbba_local_bundle_adjustment_device", lba),
                             (dict(n_frames=0), "orbba_pose_optimize_batch_device", pob), (dict(edge_off=None), "orbba_pose_optimize_batch_device", pob),
                             (dict(chi2=None), "orbba_pose_optimize_batch_device", pob), (dict(inlier=None), "orbba_pose_optimize_batch_device", pob),
                             (dict(n2=-1), "orbba_pose_edges_device", "bad argument"), (dict(frame_mp=None), "orbba_pose_edges_device", "bad argument"),
                             (dict(edge_off=None), "orbba_pose_edges_device", "bad argument"),
                             (dict(n2=-1), "orbba_pose_drop_outliers_device", "bad argument"), (dict(inlier=None), "orbba_pose_drop_outliers_device", "bad argument"),
                             (dict(n_frames=0), "orbba_pose_optimize_batch", "bad sizes / null arrays"),
                             (dict(edge_off=None), "orbba_pose_optimize_batch", "bad sizes / null arrays"),
                             (dict(out_R=None), "orbba_pose_optimize_batch", "null output array")]:
        assert returns(E_ARG, _device_calls(ba, **over)[name], what=(over, name)) == text


def test_a_valid_call_fails_loudly_without_a_gpu(ba):
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    keep = []
    calls = dict(_device_calls(ba))
    for name, problem in VALID.items():
        calls.update({"%s(%s)" % (k, name): v for k, v in _host_calls(ba, _host_problem(ba, *problem, keep)).items()})
    calls["orbba_linearize(no edges)"] = _host_calls(ba, _host_problem(ba, FIXED, 5, [], [], keep))["orbba_linearize"]
    assert len(calls) == 5 + 2 * 3 + 1
    for name, call in calls.items():
        returns(E_NO_DEVICE, call, what=name)                   # and "no HIP device" in the message
