"""The ABI of orbvi_pose_optimize_device without a GPU: include/orbvi_loop.h declares it, the built library exports it and
monoorbslam3_amd.vi mirrors it; the options' layout and the macros are the header's; every argument check returns its code before the
device is looked for (tests/abi_checks.py's rule of the fake pointer: no call that passes the checks is made where a device is present);
the header, orbvi.h and the README say what the call does and what is still the caller's."""
import ctypes as C
import re

import pytest

import inertial_loop as il
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, built, declared, exported, flat, header, returns, stripped

NAME = "orbvi_pose_optimize_device"
NAN = float("nan")


@pytest.fixture(scope="module")
def vi():
    return built("vi")


def test_the_declaration_the_macros_and_the_mirror_agree(vi):
    from monoorbslam3_amd import imu
    txt = stripped("orbvi_loop.h")
    assert declared("orbvi_", "orbvi_loop.h") == {NAME} and '#include "orbvi.h"' in txt and "orbvi_loop" not in header("orbvi.h").split("#ifndef")[1]
    exported({NAME})
    assert NAME in vi._SIGS and callable(vi.pose_optimize_device) and getattr(vi._L(), NAME).argtypes == vi._SIGS[NAME]
    one = re.sub(r"\s+", " ", txt)
    for name, value in [("MAX_ROUNDS", vi.LOOP_MAX_ROUNDS), ("MAX_ITERATIONS", vi.LOOP_MAX_ITERATIONS), ("MAX_TRIALS", vi.LOOP_MAX_TRIALS),
                        ("MAX_PRIOR_JOBS", vi.LOOP_MAX_PRIOR_JOBS), ("EDGE_WORK", vi.LOOP_EDGE_WORK), ("FIXED_WORK", vi.LOOP_FIXED_WORK), ("TRACE", vi.LOOP_TRACE),
                        ("SUMMARY", vi.LOOP_SUMMARY)]:
        assert "#define ORBVI_LOOP_%s %d " % (name, value) in one, name
    assert "#define ORBVI_R_EDGE_REFUSED %d " % vi.R_EDGE_REFUSED in one
    assert vi.LOOP_TRACE == len(il.FIELDS) and vi.LOOP_MAX_TRIALS == il.MAX_TRIALS and vi.LOOP_EDGE_WORK == vi.EDGE_WORK + 2
    # the options: field by field as the header has them, 96 bytes
    body = re.search(r"typedef struct orbvi_loop_options \{(.*?)\} orbvi_loop_options;", txt, re.S).group(1)
    fields = [(t, n, int(k) if k else 1) for t, n, k in re.findall(r"(int32_t|double|float) (\w+)(?:\[(\d+)\])?[;,]", body)]
    fields += [("float", "pad2", 1)] if ("float", "pad2", 1) not in fields else []
    ctype = {"int32_t": C.c_int32, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t] * k if k > 1 else ctype[t]) for t, n, k in fields] == [(n, t) for n, t in vi.LoopOptions._fields_], fields
    assert C.sizeof(vi.LoopOptions) == 96
    # the declaration: pointers, counts and the by-value structures where the mirror has them
    args = re.search(r"int %s\((.*?)\);" % NAME, txt, re.S).group(1)
    want = {"orbi_graph": imu.Graph, "orbi_calib": imu.Calib, "orbvi_camera": vi.Camera, "orbvi_loop_options": vi.LoopOptions}
    decls = [a.strip() for a in args.split(",")]
    assert len(decls) == len(vi._SIGS[NAME]) == 30
    for decl, ct in zip(decls, vi._SIGS[NAME]):
        assert ct is (C.c_void_p if "*" in decl else want.get(decl.split()[0], C.c_int)), (decl, ct)
    o = vi.LoopOptions.make(9.81)
    assert (o.rounds, list(o.iterations), o.max_trials, list(o.lambda_init), o.tau, o.huber_delta, o.chi2_threshold) == \
        (4, [10] * 4, 10, [0.0] * 4, il.TAU, vi.HUBER_MONO, vi.CHI2_MONO)


def _call(vi, opt=None, **over):
    """the wrapper with valid arguments (the fake device address) except for `over`; opt: what to change in the options"""
    import imu_model as im
    a = dict({k: P for k in ("Rwb", "twb", "v", "bg", "ba", "fixed", "iter", "bank", "edges", "info", "walk", "priors", "pjobs", "group_state", "edge_off", "points",
                             "z", "w", "active", "work", "chi2", "n_inliers", "trace", "summary", "result")},
             n_states=2, cap=4, n_edges=1, n_priors=1, n_pjobs=1, cap_edges=400, cap_trace=64, camera_model=0)
    a.update(over)
    c = im.calib()
    cal = vi.Calib.make(c["Rcb"], c["tcb"], c["cov_noise"], c["cov_walk"], c["gravity"])
    g = vi.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], a["fixed"], a["n_states"])
    cam = vi.Camera.make(458.0, 457.0, 367.0, 248.0, a["camera_model"])
    o = vi.LoopOptions.make(**dict(dict(gravity=c["gravity"]), **(opt or {})))
    return lambda: vi.pose_optimize_device(g, a["iter"], a["bank"], a["cap"], a["edges"], a["n_edges"], a["info"], a["walk"], a["priors"], a["n_priors"], a["pjobs"],
                                           a["n_pjobs"], cal, cam, a["cap_edges"], a["group_state"], a["edge_off"], a["points"], a["z"], a["w"], a["active"], o,
                                           a["work"], a["chi2"], a["n_inliers"], a["trace"], a["cap_trace"], a["summary"], a["result"])


def test_argument_errors_are_reported_before_the_device_is_looked_for(vi):
    null = ("Rwb", "twb", "v", "bg", "ba", "fixed", "iter", "bank", "edges", "info", "walk", "priors", "pjobs", "group_state", "edge_off", "points", "z", "w", "active",
            "work", "chi2", "n_inliers", "trace", "summary", "result")
    for k in null:
        returns(E_ARG, _call(vi, **{k: None}), what=(k, None))
    for over in (dict(n_states=-1), dict(cap=0), dict(n_edges=-1), dict(n_priors=-1), dict(n_pjobs=-1), dict(cap_edges=-1), dict(cap_trace=-1), dict(camera_model=2)):
        returns(E_ARG, _call(vi, **over), what=over)
    for opt in (dict(rounds=0), dict(max_trials=0), dict(iterations=(10, 0, 10, 10)), dict(iterations=(-1, 10, 10, 10)), dict(tau=NAN), dict(huber_delta=NAN),
                dict(chi2_threshold=NAN), dict(gravity=NAN), dict(lambda_init=(0.0, NAN, 0.0, 0.0))):
        returns(E_ARG, _call(vi, opt), what=opt)
    for over in (dict(n_states=1), dict(n_states=3), dict(n_edges=2), dict(n_pjobs=vi.LOOP_MAX_PRIOR_JOBS + 1)):
        returns(E_UNSUPPORTED, _call(vi, **over), what=over)
    for opt in (dict(rounds=vi.LOOP_MAX_ROUNDS + 1), dict(max_trials=vi.LOOP_MAX_TRIALS + 1), dict(iterations=(10, vi.LOOP_MAX_ITERATIONS + 1, 10, 10))):
        returns(E_UNSUPPORTED, _call(vi, opt), what=opt)
    # an argument error wins over the unsupported size, and both over the missing device
    returns(E_ARG, _call(vi, n_states=3, summary=None))
    returns(E_ARG, _call(vi, dict(rounds=5, tau=NAN)))
    # what is beyond `rounds` is not looked at
    returns(E_NO_DEVICE, _call(vi, dict(rounds=1, iterations=(10, 0, -5, 1000), lambda_init=(0.0, NAN, NAN, NAN))))


def test_the_wrapper_fails_loudly_without_a_gpu(vi):
    returns(E_NO_DEVICE, _call(vi))
    # poseInertialOptimize: no visual group, its arrays NULL; no trace; no priors; no inertial edge's walk flags to speak of
    returns(E_NO_DEVICE, _call(vi, dict(rounds=1), cap_edges=0, group_state=None, edge_off=None, points=None, z=None, w=None, active=None, chi2=None, n_inliers=None))
    returns(E_NO_DEVICE, _call(vi, cap_trace=0, trace=None)), returns(E_NO_DEVICE, _call(vi, n_pjobs=0, n_priors=0, priors=None, pjobs=None))
    returns(E_NO_DEVICE, _call(vi, n_edges=0)), returns(E_NO_DEVICE, _call(vi, dict(lambda_init=(-1.0, 0.0, 1e-3, 0.0)), camera_model=1))


def test_the_documents_say_what_the_call_does_and_what_stays_the_callers():
    h, v, readme, design, integ = flat("include/orbvi_loop.h"), flat("include/orbvi.h"), flat("README.md"), flat("DESIGN.md"), flat("INTEGRATION.md")
    chain = "orbi_graph_init_device -> orbi_edge_information_device -> orbvi_pose_optimize_device -> orbi_graph_recover_device"
    assert chain in h and chain in v and "ONE KERNEL LAUNCH OF ONE WORKGROUP" in h
    for phrase in ("no allocation, no copy, no wait and no read-back", "G2O CANNOT REACH THAT VALUE", "forced_lambda_init", "THE CUBE IS x*x*x", "k_pose_optimize",
                   "What remains the caller's", "restores d_iter as well", "csrc/orbvi_stages.h", "ORBX_E_UNSUPPORTED", "k_vi_pose_loop", "every barrier is in control flow uniform"):
        assert phrase in h, phrase
    assert "THE LOOP ITSELF IS NOT HERE" in v and "orbvi_loop.h" in v
    for doc, name in ((readme, "README.md"), (design, "DESIGN.md"), (integ, "INTEGRATION.md")):
        assert NAME in doc and "orbvi_loop.h" in doc, name
    assert "THE LOOP REMAINS TEST CODE" in design and "THE NEXT ITEMS" in design and "tools/vi_pose_loop_latency.py" in design
