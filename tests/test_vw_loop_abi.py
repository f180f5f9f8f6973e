"""The ABI of the window loop without a GPU: include/orbwl.h declares orbwl_window_work_doubles and orbwl_window_optimize_device, the built
library exports them and monoorbslam3_amd.vw mirrors them; the options' layout and the macros are the header's; every argument check
returns its code and its own message before the device is looked for (tests/abi_checks.py's rule of the fake pointer: no call that
passes the checks is made where a device is present); the size of the scratch block is the sum the header lists; the header and the
three documents say what the call does, that it WAITS, and what is still the caller's."""
import ctypes as C
import os
import re

import pytest

import inertial_loop as il
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, ROOT, built, declared, exported, flat, header, returns, stripped

NAMES = {"orbwl_window_work_doubles", "orbwl_window_optimize_device"}
NAME = "orbwl_window_optimize_device"
NAN = float("nan")


@pytest.fixture(scope="module")
def vw():
    return built("vw")


def test_the_declaration_the_macros_and_the_mirror_agree(vw):
    from monoorbslam3_amd import imu, vi
    txt = stripped("orbwl.h")
    assert declared("orbwl_", "orbwl.h") == NAMES and '#include "orbvi.h"' in txt
    for other in ("orbvi.h", "orbvi_loop.h", "orbi.h", "orbm.h", "orbfi.h"):       # nothing includes it
        assert "orbwl.h" not in stripped(other), other
    exported(NAMES)
    assert set(vw._LOOP_SIGS) == NAMES and getattr(vw._LL(), NAME).argtypes == vw._LOOP_SIGS[NAME] and vw._LL() is vw._L()
    assert callable(vw.window_optimize_device) and callable(vw.window_work_doubles)
    one = re.sub(r"\s+", " ", txt)
    for name, value in [("MAX_ITERATIONS", vw.LOOP_MAX_ITERATIONS), ("MAX_TRIALS", vw.LOOP_MAX_TRIALS), ("TRACE", vw.LOOP_TRACE), ("SUMMARY", vw.LOOP_SUMMARY),
                        ("R_REJECTED", vw.R_REJECTED), ("R_OUTLIER", vw.R_OUTLIER), ("R_POINT_SINGULAR", vw.R_POINT_SINGULAR)]:
        assert "#define ORBWL_%s %d " % (name, value) in one, name
    assert vw.LOOP_TRACE == len(il.FIELDS) == vi.LOOP_TRACE and vw.LOOP_MAX_TRIALS == il.MAX_TRIALS and vw.LOOP_MAX_ITERATIONS == 100
    # the options: field by field as the header has them, 48 bytes
    body = re.search(r"typedef struct orbwl_loop_options \{(.*?)\} orbwl_loop_options;", txt, re.S).group(1)
    fields = [(t, n) for t, n in re.findall(r"(int32_t|double|float) (\w+)[;,]", body)] + [("float", "pad")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(vw.WindowLoopOptions._fields_), fields
    assert C.sizeof(vw.WindowLoopOptions) == 48
    offsets = {n: getattr(vw.WindowLoopOptions, n).offset for n, _ in vw.WindowLoopOptions._fields_}
    assert offsets == dict(iterations=0, max_trials=4, lambda_init=8, huber_delta_visual=16, huber_delta_inertial=24, chi2_threshold=32, gravity=40, pad=44)
    assert "static_assert(sizeof(orbwl_loop_options) == 48" in open(os.path.join(ROOT, "monoorbslam3_amd", "csrc", "orbwl.hip")).read()
    # the declaration: pointers, counts and the by-value structures where the mirror has them
    args = re.search(r"int %s\((.*?)\);" % NAME, txt, re.S).group(1)
    want = {"orbi_graph": imu.Graph, "orbi_calib": imu.Calib, "orbvi_camera": vi.Camera, "orbwl_loop_options": vw.WindowLoopOptions}
    decls = [a.strip() for a in args.split(",")]
    assert len(decls) == len(vw._LOOP_SIGS[NAME]) == 33
    for decl, ct in zip(decls, vw._LOOP_SIGS[NAME]):
        assert ct is (C.c_void_p if "*" in decl else want.get(decl.split()[0], C.c_int)), (decl, ct)
    o = vw.WindowLoopOptions.make(9.81)
    assert (o.iterations, o.max_trials, o.lambda_init, o.huber_delta_visual, o.huber_delta_inertial, o.chi2_threshold) == (10, 10, 1.0, vw.HUBER_MONO, 0.0, vw.CHI2_MONO)


def _call(vw, opt=None, **over):
    """the wrapper with valid arguments (the fake device address) except for `over`; opt: what to change in the options"""
    import imu_model as im
    a = dict({k: P for k in ("Rwb", "twb", "v", "bg", "ba", "fixed", "iter", "bank", "edges", "info", "walk", "priors", "pjobs", "points", "edge_state", "edge_point",
                             "z", "w", "active", "work", "chi2", "outlier", "trace", "summary", "result")},
             n_states=12, cap=16, n_edges=9, n_priors=1, n_pjobs=1, n_solve=10, n_points=500, cap_edges=2000, cap_trace=64, camera_model=0, stop=None)
    a.update(over)
    c = im.calib()
    cal = vw.Calib.make(c["Rcb"], c["tcb"], c["cov_noise"], c["cov_walk"], c["gravity"])
    g = vw.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], a["fixed"], a["n_states"])
    cam = vw.Camera.make(458.0, 457.0, 367.0, 248.0, a["camera_model"])
    o = vw.WindowLoopOptions.make(**dict(dict(gravity=c["gravity"]), **(opt or {})))
    return lambda: vw.window_optimize_device(g, a["iter"], a["bank"], a["cap"], a["edges"], a["n_edges"], a["info"], a["walk"], a["priors"], a["n_priors"], a["pjobs"],
                                             a["n_pjobs"], cal, cam, a["n_solve"], a["n_points"], a["cap_edges"], a["points"], a["edge_state"], a["edge_point"], a["z"],
                                             a["w"], a["active"], o, a["work"], a["chi2"], a["outlier"], a["trace"], a["cap_trace"], a["summary"], a["result"],
                                             stop=a["stop"])


def test_argument_errors_are_reported_before_the_device_is_looked_for(vw):
    graph, inertial, priors, visual = "null graph array or result", "inertial edge list or information", "prior jobs without", "null point or EdgeMono array"
    outputs, scratch = "null d_chi2, d_outlier, summary or trace", "16-byte aligned"
    null = dict(Rwb=graph, twb=graph, v=graph, bg=graph, ba=graph, fixed=graph, result=graph, iter=inertial, bank=inertial, edges=inertial, info=inertial, walk=inertial,
                priors=priors, pjobs=priors, points=visual, edge_state=visual, edge_point=visual, z=visual, w=visual, work=scratch, chi2=outputs, outlier=outputs,
                trace=outputs, summary=outputs)
    for k, text in null.items():
        assert text in returns(E_ARG, _call(vw, **{k: None}), what=(k, None)), k
    for over, text in ((dict(n_states=-1), graph), (dict(cap=0), inertial), (dict(n_edges=-1), inertial), (dict(n_priors=-1), priors), (dict(n_pjobs=-1), priors),
                       (dict(n_points=0), visual), (dict(n_points=-1), visual), (dict(cap_edges=-1), visual), (dict(n_solve=0), "n_solve outside"),
                       (dict(n_solve=13), "n_solve outside"), (dict(work=P + 8), scratch), (dict(cap_trace=-1), outputs), (dict(camera_model=2), "camera_model"),
                       (dict(camera_model=-1), "camera_model")):
        assert text in returns(E_ARG, _call(vw, **over), what=over), over
    for opt, text in ((dict(iterations=0), "iterations or max_trials < 1"), (dict(max_trials=0), "iterations or max_trials < 1"), (dict(iterations=-3), "iterations or max_trials"),
                      (dict(lambda_init=NAN), "not a number"), (dict(huber_delta_visual=NAN), "not a number"), (dict(huber_delta_inertial=NAN), "not a number"),
                      (dict(chi2_threshold=NAN), "not a number"), (dict(gravity=NAN), "not a number")):
        assert text in returns(E_ARG, _call(vw, opt), what=opt), opt
    for over, text in ((dict(n_solve=vw.MAX_SOLVE_STATES + 1, n_states=40), "ORBVW_MAX_SOLVE_STATES"), (dict(cap_edges=vw.MAX_EDGES + 1), "ORBVW_MAX_EDGES"),
                       (dict(n_points=vw.MAX_POINTS + 1), "ORBVW_MAX_POINTS"), (dict(n_states=4097), "ORBI_MAX_JOBS"), (dict(n_edges=4097), "ORBI_MAX_JOBS"),
                       (dict(n_pjobs=4097), "ORBI_MAX_JOBS")):
        assert text in returns(E_UNSUPPORTED, _call(vw, **over), what=over), over
    for opt, text in ((dict(iterations=vw.LOOP_MAX_ITERATIONS + 1), "ORBWL_MAX_ITERATIONS"), (dict(max_trials=vw.LOOP_MAX_TRIALS + 1), "ORBWL_MAX_TRIALS"),
                      (dict(lambda_init=0.0), "computeLambdaInit")):
        assert text in returns(E_UNSUPPORTED, _call(vw, opt), what=opt), opt
    # an argument error wins over the unsupported size, and both over the missing device
    returns(E_ARG, _call(vw, n_solve=vw.MAX_SOLVE_STATES + 1, n_states=40, summary=None))
    returns(E_ARG, _call(vw, dict(lambda_init=0.0, chi2_threshold=NAN)))
    returns(E_ARG, _call(vw, dict(iterations=101), work=None))


def test_the_wrapper_fails_loudly_without_a_gpu(vw):
    returns(E_NO_DEVICE, _call(vw))
    # what is optional is optional, the limits themselves are supported, both lambda inits and a flag in host memory: still the device that is missing
    returns(E_NO_DEVICE, _call(vw, active=None)), returns(E_NO_DEVICE, _call(vw, cap_trace=0, trace=None))
    returns(E_NO_DEVICE, _call(vw, n_pjobs=0, n_priors=0, priors=None, pjobs=None)), returns(E_NO_DEVICE, _call(vw, n_edges=0, cap_edges=0))
    returns(E_NO_DEVICE, _call(vw, dict(lambda_init=-1.0, iterations=25), camera_model=1)), returns(E_NO_DEVICE, _call(vw, dict(lambda_init=1e-2), stop=C.c_int32(0)))
    returns(E_NO_DEVICE, _call(vw, dict(iterations=vw.LOOP_MAX_ITERATIONS, max_trials=vw.LOOP_MAX_TRIALS), n_solve=vw.MAX_SOLVE_STATES, n_states=4096,
                               cap_edges=vw.MAX_EDGES, n_points=vw.MAX_POINTS, n_edges=4096, n_pjobs=4096))


def _even(n):
    return (n + 1) // 2 * 2


def _work_doubles(n_states, n_solve, n_points, cap_edges, n_edges, n_prior_jobs):
    """the header's list, restated: every slice rounded up to an even number of doubles; int32 slices at two to a double"""
    S, N, L, E, J, Pj = n_states, 15 * n_solve, n_points, cap_edges, n_edges, n_prior_jobs
    slices = [225 * S, 225 * J, 15 * S,                                  # H_diag, H_off, b
              488 * J, 9 * J, 3 * J, 3 * Pj, 4,                          # the inertial work, errors, chi2, prior chi2, totals (mode 0 and mode 1)
              24 * E, 2 * E, 4, 9 * L, 3 * L, 18 * E, (L + 1 + 1) // 2,  # the EdgeMono work, errors, totals, Hll, bl, Hlp, point_off
              N * N, N, 9 * L, 3 * L, N, 3 * L,                          # S, rhs, Hll_inv, tl, dx, xl
              3 * L,                                                     # the second point buffer
              3, 1, 1,                                                   # d_out, d_out_points, d_lambda
              21 * n_solve, (n_solve + 1) // 2,                          # the saved vertices with their d_iter
              16,                                                        # the control block
              9 * 8 // 2]                                                # one 8-int result slot per stage call
    return sum(_even(s) for s in slices)


def test_the_scratch_block_is_the_sum_the_header_lists(vw):
    from monoorbslam3_amd import imu
    assert imu.EDGE_WORK == 488 and vw.EDGE_WORK == 24
    h = flat("include/orbwl.h")
    for phrase in ("H_diag 225 S, H_off 225 J, b 15 S", "the inertial work 488 J (ORBI_EDGE_WORK), errors 9 J, chi2 3 J, prior chi2 3 P, totals 4",
                   "the EdgeMono work 24 E, errors 2 E, totals 4, Hll 9 L, bl 3 L, Hlp 18 E, point_off (L + 1) int32", "S N N, rhs N, Hll_inv 9 L, tl 3 L, dx N, xl 3 L",
                   "the second point buffer 3 L", "d_out 3, d_out_points 1, d_lambda 1", "the saved vertices 21 n_solve with their d_iter n_solve int32",
                   "the control block 16", "one 8-int result slot per stage call, 9 slots", "each rounded up to an even number of doubles"):
        assert phrase in h, phrase
    for case in ((5, 3, 63, 63 * 4, 2, 1), (7, 4, 65, 65 * 5, 3, 1), (32, 32, 1025, 4000, 31, 1), (40, 32, 1025, 4001, 31, 0), (1, 1, 1, 0, 0, 0)):
        assert vw.window_work_doubles(*case) == _work_doubles(*case) and vw.window_work_doubles(*case) % 2 == 0, case
    for bad in ((-1, 3, 63, 200, 2, 1), (5, -1, 63, 200, 2, 1), (5, 3, -1, 200, 2, 1), (5, 3, 63, -1, 2, 1), (5, 3, 63, 200, -1, 1), (5, 3, 63, 200, 2, -1),
                (5, 0, 63, 200, 2, 1), (5, 6, 63, 200, 2, 1), (5, 3, 0, 200, 2, 1)):
        assert vw.window_work_doubles(*bad) < 0, bad
    # the largest supported window does not overflow the count
    top = (4096, 32, vw.MAX_POINTS, vw.MAX_EDGES, 4096, 4096)
    assert vw.window_work_doubles(*top) == _work_doubles(*top) > 2 ** 25


def test_the_documents_say_what_the_call_does_and_that_it_waits():
    h, w, readme, design, integ = flat("include/orbwl.h"), flat("include/orbvw.h"), flat("README.md"), flat("DESIGN.md"), flat("INTEGRATION.md")
    chain = ("orbm_inertial_window_problem_device -> orbi_graph_init_device -> orbi_edge_information_device -> orbwl_window_optimize_device -> "
             "orbi_graph_recover_device -> orbm_local_ba_apply_device (with this call's d_outlier) -> orbi_prior_information_device")
    assert chain in h
    for phrase in ("THIS CALL WAITS ON THE CALLER'S STREAM, ONCE PER TRIAL AND ONCE AT THE END", "orbba_local_bundle_adjustment_device does the same",
                   "second exception to \"never waits\"", "ONE 16-byte verdict", "G2O CANNOT REACH THAT VALUE", "THE CUBE IS x*x*x", "csrc/orb_lm_policy.h",
                   "EVERY EDGE IS CLASSIFIED", "no parity with where g2o tests its force-stop flag is claimed", "a HOST pointer", "two host threads may be inside the call at once",
                   "Any HIP error ends the call at once", "ON THE STATES [0, n_solve) ONLY", "ORBX_E_UNSUPPORTED", "k_vwl_decide", "inertial_loop.FIELDS"):
        assert phrase in h, phrase
    assert "THE LOOP ITSELF IS NOT HERE" in w and "orbwl.h" in w
    assert "orbvw" not in header("orbwl.h")                          # like orbm.h it names the visual window's calls by what they do
    for doc, name in ((readme, "README.md"), (design, "DESIGN.md"), (integ, "INTEGRATION.md")):
        assert NAME in doc and "orbwl.h" in doc, name
    assert "The window loop closed by the host" in design and "tools/vw_window_loop_latency.py" in design
    # the policy stands once: DESIGN.md names the header as the one definition, the loops that call it, and the one that measured slower with it
    assert ("`csrc/orb_lm_policy.h` is the one definition of g2o's trial policy" in design and "`k_vwl_decide`, `k_vi_pose_loop` and the host's `lm_loop` call it" in design
            and "`k_pose_optimize` alone keeps its copy" in design and "two copies" not in design and "profiles/lm_policy_shared.txt" in design)
    assert "once per trial and once at the end" in design and "once per trial and once at the end" in integ
    order = ["orbm_inertial_window_problem_device", "orbi_graph_init_device", "orbi_edge_information_device", NAME, "orbi_graph_recover_device",
             "orbm_local_ba_apply_device", "orbi_prior_information_device"]
    step = integ[integ.index("The inertial mapper step with the library's loop"):]
    step = step[step.index("```"):]                                 # the chain's listing
    at =[step.index(n) for n in order]
    assert at == sorted(at), at
