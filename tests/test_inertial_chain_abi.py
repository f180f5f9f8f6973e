"""The ABI of localInertialBundleAdjustment on the device without a GPU: include/orbil.h declares orbil_chain_solve_device and
orbil_chain_optimize_device and include/orbm.h ("The inertial chain on the device-resident map") the assembly and the velocity priors; the
built library exports them and monoorbslam3_amd.chain / .matcher mirror them; the options' layout and the macros are the headers'; every
argument check returns its code before the device is looked for (tests/abi_checks.py's rule of the fake pointer: no call that passes the
checks is made where a device is present); the documents say what the calls do."""
import ctypes as C
import re

import pytest

import inertial_chain_model as cm
import inertial_loop as il
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, built, declared, exported_and_mirrored, flat, header, returns, stripped

SOLVE, OPTIMIZE = "orbil_chain_solve_device", "orbil_chain_optimize_device"
PROBLEM, VELOCITY = "orbm_inertial_chain_problem_device", "orbm_inertial_chain_velocity_priors_device"
NAN = float("nan")


@pytest.fixture(scope="module")
def chain():
    return built("chain")


@pytest.fixture(scope="module")
def mlib():
    matcher = built("matcher")
    return matcher._mlib(), matcher


def test_the_declarations_the_macros_and_the_mirror_agree(chain):
    from monoorbslam3_amd import imu, vi
    txt = stripped("orbil.h")
    assert declared("orbil_", "orbil.h") == {SOLVE, OPTIMIZE} and '#include "orbvi.h"' in txt
    for other in ("orbi.h", "orbi_factors.h", "orbvi.h", "orbvi_loop.h", "orbvw.h", "orbm.h", "orbx.h"):      # nothing includes it
        assert "orbil.h" not in stripped(other), other
    exported_and_mirrored(chain, "orbil_", {SOLVE, OPTIMIZE}, True)
    for name in (SOLVE, OPTIMIZE):
        assert getattr(chain._L(), name).argtypes == chain._SIGS[name]
    one = re.sub(r"\s+", " ", txt)
    assert "#define ORBIL_MAX_STATES %d " % chain.MAX_STATES in one and "#define ORBIL_LOOP_WORK %d " % chain.LOOP_WORK in one
    assert "#define ORBIL_SUMMARY %d " % chain.SUMMARY in one and "#define ORBIL_SOLVE_WORK(n) (450 * (n))" in one and chain.solve_work(7) == 450 * 7
    assert chain.MAX_STATES == 20 == cm.MAX_WINDOW and chain.LOOP_TRACE == len(il.FIELDS) == vi.LOOP_TRACE and chain.LOOP_MAX_TRIALS == il.MAX_TRIALS
    # the options: field by field as the header has them, 40 bytes
    body = re.search(r"typedef struct orbil_chain_options \{(.*?)\} orbil_chain_options;", txt, re.S).group(1)
    fields = [(t, n) for t, n in re.findall(r"(int32_t|double|float) (\w+)[;,]", body)] + [("float", "pad")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(chain.ChainOptions._fields_), fields
    assert C.sizeof(chain.ChainOptions) == 40
    o = chain.ChainOptions.make(9.81)
    assert (o.iterations, o.max_trials, o.lambda_init, o.tau, o.huber_delta) == (10, il.MAX_TRIALS, 0.0, il.TAU, 0.0)
    # the declarations: pointers, counts and the by-value structures where the mirror has them
    want = {"orbi_graph": imu.Graph, "orbil_chain_options": chain.ChainOptions}
    for name, count in ((SOLVE, 14), (OPTIMIZE, 19)):
        decls = [a.strip() for a in re.search(r"int %s\((.*?)\);" % name, txt, re.S).group(1).split(",")]
        assert len(decls) == len(chain._SIGS[name]) == count, name
        for decl, ct in zip(decls, chain._SIGS[name]):
            assert ct is (C.c_void_p if "*" in decl else want.get(decl.split()[0], C.c_int)), (decl, ct)


def _solve(chain, **over):
    a = dict({k: P for k in ("fixed", "edges", "H_diag", "H_off", "b", "lam", "work", "dx", "out", "result")}, n_states=10, n_edges=9, cap=12)
    a.update(over)
    return lambda: chain.chain_solve_device(a["n_states"], a["fixed"], a["edges"], a["n_edges"], a["cap"], a["H_diag"], a["H_off"], a["b"], a["lam"], a["work"],
                                            a["dx"], a["out"], a["result"])


def _optimize(chain, opt=None, **over):
    """the wrapper with valid arguments (the fake device address) except for `over`; opt: what to change in the options"""
    a = dict({k: P for k in ("Rwb", "twb", "v", "bg", "ba", "fixed", "iter", "bank", "edges", "info", "walk", "priors", "pjobs", "work", "trace", "summary", "result")},
             n_states=10, cap=12, n_edges=9, n_priors=1, n_pjobs=1, cap_trace=64)
    a.update(over)
    g = chain.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], a["fixed"], a["n_states"])
    o = chain.ChainOptions.make(**dict(dict(gravity=9.81), **(opt or {})))
    return lambda: chain.chain_optimize_device(g, a["iter"], a["bank"], a["cap"], a["edges"], a["n_edges"], a["info"], a["walk"], a["priors"], a["n_priors"], a["pjobs"],
                                               a["n_pjobs"], o, a["work"], a["trace"], a["cap_trace"], a["summary"], a["result"])


def test_the_solves_argument_errors_are_reported_before_the_device_is_looked_for(chain):
    for k in ("fixed", "edges", "H_diag", "H_off", "b", "lam", "work", "dx", "out", "result"):
        returns(E_ARG, _solve(chain, **{k: None}), what=(k, None))
    for over in (dict(n_states=0), dict(n_states=-1), dict(n_edges=-1), dict(cap=0)):
        returns(E_ARG, _solve(chain, **over), what=over)
    for over in (dict(n_states=1, n_edges=0), dict(n_states=chain.MAX_STATES + 1), dict(n_edges=4097)):
        returns(E_UNSUPPORTED, _solve(chain, **over), what=over)
    returns(E_ARG, _solve(chain, n_states=21, out=None))                 # an argument error wins over the unsupported size
    returns(E_NO_DEVICE, _solve(chain)), returns(E_NO_DEVICE, _solve(chain, n_states=2, n_edges=1)), returns(E_NO_DEVICE, _solve(chain, n_states=chain.MAX_STATES))
    returns(E_NO_DEVICE, _solve(chain, n_edges=0, edges=None, H_off=None)), returns(E_NO_DEVICE, _solve(chain, n_states=3, n_edges=40))   # edges outside the band are dropped on the device


def test_the_loops_argument_errors_are_reported_before_the_device_is_looked_for(chain):
    for k in ("Rwb", "twb", "v", "bg", "ba", "fixed", "iter", "bank", "edges", "info", "walk", "priors", "pjobs", "work", "trace", "summary", "result"):
        returns(E_ARG, _optimize(chain, **{k: None}), what=(k, None))
    for over in (dict(n_states=0), dict(n_states=-1), dict(cap=0), dict(n_edges=-1), dict(n_priors=-1), dict(n_pjobs=-1), dict(cap_trace=-1)):
        returns(E_ARG, _optimize(chain, **over), what=over)
    for opt in (dict(iterations=0), dict(max_trials=0), dict(iterations=-1), dict(tau=NAN), dict(huber_delta=NAN), dict(gravity=NAN), dict(lambda_init=NAN)):
        returns(E_ARG, _optimize(chain, opt), what=opt)
    for over in (dict(n_states=1, n_edges=0), dict(n_states=chain.MAX_STATES + 1), dict(n_edges=10), dict(n_pjobs=chain.LOOP_MAX_PRIOR_JOBS + 1)):
        returns(E_UNSUPPORTED, _optimize(chain, **over), what=over)
    for opt in (dict(iterations=chain.LOOP_MAX_ITERATIONS + 1), dict(max_trials=chain.LOOP_MAX_TRIALS + 1)):
        returns(E_UNSUPPORTED, _optimize(chain, opt), what=opt)
    # an argument error wins over the unsupported size, and both over the missing device
    returns(E_ARG, _optimize(chain, n_states=21, summary=None)), returns(E_ARG, _optimize(chain, dict(max_trials=11, tau=NAN)))


def test_the_loop_fails_loudly_without_a_gpu(chain):
    returns(E_NO_DEVICE, _optimize(chain))
    returns(E_NO_DEVICE, _optimize(chain, n_states=2, n_edges=1)), returns(E_NO_DEVICE, _optimize(chain, n_states=chain.MAX_STATES, n_edges=chain.MAX_STATES - 1))
    # the reference's call: no priors; no trace; no edges at all; the three kinds of lambda init
    returns(E_NO_DEVICE, _optimize(chain, n_pjobs=0, n_priors=0, priors=None, pjobs=None)), returns(E_NO_DEVICE, _optimize(chain, cap_trace=0, trace=None))
    returns(E_NO_DEVICE, _optimize(chain, n_edges=0, edges=None, info=None, walk=None))
    returns(E_NO_DEVICE, _optimize(chain, dict(lambda_init=-1.0))), returns(E_NO_DEVICE, _optimize(chain, dict(lambda_init=1e-2, iterations=100, max_trials=1)))


# ---- the map side -------------------------------------------------------------------------------------------------------------------------
OUTPUTS = ("init_jobs", "fixed", "inertial_edges", "recover_jobs", "bias_ids", "velo_jobs", "state_kf", "result")


def _problem(L, **over):
    a = dict({k: P for k in ("bad", "window", "kf_imu") + OUTPUTS}, n_kf=8, n_window=3, n_src=10, cap_bank=11, n_priors=9)
    a.update(over)
    return L.orbm_inertial_chain_problem_device(None, a["n_kf"], a["bad"], a["window"], a["n_window"], a["kf_imu"], a["n_src"], a["cap_bank"], a["n_priors"],
                                                *[a[k] for k in OUTPUTS], None)


def _velocity(L, **over):
    a = dict(priors=P, n_priors=9, src=P, n_src=10, velo_jobs=P, n=3, result=P)
    a.update(over)
    return L.orbm_inertial_chain_velocity_priors_device(None, a["priors"], a["n_priors"], a["src"], a["n_src"], a["velo_jobs"], a["n"], a["result"], None)


def test_the_map_side_is_declared_exported_and_mirrored(mlib):
    L, matcher = mlib
    names = declared("orbm_", "orbm.h")
    for name, count in ((PROBLEM, 18), (VELOCITY, 9)):
        assert name in names, name
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.argtypes[0] is C.c_void_p and fn.restype is C.c_int and len(fn.argtypes) == count, name
        decls = [a.strip() for a in re.search(r"int %s\((.*?)\);" % name, stripped("orbm.h"), re.S).group(1).split(",")]
        assert [C.c_void_p if "*" in d else C.c_int for d in decls] == list(fn.argtypes), name
    for method in ("InertialChainProblemDevice", "InertialChainVelocityPriorsDevice"):
        assert callable(getattr(matcher.ORBMatcher, method)), method
    assert callable(matcher.inertial_chain_problem_device) and callable(matcher.inertial_chain_velocity_priors_device)
    assert dict(re.findall(r"#define (ORBM_IC_[A-Z_]+) (\d+)", header("orbm.h"))) == {"ORBM_IC_MAX_WINDOW": str(cm.MAX_WINDOW)}
    assert (cm.REFUSE_WINDOW, cm.REFUSE_IMU) == (8, 32)                 # the window assembly's bits


def test_the_map_side_checks_its_arguments_before_any_device_call(mlib):
    L, _ = mlib

    def problem(**over):
        return _problem(L, **over)

    def velocity(**over):
        return _velocity(L, **over)

    for key in ("bad", "window", "kf_imu") + OUTPUTS:
        returns(E_ARG, problem, **{key: None})
    for key in ("n_kf", "n_src", "cap_bank", "n_priors"):
        returns(E_ARG, problem, **{key: -1})
    returns(E_ARG, problem, n_window=1), returns(E_ARG, problem, n_window=0), returns(E_ARG, problem, n_window=-2)   # a chain has two key frames at least
    returns(E_ARG, problem, n_window=21, result=None)                    # the argument error first
    returns(E_UNSUPPORTED, problem, n_window=cm.MAX_WINDOW + 1)
    for key in ("priors", "src", "velo_jobs", "result"):
        returns(E_ARG, velocity, **{key: None})
    returns(E_ARG, velocity, n_priors=-1), returns(E_ARG, velocity, n_src=-1), returns(E_ARG, velocity, n=-1)
    returns(E_UNSUPPORTED, velocity, n=cm.MAX_WINDOW + 1)
    returns(E_NO_DEVICE, problem), returns(E_NO_DEVICE, problem, n_window=2), returns(E_NO_DEVICE, problem, n_window=cm.MAX_WINDOW, n_kf=0)
    returns(E_NO_DEVICE, velocity), returns(E_NO_DEVICE, velocity, n=0, n_priors=0, n_src=0)


def test_the_documents_say_what_the_calls_do_and_what_stays_the_callers():
    h, m, readme, design, integ = flat("include/orbil.h"), flat("include/orbm.h"), flat("README.md"), flat("DESIGN.md"), flat("INTEGRATION.md")
    chain_text = ("orbi_graph_init_device -> orbi_edge_information_device -> orbil_chain_optimize_device -> orbi_graph_recover_device -> orbi_set_bias_device -> "
                  "orbm_inertial_chain_velocity_priors_device")
    assert chain_text in h and "ONE KERNEL LAUNCH OF ONE WORKGROUP" in h and "THE CHAIN HAS NO READ-BACK AT ALL" in m
    for phrase in ("no allocation, no copy, no wait and no read-back", "G2O CANNOT REACH THAT VALUE", "restores d_iter as well", "csrc/orbvi_stages.h", "ORBX_E_UNSUPPORTED",
                   "k_il_chain_loop", "k_il_chain_solve", "every barrier is in control flow uniform", "Where the factor lives", "products with an exact zero",
                   "csrc/orb_lm_policy.h", "|i - j| != 1"):
        assert phrase in h, phrase
    for phrase in ("THE REFUSAL IS HONOURED ON THE DEVICE", "NOTHING IS SKIPPED", "setFixed(i == 0)", "KeyFrame::setVelocity", "k_ic_problem", "k_ic_velocity_priors"):
        assert phrase in m, phrase
    for doc, name in ((readme, "README.md"), (design, "DESIGN.md"), (integ, "INTEGRATION.md")):
        for word in (OPTIMIZE, "orbil.h", PROBLEM):
            assert word in doc, (name, word)
    for path in ("include/orbi.h", "include/orbvi_loop.h", "include/orbwl.h", "include/orbii.h", "include/orbvi.h"):
        assert "orbil.h" in flat(path), path
    assert "tools/chain_loop_latency.py" in design and "not g2o's time" in design
