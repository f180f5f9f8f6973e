"""The ABI of fullInertialOptimize's shared-bias graph without a GPU: every orbfi_* name include/orbfi.h declares is exported by the
built library and bound by its Python mirror with the documented signature; the #defines equal the mirror's and the model's; bad
arguments are refused before the device is looked for, in the documented order (ORBX_E_ARG, then ORBX_E_UNSUPPORTED, then
ORBX_E_NO_DEVICE); the documents name what is built now."""
import ctypes as C
import os
import re

import pytest

import full_inertial_model as fim
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, ROOT, built, exported_and_mirrored, flat, header, returns, stripped

ENTRY_POINTS = {"orbfi_jobs_device": 14, "orbfi_linearize_device": 25, "orbfi_recover_device": 12}      # name -> arguments


@pytest.fixture(scope="module")
def fi():
    return built("full_inertial")


def test_every_declared_entry_point_is_exported_and_mirrored_with_its_signature(fi):
    from monoorbslam3_amd import imu
    txt = stripped("orbfi.h")
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\bint (orbfi_[a-z0-9_]+)\s*\(([^;]*)\);", txt)}
    assert set(declared) == set(ENTRY_POINTS), sorted(declared)
    exported_and_mirrored(fi, "orbfi_", declared, sigs_equal=True)
    for n, args in declared.items():
        assert len(args.split(",")) == ENTRY_POINTS[n] == len(fi._SIGS[n]), (n, len(args.split(",")), len(fi._SIGS[n]))
        for decl, ct in zip(args.split(","), fi._SIGS[n]):        # pointers, ints, floats and doubles where the header has them
            decl = decl.strip()
            want = C.c_void_p if "*" in decl else imu.Graph if decl.startswith("orbi_graph") else imu.Calib if decl.startswith("orbi_calib") else \
                C.c_float if decl.startswith("float") else C.c_double if decl.startswith("double") else C.c_int
            assert ct is want, (n, decl, ct)
    assert fi.Calib is imu.Calib and fi.Graph is imu.Graph
    assert '#include "orbi.h"' in txt and "orbvw" not in header("orbfi.h")     # like orbm.h it names the visual window's calls by what they do
    for other in os.listdir(os.path.join(ROOT, "include")):         # nothing includes it
        assert other == "orbfi.h" or "orbfi.h" not in header(other), other
    assert "orbfi.hip" in open(os.path.join(ROOT, "monoorbslam3_amd", "csrc", "Makefile")).read()


def test_the_defines_equal_the_mirrors_and_the_models(fi):
    from monoorbslam3_amd import vw
    h = header("orbfi.h")
    assert int(re.search(r"#define ORBFI_MAX_KEYFRAMES (\d+) +/\* ORBVW_MAX_SOLVE_STATES - 1", h).group(1)) == vw.MAX_SOLVE_STATES - 1 == fi.MAX_KEYFRAMES == fim.MAX_KEYFRAMES == 31
    assert int(re.search(r"#define ORBFI_EDGE_WORK (\d+)", h).group(1)) == fi.EDGE_WORK == fim.EDGE_WORK
    assert float(re.search(r"#define ORBFI_HUBER_DELTA ([\d.]+)", h).group(1)) == fi.HUBER_DELTA == fim.HUBER_DELTA == 4.1134


def _graph(n=6, **over):
    from monoorbslam3_amd import imu
    a = dict(Rwb=P, twb=P, v=P, bg=P, ba=P, fixed=P)
    a.update(over)
    return imu.Graph(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], a["fixed"], n, 0)


def _calls(fi):
    from monoorbslam3_amd import imu
    L = fi._L()
    cal = imu.Calib.make([1, 0, 0, 0, 1, 0, 0, 0, 1], [0, 0, 0], [1] * 6, [1] * 6)

    def jobs(**o):
        a = dict(init=P, edges=P, rec=P, n_kf=5, n_src=9, cap=9, fixed=P, init_out=P, edges_out=P, rec_out=P, prior_rec=P, result=P)
        a.update(o)
        return L.orbfi_jobs_device(a["init"], a["edges"], a["rec"], a["n_kf"], 1, a["n_src"], a["cap"], a["fixed"], a["init_out"], a["edges_out"], a["rec_out"],
                                   a["prior_rec"], a["result"], None)

    def linearize(**o):
        a = dict(graph=_graph(), bank=P, cap=9, edges=P, n_edges=4, info=P, bias_state=5, prior_rec=4, huber=4.1134, mode=0, work=P, err=P, chi2=P, chi2_prior=P,
                 total=P, H_diag=P, b=P, off_edges=P, H_off=P, flt=None, result=P)
        a.update(o)
        return L.orbfi_linearize_device(a["graph"], a["bank"], a["cap"], 9.8, a["edges"], a["n_edges"], a["info"], a["bias_state"], a["prior_rec"], 1e6, 1e12,
                                        a["huber"], a["mode"], a["work"], a["err"], a["chi2"], a["chi2_prior"], a["total"], a["H_diag"], a["b"], a["off_edges"],
                                        a["H_off"], a["flt"], a["result"], None)

    def recover(**o):
        a = dict(graph=_graph(), bias_state=5, jobs=P, n=5, dst=P, n_dst=9, bias=P, pose_R=P, pose_t=P, result=P)
        a.update(o)
        return L.orbfi_recover_device(a["graph"], cal, a["bias_state"], a["jobs"], a["n"], a["dst"], a["n_dst"], a["bias"], a["pose_R"], a["pose_t"], a["result"], None)

    return dict(jobs=(jobs, ("init", "edges", "rec", "fixed", "init_out", "edges_out", "rec_out", "prior_rec", "result"), ("n_kf", "n_src", "cap")),
                linearize=(linearize, ("bank", "edges", "info", "work", "err", "chi2", "chi2_prior", "total", "H_diag", "b", "off_edges", "H_off", "result"), ("cap",)),
                recover=(recover, ("jobs", "dst", "bias", "result"), ("n_dst",)))


def test_bad_arguments_are_refused_before_the_device_in_the_documented_order(fi):
    """a null pointer, a negative count, bias_state out of range, a mode outside 0..1, a huber_delta that is not a number, 32 key frames
    refused; an argument error wins over the limit; without a device a valid call fails with ORBX_E_NO_DEVICE"""
    calls = _calls(fi)
    for name, (call, pointers, counts) in calls.items():
        for key in pointers:
            returns(E_ARG, call, **{key: None})
        for key in counts:
            returns(E_ARG, call, **{key: 0}), returns(E_ARG, call, **{key: -1})
        large = dict(n_kf=32) if name == "jobs" else dict(graph=_graph(33), bias_state=32)
        limit = dict(n_kf=31) if name == "jobs" else dict(graph=_graph(32), bias_state=31)
        returns(E_UNSUPPORTED, call, **large), returns(E_ARG, call, **dict(large, **{pointers[0]: None}))     # the argument error first
        if name != "jobs":
            for field in ("Rwb", "twb", "v", "bg", "ba", "fixed"):
                returns(E_ARG, call, graph=_graph(6, **{field: None}), what=(name, field))
            returns(E_ARG, call, graph=_graph(-1)), returns(E_ARG, call, bias_state=6), returns(E_ARG, call, bias_state=-1)
            returns(E_ARG, call, bias_state=40, **{k: v for k, v in large.items() if k == "graph"})
        returns(E_NO_DEVICE, call), returns(E_NO_DEVICE, call, **limit)
    lin, rec = calls["linearize"][0], calls["recover"][0]
    returns(E_ARG, lin, n_edges=-1), returns(E_UNSUPPORTED, lin, n_edges=4097), returns(E_ARG, rec, n=-1), returns(E_UNSUPPORTED, rec, n=4097)
    returns(E_ARG, lin, mode=2), returns(E_ARG, lin, mode=-1), returns(E_ARG, lin, huber=float("nan"))
    returns(E_ARG, rec, pose_R=None), returns(E_ARG, rec, pose_t=None)
    # what is optional is optional: still the device that is missing, not an argument (with a device: tests/test_full_inertial_gpu.py)
    returns(E_NO_DEVICE, lin, mode=1, H_diag=None, b=None, off_edges=None, H_off=None), returns(E_NO_DEVICE, lin, n_edges=0)
    returns(E_NO_DEVICE, rec, pose_R=None, pose_t=None), returns(E_NO_DEVICE, lin, prior_rec=-1), returns(E_NO_DEVICE, lin, flt=P)


def test_the_documents_name_what_is_built():
    design, integration, readme = flat("DESIGN.md"), flat("INTEGRATION.md"), flat("README.md")
    for name in ENTRY_POINTS:
        assert name in design and name in integration, name
    assert "orbfi.h" in readme and "fullInertialOptimize" in design and "gravityOptimize" in design
    assert "fullInertialOptimize as a chain on one stream" in integration and "ORBI_EDGE_WALKS" in integration
    header = flat("include/orbfi.h")
    for call in ("orbm_inertial_window_problem_device", "orbfi_jobs_device", "orbi_graph_init_device", "orbi_edge_information_device", "orbfi_linearize_device",
                 "orbvw_linearize_device", "orbvw_reduce_device", "orbvw_solve_device", "orbvw_backsub_device", "orbi_graph_oplus_device", "orbfi_recover_device",
                 "orbm_local_ba_apply_device", "orbi_set_bias_device", "orbi_prior_information_device", "orbm_inertial_window_velocity_prior_device",
                 "orbm_build_observations_device", "orbm_refresh_points_device"):
        assert call in integration and (call in header or call.startswith("orbvw_")), call
    assert "ORBFI_MAX_KEYFRAMES" in header and "LIMIT" in header and "ORBI_EDGE_WALKS" in header
