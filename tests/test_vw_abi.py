"""The ABI of the visual window of the inertial local bundle adjustment without a GPU: every orbvw_* name include/orbvw.h declares is
exported by the built library and resolved by monoorbslam3_amd.vw; the constants are the header's; bad arguments are reported before
the device is looked for; each limit is ORBX_E_UNSUPPORTED; without a GPU every call fails with ORBX_E_NO_DEVICE; nothing includes
orbvw.h."""
import ctypes as C
import os
import re

import pytest

import vw_model as wm
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, ROOT, built, declared, exported_and_mirrored, header, returns, stripped

ENTRY_POINTS = ["orbvw_linearize_device", "orbvw_reduce_device", "orbvw_solve_device", "orbvw_backsub_device"]


@pytest.fixture(scope="module")
def vw():
    return built("vw")


def test_every_declared_entry_point_is_exported_and_mirrored(vw):
    from monoorbslam3_amd import imu, vi
    txt, names = stripped("orbvw.h"), declared("orbvw_", "orbvw.h")
    assert names == set(ENTRY_POINTS), sorted(names)
    exported_and_mirrored(vw, "orbvw_", names, sigs_equal=True)
    assert vw.Graph is imu.Graph and vw.Calib is imu.Calib and vw.Camera is vi.Camera and C.sizeof(vw.Camera) == 72 and imu.EDGE.itemsize == 16
    header = re.sub(r"\s+", " ", txt)
    for name, text, value in [("ORBVW_MAX_SOLVE_STATES", "32", vw.MAX_SOLVE_STATES), ("ORBVW_MAX_EDGES", "(1 << 20)", vw.MAX_EDGES),
                              ("ORBVW_MAX_POINTS", "(1 << 18)", vw.MAX_POINTS), ("ORBVW_MAX_OBS", "256", vw.MAX_OBS), ("ORBVW_EDGE_WORK", "24", vw.EDGE_WORK),
                              ("ORBVW_R_OUTLIER", "5", vw.R_OUTLIER), ("ORBVW_R_POINT_SINGULAR", "6", vw.R_POINT_SINGULAR)]:
        assert "#define %s %s " % (name, text) in header, name
        assert eval(text) == value == getattr(wm, name[len("ORBVW_"):]), name
    assert vw.HUBER_MONO == wm.HUBER_MONO and vw.CHI2_MONO == wm.CHI2_MONO and vw.R_NONFINITE == wm.R_NONFINITE
    assert '#include "orbvi.h"' in txt


def test_nothing_includes_orbvw_h():
    for name in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if name != "orbvw.h":
            assert "orbvw" not in header(name), name
    csrc = os.path.join(ROOT, "monoorbslam3_amd", "csrc")
    for name in sorted(os.listdir(csrc)):
        if name.endswith((".hip", ".h")) and name != "orbvw.hip":
            assert "orbvw" not in open(os.path.join(csrc, name)).read(), name


LIN = ("Rwb", "twb", "v", "bg", "ba", "gfixed", "points", "edge_state", "edge_point", "z", "w", "point_off", "err", "chi2", "total", "work", "H_diag", "b", "Hll", "bl", "Hlp")


def _calls(vw, **over):
    """the four wrappers with valid arguments (the fake device address) except for `over`"""
    p = P
    a = dict({k: p for k in LIN + ("active", "outlier", "result", "fixed", "edges", "H_off", "lam", "S", "rhs", "Hll_inv", "tl", "out", "dx", "xl", "points_out",
                                   "out_points")},
             n_states=12, n_solve=10, n_points=500, cap_edges=2000, delta=wm.HUBER_MONO, threshold=wm.CHI2_MONO, mode=0, camera_model=0, n_edges=9, cap=16)
    a["points_out"] = 2 * P                                     # the updated points may not be the points
    a.update(over)
    import imu_model as im
    c = im.calib()
    cal = vw.Calib.make(c["Rcb"], c["tcb"], c["cov_noise"], c["cov_walk"], c["gravity"])
    g = vw.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], a["gfixed"], a["n_states"])
    cam = vw.Camera.make(458.0, 457.0, 367.0, 248.0, a["camera_model"])
    return dict(
        linearize=lambda: vw.linearize_device(g, cal, cam, a["n_solve"], a["n_points"], a["cap_edges"], a["points"], a["edge_state"], a["edge_point"], a["z"], a["w"],
                                              a["point_off"], a["err"], a["chi2"], a["result"], a["active"], a["delta"], a["threshold"], a["mode"], a["total"],
                                              a["work"], a["H_diag"], a["b"], a["Hll"], a["bl"], a["Hlp"], a["outlier"]),
        reduce=lambda: vw.reduce_device(a["n_solve"], a["fixed"], a["edges"], a["n_edges"], a["cap"], a["H_diag"], a["H_off"], a["b"], a["lam"], a["n_points"],
                                        a["cap_edges"], a["point_off"], a["edge_state"], a["Hll"], a["bl"], a["Hlp"], a["S"], a["rhs"], a["Hll_inv"], a["tl"], a["out"],
                                        a["result"]),
        solve=lambda: vw.solve_device(a["n_solve"], a["S"], a["rhs"], a["b"], a["lam"], a["dx"], a["out"], a["result"]),
        backsub=lambda: vw.backsub_device(a["n_solve"], a["n_points"], a["cap_edges"], a["point_off"], a["edge_state"], a["Hlp"], a["Hll_inv"], a["bl"], a["dx"],
                                          a["lam"], a["points"], a["xl"], a["points_out"], a["out_points"], a["result"]))


def test_argument_errors_are_reported_before_the_device_is_looked_for(vw):
    every, lin, red, sol, bck = ("linearize", "reduce", "solve", "backsub"), ("linearize",), ("reduce",), ("solve",), ("backsub",)
    cases = [(dict(result=None), every), (dict(n_solve=0), every), (dict(n_solve=-1), every), (dict(b=None), ("linearize", "reduce", "solve")),
             (dict(lam=None), ("reduce", "solve", "backsub")), (dict(n_points=0), ("linearize", "reduce", "backsub")), (dict(n_points=-1), ("linearize", "reduce", "backsub")),
             (dict(cap_edges=-1), ("linearize", "reduce", "backsub")), (dict(point_off=None), ("linearize", "reduce", "backsub")),
             (dict(edge_state=None), ("linearize", "reduce", "backsub")), (dict(Hlp=None), ("linearize", "reduce", "backsub")),
             (dict(bl=None), ("linearize", "reduce", "backsub")), (dict(Hll=None), ("linearize", "reduce")), (dict(H_diag=None), ("linearize", "reduce")),
             (dict(S=None), ("reduce", "solve")), (dict(rhs=None), ("reduce", "solve")), (dict(out=None), ("reduce", "solve")), (dict(Hll_inv=None), ("reduce", "backsub")),
             (dict(dx=None), ("solve", "backsub")), (dict(points=None), ("linearize", "backsub"))]
    cases += [(dict([(k, None)]), lin) for k in ("Rwb", "twb", "v", "bg", "ba", "gfixed", "edge_point", "z", "w", "err", "chi2", "total", "work")]
    cases += [(dict(n_states=-1), lin), (dict(n_solve=13), lin), (dict(mode=3), lin), (dict(mode=-1), lin), (dict(delta=float("nan")), lin),
              (dict(threshold=float("nan")), lin), (dict(camera_model=2), lin), (dict(camera_model=-1), lin), (dict(mode=2, outlier=None), lin),
              (dict(mode=1, total=None), lin)]
    cases += [(dict([(k, None)]), red) for k in ("fixed", "edges", "H_off", "tl")] + [(dict(n_edges=-1), red), (dict(cap=0), red)]
    cases += [(dict([(k, None)]), bck) for k in ("xl", "points_out", "out_points")] + [(dict(points_out=P), bck)]
    for over, names in cases:
        for name in names:
            returns(E_ARG, _calls(vw, **over)[name], what=(over, name))
    limits = [(dict(n_solve=vw.MAX_SOLVE_STATES + 1, n_states=40), every), (dict(cap_edges=vw.MAX_EDGES + 1), ("linearize", "reduce", "backsub")),
              (dict(n_points=vw.MAX_POINTS + 1), ("linearize", "reduce", "backsub")), (dict(n_states=4097), lin), (dict(n_edges=4097), red)]
    for over, names in limits:
        for name in names:
            returns(E_UNSUPPORTED, _calls(vw, **over)[name], what=(over, name))
    # an argument error wins over the unsupported size, and both over the missing device
    for name, over in (("linearize", dict(err=None)), ("reduce", dict(S=None)), ("solve", dict(dx=None)), ("backsub", dict(xl=None))):
        returns(E_ARG, _calls(vw, n_solve=vw.MAX_SOLVE_STATES + 1, n_states=40, **over)[name], what=name)


def test_every_wrapper_fails_loudly_without_a_gpu(vw):
    for name, call in _calls(vw).items():
        returns(E_NO_DEVICE, call, what=name)                   # and "no HIP device" in the message
    # the optional arguments are optional and the limits themselves are supported: still the device that is missing
    null0 = dict(work=None, H_diag=None, b=None, Hll=None, bl=None, Hlp=None)
    returns(E_NO_DEVICE, _calls(vw, mode=1, active=None, outlier=None, **null0)["linearize"])
    returns(E_NO_DEVICE, _calls(vw, mode=2, active=None, total=None, **null0)["linearize"])
    returns(E_NO_DEVICE, _calls(vw, active=None, outlier=None)["linearize"]), returns(E_NO_DEVICE, _calls(vw, camera_model=1, cap_edges=0)["linearize"])
    returns(E_NO_DEVICE, _calls(vw, n_edges=0, edges=None, H_off=None)["reduce"])
    top = dict(n_solve=vw.MAX_SOLVE_STATES, n_states=vw.MAX_SOLVE_STATES, cap_edges=vw.MAX_EDGES, n_points=vw.MAX_POINTS, n_edges=4096)
    for name, call in _calls(vw, **top).items():
        returns(E_NO_DEVICE, call, what=name)
