"""The ABI of the visual edges on the inertial graph and of the damped step without a GPU: every orbvi_* name include/orbvi.h declares
is exported by the built library and resolved by monoorbslam3_amd.vi; the layouts and constants are the header's; bad arguments are
reported before the device is looked for; without a GPU every call fails with ORBX_E_NO_DEVICE; orbi.h does not include orbvi.h."""
import ctypes as C
import re

import pytest

import vi_model as vm
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, built, declared, exported_and_mirrored, header, returns, stripped

ENTRY_POINTS = ["orbvi_linearize_device", "orbvi_solve_device"]


@pytest.fixture(scope="module")
def vi():
    return built("vi")


def test_every_declared_entry_point_is_exported_and_mirrored(vi):
    from monoorbslam3_amd import imu
    txt, names = stripped("orbvi.h"), declared("orbvi_", "orbvi.h")
    assert names == set(ENTRY_POINTS), sorted(names)
    exported_and_mirrored(vi, "orbvi_", names, sigs_equal=False)
    assert C.sizeof(vi.Camera) == 72 and vi.Graph is imu.Graph and vi.Calib is imu.Calib and C.sizeof(vi.Graph) == 56
    header = re.sub(r"\s+", " ", txt)
    for name, value in [("ORBVI_MAX_STATES", vi.MAX_STATES), ("ORBVI_EDGE_WORK", vi.EDGE_WORK), ("ORBVI_R_NONFINITE", vi.R_NONFINITE)]:
        assert "#define %s %d " % (name, value) in header, name
        assert getattr(vm, name[len("ORBVI_"):]) == value, name
    assert vi.HUBER_MONO == vm.HUBER_MONO and vi.CHI2_MONO == vm.CHI2_MONO
    assert '#include "orbi.h"' in txt


def test_the_binder_binds_once_and_a_missing_symbol_raises(vi):
    """_lib.binder, which every module's _L() is: nothing is loaded before the first use, the first use sets every signature, a second
    use neither loads nor binds again, and a name the library lacks raises AttributeError at first use -- with the built library too"""
    from monoorbslam3_amd import _lib

    class Fn:
        restype = argtypes = "unset"

    class Lib:
        def __init__(self):
            self.orbt_a, self.orbt_b = Fn(), Fn()

    loads = []

    def load():
        loads.append(Lib())
        return loads[-1]

    get = _lib.binder({"orbt_a": [C.c_int], "orbt_b": (None, [C.c_void_p])}, load)
    assert not loads
    L = get()
    assert (L.orbt_a.restype, L.orbt_a.argtypes, L.orbt_b.restype, L.orbt_b.argtypes) == (C.c_int, [C.c_int], None, [C.c_void_p])
    L.orbt_a.argtypes = "kept"
    assert get() is L and len(loads) == 1 and L.orbt_a.argtypes == "kept"
    missing = _lib.binder({"orbt_a": [], "orbt_missing": []}, load)
    for _ in range(2):
        with pytest.raises(AttributeError):
            missing()
    with pytest.raises(AttributeError):
        _lib.binder({"orbvi_no_such_entry_point": []})()
    assert vi._L() is _lib.lib() and vi._L() is vi._L()
    for name, args in vi._SIGS.items():
        assert getattr(vi._L(), name).argtypes == args and getattr(vi._L(), name).restype is C.c_int, name


def test_orbi_h_still_does_not_include_orbvi_h():
    for name in ("orbi.h", "orbi_factors.h", "orbx.h", "orbba.h"):
        assert "orbvi" not in header(name), name


def _calls(vi, **over):
    """both wrappers with valid arguments (the fake device address) except for `over`"""
    p = P
    a = dict(Rwb=p, twb=p, v=p, bg=p, ba=p, fixed=p, n_states=2, n_groups=1, cap_edges=400, group_state=p, edge_off=p, points=p, z=p, w=p,
             active=p, delta=vm.HUBER_MONO, threshold=vm.CHI2_MONO, mode=0, work=p, err=p, chi2=p, total=p, H_diag=p, b=p, n_inliers=p, result=p,
             camera_model=0, edges=p, n_edges=1, cap=4, H_off=p, lam=p, dx=p, out=p)
    a.update(over)
    import imu_model as im
    c = im.calib()
    cal = vi.Calib.make(c["Rcb"], c["tcb"], c["cov_noise"], c["cov_walk"], c["gravity"])
    g = vi.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], a["fixed"], a["n_states"])
    cam = vi.Camera.make(458.0, 457.0, 367.0, 248.0, a["camera_model"])
    return dict(
        linearize=lambda: vi.linearize_device(g, cal, cam, a["n_groups"], a["cap_edges"], a["group_state"], a["edge_off"], a["points"], a["z"], a["w"],
                                              a["err"], a["chi2"], a["result"], a["active"], a["delta"], a["threshold"], a["mode"], a["total"],
                                              a["H_diag"], a["b"], a["n_inliers"], a["work"]),
        solve=lambda: vi.solve_device(a["n_states"], a["fixed"], a["edges"], a["n_edges"], a["cap"], a["H_diag"], a["H_off"], a["b"], a["lam"],
                                      a["dx"], a["out"], a["result"]))


def test_argument_errors_are_reported_before_the_device_is_looked_for(vi):
    both, lin, sol = ("linearize", "solve"), ("linearize",), ("solve",)
    cases = [(dict(result=None), both), (dict(fixed=None), both), (dict(H_diag=None), both), (dict(b=None), both), (dict(n_states=-1), both)]
    cases += [(dict([(k, None)]), lin) for k in ("Rwb", "twb", "v", "bg", "ba", "group_state", "edge_off", "points", "z", "w", "err", "chi2", "total", "work")]
    cases += [(dict(n_groups=-1), lin), (dict(cap_edges=-1), lin), (dict(mode=3), lin), (dict(mode=-1), lin), (dict(delta=float("nan")), lin),
              (dict(threshold=float("nan")), lin), (dict(camera_model=2), lin), (dict(camera_model=-1), lin),
              (dict(mode=2, active=None), lin), (dict(mode=2, n_inliers=None), lin), (dict(mode=1, total=None), lin)]
    cases += [(dict([(k, None)]), sol) for k in ("edges", "H_off", "lam", "dx", "out")]
    cases += [(dict(n_edges=-1), sol), (dict(cap=0), sol), (dict(n_states=0), sol)]
    for over, names in cases:
        for name in names:
            returns(E_ARG, _calls(vi, **over)[name], what=(over, name))
    for over, names in [(dict(n_states=vi.MAX_STATES + 1), sol), (dict(n_edges=4097), sol), (dict(n_groups=4097), lin), (dict(n_states=4097), lin)]:
        for name in names:
            returns(E_UNSUPPORTED, _calls(vi, **over)[name], what=(over, name))
    # an argument error wins over the unsupported size, and both over the missing device
    returns(E_ARG, _calls(vi, n_states=vi.MAX_STATES + 1, dx=None)["solve"])


def test_every_wrapper_fails_loudly_without_a_gpu(vi):
    for name, call in _calls(vi).items():
        returns(E_NO_DEVICE, call, what=name)                   # and "no HIP device" in the message
    # the optional arguments are optional: still the device that is missing, not an argument
    returns(E_NO_DEVICE, _calls(vi, mode=1, H_diag=None, b=None, work=None, active=None, n_inliers=None)["linearize"])
    returns(E_NO_DEVICE, _calls(vi, mode=2, H_diag=None, b=None, work=None, total=None)["linearize"])
    returns(E_NO_DEVICE, _calls(vi, active=None, n_inliers=None)["linearize"])
    returns(E_NO_DEVICE, _calls(vi, n_groups=0, cap_edges=0)["linearize"]), returns(E_NO_DEVICE, _calls(vi, camera_model=1)["linearize"])
    returns(E_NO_DEVICE, _calls(vi, n_edges=0, edges=None, H_off=None)["solve"]), returns(E_NO_DEVICE, _calls(vi, n_states=vi.MAX_STATES)["solve"])
