"""The ABI of the inertial factors without a GPU: every orbi_* name that include/orbi.h declares -- itself or through the
orbi_factors.h it includes -- is exported by the built library and resolved by monoorbslam3_amd.imu; the layouts are the header's;
bad arguments are reported before the device is looked for; without a GPU every call fails with ORBX_E_NO_DEVICE."""
import ctypes as C
import re

import pytest

import abi_checks as abi
import factors_model as fm
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, returns

FACTOR_ENTRY_POINTS = ["orbi_edge_information_device", "orbi_graph_init_device", "orbi_graph_oplus_device", "orbi_graph_recover_device",
                       "orbi_linearize_device", "orbi_prior_information_device"]


@pytest.fixture(scope="module")
def imu():
    return abi.built("imu")


def test_every_declared_entry_point_is_exported_and_mirrored(imu):
    declared = abi.declared("orbi_", "orbi.h", follow_includes=True)      # itself or through the orbi_factors.h it includes
    assert set(FACTOR_ENTRY_POINTS) <= declared and len(declared) == 12, sorted(declared)
    abi.exported_and_mirrored(imu, "orbi_", declared, sigs_equal=False)
    assert imu.EDGE == fm.EDGE and imu.PRIOR == fm.PRIOR and imu.PRIOR_JOB == fm.PRIOR_JOB and C.sizeof(imu.Graph) == 56
    header = re.sub(r"\s+", " ", abi.header("orbi_factors.h"))
    for name, value in [("ORBI_FIX_POSE", imu.FIX_POSE), ("ORBI_FIX_VELO", imu.FIX_VELO), ("ORBI_FIX_GYRO", imu.FIX_GYRO), ("ORBI_FIX_ACC", imu.FIX_ACC),
                        ("ORBI_EDGE_WALKS", imu.EDGE_WALKS), ("ORBI_PRIOR_VELO", imu.PRIOR_VELO), ("ORBI_PRIOR_GYRO", imu.PRIOR_GYRO),
                        ("ORBI_PRIOR_ACC", imu.PRIOR_ACC), ("ORBI_PRIOR_ACC_GYRO_INFO", imu.PRIOR_ACC_GYRO_INFO), ("ORBI_RECOVER_POSE", imu.RECOVER_POSE),
                        ("ORBI_R_PRIOR_DONE", imu.R_PRIOR_DONE), ("ORBI_R_PRIOR_RANGE", imu.R_PRIOR_RANGE), ("ORBI_EDGE_WORK", imu.EDGE_WORK),
                        ("ORBI_JACOBI_SWEEPS", imu.JACOBI_SWEEPS)]:
        assert "#define %s %d " % (name, value) in header, name
        assert getattr(fm, name[len("ORBI_"):], value) == value, name


def _calls(imu, **over):
    """every wrapper with valid arguments (the fake device address) except for `over`"""
    p = P
    a = dict(Rwb=p, twb=p, v=p, bg=p, ba=p, fixed=p, n_states=3, bank=p, cap=8, src=p, n_src=3, jobs=p, n=2, result=p, priors=p, n_priors=2,
             edges=p, n_edges=2, info=p, walk=p, work=p, err=p, chi2=p, total=p, pjobs=p, n_pjobs=1, chi2_prior=p, delta=4.1134, mode=0,
             H_diag=p, H_off=p, b=p, J=p, flt=p, dx=p, it=p, dst=p, n_dst=3, bias=p, pose_R=p, pose_t=p)
    a.update(over)
    import imu_model as im
    c = im.calib()
    cal = imu.Calib.make(c["Rcb"], c["tcb"], c["cov_noise"], c["cov_walk"], c["gravity"])
    g = imu.Graph.make(a["Rwb"], a["twb"], a["v"], a["bg"], a["ba"], a["fixed"], a["n_states"])
    return dict(
        prior_information=lambda: imu.prior_information_device(a["priors"], a["n_priors"], a["bank"], a["cap"], a["jobs"], a["n"], a["result"], a["src"], a["n_src"]),
        graph_init=lambda: imu.graph_init_device(g, a["bank"], a["cap"], a["src"], a["n_src"], a["jobs"], a["n"], a["result"]),
        edge_information=lambda: imu.edge_information_device(a["bank"], a["cap"], a["edges"], a["n_edges"], a["info"], a["walk"], a["result"]),
        linearize=lambda: imu.linearize_device(g, a["bank"], a["cap"], 9.8, a["edges"], a["n_edges"], a["info"], a["walk"], a["work"], a["err"], a["chi2"],
                                               a["total"], a["result"], a["priors"], a["n_priors"], a["pjobs"], a["n_pjobs"], a["chi2_prior"], a["delta"],
                                               a["mode"], a["H_diag"], a["H_off"], a["b"], a["J"], a["flt"]),
        graph_oplus=lambda: imu.graph_oplus_device(g, a["dx"], a["it"], a["result"]),
        graph_recover=lambda: imu.graph_recover_device(g, cal, a["jobs"], a["n"], a["dst"], a["n_dst"], a["bias"], a["result"], a["pose_R"], a["pose_t"]))


GRAPH_CALLS = ("graph_init", "linearize", "graph_oplus", "graph_recover")


def test_argument_errors_are_reported_before_the_device_is_looked_for(imu):
    every = tuple(_calls(imu))
    cases = [(dict(result=None), every), (dict(n_states=-1), GRAPH_CALLS), (dict(bank=None), ("prior_information", "graph_init", "edge_information", "linearize")),
             (dict(cap=0), ("prior_information", "graph_init", "edge_information", "linearize")),
             (dict(jobs=None), ("prior_information", "graph_init", "graph_recover")), (dict(n=-1), ("prior_information", "graph_init", "graph_recover")),
             (dict(priors=None), ("prior_information", "linearize")), (dict(n_priors=0), ("prior_information",)), (dict(n_src=-1), ("prior_information",)),
             (dict(src=None), ("graph_init",)), (dict(n_src=0), ("graph_init",)),
             (dict(edges=None), ("edge_information", "linearize")), (dict(n_edges=-1), ("edge_information", "linearize")),
             (dict(info=None), ("edge_information", "linearize")), (dict(walk=None), ("edge_information", "linearize")),
             (dict(dx=None), ("graph_oplus",)), (dict(it=None), ("graph_oplus",)),
             (dict(dst=None), ("graph_recover",)), (dict(n_dst=0), ("graph_recover",)), (dict(bias=None), ("graph_recover",)),
             (dict(pose_R=None), ("graph_recover",)), (dict(pose_t=None), ("graph_recover",))]
    cases += [(dict([(k, None)]), GRAPH_CALLS) for k in ("Rwb", "twb", "v", "bg", "ba", "fixed")]
    cases += [(dict([(k, None)]), ("linearize",)) for k in ("work", "err", "chi2", "total", "pjobs", "chi2_prior", "H_diag", "H_off", "b")]
    cases += [(dict(mode=2), ("linearize",)), (dict(mode=-1), ("linearize",)), (dict(delta=float("nan")), ("linearize",)), (dict(n_pjobs=-1), ("linearize",))]
    for over, names in cases:
        for name in names:
            returns(E_ARG, _calls(imu, **over)[name], what=(over, name))
    for over, names in [(dict(n=imu.MAX_JOBS + 1), ("prior_information", "graph_init", "graph_recover")), (dict(n_states=imu.MAX_JOBS + 1), GRAPH_CALLS),
                        (dict(n_edges=imu.MAX_JOBS + 1), ("edge_information", "linearize")), (dict(n_pjobs=imu.MAX_JOBS + 1), ("linearize",))]:
        for name in names:
            returns(E_UNSUPPORTED, _calls(imu, **over)[name], what=(over, name))


def test_every_wrapper_fails_loudly_without_a_gpu(imu):
    for name, call in _calls(imu).items():
        returns(E_NO_DEVICE, call, what=name)                   # and "no HIP device" in the message
    # the optional arguments are optional: still the device that is missing, not an argument
    returns(E_NO_DEVICE, _calls(imu, mode=1, H_diag=None, H_off=None, b=None, J=None, flt=None)["linearize"])
    returns(E_NO_DEVICE, _calls(imu, n_pjobs=0, pjobs=None, priors=None, chi2_prior=None, n_priors=0)["linearize"])
    returns(E_NO_DEVICE, _calls(imu, pose_R=None, pose_t=None)["graph_recover"]), returns(E_NO_DEVICE, _calls(imu, src=None, n_src=0)["prior_information"])
    returns(E_NO_DEVICE, _calls(imu, n=0)["graph_init"]), returns(E_NO_DEVICE, _calls(imu, n_edges=0)["linearize"])
