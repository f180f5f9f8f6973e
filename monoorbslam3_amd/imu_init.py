"""Python mirror of the steps of the IMU initialisation on the device (include/orbii.h).

LocalMapping::initializeIMU (reference modules/Frontend/LocalMapping.cpp:374-482) for a caller who keeps the Levenberg-Marquardt loop:
the prior of the gravity direction and the velocities, the graph of Optimize::inertialOptimize (modules/Backend/Optimize.cpp:93-205), the
stages of one of its iterations and its recovery.  Every wrapper takes torch device tensors, enqueues on `stream` (torch's current stream
when None, _lib.stream_arg) and neither copies nor waits.  The records, the edges, the prior slots and the calibration are imu.RECORD,
imu.EDGE, imu.PRIOR and imu.Calib.

One trial of the loop is a chain on one stream ("IMU initialisation as a chain on one stream"):
  *d_lambda <- lambda; damp_device; vw.solve_device(n // 15, d_S, d_rhs, d_b, d_lambda, d_dx, d_out, ...) -- the ordered Cholesky for
  N <= 480 of include/orbvw.h, unchanged; push (copies of v, shared, iter); oplus_device; linearize_device(mode=1)
and the caller reads back the total and d_out[0] (with the solve's d_result).  The map rescale behind the recovery is
matcher.ORBMatcher.ApplyScaleRotationDevice.
"""
import ctypes as C

import numpy as np

from . import _lib
from .imu import Calib, _p

MAX_KF = 157
EDGE_WORK = 240
KIND_GS, KIND_G = 0, 1
SHARED_BG, SHARED_BA, SHARED_RWG, SHARED_SCALE = 0, 3, 6, 15
SUMMARY = 10


def system_size(n_kf):
    """ORBII_N: the unknowns of the padded dense system, 15 * ceil((9 + 3 n_kf) / 15)"""
    return 15 * ((9 + 3 * n_kf + 14) // 15)


class Bias(C.Structure):
    """orbii_bias: ImuCalib::initial_bias"""
    _fields_ = [("bg", C.c_float * 3), ("ba", C.c_float * 3)]

    @classmethod
    def make(cls, bias6):
        b = [float(v) for v in np.asarray(bias6, np.float32).reshape(6)]
        return cls((C.c_float * 3)(*b[:3]), (C.c_float * 3)(*b[3:]))


class Graph(C.Structure):
    """orbii_graph: device addresses of f64 v [n_kf, 3], shared [16], i32 iter [1] and the constants f64 Rwb [n_kf, 9], twb, Oc, Pcb [n_kf, 3]"""
    _fields_ = [("v", C.c_void_p), ("shared", C.c_void_p), ("iter", C.c_void_p), ("Rwb", C.c_void_p), ("twb", C.c_void_p), ("Oc", C.c_void_p),
                ("Pcb", C.c_void_p), ("n_kf", C.c_int32), ("pad", C.c_int32)]

    @classmethod
    def make(cls, d_v, d_shared, d_iter, d_Rwb, d_twb, d_Oc, d_Pcb, n_kf):
        return cls(_p(d_v), _p(d_shared), _p(d_iter), _p(d_Rwb), _p(d_twb), _p(d_Oc), _p(d_Pcb), n_kf, 0)


_vp, _i32, _f32, _f64 = C.c_void_p, C.c_int, C.c_float, C.c_double
_SIGS = {
    "orbii_prior_device": [_vp, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp],
    "orbii_graph_init_device": [Graph, Calib, _vp, _vp, _i32, _vp, _i32, _vp, Bias, _vp, _f64, _vp, _vp],
    "orbii_linearize_device": [Graph, _vp, _i32, _f32, _vp, _vp, Bias, _f32, _f32, _i32, _i32] + [_vp] * 10,
    "orbii_damp_device": [_i32, _i32] + [_vp] * 8,
    "orbii_oplus_device": [Graph, _i32, _vp, _vp, _vp],
    "orbii_recover_device": [Graph, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp],
}
_L = _lib.binder(_SIGS)


def prior_device(d_pose_R, d_pose_t, n_pose, d_state, n_src, d_bank, cap, d_priors, n_priors, d_jobs, n, d_Rwg, d_result, stream=None):
    """orbii_prior_device: LocalMapping.cpp:391-407 for n jobs (pose row, state row, record, prior slot) of d_jobs i32 [n, 4], oldest key
    frame first.  d_pose_R f64 [n_pose, 9], d_pose_t f64 [n_pose, 3]; d_state f32 [n_src, 15] and d_priors (u8 holding imu.PRIOR records):
    the velocities are written; d_Rwg f64 [9] (written)."""
    _lib.check(_L().orbii_prior_device(_p(d_pose_R), _p(d_pose_t), n_pose, _p(d_state), n_src, _p(d_bank), cap, _p(d_priors), n_priors, _p(d_jobs), n,
                                       _p(d_Rwg), _p(d_result), _lib.stream_arg(stream)))


def graph_init_device(graph, calib, d_pose_R, d_pose_t, n_pose, d_state, n_src, d_jobs, initial_bias, d_result, d_Rwg=None, scale=1.0, stream=None):
    """orbii_graph_init_device: the vertices and the edges' constants from the graph.n_kf jobs; initial_bias a Bias; d_Rwg f64 [9] or None
    (the identity)."""
    _lib.check(_L().orbii_graph_init_device(graph, calib, _p(d_pose_R), _p(d_pose_t), n_pose, _p(d_state), n_src, _p(d_jobs), initial_bias, _p(d_Rwg),
                                            float(scale), _p(d_result), _lib.stream_arg(stream)))


def linearize_device(graph, d_bank, cap, gravity, d_edges, d_info, initial_bias, priori_g, priori_a, kind, d_work, d_err, d_chi2, d_chi2_prior, d_total,
                     d_result, mode=0, d_H=None, d_b=None, d_float=None, stream=None):
    """orbii_linearize_device.  d_edges: u8 holding n_kf - 1 imu.EDGE records (only rec is read); f64: d_info [n_kf - 1, 81] (what
    imu.edge_information_device leaves), d_work [n_kf - 1, EDGE_WORK], d_err [n_kf - 1, 9], d_chi2 [n_kf - 1], d_chi2_prior [2], d_total [1],
    d_H [N, N], d_b [N] with N = system_size(n_kf); d_float f32 [n_kf - 1, 15].  mode 1 is computeError only."""
    _lib.check(_L().orbii_linearize_device(graph, _p(d_bank), cap, float(np.float32(gravity)), _p(d_edges), _p(d_info), initial_bias,
                                           float(np.float32(priori_g)), float(np.float32(priori_a)), kind, mode, _p(d_work), _p(d_err), _p(d_chi2),
                                           _p(d_chi2_prior), _p(d_total), _p(d_H), _p(d_b), _p(d_float), _p(d_result), _lib.stream_arg(stream)))


def damp_device(n_kf, kind, d_H, d_b, d_lambda, d_S, d_rhs, d_out, d_result, stream=None):
    """orbii_damp_device: d_S f64 [N, N] = d_H with *d_lambda on the free diagonal, d_rhs f64 [N] = d_b, d_out f64 [3]: [1] the largest
    undamped free diagonal entry.  (d_S, d_rhs) is what vw.solve_device(N // 15, d_S, d_rhs, d_b, d_lambda, d_dx, d_out, ...) takes."""
    _lib.check(_L().orbii_damp_device(n_kf, kind, _p(d_H), _p(d_b), _p(d_lambda), _p(d_S), _p(d_rhs), _p(d_out), _p(d_result), _lib.stream_arg(stream)))


def oplus_device(graph, kind, d_dx, d_result, stream=None):
    """orbii_oplus_device: the solve's d_dx f64 [N] applied to the biases, the gravity direction, the scale (kind 0) and the velocities"""
    _lib.check(_L().orbii_oplus_device(graph, kind, _p(d_dx), _p(d_result), _lib.stream_arg(stream)))


def recover_device(graph, d_jobs, d_state, n_src, d_priors, n_priors, d_bias, d_summary, d_result, stream=None):
    """orbii_recover_device: the velocities into d_state f32 [n_src, 15] and the prior slots; d_bias f32 [n_kf, 6], what imu.set_bias_device
    takes; d_summary f32 [SUMMARY] = (Rwg, scale), what ORBMatcher.ApplyScaleRotationDevice reads."""
    _lib.check(_L().orbii_recover_device(graph, _p(d_jobs), _p(d_state), n_src, _p(d_priors), n_priors, _p(d_bias), _p(d_summary), _p(d_result),
                                         _lib.stream_arg(stream)))
