"""Python mirror of fullInertialOptimize's shared-bias graph on the device (include/orbfi.h).

Optimize::fullInertialOptimize (reference modules/Backend/Optimize.cpp:239-442), the third step of LocalMapping::initializeIMU, for a
caller who keeps the Levenberg-Marquardt loop: one gyro and one accelerometer bias vertex for the whole map, held by a carrier state
behind the key frames of an imu.Graph.  Every wrapper takes torch device tensors, enqueues on `stream` (torch's current stream when
None, _lib.stream_arg) and neither copies nor waits.  The records, the edges and the calibration are imu.RECORD, imu.EDGE and imu.Calib.

One iteration of the loop is a chain on one stream ("fullInertialOptimize as a chain on one stream"):
  linearize_device; vw.linearize_device (n_solve = n_states = n_kf + 1); vw.reduce_device with d_off_edges / d_H_off as its edges
  (3 * n_edges of them); vw.solve_device; vw.backsub_device; imu.graph_oplus_device; both linearisations in mode 1 at the trial
and the caller reads back the totals and the two scale terms.
"""
import ctypes as C

import numpy as np

from . import _lib
from .imu import Calib, Graph, _p

MAX_KEYFRAMES = 31
EDGE_WORK = 482
HUBER_DELTA = 4.1134

_vp, _i32, _f32, _f64 = C.c_void_p, C.c_int, C.c_float, C.c_double
_SIGS = {
    "orbfi_jobs_device": [_vp, _vp, _vp, _i32, _i32, _i32, _i32] + [_vp] * 7,
    "orbfi_linearize_device": [Graph, _vp, _i32, _f32, _vp, _i32, _vp, _i32, _i32, _f32, _f32, _f64, _i32] + [_vp] * 12,
    "orbfi_recover_device": [Graph, Calib, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp],
}
_L = _lib.binder(_SIGS)


def jobs_device(d_init_jobs, d_inertial_edges, d_recover_jobs, n_kf, fix_first, n_src, cap, d_fixed, d_init_out, d_edges_out, d_recover_out,
                d_prior_rec, d_result, stream=None):
    """orbfi_jobs_device: from the lists of an all-key-frame ORBMatcher.InertialWindowProblemDevice (i32 [n_kf, 3], imu.EDGE [n_kf - 1],
    i32 [n_kf, 3]) the lists of the shared-bias graph: d_fixed u8 [n_kf + 1], d_init_out i32 [n_kf + 1, 3], d_edges_out imu.EDGE [n_kf - 1],
    d_recover_out i32 [n_kf, 3], d_prior_rec i32 [1]."""
    _lib.check(_L().orbfi_jobs_device(_p(d_init_jobs), _p(d_inertial_edges), _p(d_recover_jobs), n_kf, int(bool(fix_first)), n_src, cap, _p(d_fixed),
                                      _p(d_init_out), _p(d_edges_out), _p(d_recover_out), _p(d_prior_rec), _p(d_result), _lib.stream_arg(stream)))


def linearize_device(graph, d_bank, cap, gravity, d_edges, n_edges, d_info, bias_state, prior_rec, prior_g, prior_a, d_work, d_err, d_chi2,
                     d_chi2_prior, d_total, d_result, huber_delta=HUBER_DELTA, mode=0, d_H_diag=None, d_b=None, d_off_edges=None, d_H_off=None,
                     d_float=None, stream=None):
    """orbfi_linearize_device.  f64: d_info [n_edges, 81], d_work [n_edges, EDGE_WORK], d_err [n_edges, 9], d_chi2 [n_edges], d_chi2_prior [2],
    d_total [2], d_H_diag [n_states, 225], d_b [n_states, 15], d_H_off [3 * n_edges, 225]; d_off_edges: u8 holding 3 * n_edges imu.EDGE
    records; d_float f32 [n_edges, 15].  mode 1 is computeError only."""
    _lib.check(_L().orbfi_linearize_device(graph, _p(d_bank), cap, float(np.float32(gravity)), _p(d_edges), n_edges, _p(d_info), bias_state, prior_rec,
                                           float(np.float32(prior_g)), float(np.float32(prior_a)), float(huber_delta), mode, _p(d_work), _p(d_err),
                                           _p(d_chi2), _p(d_chi2_prior), _p(d_total), _p(d_H_diag), _p(d_b), _p(d_off_edges), _p(d_H_off), _p(d_float),
                                           _p(d_result), _lib.stream_arg(stream)))


def recover_device(graph, calib, bias_state, d_jobs, n, d_dst, n_dst, d_bias, d_result, d_pose_R=None, d_pose_t=None, stream=None):
    """orbfi_recover_device: n jobs (state, destination, flags) of d_jobs i32 [n, 3]; d_dst f32 [n_dst, 15]; d_bias f32 [n, 6]: the carrier's
    bias in every row, what imu.set_bias_device takes; d_pose_R f64 [n, 9] / d_pose_t f64 [n, 3]: T_cw for local_ba_apply_device."""
    _lib.check(_L().orbfi_recover_device(graph, calib, bias_state, _p(d_jobs), n, _p(d_dst), n_dst, _p(d_bias), _p(d_pose_R), _p(d_pose_t), _p(d_result),
                                         _lib.stream_arg(stream)))
