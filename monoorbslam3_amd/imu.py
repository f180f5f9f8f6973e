"""Python mirror of the device-resident IMU preintegration and pose prediction (include/orbi.h).

The reference's PreIntegrator (modules/Sensor/Imu.cpp:76-204), Frame::computePreIntegration (Frame.cpp:73-88) and the tracker's
prediction (Tracking.cpp:185-243, Frame.cpp:57-71) on a bank of records, a measurement pool and poses that live in device memory:
every wrapper takes torch device tensors, enqueues on `stream` (torch's current stream when None, _lib.stream_arg) and neither
copies nor waits.  The numpy dtypes below are the header's layouts.

The second half mirrors the header's section "Inertial factors linearised on the device" (include/orbi_factors.h): the vertices of
the inertial optimisers (Optimize.cpp:547-608, :610-760, :960-1060, :1090-1250) as a Graph of device arrays, and the per-iteration
linearisation of their inertial edges, bias walks and priors for a caller who keeps g2o's solver.
"""
import ctypes as C

import numpy as np

from . import _lib

MAX_JOBS = 4096
RECORD_BYTES = 1232
R_DONE, R_RANGE, R_DUPLICATE, R_REFUSED, R_NEED, R_REINTEGRATED, R_NOOP = range(7)

RECORD = np.dtype([("bias", "<f4", 6), ("updated_bias", "<f4", 6), ("delta_bias", "<f4", 6), ("delta_t", "<f4"), ("dR", "<f4", 9),
                   ("dV", "<f4", 3), ("dP", "<f4", 3), ("JRg", "<f4", 9), ("JVg", "<f4", 9), ("JVa", "<f4", 9), ("JPg", "<f4", 9),
                   ("JPa", "<f4", 9), ("C", "<f4", 225), ("n_meas", "<i4"), ("pad", "<i4", 3)])
SAMPLE = np.dtype([("w", "<f4", 3), ("a", "<f4", 3), ("t", "<f8")])
JOB = np.dtype([("id", "<i4"), ("first", "<i4"), ("count", "<i4"), ("pad", "<i4"), ("timestamp", "<f8"), ("end_time", "<f8")])
assert RECORD.itemsize == RECORD_BYTES and SAMPLE.itemsize == 32 and JOB.itemsize == 32

# ---- inertial factors (include/orbi_factors.h) ----
FIX_POSE, FIX_VELO, FIX_GYRO, FIX_ACC = 1, 2, 4, 8
EDGE_WALKS = 1
PRIOR_VELO, PRIOR_GYRO, PRIOR_ACC, PRIOR_ACC_GYRO_INFO = 1, 2, 4, 8
RECOVER_POSE = 1
R_PRIOR_DONE, R_PRIOR_RANGE = 4, 5
EDGE_WORK = 488
JACOBI_SWEEPS = 6
EDGE = np.dtype([("i", "<i4"), ("j", "<i4"), ("rec", "<i4"), ("flags", "<i4")])
PRIOR = np.dtype([("velo_priori", "<f4", 3), ("bias_priori", "<f4", 6), ("velo_info", "<f4", 9), ("gyro_info", "<f4", 9), ("acc_info", "<f4", 9)])
PRIOR_JOB = np.dtype([("state", "<i4"), ("prior", "<i4"), ("mask", "<i4")])
assert EDGE.itemsize == 16 and PRIOR.itemsize == 144 and PRIOR_JOB.itemsize == 12


class Calib(C.Structure):
    """orbi_calib: ImuCalib's T_cb, the diagonals of its two covariances, GRAVITY_VALUE"""
    _fields_ = [("Rcb", C.c_float * 9), ("tcb", C.c_float * 3), ("cov_noise", C.c_float * 6), ("cov_walk", C.c_float * 6),
                ("gravity", C.c_float)]

    @classmethod
    def make(cls, Rcb, tcb, cov_noise, cov_walk, gravity=9.8):
        f = lambda a, n: (C.c_float * n)(*[float(v) for v in np.asarray(a, np.float32).reshape(n)])  # noqa: E731
        return cls(f(Rcb, 9), f(tcb, 3), f(cov_noise, 6), f(cov_walk, 6), float(np.float32(gravity)))


class Graph(C.Structure):
    """orbi_graph: the vertices, device addresses of f64 [n, 9], [n, 3] x 4 and u8 [n]"""
    _fields_ = [("Rwb", C.c_void_p), ("twb", C.c_void_p), ("v", C.c_void_p), ("bg", C.c_void_p), ("ba", C.c_void_p), ("fixed", C.c_void_p),
                ("n_states", C.c_int32), ("pad", C.c_int32)]

    @classmethod
    def make(cls, d_Rwb, d_twb, d_v, d_bg, d_ba, d_fixed, n_states):
        return cls(_p(d_Rwb), _p(d_twb), _p(d_v), _p(d_bg), _p(d_ba), _p(d_fixed), n_states, 0)


_vp, _i32 = C.c_void_p, C.c_int
_SIGS = {
    "orbi_reset_device": [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp],
    "orbi_integrate_device": [Calib, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp],
    "orbi_set_bias_device": [Calib, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp],
    "orbi_merge_next_device": [Calib, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp],
    "orbi_predict_device": [Calib, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "orbi_imu_pose_device": [Calib, _vp, _vp, _vp, _vp],
    "orbi_prior_information_device": [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp],
    "orbi_graph_init_device": [Graph, _vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp],
    "orbi_edge_information_device": [_vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp],
    "orbi_linearize_device": [Graph, _vp, _i32, C.c_float, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, C.c_double, _i32] + [_vp] * 12,
    "orbi_graph_oplus_device": [Graph, _vp, _vp, _vp, _vp],
    "orbi_graph_recover_device": [Graph, Calib, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp],
}
_L = _lib.binder(_SIGS)


def _p(t):
    """device address of a torch tensor, None for None, a plain int passed through (a raw device pointer)"""
    return None if t is None else t if isinstance(t, int) else t.data_ptr()


def reset_device(d_bank, cap, d_ids, n, d_result, d_src=None, d_bias=None, stream=None):
    """orbi_reset_device: Reset(bias) / the three constructors for the records d_ids[0..n).  d_bank: u8 [cap * 1232]; d_ids, d_src i32;
    d_bias f32 [n, 6]; d_result i32 [8] (written)."""
    _lib.check(_L().orbi_reset_device(_p(d_bank), cap, _p(d_ids), _p(d_src), _p(d_bias), n, _p(d_result), _lib.stream_arg(stream)))


def integrate_device(calib, d_bank, d_pool, cap, cap_meas, d_jobs, n, d_samples, n_samples, d_result, stream=None):
    """orbi_integrate_device: computePreIntegration for n jobs.  d_pool: f32 [cap, cap_meas, 7]; d_jobs: u8 holding JOB records;
    d_samples: u8 holding SAMPLE records."""
    _lib.check(_L().orbi_integrate_device(calib, _p(d_bank), _p(d_pool), cap, cap_meas, _p(d_jobs), n, _p(d_samples), n_samples, _p(d_result),
                                          _lib.stream_arg(stream)))


def set_bias_device(calib, d_bank, d_pool, cap, cap_meas, d_ids, d_bias, n, d_result, stream=None):
    """orbi_set_bias_device: setNewBias (with ReIntegrate past 0.01) for the records d_ids[0..n), one bias of d_bias f32 [n, 6] each."""
    _lib.check(_L().orbi_set_bias_device(calib, _p(d_bank), _p(d_pool), cap, cap_meas, _p(d_ids), _p(d_bias), n, _p(d_result),
                                         _lib.stream_arg(stream)))


def merge_next_device(calib, d_bank, d_pool, cap, cap_meas, d_ids, d_next, n, d_result, stream=None):
    """orbi_merge_next_device: MergeNext, record d_ids[j] takes in the measurements of record d_next[j]."""
    _lib.check(_L().orbi_merge_next_device(calib, _p(d_bank), _p(d_pool), cap, cap_meas, _p(d_ids), _p(d_next), n, _p(d_result),
                                           _lib.stream_arg(stream)))


def predict_device(calib, d_bank, cap, rec_id, d_src, d_dst, d_pose_R=None, d_pose_t=None, stream=None):
    """orbi_predict_device: the new frame's (Rwb, twb, v) in d_dst f32 [15] from d_src f32 [15] and record rec_id; T_cw in d_pose_R f64 [9],
    d_pose_t f64 [3] -- the `pose_R` / `pose_t` that ORBMatcher.Project*Device and ba.pose_optimize_batch_device read."""
    _lib.check(_L().orbi_predict_device(calib, _p(d_bank), cap, rec_id, _p(d_src), _p(d_dst), _p(d_pose_R), _p(d_pose_t), _lib.stream_arg(stream)))


def imu_pose_device(calib, d_pose_R, d_pose_t, d_dst, stream=None):
    """orbi_imu_pose_device: T_wb = T_cw.inverse() * T_cb into d_dst[0..12) from the doubles poseOptimize leaves; d_dst[12..15) untouched."""
    _lib.check(_L().orbi_imu_pose_device(calib, _p(d_pose_R), _p(d_pose_t), _p(d_dst), _lib.stream_arg(stream)))


def prior_information_device(d_priors, n_priors, d_bank, cap, d_jobs, n, d_result, d_src=None, n_src=0, stream=None):
    """orbi_prior_information_device: setPrioriInformation and the constructor's priors for n jobs (prior slot, record, source state) of
    d_jobs i32 [n, 3].  d_priors: u8 holding PRIOR records; d_src f32 [n_src, 15]."""
    _lib.check(_L().orbi_prior_information_device(_p(d_priors), n_priors, _p(d_bank), cap, _p(d_src), n_src, _p(d_jobs), n, _p(d_result),
                                                  _lib.stream_arg(stream)))


def graph_init_device(graph, d_bank, cap, d_src, n_src, d_jobs, n, d_result, stream=None):
    """orbi_graph_init_device: the vertices of n jobs (state, source state, record or -1) of d_jobs i32 [n, 3] from d_src f32 [n_src, 15]
    and the records' updated_bias."""
    _lib.check(_L().orbi_graph_init_device(graph, _p(d_bank), cap, _p(d_src), n_src, _p(d_jobs), n, _p(d_result), _lib.stream_arg(stream)))


def edge_information_device(d_bank, cap, d_edges, n_edges, d_info, d_walk_info, d_result, stream=None):
    """orbi_edge_information_device: d_info f64 [n_edges, 81] and d_walk_info f64 [n_edges, 18] of the edges (u8 holding EDGE records)."""
    _lib.check(_L().orbi_edge_information_device(_p(d_bank), cap, _p(d_edges), n_edges, _p(d_info), _p(d_walk_info), _p(d_result),
                                                 _lib.stream_arg(stream)))


def linearize_device(graph, d_bank, cap, gravity, d_edges, n_edges, d_info, d_walk_info, d_work, d_err, d_chi2, d_total, d_result, d_priors=None,
                     n_priors=0, d_prior_jobs=None, n_prior_jobs=0, d_chi2_prior=None, huber_delta=0.0, mode=0, d_H_diag=None, d_H_off=None,
                     d_b=None, d_J=None, d_float=None, stream=None):
    """orbi_linearize_device.  f64: d_work [n_edges, EDGE_WORK], d_err [n_edges, 9], d_chi2 [n_edges, 3], d_chi2_prior [n_prior_jobs, 3],
    d_total [2], d_H_diag [n_states, 225], d_H_off [n_edges, 225], d_b [n_states, 15], d_J [n_edges, 270]; d_float f32 [n_edges, 15].
    mode 1 is computeError only."""
    _lib.check(_L().orbi_linearize_device(graph, _p(d_bank), cap, float(np.float32(gravity)), _p(d_edges), n_edges, _p(d_info), _p(d_walk_info),
                                          _p(d_priors), n_priors, _p(d_prior_jobs), n_prior_jobs, float(huber_delta), mode, _p(d_work), _p(d_err),
                                          _p(d_chi2), _p(d_chi2_prior), _p(d_total), _p(d_H_diag), _p(d_H_off), _p(d_b), _p(d_J), _p(d_float),
                                          _p(d_result), _lib.stream_arg(stream)))


def graph_oplus_device(graph, d_dx, d_iter, d_result, stream=None):
    """orbi_graph_oplus_device: d_dx f64 [n_states, 15] applied to every vertex that is not fixed; d_iter i32 [n_states]."""
    _lib.check(_L().orbi_graph_oplus_device(graph, _p(d_dx), _p(d_iter), _p(d_result), _lib.stream_arg(stream)))


def graph_recover_device(graph, calib, d_jobs, n, d_dst, n_dst, d_bias, d_result, d_pose_R=None, d_pose_t=None, stream=None):
    """orbi_graph_recover_device: n jobs (state, destination, flags) of d_jobs i32 [n, 3]; d_dst f32 [n_dst, 15]; d_bias f32 [n, 6], what
    set_bias_device takes; d_pose_R f64 [n, 9] / d_pose_t f64 [n, 3]."""
    _lib.check(_L().orbi_graph_recover_device(graph, calib, _p(d_jobs), n, _p(d_dst), n_dst, _p(d_bias), _p(d_pose_R), _p(d_pose_t), _p(d_result),
                                              _lib.stream_arg(stream)))
