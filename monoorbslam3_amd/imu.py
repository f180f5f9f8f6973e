"""Python mirror of the device-resident IMU preintegration and pose prediction (include/orbi.h).

The reference's PreIntegrator (modules/Sensor/Imu.cpp:76-204), Frame::computePreIntegration (Frame.cpp:73-88) and the tracker's
prediction (Tracking.cpp:185-243, Frame.cpp:57-71) on a bank of records, a measurement pool and poses that live in device memory:
every wrapper takes torch device tensors, enqueues on `stream` (torch's current stream when None, _lib.stream_arg) and neither
copies nor waits.  The numpy dtypes below are the header's layouts.
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


class Calib(C.Structure):
    """orbi_calib: ImuCalib's T_cb, the diagonals of its two covariances, GRAVITY_VALUE"""
    _fields_ = [("Rcb", C.c_float * 9), ("tcb", C.c_float * 3), ("cov_noise", C.c_float * 6), ("cov_walk", C.c_float * 6),
                ("gravity", C.c_float)]

    @classmethod
    def make(cls, Rcb, tcb, cov_noise, cov_walk, gravity=9.8):
        f = lambda a, n: (C.c_float * n)(*[float(v) for v in np.asarray(a, np.float32).reshape(n)])  # noqa: E731
        return cls(f(Rcb, 9), f(tcb, 3), f(cov_noise, 6), f(cov_walk, 6), float(np.float32(gravity)))


_vp, _i32 = C.c_void_p, C.c_int
_SIGS = {
    "orbi_reset_device": [_vp, _i32, _vp, _vp, _vp, _i32, _vp, _vp],
    "orbi_integrate_device": [Calib, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _vp],
    "orbi_set_bias_device": [Calib, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp],
    "orbi_merge_next_device": [Calib, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp],
    "orbi_predict_device": [Calib, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp],
    "orbi_imu_pose_device": [Calib, _vp, _vp, _vp, _vp],
}
_bound = None


def _L():
    global _bound
    if _bound is None:
        L = _lib.lib()
        for name, args in _SIGS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.restype, fn.argtypes = C.c_int, args
        _bound = L
    return _bound


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
