"""Python mirror of the visual window of the inertial local bundle adjustment (include/orbvw.h).

Optimize::localFullBundleAdjustment (reference modules/Backend/Optimize.cpp:1064-1310) per iteration, for a caller who keeps the
Levenberg-Marquardt loop: EdgeMono (G2oTypes.cpp:59-69) linearised on the VertexPose of an imu.Graph and on the map points, the Schur
complement over the points, the ordered Cholesky solve of the reduced system and the back-substitution.  Every wrapper takes torch
device tensors, enqueues on `stream` (torch's current stream when None, _lib.stream_arg) and neither copies nor waits.  The graph, the
calibration, the camera and the inertial edges are imu.Graph, imu.Calib, vi.Camera and imu.EDGE.  For a caller who does not keep the
loop: window_optimize_device (include/orbwl.h) closes it over these calls on the host, and is the one wrapper here that WAITS.
"""
import ctypes as C

from . import _lib
from .imu import Calib, Graph, _p
from .vi import CHI2_MONO, HUBER_MONO, R_NONFINITE, Camera

MAX_SOLVE_STATES = 32
MAX_EDGES = 1 << 20
MAX_POINTS = 1 << 18
MAX_OBS = 256
EDGE_WORK = 24
R_OUTLIER = 5
R_POINT_SINGULAR = 6

_vp, _i32 = C.c_void_p, C.c_int
_SIGS = {
    "orbvw_linearize_device": [Graph, Calib, Camera, _i32, _i32, _i32] + [_vp] * 6 + [C.c_double, C.c_double, _i32] + [_vp] * 13,
    "orbvw_reduce_device": [_i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _i32] + [_vp] * 12,
    "orbvw_solve_device": [_i32] + [_vp] * 8,
    "orbvw_backsub_device": [_i32, _i32, _i32] + [_vp] * 13,
}
_L = _lib.binder(_SIGS)

# the window loop (include/orbwl.h): the four calls above closed into optimizer.optimize() by the library
LOOP_MAX_ITERATIONS, LOOP_MAX_TRIALS, LOOP_TRACE, LOOP_SUMMARY = 100, 10, 13, 8
R_REJECTED = 2


class WindowLoopOptions(C.Structure):
    """orbwl_loop_options: the iterations, g2o's trial bound, the user lambda init and the thresholds of window_optimize_device"""
    _fields_ = [("iterations", C.c_int32), ("max_trials", C.c_int32), ("lambda_init", C.c_double), ("huber_delta_visual", C.c_double),
                ("huber_delta_inertial", C.c_double), ("chi2_threshold", C.c_double), ("gravity", C.c_float), ("pad", C.c_float)]

    @classmethod
    def make(cls, gravity, iterations=10, lambda_init=1e0, max_trials=10, huber_delta_visual=HUBER_MONO, huber_delta_inertial=0.0, chi2_threshold=CHI2_MONO):
        """localFullBundleAdjustment's defaults; beLarge is iterations=25, lambda_init=1e-2.  lambda_init > 0: setUserLambdaInit, < 0:
        exactly 0, which g2o cannot reach (the refused-solve path); 0 is refused (ORBX_E_UNSUPPORTED)"""
        return cls(int(iterations), int(max_trials), float(lambda_init), float(huber_delta_visual), float(huber_delta_inertial), float(chi2_threshold),
                   float(gravity), 0.0)


_LOOP_SIGS = {
    "orbwl_window_work_doubles": (C.c_int64, [_i32] * 6),
    "orbwl_window_optimize_device": [Graph, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, Calib, Camera, _i32, _i32, _i32] + [_vp] * 6
                                    + [WindowLoopOptions] + [_vp] * 4 + [_i32] + [_vp] * 4,
}
_LL = _lib.binder(_LOOP_SIGS)


def window_work_doubles(n_states, n_solve, n_points, cap_edges, n_edges, n_prior_jobs):
    """orbwl_window_work_doubles: the doubles of window_optimize_device's d_work; host arithmetic, negative on a bad count"""
    return int(_LL().orbwl_window_work_doubles(n_states, n_solve, n_points, cap_edges, n_edges, n_prior_jobs))


def window_optimize_device(graph, d_iter, d_bank, cap, d_edges, n_edges, d_info, d_walk_info, d_priors, n_priors, d_prior_jobs, n_prior_jobs, calib, camera,
                           n_solve, n_points, cap_edges, d_points, d_edge_state, d_edge_point, d_edge_z, d_edge_inv_sigma2, d_active, options, d_work, d_chi2,
                           d_outlier, d_trace, cap_trace, d_summary, d_result, stop=None, stream=None):
    """orbwl_window_optimize_device: localFullBundleAdjustment's optimize(iterations) and classification whole -- g2o's policy, push / pop,
    the trace and the counters on the device, the loop closed by the host.  UNLIKE THE CALLS ABOVE IT WAITS on `stream`, once per trial and
    once at the end.  d_iter i32 [n_states]; d_edges: imu.EDGE records with d_info / d_walk_info of imu.edge_information_device; options:
    WindowLoopOptions; f64: d_points [n_points, 3] (in and out), d_work [window_work_doubles(...)] (scratch, 16-byte aligned), d_chi2
    [cap_edges], d_trace [cap_trace, LOOP_TRACE] (a row per trial: inertial_loop.FIELDS), d_summary [LOOP_SUMMARY]; u8: d_active (None: every
    edge), d_outlier [cap_edges]; stop: a ctypes c_int32 in HOST memory (or its address) that another thread raises, None for no flag."""
    if stop is not None and not isinstance(stop, int):
        stop = C.addressof(stop)
    _lib.check(_LL().orbwl_window_optimize_device(graph, _p(d_iter), _p(d_bank), cap, _p(d_edges), n_edges, _p(d_info), _p(d_walk_info), _p(d_priors), n_priors,
                                                  _p(d_prior_jobs), n_prior_jobs, calib, camera, n_solve, n_points, cap_edges, _p(d_points), _p(d_edge_state),
                                                  _p(d_edge_point), _p(d_edge_z), _p(d_edge_inv_sigma2), _p(d_active), options, _p(d_work), _p(d_chi2),
                                                  _p(d_outlier), _p(d_trace), cap_trace, _p(d_summary), _p(d_result), stop, _lib.stream_arg(stream)))


def linearize_device(graph, calib, camera, n_solve, n_points, cap_edges, d_points, d_edge_state, d_edge_point, d_edge_z, d_edge_inv_sigma2,
                     d_point_off, d_err, d_chi2, d_result, d_active=None, huber_delta=HUBER_MONO, chi2_threshold=CHI2_MONO, mode=0, d_total=None,
                     d_work=None, d_H_diag=None, d_b=None, d_Hll=None, d_bl=None, d_Hlp=None, d_outlier=None, stream=None):
    """orbvw_linearize_device.  i32: d_edge_state [cap_edges], d_edge_point [cap_edges] (non-decreasing), d_point_off [n_points + 1]
    (WRITTEN); f64: d_points [n_points, 3], d_edge_z [cap_edges, 2], d_edge_inv_sigma2 [cap_edges], d_err [cap_edges, 2], d_chi2 [cap_edges],
    d_total [2], d_work [cap_edges, EDGE_WORK] (mode 0: scratch), d_H_diag [n_states, 225] and d_b [n_states, 15] (mode 0: ADDED to), d_Hll
    [n_points, 9], d_bl [n_points, 3], d_Hlp [cap_edges, 18] (mode 0: written); u8: d_active [cap_edges] (read), d_outlier [cap_edges] (mode 2).
    mode 1: errors and totals only; mode 2: d_outlier from chi2_threshold."""
    _lib.check(_L().orbvw_linearize_device(graph, calib, camera, n_solve, n_points, cap_edges, _p(d_points), _p(d_edge_state), _p(d_edge_point),
                                           _p(d_edge_z), _p(d_edge_inv_sigma2), _p(d_active), float(huber_delta), float(chi2_threshold), mode,
                                           _p(d_point_off), _p(d_work), _p(d_err), _p(d_chi2), _p(d_total), _p(d_H_diag), _p(d_b), _p(d_Hll), _p(d_bl),
                                           _p(d_Hlp), _p(d_outlier), _p(d_result), _lib.stream_arg(stream)))


def reduce_device(n_solve, d_fixed, d_edges, n_edges, cap, d_H_diag, d_H_off, d_b, d_lambda, n_points, cap_edges, d_point_off, d_edge_state, d_Hll,
                  d_bl, d_Hlp, d_S, d_rhs, d_Hll_inv, d_tl, d_out, d_result, stream=None):
    """orbvw_reduce_device: the reduced system d_S f64 [15 n_solve, 15 n_solve], d_rhs f64 [15 n_solve]; d_Hll_inv [n_points, 9], d_tl
    [n_points, 3]; d_out[1] = the largest undamped diagonal entry.  d_edges u8 holding imu.EDGE records; d_lambda f64 [1]."""
    _lib.check(_L().orbvw_reduce_device(n_solve, _p(d_fixed), _p(d_edges), n_edges, cap, _p(d_H_diag), _p(d_H_off), _p(d_b), _p(d_lambda), n_points,
                                        cap_edges, _p(d_point_off), _p(d_edge_state), _p(d_Hll), _p(d_bl), _p(d_Hlp), _p(d_S), _p(d_rhs), _p(d_Hll_inv),
                                        _p(d_tl), _p(d_out), _p(d_result), _lib.stream_arg(stream)))


def solve_device(n_solve, d_S, d_rhs, d_b, d_lambda, d_dx, d_out, d_result, stream=None):
    """orbvw_solve_device: d_S*dx = d_rhs by the ordered Cholesky, d_S OVERWRITTEN with L.  d_dx f64 [n_solve, 15]; d_out f64 [3]: [0] the
    pose side of g2o's computeScale (from d_b and d_lambda), [2] the smallest pivot."""
    _lib.check(_L().orbvw_solve_device(n_solve, _p(d_S), _p(d_rhs), _p(d_b), _p(d_lambda), _p(d_dx), _p(d_out), _p(d_result), _lib.stream_arg(stream)))


def backsub_device(n_solve, n_points, cap_edges, d_point_off, d_edge_state, d_Hlp, d_Hll_inv, d_bl, d_dx, d_lambda, d_points, d_xl, d_points_out,
                   d_out_points, d_result, stream=None):
    """orbvw_backsub_device: d_xl f64 [n_points, 3], d_points_out = d_points + d_xl (not d_points itself), d_out_points f64 [1] = the points'
    side of computeScale."""
    _lib.check(_L().orbvw_backsub_device(n_solve, n_points, cap_edges, _p(d_point_off), _p(d_edge_state), _p(d_Hlp), _p(d_Hll_inv), _p(d_bl), _p(d_dx),
                                         _p(d_lambda), _p(d_points), _p(d_xl), _p(d_points_out), _p(d_out_points), _p(d_result),
                                         _lib.stream_arg(stream)))
