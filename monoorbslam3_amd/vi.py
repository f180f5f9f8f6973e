"""Python mirror of the visual edges of the inertial optimisers and their damped step (include/orbvi.h).

poseFullOptimize / poseInertialOptimize (reference modules/Backend/Optimize.cpp:547-764) per iteration, for a caller who keeps the
Levenberg-Marquardt loop: EdgeMonoOnlyPose (G2oTypes.cpp:49-57) linearised on the VertexPose of an imu.Graph, and the solve of the
assembled system.  Every wrapper takes torch device tensors, enqueues on `stream` (torch's current stream when None,
_lib.stream_arg) and neither copies nor waits.  The graph, the calibration and the edges are imu.Graph, imu.Calib and imu.EDGE.
"""
import ctypes as C

from . import _lib
from .imu import Calib, Graph, _p

MAX_STATES = 4
EDGE_WORK = 16
R_NONFINITE = 4
LOOP_MAX_ROUNDS, LOOP_MAX_ITERATIONS, LOOP_MAX_TRIALS, LOOP_MAX_PRIOR_JOBS = 4, 100, 10, 64
LOOP_EDGE_WORK, LOOP_FIXED_WORK, LOOP_TRACE, LOOP_SUMMARY = 18, 2048, 13, 32
R_EDGE_REFUSED = 7
HUBER_MONO = 2.4476518630981445      # (double)sqrtf(5.991), Optimize.cpp:683
CHI2_MONO = 5.991                    # Optimize.cpp:728


class Camera(C.Structure):
    """orbvi_camera: the camera fields of orbba_pose_problem"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("camera_model", C.c_int32), ("pad", C.c_int32),
                ("fisheye_k", C.c_double * 4)]

    @classmethod
    def make(cls, fx, fy, cx, cy, camera_model=0, fisheye_k=(0.0, 0.0, 0.0, 0.0)):
        return cls(float(fx), float(fy), float(cx), float(cy), int(camera_model), 0, (C.c_double * 4)(*[float(k) for k in fisheye_k]))


class LoopOptions(C.Structure):
    """orbvi_loop_options: the rounds, iterations and lambda inits of orbvi_pose_optimize_device, g2o's policy constants and the thresholds"""
    _fields_ = [("rounds", C.c_int32), ("iterations", C.c_int32 * 4), ("max_trials", C.c_int32), ("pad", C.c_int32 * 2), ("lambda_init", C.c_double * 4),
                ("tau", C.c_double), ("huber_delta", C.c_double), ("chi2_threshold", C.c_double), ("gravity", C.c_float), ("pad2", C.c_float)]

    @classmethod
    def make(cls, gravity, rounds=4, iterations=(10, 10, 10, 10), lambda_init=(0.0, 0.0, 0.0, 0.0), tau=1e-5, max_trials=10, huber_delta=HUBER_MONO,
             chi2_threshold=CHI2_MONO):
        """poseFullOptimize's defaults; poseInertialOptimize is rounds=1 with cap_edges=0.  lambda_init[k] > 0: setUserLambdaInit, 0:
        computeLambdaInit, < 0: exactly 0, which g2o cannot reach (the refused-solve path)"""
        return cls(int(rounds), (C.c_int32 * 4)(*[int(i) for i in iterations]), int(max_trials), (C.c_int32 * 2)(0, 0),
                   (C.c_double * 4)(*[float(x) for x in lambda_init]), float(tau), float(huber_delta), float(chi2_threshold), float(gravity), 0.0)


_vp, _i32 = C.c_void_p, C.c_int
_SIGS = {
    "orbvi_linearize_device": [Graph, Calib, Camera, _i32, _i32] + [_vp] * 6 + [C.c_double, C.c_double, _i32] + [_vp] * 9,
    "orbvi_solve_device": [_i32, _vp, _vp, _i32, _i32] + [_vp] * 8,
    "orbvi_pose_optimize_device": [Graph, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, Calib, Camera, _i32] + [_vp] * 6 + [LoopOptions] + [_vp] * 4
                                  + [_i32] + [_vp] * 3,
}
_L = _lib.binder(_SIGS)


def linearize_device(graph, calib, camera, n_groups, cap_edges, d_group_state, d_edge_off, d_points, d_edge_z, d_edge_inv_sigma2, d_err, d_chi2,
                     d_result, d_active=None, huber_delta=HUBER_MONO, chi2_threshold=CHI2_MONO, mode=0, d_total=None, d_H_diag=None, d_b=None,
                     d_n_inliers=None, d_work=None, stream=None):
    """orbvi_linearize_device.  d_group_state i32 [n_groups]; d_edge_off i32 [n_groups + 1]; f64: d_points [cap_edges, 3], d_edge_z
    [cap_edges, 2], d_edge_inv_sigma2 [cap_edges], d_err [cap_edges, 2], d_chi2 [cap_edges], d_total [n_groups, 2], d_H_diag [n_states, 225]
    and d_b [n_states, 15] (mode 0: ADDED to), d_work [cap_edges, EDGE_WORK] (mode 0: scratch); d_active u8 [cap_edges]; d_n_inliers i32 [n_groups].  mode 1: errors and totals only;
    mode 2: d_active and d_n_inliers from chi2_threshold."""
    _lib.check(_L().orbvi_linearize_device(graph, calib, camera, n_groups, cap_edges, _p(d_group_state), _p(d_edge_off), _p(d_points), _p(d_edge_z),
                                           _p(d_edge_inv_sigma2), _p(d_active), float(huber_delta), float(chi2_threshold), mode, _p(d_work), _p(d_err),
                                           _p(d_chi2), _p(d_total), _p(d_H_diag), _p(d_b), _p(d_n_inliers), _p(d_result),
                                           _lib.stream_arg(stream)))


def solve_device(n_states, d_fixed, d_edges, n_edges, cap, d_H_diag, d_H_off, d_b, d_lambda, d_dx, d_out, d_result, stream=None):
    """orbvi_solve_device: (H + lambda*I)*dx = b over the free dof.  d_fixed u8 [n_states]; d_edges u8 holding imu.EDGE records; f64:
    d_H_diag [n_states, 225], d_H_off [n_edges, 225], d_b [n_states, 15], d_lambda [1], d_dx [n_states, 15], d_out [3] (the scale of
    g2o's computeScale, the largest free H_jj, the smallest pivot)."""
    _lib.check(_L().orbvi_solve_device(n_states, _p(d_fixed), _p(d_edges), n_edges, cap, _p(d_H_diag), _p(d_H_off), _p(d_b), _p(d_lambda),
                                       _p(d_dx), _p(d_out), _p(d_result), _lib.stream_arg(stream)))


def pose_optimize_device(graph, d_iter, d_bank, cap, d_edges, n_edges, d_info, d_walk_info, d_priors, n_priors, d_prior_jobs, n_prior_jobs, calib, camera,
                         cap_edges, d_group_state, d_edge_off, d_points, d_edge_z, d_edge_inv_sigma2, d_active, options, d_work, d_chi2, d_n_inliers,
                         d_trace, cap_trace, d_summary, d_result, stream=None):
    """orbvi_pose_optimize_device: poseFullOptimize (cap_edges > 0) or poseInertialOptimize (cap_edges == 0, the visual arrays None) whole, in
    one launch: the rounds, g2o's Levenberg-Marquardt policy, push / pop and the classification.  graph: exactly 2 states; d_iter i32 [2];
    d_edges: at most one imu.EDGE with d_info / d_walk_info of imu.edge_information_device; options: LoopOptions.  f64: d_work [cap_edges *
    LOOP_EDGE_WORK + LOOP_FIXED_WORK] (scratch), d_chi2 [cap_edges], d_trace [cap_trace, LOOP_TRACE] (a row per trial: inertial_loop.FIELDS),
    d_summary [LOOP_SUMMARY]; d_active u8 [cap_edges] (read as the first round's levels, written); d_n_inliers i32 [1]."""
    _lib.check(_L().orbvi_pose_optimize_device(graph, _p(d_iter), _p(d_bank), cap, _p(d_edges), n_edges, _p(d_info), _p(d_walk_info), _p(d_priors), n_priors,
                                               _p(d_prior_jobs), n_prior_jobs, calib, camera, cap_edges, _p(d_group_state), _p(d_edge_off), _p(d_points),
                                               _p(d_edge_z), _p(d_edge_inv_sigma2), _p(d_active), options, _p(d_work), _p(d_chi2), _p(d_n_inliers),
                                               _p(d_trace), cap_trace, _p(d_summary), _p(d_result), _lib.stream_arg(stream)))
