"""Python mirror of localInertialBundleAdjustment on the device (include/orbil.h).

Optimize::localInertialBundleAdjustment (reference modules/Backend/Optimize.cpp:953-1062): a chain of up to MAX_STATES key frames with
every pose fixed, one EdgeInertialOnly with its bias walks between neighbours.  chain_solve_device is the damped step of such a chain, by a
walk along its band; chain_optimize_device is the whole optimisation in one launch.  Every wrapper takes torch device tensors, enqueues on
`stream` (torch's current stream when None, _lib.stream_arg) and neither copies nor waits.  The graph and the edges are imu.Graph and
imu.EDGE; the assembly and the velocity priors of the chain are matcher.inertial_chain_problem_device and
matcher.inertial_chain_velocity_priors_device.
"""
import ctypes as C

from . import _lib
from .imu import Graph, _p
from .vi import LOOP_MAX_ITERATIONS, LOOP_MAX_PRIOR_JOBS, LOOP_MAX_TRIALS, LOOP_TRACE, R_EDGE_REFUSED  # noqa: F401

MAX_STATES = 20
LOOP_WORK = 32768
SUMMARY = 8


def solve_work(n_states):
    """ORBIL_SOLVE_WORK: the doubles of chain_solve_device's d_work"""
    return 450 * n_states


class ChainOptions(C.Structure):
    """orbil_chain_options: the iterations and the lambda init of orbil_chain_optimize_device and g2o's policy constants"""
    _fields_ = [("iterations", C.c_int32), ("max_trials", C.c_int32), ("lambda_init", C.c_double), ("tau", C.c_double), ("huber_delta", C.c_double),
                ("gravity", C.c_float), ("pad", C.c_float)]

    @classmethod
    def make(cls, gravity, iterations=10, max_trials=10, lambda_init=0.0, tau=1e-5, huber_delta=0.0):
        """localInertialBundleAdjustment's defaults.  lambda_init > 0: setUserLambdaInit, 0: computeLambdaInit, < 0: exactly 0, which g2o
        cannot reach (the refused-solve path)"""
        return cls(int(iterations), int(max_trials), float(lambda_init), float(tau), float(huber_delta), float(gravity), 0.0)


_vp, _i32 = C.c_void_p, C.c_int
_SIGS = {
    "orbil_chain_solve_device": [_i32, _vp, _vp, _i32, _i32] + [_vp] * 9,
    "orbil_chain_optimize_device": [Graph, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _vp, _i32, ChainOptions, _vp, _vp, _i32, _vp, _vp, _vp],
}
_L = _lib.binder(_SIGS)


def chain_solve_device(n_states, d_fixed, d_edges, n_edges, cap, d_H_diag, d_H_off, d_b, d_lambda, d_work, d_dx, d_out, d_result, stream=None):
    """orbil_chain_solve_device: (H + lambda*I)*dx = b over the free dof of a chain of 2 .. MAX_STATES states.  The arguments of
    vi.solve_device and d_work f64 [solve_work(n_states)] (scratch: the band).  An edge whose states are not neighbours is dropped."""
    _lib.check(_L().orbil_chain_solve_device(n_states, _p(d_fixed), _p(d_edges), n_edges, cap, _p(d_H_diag), _p(d_H_off), _p(d_b), _p(d_lambda), _p(d_work),
                                             _p(d_dx), _p(d_out), _p(d_result), _lib.stream_arg(stream)))


def chain_optimize_device(graph, d_iter, d_bank, cap, d_edges, n_edges, d_info, d_walk_info, d_priors, n_priors, d_prior_jobs, n_prior_jobs, options, d_work,
                          d_trace, cap_trace, d_summary, d_result, stream=None):
    """orbil_chain_optimize_device: the optimisation of localInertialBundleAdjustment whole, in one launch.  graph: 2 .. MAX_STATES states;
    d_iter i32 [n_states]; d_edges: at most n_states - 1 imu.EDGE with d_info / d_walk_info of imu.edge_information_device; options:
    ChainOptions.  f64: d_work [LOOP_WORK] (scratch), d_trace [cap_trace, LOOP_TRACE] (a row per trial: inertial_loop.FIELDS), d_summary
    [SUMMARY] (iterations, trials, accepted, refused solves, the last lambda, trials in all, trials without a row)."""
    _lib.check(_L().orbil_chain_optimize_device(graph, _p(d_iter), _p(d_bank), cap, _p(d_edges), n_edges, _p(d_info), _p(d_walk_info), _p(d_priors), n_priors,
                                                _p(d_prior_jobs), n_prior_jobs, options, _p(d_work), _p(d_trace), cap_trace, _p(d_summary), _p(d_result),
                                                _lib.stream_arg(stream)))
