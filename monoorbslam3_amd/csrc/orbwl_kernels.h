// What the window loop's host driver needs of its four kernels (orbwl.hip): their arguments and their launches.  Internal.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/orbwl.h"

// the control block in the caller's scratch: WL_CTRL_DOUBLES doubles.  The policy's doubles first, then its counters as int32
enum { WLC_NI, WLC_CURRENT, WLC_RHO, WLC_INTS, WL_CTRL_DOUBLES = 16 };
enum { WLI_IT, WLI_QMAX, WLI_ITS, WLI_ROWS, WLI_ACCEPTED, WLI_REJECTED, WLI_REFUSED, WLI_WORDS };
static_assert(WLC_INTS * 2 + WLI_WORDS <= WL_CTRL_DOUBLES * 2, "the counters fit behind the doubles");
// the verdict in the page-locked block, four int32
enum { WLV_NEXT, WLV_ACCEPTED, WLV_REFUSED, WLV_TRIALS };
enum { WL_NEXT_TRIAL = 0, WL_NEXT_ITERATION = 1, WL_NEXT_END = 2 };

struct WlDecide {
    orbi_graph g;                  // the vertices a pop restores, the states [0, n_solve)
    int32_t *iter;
    int n_solve, first;            // first: the iteration's first trial, whose `current` is the linearisation's
    const double *lin_inertial, *lin_visual, *try_inertial, *try_visual;   // the totals (plain, robustified) of mode 0 and of mode 1
    const double *out, *out_points;                                        // [0]: the two sides of computeScale
    const int32_t *solve_result;   // the solve's own slot: the refusal survives the calls behind it
    double *lambda, *ctrl;
    const double *saved;           // [n_solve][21], then the int32 counters
    const int32_t *saved_iter;
    double *trace;
    int cap_trace, max_trials, iterations;
    int32_t *verdict;              // page-locked host memory
};

struct WlEnd {
    const double *lambda, *ctrl;
    const int32_t *classify_result, *inertial_result, *reduce_result;      // slots of the last evaluation; the last two mean nothing without a trial
    int cap_trace, stopped;
    double *summary;
    int32_t *result;
};

hipError_t wl_launch_begin(double *ctrl, double *summary, double *lambda, double lambda_init, hipStream_t s);
hipError_t wl_launch_push(orbi_graph g, const int32_t *iter, int n_solve, double *saved, int32_t *saved_iter, hipStream_t s);
hipError_t wl_launch_decide(const WlDecide &a, hipStream_t s);
hipError_t wl_launch_end(const WlEnd &a, hipStream_t s);
