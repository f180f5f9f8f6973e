// g2o's Levenberg-Marquardt trial policy (OptimizationAlgorithmLevenberg::solve, g2o 20201223, not vendored) as tests/inertial_loop.py's
// optimize restates it, line by line, in IEEE double and in its expression order: what ONE lane of a decision kernel, or the host, runs
// behind the error evaluation of a trial.  No stage formula is here -- the totals, the scales and the refusal come from the stages' outputs.
// THE ONE DEFINITION: k_vwl_decide (orbwl.hip), k_vi_pose_loop (orbvi_loop.hip) and the host's lm_loop (orbba.hip) take their arithmetic
// from here; k_pose_optimize (orbba.hip) alone keeps a copy, because with these calls it measured slower ("The window loop
// closed by the host": the policy, written once).  The header stands alone: any .hip file may include it in any order, and the host
// compiler takes it without HIP (tests/cpp/lm_policy.cpp).
#pragma once
#include <float.h>
#include <math.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else                                                              // no HIP compiler: the qualifiers mean nothing
#define __host__
#define __device__
#define __forceinline__ inline __attribute__((always_inline))
#endif
#ifdef __clang__                                                   // another compiler is told on its command line (-ffp-contract=off)
#pragma clang fp contract(off)
#endif

// what the policy carries from trial to trial; lambda is g2o's _currentLambda, ni its _ni, lower and upper its goodStepLowerScale and
// goodStepUpperScale
struct LmPolicy {
    double lam, ni, current, rho;
    int qmax;
    double lower = 1.0 / 3.0, upper = 2.0 / 3.0;
};
// one trial's figures, as a row of the trace has them
struct LmTrial {
    double temp, scale, rho;
    bool accepted;
    bool left; // the trial loop was left on a lambda that is not finite: qmax is not counted
};

// g2o's pow(2 * rho - 1, 3).  The two sides differ ON PURPOSE, each keeping the bits its loops have always given.  The device loops
// have the cube as x*x*x (two roundings; no call into a math library from one lane of a kernel at its register limit); the host's lm_loop
// has pow, as g2o writes it, which the host compiler does not turn into multiplications without fast-math.  A correctly rounded pow and
// x*x*x differ in the last bit for a fair share of x, so lambda may differ by an ulp per accepted trial between a host and a device loop
__host__ __device__ __forceinline__ double lm_cube(double x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return x * x * x;
#else
    return pow(x, 3);
#endif
}

// the start of an iteration's trial loop: `current` is activeRobustChi2 of the linearisation
__host__ __device__ __forceinline__ void lm_policy_iteration(LmPolicy &p, double current)
{
    p.current = current, p.rho = 0.0, p.qmax = 0;
}

// behind a trial's error evaluation.  ok: the solve was not refused; ti, tv: the robustified totals at the trial point; scale_pose,
// scale_points: the two sides of computeScale.  Updates lambda, ni, current, rho and qmax.  The clamp's two ternaries are std::min(alpha,
// upper) and std::max(lower, m), and fmin / fmax, to the bit on every input that reaches them: accepted implies that rho is not a NaN, so
// alpha is none either (an infinite rho gives -inf), and the bounds are positive, so no pair of zeros of unlike sign is compared
__host__ __device__ __forceinline__ LmTrial lm_policy_trial(LmPolicy &p, bool ok, double ti, double tv, double scale_pose, double scale_points)
{
    LmTrial t;
    t.temp = ok ? ti + tv : DBL_MAX;                               // a refused solve
    t.scale = (scale_pose + scale_points) + 1e-3;                  // computeScale + 1e-3
    t.rho = (p.current - t.temp) / t.scale;                        // DBL_MAX over a small scale is -inf, as in g2o
    t.accepted = t.rho > 0 && __builtin_isfinite(t.temp);
    t.left = false;
    if (t.accepted) {
        const double alpha = 1.0 - lm_cube(2 * t.rho - 1);
        const double m = p.upper < alpha ? p.upper : alpha;
        p.lam = p.lam * (m > p.lower ? m : p.lower);
        p.ni = 2.0;
        p.current = t.temp;
    } else {
        p.lam = p.lam * p.ni;
        p.ni = p.ni * 2;
        t.left = !__builtin_isfinite(p.lam);
    }
    if (!t.left) ++p.qmax;
    p.rho = t.rho;
    return t;
}

// do { ... } while (rho < 0 && qmax < max_trials): another trial of this iteration
__host__ __device__ __forceinline__ bool lm_policy_again(const LmPolicy &p, const LmTrial &t, int max_trials)
{
    return !t.left && p.rho < 0 && p.qmax < max_trials;
}

// behind an iteration: g2o's Terminate
__host__ __device__ __forceinline__ bool lm_policy_terminate(const LmPolicy &p, int max_trials)
{
    return p.qmax == max_trials || p.rho == 0 || !__builtin_isfinite(p.lam);
}

// a trial's row of the trace, the 13 doubles of tests/inertial_loop.py's FIELDS: it, trial, lam and current are the values BEFORE the
// trial's update
constexpr int LM_TRACE_ROW = 13;
__host__ __device__ __forceinline__ void lm_trace_row(double *r, int it, int trial, double lam, double current, const LmTrial &t, bool ok, double ti,
                                                      double tv, double scale_pose, double scale_points)
{
    r[0] = it, r[1] = trial, r[2] = lam, r[3] = current, r[4] = t.temp, r[5] = t.scale, r[6] = t.rho, r[7] = ok ? 1.0 : 0.0;
    r[8] = ti, r[9] = tv, r[10] = scale_pose, r[11] = scale_points, r[12] = t.accepted ? 1.0 : 0.0;
}
