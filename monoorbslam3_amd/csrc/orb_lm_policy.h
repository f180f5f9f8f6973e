// g2o's Levenberg-Marquardt trial policy (OptimizationAlgorithmLevenberg::solve, g2o 20201223, not vendored) as tests/inertial_loop.py's
// optimize restates it, line by line, in IEEE double and in its expression order: what ONE lane of a decision kernel runs behind the
// error evaluation of a trial.  No stage formula is here -- the totals, the scales and the refusal come from the stages' outputs.
// k_vwl_decide (orbwl.hip) takes its arithmetic from here; k_vi_pose_loop (orbvi_loop.hip) keeps its own copy, which its register
// budget was fitted around ("The window loop closed by the host": why two copies exist).
#pragma once
#include <float.h>

#pragma clang fp contract(off)

// what the policy carries from trial to trial; lambda is g2o's _currentLambda, ni its _ni
struct LmPolicy {
    double lam, ni, current, rho;
    int qmax;
};
// one trial's figures, as a row of the trace has them
struct LmTrial {
    double temp, scale, rho;
    bool accepted;
    bool left; // the trial loop was left on a lambda that is not finite: qmax is not counted
};

// the start of an iteration's trial loop: `current` is activeRobustChi2 of the linearisation
__host__ __device__ __forceinline__ void lm_policy_iteration(LmPolicy &p, double current)
{
    p.current = current, p.rho = 0.0, p.qmax = 0;
}

// behind a trial's error evaluation.  ok: the solve was not refused; ti, tv: the robustified totals at the trial point; scale_pose,
// scale_points: the two sides of computeScale.  Updates lambda, ni, current, rho and qmax
__host__ __device__ __forceinline__ LmTrial lm_policy_trial(LmPolicy &p, bool ok, double ti, double tv, double scale_pose, double scale_points)
{
    LmTrial t;
    t.temp = ok ? ti + tv : DBL_MAX;                               // a refused solve
    t.scale = (scale_pose + scale_points) + 1e-3;                  // computeScale + 1e-3
    t.rho = (p.current - t.temp) / t.scale;                        // DBL_MAX over a small scale is -inf, as in g2o
    t.accepted = t.rho > 0 && __builtin_isfinite(t.temp);
    t.left = false;
    if (t.accepted) {
        const double x = 2 * t.rho - 1, alpha = 1.0 - x * x * x;   // the cube is x*x*x, not pow
        const double m = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;
        p.lam = p.lam * (m > (1.0 / 3.0) ? m : (1.0 / 3.0));
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
