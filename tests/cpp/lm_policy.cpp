// The Levenberg-Marquardt trial policy (monoorbslam3_amd/csrc/orb_lm_policy.h) on its own, without HIP or the library: runs the header's
// four functions in the loop shape of orbba.hip's lm_loop over a script from stdin (tests/test_lm_policy_cpu.py).  Built twice: as it is
// (the host's cube, pow) and with -D__HIP_DEVICE_COMPILE__ (the device loops' cube, x*x*x, on the CPU).
//   in:  lambda max_trials iterations lower upper; then per iteration `current`, and per trial of it `ok ti tv scale_pose scale_points`
//        (reals as %lf takes them: decimal, hexadecimal, inf, nan), read as the policy asks for them
//   out: one line per trial, the 13 doubles of lm_trace_row as %a; then "end <lambda as %a> <iterations run> <trials>"
#include <stdio.h>

#include "orb_lm_policy.h"

int main()
{
    double lam = 0.0, lower = 0.0, upper = 0.0;
    int max_trials = 0, iterations = 0;
    if (scanf("%lf %d %d %lf %lf", &lam, &max_trials, &iterations, &lower, &upper) != 5) return 2;
    LmPolicy p = {lam, 2.0, 0.0, 0.0, 0, lower, upper};
    int its = 0, trials = 0;
    for (int it = 0; it < iterations; ++it) {
        double current = 0.0;
        if (scanf("%lf", &current) != 1) return 2;
        lm_policy_iteration(p, current);
        LmTrial t;
        do {
            int ok = 0;
            double ti = 0.0, tv = 0.0, scale_pose = 0.0, scale_points = 0.0, row[LM_TRACE_ROW];
            if (scanf("%d %lf %lf %lf %lf", &ok, &ti, &tv, &scale_pose, &scale_points) != 5) return 2;
            const LmPolicy before = p;
            t = lm_policy_trial(p, ok != 0, ti, tv, scale_pose, scale_points);
            lm_trace_row(row, it, before.qmax, before.lam, before.current, t, ok != 0, ti, tv, scale_pose, scale_points);
            for (int k = 0; k < LM_TRACE_ROW; ++k) printf("%a%c", row[k], k + 1 < LM_TRACE_ROW ? ' ' : '\n');
            ++trials;
        } while (lm_policy_again(p, t, max_trials));
        ++its;
        if (lm_policy_terminate(p, max_trials)) break;
    }
    printf("end %a %d %d\n", p.lam, its, trials);
    return 0;
}
