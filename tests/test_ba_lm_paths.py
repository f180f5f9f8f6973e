"""The bundle-adjustment Levenberg-Marquardt loop (lm_loop in csrc/orbba.hip and its kernels) off the straight line: rejected trials
and the pop() that follows them, the three ways out of the loop, every field of orbba_lm_options, edge masks that leave a point or a
free pose without an active edge, and local BA on a scene whose first round rejects.

Hard scenes amplify rounding, and the device differs from numpy in summation order and in the dense Cholesky.  So a case is ADMITTED
on the CPU before the GPU is asked anything (test_every_case_is_admitted):
  * every trial of the oracle's trace decides with |current - temp| / current >= 1e-3: three orders above what rounding moves;
  * its (iterations, trials) survive eight jitter draws of relative 2^-50 on pose_t, points and edge_z;
  * its jitter sensitivity delta -- the largest relative change (in the sense of test_ba._close) of R, t, P, chi2_final and lambda
    over those eight draws -- is at most 1e-7.
These are conditions on the inputs.  A scene that fails one is replaced by another seed or a shorter run, never skipped.  Each case
records its delta (test_the_recorded_sensitivities_hold re-measures it: within a factor 3) and is compared on the device at
tol = max(1e-6, 100 delta), per-edge chi2 at max(1e-5, 100 delta): at most 1e-5, where a wrong branch moves these scenes by 1e-2 and
changes `trials` outright.  A delta below 1e-12 is recorded and compared as 1e-12: twelve orders below it nothing depends on it, and
there it is the jitter itself (2^-50 = 9e-16) that is measured.

Not forced: the non-positive-pivot branch of the two Cholesky kernels.  With finite input and lambda > 0 the reduced system is positive
definite, so only rounding reaches that branch; no admitted case does, and a case built to reach it could not be admitted.  Neither are
a mask without any active edge (lambda0 = 0: the oracle's inverse raises) and non-finite inputs."""
import numpy as np
import pytest

from test_ba import _close, _perturbed

HUBER = float(np.sqrt(np.float32(5.991)))  # ba.HUBER_MONO, without loading the library
BIG = dict(rot=0.3, trans=1.0, pts=2.0)
EASY = dict()                              # _perturbed's defaults: 0.01 rad / 0.05 m / 0.05 m
N_DRAWS = 8
DELTA_FLOOR = 1e-12


# ----------------------------------------------------------------------------------------------------------------- masks
def _mask_point_and_last_free_pose(args):
    """every edge of one point (the one with the most edges among the first ten) and every edge of the last free pose off"""
    fixed, ep, el = np.asarray(args[3], bool), np.asarray(args[5]), np.asarray(args[6])
    point = int(np.argmax(np.bincount(el)[:10]))
    pose = int(np.flatnonzero(~fixed)[-1])
    return (el != point) & (ep != pose)


def _mask_single_free_pose(args):
    """only the first free pose keeps its edges among the free ones; the fixed poses keep theirs"""
    fixed, ep = np.asarray(args[3], bool), np.asarray(args[5])
    keep = int(np.flatnonzero(~fixed)[0])
    return fixed[ep] | (ep == keep)


MASKS = {"point_and_last_free_pose": _mask_point_and_last_free_pose, "single_free_pose": _mask_single_free_pose}


# ----------------------------------------------------------------------------------------------------------------- the cases
def _case(scene, delta, iterations=10, huber=False, mask=None, lambda_init=None, **knobs):
    """scene: (n_poses, n_points, seed, keywords of _perturbed); knobs: lm_optimize's keywords; lambda_init: (case, factor) -- the
    lambda0 that case's oracle run computed, times factor, as user_lambda_init; delta: the recorded jitter sensitivity"""
    return dict(scene=scene, delta=delta, iterations=iterations, huber=huber, mask=mask, lambda_init=lambda_init, knobs=knobs)


S5, S7 = (6, 200, 5, BIG), (6, 200, 7, BIG)
CASES = {
    # rejection bursts, no kernel, tau 1e-9
    "burst_6x200_s5": _case(S5, 2.8e-9, iterations=8, tau=1e-9),
    "burst_3x17_s1": _case((3, 17, 1, dict(rot=0.4, trans=1.5, pts=2.0)), 1.4e-10, tau=1e-9),
    "burst_25x300_s7": _case((25, 300, 7, dict(rot=0.3, trans=1.5, pts=2.0)), 2.9e-10, iterations=8, tau=1e-9),   # 23 free poses: the largest LDS system
    "burst_26x300_s7": _case((26, 300, 7, dict(rot=0.3, trans=1.5, pts=2.0)), 1.9e-8, iterations=3, tau=1e-9),   # the first global-memory one
    "huber_6x200_s7": _case(S7, 1.8e-9, huber=True, tau=1e-9),
    # max_trials: 1 and 2 end on a rejection, 3 on an acceptance that still terminates (g2o's quirk)
    "max_trials_1": _case(S7, 1.1e-15, tau=1e-9, max_trials=1),
    "max_trials_2": _case(S7, 1.1e-15, tau=1e-9, max_trials=2),
    "max_trials_3": _case(S7, 1.2e-10, tau=1e-9, max_trials=3),
    # the other knobs
    "tau_1e3": _case((6, 200, 1, BIG), 2.9e-13, iterations=6, tau=1e3),   # heavy damping, tiny steps (s5 decides its first trial by 9.5e-4)
    "good_step_0.9": _case(S5, 4.7e-12, iterations=8, tau=1e-9, lower=0.9, upper=0.9),
    "lambda_init_same": _case(S5, 2.8e-9, iterations=8, tau=1e-9, lambda_init=("burst_6x200_s5", 1.0)),
    "lambda_init_x100": _case(S5, 6.9e-13, iterations=5, tau=1e-9, lambda_init=("burst_6x200_s5", 100.0)),
    "no_iterations": _case(S5, 9.6e-16, iterations=0, tau=1e-9),
    # masks on the easy scene, g2o's defaults
    "mask_point_and_pose": _case((6, 200, 5, EASY), 1.7e-14, iterations=6, huber=True, mask="point_and_last_free_pose"),
    "mask_single_free_pose": _case((6, 200, 5, EASY), 2.1e-14, iterations=6, huber=True, mask="single_free_pose"),
    # Kannala-Brandt camera
    "fisheye_6x200_s8": _case((6, 200, 8, dict(BIG, camera="fisheye")), 1.1e-10, iterations=7, tau=1e-9),
}
# 6x200 s5 run on for 30 iterations, not admitted and its counts not compared (test_gpu_converged_regime); delta of chi2_final alone
CONVERGED = dict(scene=S5, iterations=30, knobs=dict(tau=1e-9), delta_chi=8.9e-9)
# local BA off the easy path: _perturbed(6, 200, seed, outliers=40) at BIG's sigmas through Optimize.cpp:892-922
LOCAL_BA = dict(scene=(6, 200, 14, dict(BIG, outliers=40)), delta=1.7e-10)

_memo = {}


def _args(scene):
    if ("args", scene[:3], tuple(sorted(scene[3].items()))) not in _memo:
        _memo["args", scene[:3], tuple(sorted(scene[3].items()))] = _perturbed(*scene[:3], **scene[3])[1]
    return _memo["args", scene[:3], tuple(sorted(scene[3].items()))]


def _jitter(args, draw):
    """relative 2^-50 on pose_t, points and edge_z"""
    rng = np.random.RandomState(1000 + draw)
    out = list(args)
    for k in (2, 4, 7):
        a = np.asarray(args[k], np.float64)
        out[k] = a * (1.0 + 2.0 ** -50 * rng.uniform(-1, 1, a.shape))
    return tuple(out)


def _setup(name):
    """-> (args, Huber delta, iterations, mask or None, lm_optimize's keywords)"""
    c = CASES[name]
    args = _args(c["scene"])
    knobs = dict(c["knobs"])
    if c["lambda_init"]:
        base, factor = c["lambda_init"]
        knobs["user_lambda_init"] = factor * _oracle(base)["trace"][0][2]
    mask = MASKS[c["mask"]](args) if c["mask"] else None
    return args, HUBER if c["huber"] else 0.0, c["iterations"], mask, knobs


def _oracle(name, draw=None):
    """the oracle on a case (draw: on its jittered inputs), computed once, shared, never changed"""
    from oracle import ba_ref
    if ("run", name, draw) not in _memo:
        args, delta, its, mask, knobs = _setup(name)
        if draw is not None:
            args = _jitter(args, draw)
        _memo["run", name, draw] = ba_ref.lm_optimize(*args, delta, its, edge_active=mask, **knobs)
    return _memo["run", name, draw]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a - b).max())


def _sensitivity(ref, runs, keys=("pose_R", "pose_t", "points", "chi2_final", "lam")):
    return max(_rel(r[k], ref[k]) for r in runs for k in keys)


def _measured_delta(name):
    return _sensitivity(_oracle(name), [_oracle(name, d) for d in range(N_DRAWS)])


def _margin(trace):
    return min(abs(cur - temp) / cur for _, _, _, cur, temp, _, _, _ in trace) if trace else np.inf


def _tol(delta, floor=1e-6):
    return max(floor, 100.0 * delta)


def _same_within_3(measured, recorded):
    m, r = max(measured, DELTA_FLOOR), max(recorded, DELTA_FLOOR)
    return r / 3.0 <= m <= 3.0 * r


# ----------------------------------------------------------------------------------------------------------------- CPU: admission
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_is_admitted(name):
    ref = _oracle(name)
    margin = _margin(ref["trace"])
    counts = {(r["iterations"], r["trials"]) for r in (_oracle(name, d) for d in range(N_DRAWS))}
    delta = _measured_delta(name)
    print("%s: its / trials %d / %d, smallest margin %.3g, delta %.3g, tol %.3g" %
          (name, ref["iterations"], ref["trials"], margin, delta, _tol(CASES[name]["delta"])))
    assert len(ref["trace"]) == ref["trials"] and all(ok for *_, ok in ref["trace"])  # no case reaches the failed-Cholesky branch
    assert margin >= 1e-3
    assert counts == {(ref["iterations"], ref["trials"])}
    assert delta <= 1e-7 and CASES[name]["delta"] <= 1e-7


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_recorded_sensitivities_hold(name):
    measured = _measured_delta(name)
    print("%s: delta measured %.3g, recorded %.3g" % (name, measured, CASES[name]["delta"]))
    assert _same_within_3(measured, CASES[name]["delta"])


def _rejected(tr):
    return not (tr[6] > 0 and np.isfinite(tr[4]))


def _by_iteration(trace):
    its = {}
    for tr in trace:
        its.setdefault(tr[0], []).append(tr)
    return [its[k] for k in sorted(its)]


def test_the_table_takes_every_branch():
    """from the oracle's traces: what the GPU tests then compare is the reject path and every way out of the loop, not the straight line"""
    burst4 = grown = reset_seen = end_rejected = end_accepted = all_iterations = False
    for name, c in CASES.items():
        ref = _oracle(name)
        its = _by_iteration(ref["trace"])
        max_trials = c["knobs"].get("max_trials", 10)
        after_burst = False
        for trials in its:
            rej = [_rejected(tr) for tr in trials]
            assert [tr[1] for tr in trials] == list(range(len(trials)))
            n_rej = sum(rej)
            # within an iteration lambda is multiplied by ni = 2, 4, 8, ... after each rejection in a row
            ratios = [trials[k + 1][2] / trials[k][2] for k in range(len(trials) - 1)]
            assert all(rej[:-1]) and ratios == [2.0 ** (k + 1) for k in range(len(ratios))], name
            burst4 |= n_rej >= 4
            grown |= n_rej >= 2 and not rej[-1]                   # accepted at a lambda that ni = 4 or more produced
            if after_burst and ratios:
                reset_seen = True                                  # ratios[0] == 2: ni was reset by the acceptance behind the burst
            after_burst |= n_rej >= 2 and not rej[-1]
        if its:
            last = its[-1]
            if len(last) == max_trials:
                end_rejected |= _rejected(last[-1])
                end_accepted |= not _rejected(last[-1])
                assert ref["iterations"] == len(its)
        all_iterations |= c["iterations"] > 0 and ref["iterations"] == c["iterations"]
    assert burst4 and grown and reset_seen and end_rejected and end_accepted and all_iterations
    q = _oracle("max_trials_3")
    assert (q["iterations"], q["trials"]) == (1, 3) and not _rejected(q["trace"][-1])    # accepted on the last allowed trial: still the end
    assert (_oracle("max_trials_1")["iterations"], _oracle("max_trials_1")["trials"]) == (1, 1)
    assert (_oracle("max_trials_2")["iterations"], _oracle("max_trials_2")["trials"]) == (1, 2)


def test_oracle_knobs_and_masks_do_what_the_cases_rely_on():
    """user_lambda_init equal to the computed lambda0 reproduces the default run bit for bit and 100 times it does not; no iterations
    leave everything; a point and a free pose without an active edge move by exactly 0.0"""
    base, same, far = _oracle("burst_6x200_s5"), _oracle("lambda_init_same"), _oracle("lambda_init_x100")
    for k in ("pose_R", "pose_t", "points", "chi2"):
        assert same[k].tobytes() == base[k].tobytes(), k
    assert (same["iterations"], same["trials"], same["lam"]) == (base["iterations"], base["trials"], base["lam"])
    assert far["trace"][0][2] == 100.0 * base["trace"][0][2] and far["trials"] != base["trials"]
    none = _oracle("no_iterations")
    args = _args(CASES["no_iterations"]["scene"])
    assert (none["iterations"], none["trials"], none["trace"]) == (0, 0, []) and none["chi2_initial"] == none["chi2_final"]
    assert np.array_equal(none["pose_R"], args[1]) and np.array_equal(none["pose_t"], args[2]) and np.array_equal(none["points"], args[4])
    for name in ("mask_point_and_pose", "mask_single_free_pose"):
        args, _, _, mask, _ = _setup(name)
        still_poses, still_points, moved_poses = _without_active_edge(args, mask)
        out = _oracle(name)
        assert len(still_poses) >= 1
        if name == "mask_point_and_pose":  # (points that no pose sees have no edge to begin with; the masked one had several)
            assert np.bincount(np.asarray(args[6]), minlength=len(args[4]))[still_points].max() >= 2
        assert np.array_equal(out["pose_R"][still_poses], np.asarray(args[1])[still_poses])
        assert np.array_equal(out["pose_t"][still_poses], np.asarray(args[2])[still_poses])
        assert np.array_equal(out["points"][still_points], np.asarray(args[4])[still_points])
        assert len(moved_poses) >= 1 and all(np.abs(out["pose_t"][i] - args[2][i]).max() > 0 for i in moved_poses)
    args, _, _, mask, _ = _setup("mask_single_free_pose")
    assert len(_without_active_edge(args, mask)[2]) == 1


def _without_active_edge(args, mask):
    """-> (free poses without an active edge, points without one, free poses with one)"""
    fixed, ep, el = np.asarray(args[3], bool), np.asarray(args[5]), np.asarray(args[6])
    has_pose = np.bincount(ep[mask], minlength=len(fixed)) > 0
    has_point = np.bincount(el[mask], minlength=len(np.asarray(args[4]).reshape(-1, 3))) > 0
    return np.flatnonzero(~fixed & ~has_pose), np.flatnonzero(~has_point), np.flatnonzero(~fixed & has_pose)


# ----------------------------------------------------------------------------------------------------------------- CPU: local BA, converged run
def _local_ba_args():
    s = LOCAL_BA["scene"]
    return _args(s)


def _local_ba_oracle(draw=None):
    from oracle import ba_ref
    if ("local", draw) not in _memo:
        args = _local_ba_args() if draw is None else _jitter(_local_ba_args(), draw)
        _memo["local", draw] = ba_ref.local_bundle_adjustment(*args, HUBER)
    return _memo["local", draw]


def _local_counts(r):
    return (r["first_round"]["iterations"], r["first_round"]["trials"], r["iterations"], r["trials"])


def test_the_local_ba_scene_is_admitted():
    """the admission rules on both rounds, a rejected trial in the first, and no edge whose chi2 at the end of either round lies within
    100 delta (relative) of 5.991: the demotion mask and the outlier flags are then the same on the device"""
    ref = _local_ba_oracle()
    runs = [_local_ba_oracle(d) for d in range(N_DRAWS)]
    first = ref["first_round"]
    delta = max(_sensitivity(ref, runs), _sensitivity(first, [r["first_round"] for r in runs]))
    margin = min(_margin(first["trace"]), _margin(ref["trace"]))
    gap = min(np.abs(first["chi2"] / 5.991 - 1).min(), np.abs(ref["chi2_final_estimate"] / 5.991 - 1).min())
    print("local BA: rounds %s, smallest margin %.3g, delta %.3g (recorded %.3g), nearest chi2 to 5.991: %.3g relative, %d outliers" %
          (_local_counts(ref), margin, delta, LOCAL_BA["delta"], gap, ref["outlier"].sum()))
    assert any(_rejected(tr) for tr in first["trace"])
    assert margin >= 1e-3
    assert {_local_counts(r) for r in runs} == {_local_counts(ref)}
    assert all(np.array_equal(r["outlier"], ref["outlier"]) for r in runs)
    assert delta <= 1e-7 and LOCAL_BA["delta"] <= 1e-7 and _same_within_3(delta, LOCAL_BA["delta"])
    assert gap > 100 * max(delta, LOCAL_BA["delta"])
    assert 40 <= ref["outlier"].sum() <= 200


def _converged(draw=None):
    from oracle import ba_ref
    if ("converged", draw) not in _memo:
        args = _args(CONVERGED["scene"])
        args = args if draw is None else _jitter(args, draw)
        _memo["converged", draw] = ba_ref.lm_optimize(*args, 0.0, CONVERGED["iterations"], **CONVERGED["knobs"])
    return _memo["converged", draw]


def test_the_converged_run_has_the_recorded_chi2_sensitivity():
    ref = _converged()
    runs = [_converged(d) for d in range(N_DRAWS)]
    delta_chi = _sensitivity(ref, runs, keys=("chi2_final",))
    print("converged: %d / %d, lambda %.3g; jittered counts %s; delta_chi %.3g (recorded %.3g)" %
          (ref["iterations"], ref["trials"], ref["lam"], sorted({(r["iterations"], r["trials"]) for r in runs}), delta_chi, CONVERGED["delta_chi"]))
    assert _same_within_3(delta_chi, CONVERGED["delta_chi"]) and CONVERGED["delta_chi"] <= 1e-7
    assert ref["chi2_final"] < 1e-2 * ref["chi2_initial"]


# ----------------------------------------------------------------------------------------------------------------- GPU
DEVICE_KNOB = dict(tau="tau", max_trials="max_trials", lower="good_step_lower", upper="good_step_upper", user_lambda_init="user_lambda_init")


def _device(name, chol):
    from monoorbslam3_amd import ba
    args, delta, its, mask, knobs = _setup(name)
    ba.set_variant("chol", chol)  # read per call
    try:
        return ba.optimize(*args, huber_delta=delta, iterations=its, edge_active=mask, **{DEVICE_KNOB[k]: v for k, v in knobs.items()})
    finally:
        ba.set_variant("chol", "lds")


def _same_bytes(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


def _within(got, ref, tol):
    return abs(got - ref) <= tol * abs(ref)


@pytest.mark.gpu
@pytest.mark.parametrize("chol", ["lds", "global"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_gpu_lm_paths_match_oracle(name, chol):
    """the oracle's decisions exactly, its estimates within the case's tolerance"""
    args, _, _, mask, _ = _setup(name)
    ref, got = _oracle(name), _device(name, chol)
    tol, tol_edge = _tol(CASES[name]["delta"]), _tol(CASES[name]["delta"], 1e-5)
    worst = {k: _rel(got[k], ref[k]) for k in ("pose_R", "pose_t", "points", "chi2", "chi2_initial", "chi2_final", "lam")}
    print("%s %s: device %d / %d, oracle %d / %d, tol %.3g; relative differences %s" %
          (name, chol, got["iterations"], got["trials"], ref["iterations"], ref["trials"], tol, {k: "%.2g" % v for k, v in worst.items()}))
    assert (got["iterations"], got["trials"]) == (ref["iterations"], ref["trials"])
    assert _within(got["chi2_initial"], ref["chi2_initial"], 1e-9)
    assert _within(got["chi2_final"], ref["chi2_final"], tol) and _within(got["lam"], ref["lam"], tol)
    for k in ("pose_R", "pose_t", "points"):
        assert _close(got[k], ref[k], tol), k
    assert _close(got["chi2"], ref["chi2"], tol_edge)
    fixed = np.asarray(args[3], bool)
    assert _same_bytes(got["pose_R"][fixed], np.asarray(args[1])[fixed]) and _same_bytes(got["pose_t"][fixed], np.asarray(args[2])[fixed])
    assert np.abs(got["pose_R"] @ got["pose_R"].transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
    if name == "max_trials_1":      # the only trial is rejected: what comes back is what pop() restored
        assert _same_bytes(got["pose_R"], args[1]) and _same_bytes(got["pose_t"], args[2]) and _same_bytes(got["points"], args[4])
        assert _within(got["chi2_final"], got["chi2_initial"], 1e-12) and (got["iterations"], got["trials"]) == (1, 1)
        assert ref["lam"] == 2.0 * ref["trace"][0][2] and _within(got["lam"], 2.0 * ref["trace"][0][2], tol)
    if name == "no_iterations":
        assert _same_bytes(got["pose_R"], args[1]) and _same_bytes(got["pose_t"], args[2]) and _same_bytes(got["points"], args[4])
        assert (got["iterations"], got["trials"]) == (0, 0) and got["chi2_initial"] == got["chi2_final"]
    if mask is not None:            # H_ll = 0: the inverse is I / lambda, times b_l = 0; S_ii = lambda I against a zero right-hand side
        still_poses, still_points, _ = _without_active_edge(args, mask)
        assert _same_bytes(got["pose_R"][still_poses], np.asarray(args[1])[still_poses])
        assert _same_bytes(got["pose_t"][still_poses], np.asarray(args[2])[still_poses])
        assert _same_bytes(got["points"][still_points], np.asarray(args[4])[still_points])


@pytest.mark.gpu
@pytest.mark.parametrize("chol", ["lds", "global"])
def test_gpu_local_bundle_adjustment_off_the_easy_path(chol):
    """Optimize.cpp:892-922 on a scene whose first round rejects a trial: the oracle's outlier flags exactly, its estimates within
    tolerance (tests/test_local_ba_gpu.py holds the device form against this host form bit for bit on the same scene)"""
    from monoorbslam3_amd import ba
    ref = _local_ba_oracle()
    ba.set_variant("chol", chol)
    try:
        got = ba.local_bundle_adjustment(*_local_ba_args())
    finally:
        ba.set_variant("chol", "lds")
    tol, tol_edge = _tol(LOCAL_BA["delta"]), _tol(LOCAL_BA["delta"], 1e-5)
    print("local BA %s: device %d / %d, oracle %s; relative differences %s" %
          (chol, got["iterations"], got["trials"], _local_counts(ref),
           {k: "%.2g" % _rel(got[k], ref[k]) for k in ("pose_R", "pose_t", "points", "chi2", "chi2_final", "lam")}))
    assert (got["iterations"], got["trials"]) == (ref["first_round"]["iterations"] + ref["iterations"], ref["first_round"]["trials"] + ref["trials"])
    assert np.array_equal(got["outlier"], ref["outlier"])
    assert _within(got["chi2_initial"], ref["first_round"]["chi2_initial"], 1e-9)
    assert _within(got["chi2_final"], ref["chi2_final"], tol) and _within(got["lam"], ref["lam"], tol)
    for k in ("pose_R", "pose_t", "points"):
        assert _close(got[k], ref[k], tol), k
    assert _close(got["chi2"], ref["chi2"], tol_edge)


@pytest.mark.gpu
@pytest.mark.parametrize("chol", ["lds", "global"])
def test_gpu_converged_regime(chol):
    """6x200 s5 at the large sigmas run on for 30 iterations, far beyond the 8 its burst case is admitted with.  The counts are NOT
    compared: this run is not admitted, and the longer such a run goes on the more of its accept / reject decisions rounding takes.
    On the CPU the oracle uses all 30 iterations in 48 trials (10 rejections in iterations 4 to 6, 8 more from iteration 21 on), ends at
    lambda 0.083 still creeping down a narrow valley (chi2 2.7e7 -> 1.3e4), and its smallest decision margin is 8e-3; 60 iterations
    bring the margin to 2e-4, below the admission rule, and with g2o's own tau and the Huber kernel the same scene decides one trial by a
    margin of 0.0 -- by rounding alone.  What holds whoever decides: chi2 does not rise, lambda stays finite and positive, and
    chi2_final is the oracle's within max(1e-9, 100 delta_chi), delta_chi being the jitter sensitivity of the oracle's chi2_final
    (8.9e-9 over the eight draws; test_the_converged_run_has_the_recorded_chi2_sensitivity)."""
    from monoorbslam3_amd import ba
    ref = _converged()
    ba.set_variant("chol", chol)
    try:
        got = ba.optimize(*_args(CONVERGED["scene"]), huber_delta=0.0, iterations=CONVERGED["iterations"], tau=CONVERGED["knobs"]["tau"])
    finally:
        ba.set_variant("chol", "lds")
    print("converged %s: device %d / %d lambda %.3g chi2 %.17g, oracle %d / %d lambda %.3g chi2 %.17g" %
          (chol, got["iterations"], got["trials"], got["lam"], got["chi2_final"], ref["iterations"], ref["trials"], ref["lam"], ref["chi2_final"]))
    assert got["chi2_final"] <= got["chi2_initial"]
    assert np.isfinite(got["lam"]) and got["lam"] > 0
    assert got["iterations"] <= CONVERGED["iterations"]
    assert _within(got["chi2_final"], ref["chi2_final"], _tol(CONVERGED["delta_chi"], 1e-9))
