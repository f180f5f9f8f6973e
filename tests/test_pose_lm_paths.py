"""Optimize::poseOptimize's Levenberg-Marquardt loop (k_pose_optimize in csrc/orbba.hip) off the straight line: rejected trials and the
pop() behind them, the growth and the reset of ni, rounds cut short, a round without an inlier, the failed solve, huber_delta = 0, the
edge of the LDS staging and the device form on more than one frame.

The kernel writes no trace.  It is observed through the two fields of orbba_pose_problem that nothing else sets: the same batch is run
with rounds = 1 and iterations = k for k = 1, 2, ... (the LADDER; each run is a RUNG).  Rung k returns the pose after k iterations, every
edge's chi2 there and the classification, so from one rung to the next an accepted step shows as the oracle's pose after k iterations, an
iteration that accepted nothing (or a loop that had ended) as a rung byte-equal to the one before it, and the number of trials inside an
iteration through lambda: RRRA leaves 64 times the lambda of A, and the next rung's step carries it.  Rounds 2 .. 4 are observed the same
way with `iterations` cut short (the CUTS), so that every round ends before the tail of trials that rounding decides.

Hard scenes amplify rounding, and the device differs from numpy in summation order and in the 6 x 6 solve.  So a case is ADMITTED on the
CPU before the GPU is asked anything (test_every_case_is_admitted), by conditions on its inputs alone:
  * every trial of its compared runs (the ladder up to `prefix`, and its cuts) solves and decides with |current - temp| / current >= 1e-3;
  * at every classification the comparison uses (each rung, each round's end of each cut) no edge has |chi2 - 5.991| <= 1e-3 * 5.991;
  * the accept / reject pattern and every inlier flag survive eight jitter draws of relative 2^-50 on t0, the points and z;
  * its jitter sensitivity delta -- the largest relative change (in the sense of test_ba._close) of R, t and chi2 over those draws and
    over all its compared runs -- is at most 1e-7.
A scene that fails one is replaced by another seed or a shorter prefix, never skipped.  Each case records its delta
(test_the_recorded_sensitivities_hold re-measures it: within a factor 3; below 1e-12 it counts as 1e-12) and is compared on the device
at max(the bar, 100 delta), the bars being test_ba's: 1e-7 for R, 1e-6 for t, 1e-5 for per-edge chi2.  Inlier flags and n_inliers are
compared exactly.

Not forced: the exit on a lambda that is not finite (ten doublings from 1e-5 max |H_jj| cannot reach it with finite input), and
non-finite inputs."""
import ctypes as C

import numpy as np
import pytest

from test_ba import _close, _pose_frames

HUBER = float(np.sqrt(np.float32(5.991)))  # ba.HUBER_MONO, without loading the library
N_DRAWS = 8
DELTA_FLOOR = 1e-12
BARS = dict(R=1e-7, t=1e-6, chi2=1e-5)
FAR = dict(rot=1.5, trans=5.0)                    # 1.5 rad / 5 m
NEAR8 = dict(rot=0.8, trans=3.0, depth=(1, 8))    # points 1 .. 8 m away


# ----------------------------------------------------------------------------------------------------------------- the cases
def _case(delta, prefix, cuts, n=None, seed=None, take=None, huber=True, fisheye=None, **frame):
    """n, seed, frame: _pose_frames([n], seed, **frame); take: only its first `take` edges; fisheye: (pose, seed, rot, trans) of
    _fisheye_frame; prefix: rungs of the ladder compared; cuts: the (rounds, iterations) compared; delta: the recorded sensitivity"""
    return dict(delta=delta, prefix=prefix, cuts=tuple(cuts), n=n, seed=seed, take=take, huber=huber, fisheye=fisheye, frame=frame)


CASES = {
    # rejections inside the compared prefix (the pattern of each rung's last iteration is in the comment)
    "burst_64_s4": _case(1.6e-11, 5, [(2, 2), (4, 3), (4, 5)], n=64, seed=4, **FAR),               # A A RRRA A A; every round of (4, 5) repeats it
    "burst_63_of_s5": _case(1.8e-13, 6, [(2, 2), (4, 3), (4, 5)], n=64, seed=5, take=63, **FAR),   # A RRA A A A A
    "burst_63_of_s4": _case(1.2e-13, 7, [(2, 2), (4, 3), (4, 5)], n=64, seed=4, take=63, **FAR),   # A A RRA A A A A; (4, 5): 24, 34, 40, 45 inliers
    "burst_65_s2": _case(4.4e-9, 10, [(2, 2), (4, 3), (4, 5)], n=65, seed=2, **NEAR8),            # RRRA at iteration 5; every cut round ends empty
    "two_bursts_65_s1": _case(1.0e-11, 10, [(2, 2), (4, 3), (4, 5)], n=65, seed=1, **NEAR8),       # RA at iterations 4 and 7: ni reset between
    "first_trial_300_s3": _case(2.7e-12, 10, [(2, 2), (4, 3), (4, 5)], n=300, seed=3, rot=1.0, trans=3.0),   # RA at iteration 0
    # accepts on every rung; its second round of (2, 1) has no inlier left
    "far_40_s7": _case(5.6e-13, 4, [(2, 1), (2, 2)], n=40, seed=7, rot=0.5, trans=3.0, outlier_frac=0.0),
    # exactly three edges
    "three_edges_s6": _case(2.4e-12, 10, [(2, 2), (4, 3), (4, 5)], n=3, seed=6, rot=0.5, trans=1.5),   # A A A A A RA RRA RA RRA RRA
    # huber_delta = 0: no robust kernel
    "plain_300_s3": _case(9.4e-14, 4, [(2, 2), (4, 3)], n=300, seed=3, huber=False, rot=1.0, trans=3.0),   # A RRRRA A RRRA
    "plain_64_s4": _case(6.6e-13, 6, [(2, 2), (4, 3), (4, 5)], n=64, seed=4, huber=False, **FAR),          # A A RA A A A
    # Kannala-Brandt camera
    "fisheye_p0_s2": _case(1.7e-12, 5, [(2, 2), (4, 3), (4, 5)], fisheye=(0, 2, 0.6, 2.0)),      # A RRA A A A; (4, 3): 39, 29, 31, 29 inliers
}
_memo = {}


def _fisheye_frame(pose, seed, rot, trans):
    """pose `pose` of the fisheye scene against the points it observes, as test_gpu_fisheye_matches_oracle builds it, from an initial pose
    perturbed by N(0, rot) rad / N(0, trans) m"""
    from monoorbslam3_amd import synth
    from oracle import ba_ref
    pr = synth.make_ba_problem(4, 60, seed=8, camera="fisheye")
    sel = np.flatnonzero(pr["edge_pose"] == pose)
    rng = np.random.RandomState(seed)
    dR, dt = ba_ref.se3_exp(np.concatenate([rng.normal(0, rot, 3), rng.normal(0, trans, 3)]))
    R, t = pr["pose_R"].reshape(-1, 3, 3)[pose], pr["pose_t"].reshape(-1, 3)[pose]
    return (pr["cam"], dR @ R, dR @ t + dt, np.array(pr["points"][pr["edge_point"][sel]], np.float64),
            np.array(pr["edge_z"][sel], np.float64).reshape(-1, 2), np.array(pr["edge_inv_sigma2"][sel], np.float64))


def _frame(name):
    """-> (cam, R0, t0, P, z, w) of one case"""
    if ("frame", name) not in _memo:
        c = CASES[name]
        if c["fisheye"]:
            fr = _fisheye_frame(*c["fisheye"])
        else:
            cam, R0, t0, _, P, Z, W = _pose_frames([c["n"]], c["seed"], **c["frame"])
            k = c["take"] or c["n"]
            fr = (cam, R0[0], t0[0], P[:k], Z[:k], W[:k])
        _memo["frame", name] = fr
    return _memo["frame", name]


def _jitter(fr, draw):
    """relative 2^-50 on t0, the points and z (test_ba_lm_paths._jitter's recipe)"""
    rng = np.random.RandomState(1000 + draw)
    out = list(fr)
    for k in (2, 3, 4):
        a = np.asarray(fr[k], np.float64)
        out[k] = a * (1.0 + 2.0 ** -50 * rng.uniform(-1, 1, a.shape))
    return tuple(out)


def _huber(name):
    return HUBER if CASES[name]["huber"] else 0.0


def _oracle(name, rounds, iterations, draw=None, **policy):
    """the oracle on a case (draw: on its jittered inputs), computed once, shared, never changed"""
    from oracle import ba_ref
    key = ("run", name, rounds, iterations, draw, tuple(sorted(policy.items())))
    if key not in _memo:
        fr = _frame(name) if draw is None else _jitter(_frame(name), draw)
        _memo[key] = ba_ref.pose_optimize(*fr, _huber(name), rounds=rounds, iterations=iterations, **policy)
    return _memo[key]


def _runs(name):
    """every (rounds, iterations) the GPU tests compare for this case"""
    c = CASES[name]
    return [(1, k) for k in range(1, c["prefix"] + 1)] + list(c["cuts"])


def _classifications(name):
    """every (rounds, iterations) whose classification a compared run depends on: the runs themselves and each cut's earlier rounds"""
    c = CASES[name]
    return sorted(set(_runs(name)) | {(r, its) for rounds, its in c["cuts"] for r in range(1, rounds)})


def _accepted(tr):
    return tr[7] > 0 and np.isfinite(tr[5])


def _pattern(trace):
    """{(round, iteration): "RRA"}"""
    out = {}
    for tr in trace:
        out[tr[0], tr[1]] = out.get((tr[0], tr[1]), "") + ("A" if _accepted(tr) else "R")
    return out


def _margin(trace):
    """the smallest |current - temp| / current; 0 for a trial that did not solve or started from current = 0"""
    return min((abs(tr[4] - tr[5]) / tr[4] if tr[8] and tr[4] > 0 and np.isfinite(tr[5]) else 0.0) for tr in trace) if trace else np.inf


def _band(chi2):
    return float(np.abs(np.asarray(chi2) / 5.991 - 1).min()) if len(chi2) else np.inf


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.abs(b).max(), 1e-30)
    return float(np.abs(a - b).max() / scale)


def _measured_delta(name):
    return max(_rel(_oracle(name, *run, draw=d)[k], _oracle(name, *run)[k]) for run in _runs(name) for d in range(N_DRAWS) for k in ("R", "t", "chi2"))


def _tol(name, what):
    return max(BARS[what], 100.0 * max(CASES[name]["delta"], DELTA_FLOOR))


def _same_within_3(measured, recorded):
    m, r = max(measured, DELTA_FLOOR), max(recorded, DELTA_FLOOR)
    return r / 3.0 <= m <= 3.0 * r


# ----------------------------------------------------------------------------------------------------------------- CPU: admission
@pytest.mark.parametrize("name", sorted(CASES))
def test_every_case_is_admitted(name):
    margin = min(_margin(_oracle(name, *run)["trace"]) for run in _runs(name))
    band = min(_band(_oracle(name, *run)["chi2"]) for run in _classifications(name))
    delta = _measured_delta(name)
    full = _oracle(name, 1, CASES[name]["prefix"])
    print("%s: %d edges, ladder %s, smallest margin %.3g, nearest chi2 to 5.991 %.3g relative, delta %.3g" %
          (name, len(_frame(name)[3]), " ".join(_pattern(full["trace"]).values()), margin, band, delta))
    assert 3 <= len(_frame(name)[3]) <= 300
    assert margin >= 1e-3
    assert band > 1e-3
    for run in _classifications(name):
        ref = _oracle(name, *run)
        for d in range(N_DRAWS):
            jit = _oracle(name, *run, draw=d)
            assert _pattern(jit["trace"]) == _pattern(ref["trace"]) and np.array_equal(jit["inlier"], ref["inlier"]), (run, d)
    for k in range(1, CASES[name]["prefix"] + 1):  # a rung's trace is the beginning of the next one's: the ladder climbs one run
        assert _oracle(name, 1, k)["trace"] == [tr for tr in full["trace"] if tr[1] < k]
    assert delta <= 1e-7 and CASES[name]["delta"] <= 1e-7


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_recorded_sensitivities_hold(name):
    measured = _measured_delta(name)
    print("%s: delta measured %.3g, recorded %.3g" % (name, measured, CASES[name]["delta"]))
    assert _same_within_3(measured, CASES[name]["delta"])


def _empty_round(name, cut):
    """the cut's last round starts without an inlier: no trial in it, classification at the initial pose"""
    rounds, its = cut
    return rounds >= 2 and _oracle(name, rounds - 1, its)["n_inliers"] == 0 and all(tr[0] < rounds - 1 for tr in _oracle(name, *cut)["trace"])


def test_the_table_takes_every_branch():
    """from the oracle's traces: what the GPU tests compare is the reject path, not the straight line"""
    burst3 = behind_burst = reset_seen = empty_round = all_iterations = all_accept = False
    for name, c in CASES.items():
        for run in _runs(name):
            ref = _oracle(name, *run)
            pat = _pattern(ref["trace"])
            lam = {}
            for tr in ref["trace"]:
                lam.setdefault((tr[0], tr[1]), []).append(tr[3])
            rejected_before = set()  # rounds that already saw a rejection followed by an acceptance
            for key in sorted(pat):
                p, ratios = pat[key], [b / a for a, b in zip(lam[key], lam[key][1:])]
                assert "A" not in p[:-1] and [tr for tr in ref["trace"] if tr[:2] == key][-1][2] == len(p) - 1
                assert ratios == [2.0 ** (k + 1) for k in range(len(ratios))], (name, run, key)  # ni = 2, 4, 8, ... within a burst
                burst3 |= p.count("R") >= 3
                behind_burst |= p.count("R") >= 3 and p.endswith("A")
                reset_seen |= key[0] in rejected_before and len(ratios) >= 1   # ratios[0] == 2 although ni had grown earlier in this round
                if "R" in p and p.endswith("A"):
                    rejected_before.add(key[0])
            all_iterations |= (run[0] - 1, run[1] - 1) in pat
            empty_round |= _empty_round(name, run)
        full = _pattern(_oracle(name, 1, c["prefix"])["trace"])
        all_accept |= set(full.values()) == {"A"} and len(full) == c["prefix"]
    assert burst3 and behind_burst and reset_seen and empty_round and all_iterations and all_accept
    assert any(not c["huber"] for c in CASES.values()) and any(c["fisheye"] for c in CASES.values())
    assert any(len(_frame(name)[3]) == 3 for name in CASES)
    assert sum(any("R" in p for p in _pattern(_oracle(name, 1, c["prefix"])["trace"]).values()) for name, c in CASES.items()) >= 3
    assert len({max(p.count("R") for p in _pattern(_oracle(name, 1, c["prefix"])["trace"]).values()) for name, c in CASES.items()} - {0}) >= 3


@pytest.mark.parametrize("constant", [dict(tau=1e-4), dict(lower=0.4), dict(upper=0.6)])
def test_the_cases_see_the_policy_constants(constant):
    """the kernel hard-codes tau = 1e-5 and the good-step bounds 1/3 and 2/3: with another value in its place the oracle moves a compared
    output of an admitted case by at least 100 times that case's tolerance, so a kernel with a wrong constant cannot pass"""
    seen = {}
    for name in CASES:
        for run in _runs(name):
            ref, off = _oracle(name, *run), _oracle(name, *run, **constant)
            seen[name, run] = max(_rel(off[k], ref[k]) / _tol(name, k) for k in ("R", "t", "chi2"))
    best = max(seen, key=seen.get)
    print("%s: moves %s at %s by %.3g tolerances" % (constant, best[0], best[1], seen[best]))
    assert seen[best] >= 100.0


def test_oracle_without_kernel_and_with_zero_weights():
    """huber_delta <= 0 is no kernel: the same as a delta no chi2 reaches, and not the Huber result.  Weights of zero: H = 0 and
    lambda0 = 0, no trial solves, four rounds of ten rejections leave the pose and call every edge an inlier at chi2 = 0."""
    from oracle import ba_ref
    fr = _frame("plain_300_s3")
    plain, huge, neg = (ba_ref.pose_optimize(*fr, d, rounds=1, iterations=4) for d in (0.0, 1e9, -1.0))
    for k in ("R", "t", "chi2"):
        assert plain[k].tobytes() == huge[k].tobytes() == neg[k].tobytes()
    assert plain["trace"] == huge["trace"] == neg["trace"] and all(tr[8] for tr in plain["trace"])
    huber = ba_ref.pose_optimize(*fr, HUBER, rounds=1, iterations=4)
    assert _rel(huber["t"], plain["t"]) > 1e-2
    cam, R0, t0, P, z, w = _frame("far_40_s7")
    with np.errstate(over="ignore"):   # rho = (0 - DBL_MAX) / 1e-3
        out = ba_ref.pose_optimize(cam, R0, t0, P, z, np.zeros(len(w)), HUBER)
    assert len(out["trace"]) == 40 and not any(tr[8] for tr in out["trace"]) and not any(_accepted(tr) for tr in out["trace"])
    assert np.array_equal(out["R"], R0) and np.array_equal(out["t"], t0) and out["n_inliers"] == 40 and not out["chi2"].any()


# ----------------------------------------------------------------------------------------------------------------- GPU: batches
GROUPS = {"pinhole_huber": lambda c: c["huber"] and not c["fisheye"], "pinhole_plain": lambda c: not c["huber"],
          "fisheye_huber": lambda c: bool(c["fisheye"])}
STAGING = ["burst_63_of_s5", "burst_64_s4", "burst_65_s2", "three_edges_s6", "empty"]   # 63, 64, 65, 3 and 0 edges


def _extra(kind):
    """frames outside the table: "zero_w" -- far_40_s7 with every weight 0 (the failed solve); "two" -- its first 2 edges; "empty" """
    cam, R0, t0, P, z, w = _frame("far_40_s7")
    if kind == "zero_w":
        return cam, R0, t0, P, z, np.zeros(len(w))
    k = dict(two=2, empty=0)[kind]
    return cam, R0, t0, P[:k], z[:k], w[:k]


def _group(group):
    names = sorted(n for n, c in CASES.items() if GROUPS[group](c))
    if group == "pinhole_huber":   # the failed solve between two cases, the frames below three edges behind them
        names = names[:2] + ["zero_w"] + names[2:] + ["two", "empty"]
    return names


def _batch(names):
    """-> (cam, huber_delta, dict of arrays for pose_optimize_batch, {name: (frame index, edge slice)})"""
    frames = [_frame(n) if n in CASES else _extra(n) for n in names]
    off = np.concatenate([[0], np.cumsum([len(fr[3]) for fr in frames])]).astype(np.int32)
    arrays = dict(pose_R=np.array([fr[1] for fr in frames]), pose_t=np.array([fr[2] for fr in frames]), edge_off=off,
                  points=np.concatenate([fr[3] for fr in frames]), edge_z=np.concatenate([fr[4] for fr in frames]),
                  edge_inv_sigma2=np.concatenate([fr[5] for fr in frames]))
    huber = {_huber(n) for n in names if n in CASES}
    assert len(huber) == 1 and len({tuple(fr[0]) for fr in frames}) == 1   # one camera and one kernel per launch
    where = {n: (f, slice(int(off[f]), int(off[f + 1]))) for f, n in enumerate(names)}
    return frames[0][0], huber.pop(), arrays, where


def _host(names, rounds, iterations, huber=None):
    """ba.pose_optimize_batch on a batch of named frames, once per (names, rounds, iterations, huber, the staging capacity set)"""
    from monoorbslam3_amd import ba
    key = ("host", tuple(names), rounds, iterations, huber, _memo.get("lds", 3000))
    if key not in _memo:
        cam, delta, a, _ = _batch(names)
        _memo[key] = ba.pose_optimize_batch(cam, a["pose_R"], a["pose_t"], a["edge_off"], a["points"], a["edge_z"], a["edge_inv_sigma2"],
                                            huber_delta=delta if huber is None else huber, rounds=rounds, iterations=iterations)
    return _memo[key]


class _staging_capacity:
    """ORBBA_VAR_POSE_LDS for the calls inside; 3000 again behind them, whatever happens"""
    def __init__(self, cap):
        self.cap = cap

    def __enter__(self):
        from monoorbslam3_amd import ba
        ba.set_variant("pose_lds", self.cap)
        _memo["lds"] = self.cap

    def __exit__(self, *exc):
        from monoorbslam3_amd import ba
        try:
            ba.set_variant("pose_lds", 3000)
        finally:
            _memo["lds"] = 3000


def _piece(out, where, name):
    f, sl = where[name]
    return dict(R=out["pose_R"][f], t=out["pose_t"][f], chi2=out["chi2"][sl], inlier=out["inlier"][sl], n_inliers=int(out["n_inliers"][f]))


def _bytes_equal(a, b, keys=("R", "t", "chi2", "inlier", "n_inliers")):
    return all(np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes() for k in keys)


_worst = {}


def _compare(name, run, got, where):
    """one case of one device run against the oracle's run with the same two numbers: flags exactly, estimates within the case's tolerance"""
    ref, g = _oracle(name, *run), _piece(got, where, name)
    for k in ("R", "t", "chi2"):
        _worst[name, k] = max(_worst.get((name, k), 0.0), _rel(g[k], ref[k]))
    assert g["n_inliers"] == ref["n_inliers"] and np.array_equal(g["inlier"], ref["inlier"]), (name, run)
    for k in ("R", "t", "chi2"):
        assert _close(g[k], ref[k], _tol(name, k)), (name, run, k, _rel(g[k], ref[k]), _tol(name, k))
    assert np.abs(g["R"] @ g["R"].T - np.eye(3)).max() < 1e-12


def _print_worst(names):
    for name in names:
        if (name, "R") in _worst:
            print("deviation %-20s R %.2e (tol %.1e)  t %.2e (tol %.1e)  chi2 %.2e (tol %.1e)" % (
                name, _worst[name, "R"], _tol(name, "R"), _worst[name, "t"], _tol(name, "t"), _worst[name, "chi2"], _tol(name, "chi2")))


def _check_extras(got, where, names):
    """the failed solve leaves its pose, all 40 edges inliers at chi2 = 0; below three edges nothing is done (:491)"""
    for kind in ("zero_w", "two", "empty"):
        if kind in names:
            fr, g = _extra(kind), _piece(got, where, kind)
            assert g["R"].tobytes() == fr[1].tobytes() and g["t"].tobytes() == fr[2].tobytes(), kind
            assert g["n_inliers"] == (40 if kind == "zero_w" else 0), kind
            if kind == "zero_w":
                assert g["inlier"].all() and len(g["chi2"]) == 40 and not g["chi2"].any()


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_gpu_ladder_matches_oracle_rung_by_rung(group):
    """rounds = 1, iterations = 1 .. prefix, all cases of a camera and a kernel as frames of one batch.  Each rung against the oracle's run
    with the same two numbers; between neighbouring rungs the pose differs exactly where the oracle's trace accepted a step in the new
    iteration, and the whole frame is byte-equal where it did not (pop() restores exactly) -- on the device alone."""
    names = _group(group)
    _, _, _, where = _batch(names)
    cases = [n for n in names if n in CASES]
    below = None
    for k in range(1, max(CASES[n]["prefix"] for n in cases) + 1):
        got = _host(names, 1, k)
        for name in cases:
            if k > CASES[name]["prefix"]:
                continue
            _compare(name, (1, k), got, where)
            g, stepped = _piece(got, where, name), "A" in _pattern(_oracle(name, 1, k)["trace"]).get((0, k - 1), "")
            before = _piece(below, where, name) if below else dict(R=_frame(name)[1], t=_frame(name)[2])
            if stepped:
                assert not _bytes_equal(g, before, ("R",)) and not _bytes_equal(g, before, ("t",)), (name, k)
            else:
                assert _bytes_equal(g, before, tuple(before)), (name, k)
        _check_extras(got, where, names)
        for kind in set(names) - set(cases):     # nothing accepted, nothing done: every rung is the first one
            assert below is None or _bytes_equal(_piece(got, where, kind), _piece(below, where, kind)), (kind, k)
        below = got
    _print_worst(cases)


@pytest.mark.gpu
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_gpu_cut_rounds_match_oracle(group):
    """rounds = 2 .. 4 with the iterations cut short: the restart from the initial pose, the reclassification between rounds, and the round
    that finds no inlier left and classifies at the initial pose"""
    names = _group(group)
    _, _, _, where = _batch(names)
    cases = [n for n in names if n in CASES]
    empty_seen = 0
    for cut in sorted({cut for n in cases for cut in CASES[n]["cuts"]}):
        got = _host(names, *cut)
        _check_extras(got, where, names)
        for name in cases:
            if cut not in CASES[name]["cuts"]:
                continue
            _compare(name, cut, got, where)
            if _empty_round(name, cut):
                g, fr = _piece(got, where, name), _frame(name)
                start = _oracle(name, 0, cut[1])        # no round: chi2 at the initial pose
                assert g["R"].tobytes() == fr[1].tobytes() and g["t"].tobytes() == fr[2].tobytes(), (name, cut)
                assert g["n_inliers"] == int((g["chi2"] <= 5.991).sum()) == int(g["inlier"].sum())
                assert _close(g["chi2"], start["chi2"], 1e-9)
                empty_seen += 1
    assert empty_seen >= 1 or group != "pinhole_huber"
    _print_worst(cases)


@pytest.mark.gpu
def test_gpu_huber_delta_zero_is_no_kernel():
    """the plain cases run again with the Huber kernel end far from their huber_delta = 0 results (which the ladder holds to the oracle):
    the branch matters on these frames"""
    names = _group("pinhole_plain")
    _, _, _, where = _batch(names)
    for name in names:
        run = (1, CASES[name]["prefix"])
        plain, huber = _piece(_host(names, *run), where, name), _piece(_host(names, *run, huber=HUBER), where, name)
        _compare(name, run, _host(names, *run), where)
        moved = max(_rel(huber[k], plain[k]) / _tol(name, k) for k in ("R", "t"))
        print("%s: Huber moves the pose by %.3g tolerances" % (name, moved))
        assert moved > 1e3


@pytest.mark.gpu
def test_gpu_failed_solve_leaves_the_pose_and_its_neighbours():
    """edge_inv_sigma2 = 0 on all 40 edges: H = 0, lambda0 = 0, solve6 refuses at its first pivot, ten rejections end each round.  The
    pose comes back byte for byte, chi2 is 0, all 40 are inliers -- and the frames beside it are what they are without it."""
    names = ["burst_64_s4", "zero_w", "burst_65_s2"]
    for run in [(0, 0), (1, 1), (4, 3)]:
        got, alone = _host(names, *run), _host([names[0], names[2]], *run)
        _, _, _, where = _batch(names)
        _, _, _, where_alone = _batch([names[0], names[2]])
        _check_extras(got, where, names)
        for name in (names[0], names[2]):
            assert _bytes_equal(_piece(got, where, name), _piece(alone, where_alone, name)), (name, run)


def _all_bytes(out):
    return b"".join(np.ascontiguousarray(out[k]).tobytes() for k in ("pose_R", "pose_t", "chi2", "inlier", "n_inliers"))


STAGING_RUNS = [(1, 5), (4, 3), (4, 5), (0, 0)]   # (0, 0): the reference's 4 x 10, compared across the capacities only


@pytest.mark.gpu
def test_gpu_staging_edge_and_both_paths():
    """ORBBA_VAR_POSE_LDS = 64 with frames of 63, 64, 65, 3 and 0 edges: `staged = n <= cap` at cap - 1, cap and cap + 1, the 65-edge frame
    reading global memory beside the staged ones.  Each admitted frame matches the oracle there, and the whole batch's outputs are
    byte-equal at capacities 0 (every frame from global memory), 64 and 3000 (every frame staged): "same operations in the same order"."""
    _, _, arrays, where = _batch(STAGING)
    assert np.diff(arrays["edge_off"]).tolist() == [63, 64, 65, 3, 0]
    outs = {}
    for cap in (64, 0, 3000):
        with _staging_capacity(cap):
            for run in STAGING_RUNS:
                outs[cap, run] = _host(STAGING, *run)
    for run in STAGING_RUNS:
        for name in STAGING[:4]:
            if run in _runs(name):
                _compare(name, run, outs[64, run], where)
        _check_extras(outs[64, run], where, STAGING)
        same = [_all_bytes(outs[cap, run]) == _all_bytes(outs[64, run]) for cap in (0, 3000)]
        print("staging %s: capacity 0 vs 64 %s, 3000 vs 64 %s" % (run, *("byte-equal" if s else "DIFFERENT" for s in same)))
        assert all(same), run
    _print_worst(STAGING[:4])


GUARD = 16


@pytest.mark.gpu
@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("cap", [64, 3000])
def test_gpu_device_form_equals_host_form(cap, stream_kind):
    """orbba_pose_optimize_batch_device on the staging batch: five frames in one launch, rounds and iterations set, a frame above the
    capacity at 64.  Every output is byte-equal to the host form's; the outputs start as garbage, and the guard elements behind each of
    them stay as they were."""
    import torch
    from monoorbslam3_amd import ba
    dev = torch.device("cuda", 0)
    cam, delta, a, _ = _batch(STAGING)
    B, NE = len(STAGING), int(a["edge_off"][-1])
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    d_in = [t(a[k]) for k in ("pose_R", "pose_t", "edge_off", "points", "edge_z", "edge_inv_sigma2")]
    rng = np.random.RandomState(5)
    stream = None
    if stream_kind == "explicit":
        own = torch.cuda.Stream(device=dev)
        torch.cuda.synchronize()
        stream = own.cuda_stream
        assert stream != 0
    with _staging_capacity(cap):
        for run in [(4, 3), (1, 5), (2, 2)]:
            want = _host(STAGING, *run)
            garbage = dict(R=rng.uniform(-9, 9, 9 * B + GUARD), t=rng.uniform(-9, 9, 3 * B + GUARD), inl=rng.randint(2, 250, NE + GUARD).astype(np.uint8),
                           n=rng.randint(1000, 9000, B + GUARD).astype(np.int32), chi2=rng.uniform(-9, 9, NE + GUARD))
            d = {k: t(v) for k, v in garbage.items()}
            torch.cuda.synchronize()
            ba.pose_optimize_batch_device(cam, *d_in, d["R"], d["t"], d["inl"], d["n"], d["chi2"], n_frames=B, huber_delta=delta, stream=stream,
                                          rounds=run[0], iterations=run[1])
            torch.cuda.synchronize()
            got = {k: v.cpu().numpy() for k, v in d.items()}
            for k, size in (("R", 9 * B), ("t", 3 * B), ("inl", NE), ("n", B), ("chi2", NE)):
                assert got[k][size:].tobytes() == garbage[k][size:].tobytes(), (k, run)
            assert got["R"][:9 * B].tobytes() == want["pose_R"].tobytes() and got["t"][:3 * B].tobytes() == want["pose_t"].tobytes(), run
            assert got["chi2"][:NE].tobytes() == want["chi2"].tobytes() and np.array_equal(got["n"][:B], want["n_inliers"]), run
            assert np.array_equal(got["inl"][:NE], want["inlier"].astype(np.uint8)), run


@pytest.mark.gpu
def test_gpu_host_form_without_chi2():
    """r->chi2 = NULL is allowed on the host form: OK, and the other outputs are the full call's bytes"""
    from monoorbslam3_amd import ba, _lib
    cam, delta, a, _ = _batch(STAGING)
    B, NE = len(STAGING), int(a["edge_off"][-1])
    full = _host(STAGING, 4, 3)
    out = dict(R=np.full((B, 9), 7.0), t=np.full((B, 3), 7.0), inl=np.full(NE, 9, np.uint8), n=np.full(B, -5, np.int32))
    vp = lambda x: x.ctypes.data  # noqa: E731
    prob = ba._PoseProblem(cam[0], cam[1], cam[2], cam[3], delta, B, 4, 3, vp(a["edge_off"]), vp(a["pose_R"]), vp(a["pose_t"]), vp(a["points"]),
                           vp(a["edge_z"]), vp(a["edge_inv_sigma2"]), *ba._cam_tail(cam))
    res = ba._PoseResult(vp(out["R"]), vp(out["t"]), vp(out["inl"]), vp(out["n"]), None, 0.0)
    _lib.check(ba._L().orbba_pose_optimize_batch(C.byref(prob), C.byref(res), -1))
    assert out["R"].tobytes() == full["pose_R"].tobytes() and out["t"].tobytes() == full["pose_t"].tobytes()
    assert np.array_equal(out["n"], full["n_inliers"]) and np.array_equal(out["inl"], full["inlier"].astype(np.uint8))
