"""tests/inertial_chain.py and tests/inertial_chain_model.py on their own, without the library: the model loop of every chain scene, the
condition a scene must meet before a device loop may be compared with it (tests/test_inertial_loop_cpu.py's, by its method), the figures
the GPU test's bars come from, and the array models of the assembly and the velocity priors at their edges.  Model runs are computed
once per scene and shared; nobody changes them."""
import numpy as np
import pytest

import factors_model as fm
import inertial_chain as ic
import inertial_chain_model as cm
import inertial_loop as il
import vi_model as vm
from test_inertial_loop_cpu import TRIAL, _rel, trial_deviation

RUNS = 8                                                                 # perturbed runs per scene
OUTPUTS = ("v", "bg", "ba", "total", "lam") + TRIAL

# Measured with `pytest tests/test_inertial_chain_cpu.py -s -k spread`, which prints these lines: over RUNS model loops whose every trial
# output (dx, the updated vertices, the two scalars) is multiplied by 1 + 1e-9 N(0, 1), the largest deviation of the final estimate from the
# unperturbed loop's, per output relative to the output's largest entry (every pose is fixed: Rwb and twb do not move and have no entry);
# "total" and "lam" are the final total and lambda; "trial ..." the largest deviations of a trial's read-backs, as
# tests/test_inertial_loop_cpu.py defines them.  This file holds a fresh measurement to within 2 x of these, either way.
# The longer chains end at a total of 4 to 5 from 1e11: a 1e-9 of the start is a thousandth of the end, which is what their figures show.
MEASURED_SPREAD = {
    "chain 2": {"v": 1.95e-09, "bg": 9.02e-06, "ba": 3.36e-08, "total": 1.81e-05, "lam": 8.08e-05, "trial lam": 8.08e-05, "trial total": 5.29e-05, "trial scale": 1.34e-03},
    "chain 3": {"v": 2.27e-09, "bg": 8.51e-09, "ba": 4.17e-08, "total": 2.06e-06, "lam": 1.41e-09, "trial lam": 1.41e-09, "trial total": 2.96e-05, "trial scale": 4.20e-02},
    "chain 10": {"v": 2.26e-08, "bg": 9.17e-04, "ba": 1.14e-05, "total": 1.81e-03, "lam": 1.76e-01, "trial lam": 1.76e-01, "trial total": 1.81e-03, "trial scale": 2.01e-01},
    "chain 20": {"v": 1.50e-08, "bg": 8.28e-03, "ba": 4.81e-05, "total": 1.66e-02, "lam": 4.82e-01, "trial lam": 4.82e-01, "trial total": 1.66e-02, "trial scale": 3.14e-01},
    "chain 10 rejecting": {"v": 1.79e-05, "bg": 1.23e-04, "ba": 4.95e-05, "total": 3.38e-05, "lam": 4.84e-02, "trial lam": 2.44e-02, "trial total": 1.58e-03, "trial scale": 1.97e-02},
    "chain 4 refused": {"v": 0.00e+00, "bg": 0.00e+00, "ba": 0.00e+00, "total": 0.00e+00, "lam": 0.00e+00, "trial lam": 0.00e+00, "trial total": 3.07e-09, "trial scale": 0.00e+00},
}
_cache = {}


@pytest.mark.parametrize("name", list(ic.SCENES))
def test_the_model_loop_does_something(name):
    r = ic.model_run(name)
    x = r["rounds"][0]
    tr, dec = x["trace"], il.decisions(r["rounds"])[0]
    best = min([t[4] for t in tr if t[-1]] + [tr[0][3]])
    print(name, dec, "iterations", x["iterations"], "refused", r["refused"], "total %.10g -> %.10g, lambda %.3g" % (tr[0][3], best, x["lam"]))
    sc = ic.scene(name)
    n = ic.SCENES[name][0]
    assert sc["graph"].n == n and len(sc["edges"]) == n - 1 and sc["graph"].fixed.tolist() == [15] + [fm.FIX_POSE] * (n - 1) and len(sc["pjobs"]) == 0
    if name == ic.REFUSED:
        # every solve refused, every trial rejected, lambda * nu stays 0, max_trials ends it with the estimate untouched
        assert dec == "r" * il.MAX_TRIALS and x["iterations"] == 1 and r["refused"] == il.MAX_TRIALS
        assert all(t[2] == 0.0 and t[4] == il.DBL_MAX and not t[7] for t in tr)
        assert sc["edges"]["flags"][-1] == 0 and sc["edges"]["flags"][:-1].all()
        for k in il.STATE:
            assert r["estimate"][k].tobytes() == getattr(sc["graph"], k).tobytes(), k
        # the pivot that refuses is the first bias dof of the last state, and it is exactly 0
        o = ic.start_linearization(name)
        _, out, res = vm.solve(sc["graph"].fixed, sc["edges"], len(sc["recs"]), o["H_diag"], o["H_off"], o["b"], 0.0)
        assert res[vm.R_REFUSED] == 1 and out[2] == 0.0 and not o["H_diag"][n - 1][9:, 9:].any()
    else:
        assert r["refused"] == 0 and best < tr[0][3] and tr[0][-1] and sc["edges"]["flags"].all()
    if name == ic.REJECTING:
        assert "ra" in dec and dec.count("r") >= 3
    if name in ("chain 2", "chain 3", "chain 10", "chain 20"):
        assert x["iterations"] == ic.ITERATIONS                          # still gaining when the iterations run out: nothing is decided on rounding


def measure(name):
    """RUNS perturbed model loops against the unperturbed one: (the runs, the spread per output)"""
    if name not in _cache:
        ref = ic.model_run(name)
        y = ref["rounds"][0]
        last = lambda x: min([t[4] for t in x["trace"] if t[-1]] + [x["trace"][0][3]])  # noqa: E731
        spread, runs = dict.fromkeys(OUTPUTS, 0.0), []
        for k in range(RUNS):
            r = ic.run(name, ic.model_backend(name, il.Noise(1000 + k)))
            runs.append(r)
            x = r["rounds"][0]
            for o in ("v", "bg", "ba"):
                spread[o] = max(spread[o], _rel(r["estimate"][o], ref["estimate"][o]))
            spread["total"] = max(spread["total"], abs(last(x) - last(y)) / last(y))
            spread["lam"] = max(spread["lam"], abs(x["lam"] - y["lam"]) / y["lam"] if y["lam"] else abs(x["lam"]))
            for a, b in zip(x["trace"], y["trace"]):
                for key, dev in zip(TRIAL, trial_deviation(a, b)):
                    spread[key] = max(spread[key], dev)
        _cache[name] = (runs, spread)
    return _cache[name]


@pytest.mark.parametrize("name", list(ic.SCENES))
def test_the_scene_is_stable_and_the_spread_is_what_is_written(name):
    """THE CONDITION ON A SCENE, not a measurement of the code: a stage error of the size the stage tests allow (1e-9) in every trial
    output changes no decision, and no decision hangs on a rho below inertial_loop.RHO_MIN -- no chain scene reaches its minimum within
    its iterations, so none needs the exemption behind flat_from().  A scene that fails this is changed, never the condition."""
    ref = ic.model_run(name)
    runs, spread = measure(name)
    y = ref["rounds"][0]
    assert il.flat_from(y["trace"]) == len(y["trace"]), (name, [t[6] for t in y["trace"]])
    for r in runs:
        x = r["rounds"][0]
        assert il.decisions([x]) == il.decisions([y]) and x["iterations"] == y["iterations"] and r["refused"] == ref["refused"], name
        for o in ("Rwb", "twb"):                                         # fixed: not a byte moves, perturbed or not
            assert r["estimate"][o].tobytes() == ic.scene(name)["graph"].__dict__[o].tobytes(), o
    print('    "%s": {%s},' % (name, ", ".join('"%s": %.2e' % kv for kv in spread.items())))
    assert name in MEASURED_SPREAD, "no figures written for this scene"
    for k, v in spread.items():                                          # both sides: a figure written too large would widen the GPU test's bars
        w = MEASURED_SPREAD[name][k]
        assert w / 2 <= v <= 2 * w, (name, k, v, w)


# ---- the assembly and the velocity priors -------------------------------------------------------------------------------------------------
def _map(n, seed=5):
    """n_kf = n + 3 key frames, the last one bad; the window the first n of a permutation; state rows, records and prior slots three
    different permutations into arrays longer than the key-frame table (inertial_window_model.with_imu's layout)"""
    rng = np.random.RandomState(seed)
    n_kf = n + 3
    n_src, cap_bank, n_priors = n_kf + 2, n_kf + 3, n_kf + 1
    kf_imu = np.stack([rng.permutation(n_src)[:n_kf], rng.permutation(cap_bank)[:n_kf], rng.permutation(n_priors)[:n_kf]], 1).astype(np.int32)
    order = rng.permutation(n_kf - 1)
    bad = np.zeros(n_kf, np.uint8)
    bad[n_kf - 1] = 1
    return dict(bad=bad, window=order[:n].astype(np.int32), kf_imu=kf_imu, n_src=n_src, cap_bank=cap_bank, n_priors=n_priors, spare=int(order[n]))


def _problem(mp, **over):
    a = dict(mp, **over)
    return cm.problem(a["bad"], a["window"], a["kf_imu"], a["n_src"], a["cap_bank"], a["n_priors"])


@pytest.mark.parametrize("n", [2, 3, cm.MAX_WINDOW])
def test_the_assembly_model_writes_the_documented_lists(n):
    mp = _map(n)
    a = _problem(mp)
    w, imu = mp["window"], mp["kf_imu"]
    assert a["result"].tolist() == [n, 0, 0, 0, 0, 0, 0, 0]
    assert a["state_kf"].tolist() == w.tolist() and a["fixed"].tolist() == [15] + [fm.FIX_POSE] * (n - 1) == ic.chain_fixed(n).tolist()
    assert a["init_jobs"].tolist() == [[s, imu[w[s], 0], imu[w[s], 1]] for s in range(n)]
    assert a["inertial_edges"].tolist() == [[s, s + 1, imu[w[s], 1], fm.EDGE_WALKS] for s in range(n - 1)]      # the OLDER key frame's record
    assert a["recover_jobs"].tolist() == [[s, imu[w[s], 0], 0] for s in range(n)] and a["bias_ids"].tolist() == imu[w, 1].tolist()
    assert a["velo_jobs"].tolist() == imu[w][:, [0, 2]].tolist()
    for k in cm.OUT:
        assert a[k].shape == ((n - 1 if k == "inertial_edges" else n),) + ((cm.WIDTH[k],) if k in cm.WIDTH else ()), k


@pytest.mark.parametrize("case", ["bad", "repeated", "out_of_range", "negative", "imu_row", "imu_record", "imu_prior", "two"])
def test_a_refused_assembly_writes_minus_one_everywhere(case):
    n = 4
    mp = _map(n)
    w, imu = mp["window"].copy(), mp["kf_imu"].copy()
    unusable, imu_range = 1, 0
    if case == "bad":
        w[2] = len(mp["bad"]) - 1
    elif case == "repeated":
        w[3] = w[1]
    elif case == "out_of_range":
        w[0] = len(mp["bad"])
    elif case == "negative":
        w[1] = -1
    elif case == "two":
        w[0], w[3], unusable = -5, w[2], 2
        imu[w[1], 1], imu_range = mp["cap_bank"], 1
    else:
        unusable, imu_range = 0, 1
        col, v = dict(imu_row=(0, mp["n_src"]), imu_record=(1, -1), imu_prior=(2, mp["n_priors"]))[case]
        imu[w[n - 1], col] = v
    a = _problem(mp, window=w, kf_imu=imu)
    assert a["result"].tolist() == [n, (unusable != 0) * cm.REFUSE_WINDOW | (imu_range != 0) * cm.REFUSE_IMU, unusable, imu_range, 0, 0, 0, 0]
    for k in cm.OUT:
        assert (a[k] == (15 if k == "fixed" else -1)).all() and a[k].shape == _problem(mp)[k].shape, k
    # an index of a key frame outside the window does not matter
    imu2 = mp["kf_imu"].copy()
    imu2[mp["spare"]] = -7
    assert _problem(mp, kf_imu=imu2)["result"][cm.C_REFUSED] == 0


def test_the_velocity_prior_model_writes_three_floats_of_every_slot_named():
    rng = np.random.RandomState(3)
    priors, src = rng.uniform(-1, 1, (5, 36)).astype(np.float32), rng.uniform(-1, 1, (6, 15)).astype(np.float32)
    jobs = np.array([(4, 0), (1, 3), (6, 1), (2, 5), (-1, 2), (0, -1)], np.int32)
    out, res = cm.velocity_priors(priors, src, jobs)
    assert res.tolist() == [2, 4, 0, 0, 0, 0, 0, 0]
    assert out[0, :3].tobytes() == src[4, 12:].tobytes() and out[3, :3].tobytes() == src[1, 12:].tobytes()
    out[0, :3], out[3, :3] = priors[0, :3], priors[3, :3]
    assert out.tobytes() == priors.tobytes()


def test_a_chain_scene_laid_out_as_a_map_assembles_to_the_scene():
    sc = ic.scene(ic.MAP_SCENE)
    mp = cm.map_from_chain_scene(sc)
    a = cm.problem(mp["bad"], mp["window"], mp["kf_imu"], mp["n_src"], mp["cap_bank"], mp["n_priors"])
    assert a["result"][cm.C_REFUSED] == 0 and a["fixed"].tolist() == sc["graph"].fixed.tolist()
    assert a["inertial_edges"].tolist() == [[e["i"], e["j"], e["rec"], e["flags"]] for e in sc["edges"]]
    assert (mp["src"][a["init_jobs"][:, 1]] == sc["src"]).all() and a["init_jobs"][:, 2].tolist() == list(range(sc["graph"].n))
    g = fm.Graph(sc["graph"].n)
    fm.graph_init(g, sc["recs"], mp["src"], a["init_jobs"])
    for k in il.STATE:                                                   # nothing of this scene is disturbed behind graph_init
        assert getattr(g, k).tobytes() == getattr(sc["graph"], k).tobytes(), k
    assert mp["bad"][mp["bad_kf"]] == 1 and mp["bad_kf"] not in mp["window"] and mp["spare"] not in mp["window"]
