"""The graphs of tests/ba_graph_model.py before the device is asked anything: each has the structure it is in the table for, asserted
from its arrays, and each is ADMITTED by the rules of tests/test_ba_lm_paths.py -- every trial of the oracle decides by a margin of at
least 1e-3, its (iterations, trials) survive the eight 2^-50 jitter draws, its jitter sensitivity delta is at most 1e-7 and is the
recorded one within a factor 3 -- so that what tests/test_ba_graphs_gpu.py compares is the kernels and not the rounding of a decision.
A graph that fails a rule gets another seed, never a skip.  Also here: the longdouble model and the dense step against ba_ref, and
the oracle runs that both files share (computed once, never changed)."""
import numpy as np
import pytest

import ba_graph_model as gm
from test_ba_lm_paths import HUBER, N_DRAWS, _jitter, _margin, _rel, _same_within_3, _sensitivity

gm.caller_has_extended_precision()

_memo = {}
LAMBDAS = ("lambda0", "one", "lambda0_x1e6")     # user_lambda_init of the one-step runs


def _args(name, draw=None):
    args = gm.graph(name)["args"]
    return args if draw is None else _jitter(args, draw)


def _oracle(name, draw=None):
    """ba_ref.lm_optimize with Huber on a graph (draw: on its jittered inputs)"""
    from oracle import ba_ref
    if ("run", name, draw) not in _memo:
        _memo["run", name, draw] = ba_ref.lm_optimize(*_args(name, draw), HUBER, gm.GRAPHS[name]["iterations"])
    return _memo["run", name, draw]


def _local(name, draw=None):
    from oracle import ba_ref
    if ("local", name, draw) not in _memo:
        _memo["local", name, draw] = ba_ref.local_bundle_adjustment(*_args(name, draw), HUBER)
    return _memo["local", name, draw]


def _lambda(name, which):
    lam0 = _oracle(name)["trace"][0][2]
    return {"lambda0": lam0, "one": 1.0, "lambda0_x1e6": 1e6 * lam0}[which]


def _one_step(name, which, draw=None):
    """the oracle's first trial at a given lambda, through the Schur complement: max_iterations = max_trials = 1"""
    from oracle import ba_ref
    if ("step", name, which, draw) not in _memo:
        _memo["step", name, which, draw] = ba_ref.lm_optimize(*_args(name, draw), HUBER, 1, max_trials=1, user_lambda_init=_lambda(name, which))
    return _memo["step", name, which, draw]


def _dense(name, which):
    if ("dense", name, which) not in _memo:
        _memo["dense", name, which] = gm.dense_step(_args(name), HUBER, _lambda(name, which))
    return _memo["dense", name, which]


STEP_KEYS = ("pose_R", "pose_t", "points")


def _step_figures(name, which):
    """-> (the Schur route's deviation from the dense route, the step's sensitivity under the jitter draws), relative as _rel"""
    schur, dense = _one_step(name, which), _dense(name, which)
    route = max(_rel(schur[k], dense[k]) for k in STEP_KEYS)
    jitter = _sensitivity(schur, [_one_step(name, which, d) for d in range(N_DRAWS)], keys=STEP_KEYS)
    return route, jitter


def _local_counts(r):
    return (r["first_round"]["iterations"], r["first_round"]["trials"], r["iterations"], r["trials"])


# ----------------------------------------------------------------------------------------------------------------- structure
@pytest.mark.parametrize("name", sorted(gm.GRAPHS))
def test_every_graph_has_its_structure(name):
    args = _args(name)
    promise = gm.GRAPHS[name]["promise"]
    s = gm.structure(args)
    print(name, {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in s.items()})
    assert s["grouped"] and s["n_free"] == promise["n_free"]
    assert (s["obs0"], s["obs1"], s["obs2"]) == promise["obs"] and s["fixed_only"] == promise["fixed_only"]
    for count in promise.get("free_counts", ()):
        assert (s["free_edge_counts"] == count).sum() >= 1, count
    if promise.get("sparse", True):
        assert s["obs0"] >= 1 and s["obs1"] + s["obs2"] >= 1
        assert s["fixed_between_free"] >= 1
        assert s["empty_cells"] > 0.8
        assert s["unshared_pairs"] >= 1
    R = np.asarray(args[1]).reshape(-1, 3, 3)[np.asarray(args[3]) == 0]
    assert np.abs(R).min() > 0                                     # no entry of a free R is structurally 0
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-14


def test_the_table_covers_what_it_is_for():
    s = {name: gm.structure(_args(name)) for name in gm.GRAPHS}
    make = {name: g["make"] for name, g in gm.GRAPHS.items()}
    assert {23, 24, 1} <= {v["n_free"] for v in s.values()}        # the largest system in LDS, the first in global memory, one pose
    assert {255, 256, 257, 1025} <= {m["n_points"] for m in make.values()}
    assert any(m.get("camera") == "fisheye" for m in make.values())
    assert {"every_third", "reference"} <= {m.get("layout", "every_third") for m in make.values()}
    counts = np.concatenate([v["free_edge_counts"] for v in s.values()])
    assert {0, 1, 255, 256, 257} <= set(counts.tolist())
    assert not all(v["free_pose_is_affine"] for v in s.values())   # free_pose[i] != i + const somewhere
    assert max(v["n_edges"] for v in s.values()) < 6000
    for name in gm.DEVICE_FORM:                                    # what the device index build meets
        assert s[name]["obs0"] >= 1 and (s[name]["free_edge_counts"] <= 1).any() and s[name]["fixed_between_free"] >= 1
    assert set(gm.LOCAL_BA) <= set(gm.GRAPHS) and set(gm.DEVICE_FORM) <= set(gm.GRAPHS)


def test_the_sorted_and_relabelled_twins_are_the_same_graph():
    """shuffle=False undoes the shuffle and nothing else; "first" renumbers the poses of "every_third" and nothing else"""
    name = "third_12x256_b1"
    a, b, c = gm.graph(name), gm.graph(name, shuffle=False), gm.graph(name, layout="first")
    order = a["edge_order"]
    assert not np.array_equal(order, np.arange(len(order)))
    for k in (5, 6, 7, 8):
        assert np.array_equal(np.asarray(b["args"][k])[order], a["args"][k])
    for k in (1, 2, 3, 4):
        assert np.array_equal(b["args"][k], a["args"][k])
    new = c["new_of_old"]
    fixed = np.asarray(c["args"][3])
    assert fixed[:fixed.sum()].all() and not fixed[fixed.sum():].any()
    assert np.array_equal(np.asarray(c["args"][5]), new[np.asarray(a["args"][5])])
    for k in (1, 2, 3):
        assert np.array_equal(np.asarray(c["args"][k])[new], a["args"][k])
    for k in (4, 6, 7, 8):
        assert np.array_equal(c["args"][k], a["args"][k])


# ----------------------------------------------------------------------------------------------------------------- admission
@pytest.mark.parametrize("name", sorted(gm.GRAPHS))
def test_every_graph_is_admitted(name):
    ref = _oracle(name)
    runs = [_oracle(name, d) for d in range(N_DRAWS)]
    margin = _margin(ref["trace"])
    delta = _sensitivity(ref, runs)
    recorded = gm.GRAPHS[name]["delta"]
    print("%s: its / trials %d / %d, smallest margin %.3g, delta %.3g (recorded %.3g)" % (name, ref["iterations"], ref["trials"], margin, delta, recorded))
    assert len(ref["trace"]) == ref["trials"] and all(ok for *_, ok in ref["trace"])      # the Cholesky succeeds on every trial
    first = ref["trace"][0]
    assert first[6] > 0 and np.isfinite(first[4])                                          # the first trial is accepted
    assert margin >= 1e-3
    assert {(r["iterations"], r["trials"]) for r in runs} == {(ref["iterations"], ref["trials"])}
    assert delta <= 1e-7 and recorded <= 1e-7
    assert _same_within_3(delta, recorded)


@pytest.mark.parametrize("name", sorted(gm.LOCAL_BA))
def test_the_local_ba_graphs_are_admitted(name):
    """both rounds of Optimize.cpp:892-922, and no edge whose chi2 at the end of either round lies within 100 delta (relative) of 5.991"""
    ref = _local(name)
    runs = [_local(name, d) for d in range(N_DRAWS)]
    first = ref["first_round"]
    delta = max(_sensitivity(ref, runs), _sensitivity(first, [r["first_round"] for r in runs]))
    margin = min(_margin(first["trace"]), _margin(ref["trace"]))
    gap = min(np.abs(first["chi2"] / 5.991 - 1).min(), np.abs(ref["chi2_final_estimate"] / 5.991 - 1).min())
    recorded = gm.LOCAL_BA[name]
    print("%s local BA: rounds %s, smallest margin %.3g, delta %.3g (recorded %.3g), nearest chi2 to 5.991: %.3g relative, %d outliers" %
          (name, _local_counts(ref), margin, delta, recorded, gap, ref["outlier"].sum()))
    assert all(ok for r in (first, ref) for *_, ok in r["trace"])
    assert margin >= 1e-3
    assert {_local_counts(r) for r in runs} == {_local_counts(ref)}
    assert all(np.array_equal(r["outlier"], ref["outlier"]) for r in runs)
    assert delta <= 1e-7 and recorded <= 1e-7 and _same_within_3(delta, recorded)
    assert gap > 100 * max(delta, recorded)
    assert ref["outlier"].any() and not ref["outlier"].all()


@pytest.mark.parametrize("name", sorted(gm.GRAPHS))
def test_the_one_step_runs_keep_their_step(name):
    """at each of the three lambdas the oracle's only trial is accepted (what comes back is the step, not what pop() restored), and its
    two float64 routes -- Schur complement and the unmarginalised dense system -- agree far below the floor of the device comparison"""
    args = _args(name)
    for which in LAMBDAS:
        step = _one_step(name, which)
        route, jitter = _step_figures(name, which)
        tr = step["trace"][0]
        print("%s %s: lambda %.3g, rho %.3g, Schur against dense %.3g, jitter %.3g" % (name, which, tr[2], tr[6], route, jitter))
        assert (step["iterations"], step["trials"]) == (1, 1) and tr[7] and tr[6] > 0 and np.isfinite(tr[4])
        assert tr[2] == _lambda(name, which)
        assert max(np.abs(step[k] - np.asarray(a).reshape(step[k].shape)).max() for k, a in zip(STEP_KEYS, (args[1], args[2], args[4]))) > 0
        assert route <= 1e-9 and jitter <= 1e-7


# ----------------------------------------------------------------------------------------------------------------- the models
@pytest.mark.parametrize("name", ["third_12x256_b1", "fisheye_16x257_b1", "reference_24x257_b2"])
def test_the_longdouble_model_restates_the_oracle(name):
    """linearize_ld against ba_ref.linearize: per row within 1e-9 (the float64 oracle's own rounding is what remains), every zero of the
    structure exact, and the contributions sum to the blocks.  The float64 oracle is inside the derived bound of every block entry
    (block_bars, at the per-edge bar the device is given: 4 x the oracle's own largest per-edge figure) -- and outside it where an
    edge's two-term sum is taken as the term, which is why block_bars does not"""
    from oracle import ba_ref
    args = _args(name)
    ref, model = ba_ref.linearize(*args, HUBER), gm.linearize_ld(*args, HUBER)
    worst = {k: gm.row_error(ref[k], model[k]) for k in ("chi2", "error", "H_lp", "H_pp", "b_p", "H_ll", "b_l")}
    print(name, {k: "%.2g" % v for k, v in worst.items()})
    assert max(worst.values()) < 1e-9
    assert model["chi2"].dtype == np.longdouble and model["H_pp"].dtype == np.longdouble
    fixed = np.asarray(args[3], bool)
    assert not model["H_pp"][fixed].any() and not model["H_lp"][fixed[np.asarray(args[5])]].any()
    assert np.abs(model["c_H_ll"].sum(0) - model["H_ll"].sum(0)).max() <= 1e-15 * np.abs(model["c_H_ll"]).sum(0).max()
    per_edge_bar = 4.0 * max(worst[k] for k in ("chi2", "error", "H_lp"))
    ratio = {}
    for literal in (False, True):
        for k, (bar, m) in gm.block_bars(model, args[5], args[6], per_edge_bar, literal=literal).items():
            diff = np.abs(ref[k].astype(np.longdouble) - model[k])
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio[k, literal] = float(np.where(bar > 0, diff / bar, np.where(diff > 0, np.inf, 0.0)).max())
    print("    oracle error / derived bar %s; with an edge's sum as the term %s" % ({k: "%.3g" % v for (k, lit), v in ratio.items() if not lit},
                                                                                   {k: "%.3g" % v for (k, lit), v in ratio.items() if lit}))
    assert max(v for (k, lit), v in ratio.items() if not lit) <= 1.0
    if name == "reference_24x257_b2":                               # a pinhole pose with ONE edge: entry (2, 5) is pure cancellation
        assert ratio["H_pp", True] > 1.0
