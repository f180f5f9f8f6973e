"""The visual bundle adjustment of csrc/orbba.hip on the graphs of tests/ba_graph_model.py: banded visibility, edges shuffled inside
their points, fixed poses between the free ones -- the structure a local BA has and synth.make_ba_problem never draws.
  (a) orbba_linearize against the np.longdouble model, per edge row and per block entry, never by an array's global maximum;
  (b) exact metamorphic relations of the linearisation: the order of a point's edges, the numbering of the poses;
  (c) one damped step (max_iterations = max_trials = 1) at three lambdas against the UNMARGINALISED dense solve;
  (d) full LM runs and both rounds of Optimize.cpp:892-922 against the oracle, decisions exactly;
  (e) what the structure makes exact: fixed poses, points without an observation, free poses without an edge;
  (f) orbba_local_bundle_adjustment_device against the host form bit for bit, and both refusing what the index build refuses.
Every graph is admitted on the CPU first (tests/test_ba_graphs_cpu.py).  Every test prints its figures before it asserts.  A ratio
above its bar is a finding to explain from the kernels, not a bar to widen."""
import ctypes as C

import numpy as np
import pytest

import ba_graph_model as gm
from test_ba import _close
from test_ba_graphs_cpu import LAMBDAS, STEP_KEYS, _args, _dense, _lambda, _local, _local_counts, _oracle, _step_figures
from test_ba_lm_paths import HUBER, _rel, _tol

pytestmark = pytest.mark.gpu
gm.caller_has_extended_precision()

EVERY_THIRD = sorted(n for n, g in gm.GRAPHS.items() if g["make"].get("layout", "every_third") == "every_third")
PER_EDGE = ("chi2", "error", "H_lp")
BLOCKS = ("H_pp", "b_p", "H_ll", "b_l")


def _with_chol(chol, call):
    from monoorbslam3_amd import ba
    ba.set_variant("chol", chol)  # read per call
    try:
        return call()
    finally:
        ba.set_variant("chol", "lds")


def _same_bytes(a, b):
    return np.ascontiguousarray(a, np.float64).tobytes() == np.ascontiguousarray(b, np.float64).tobytes()


def _within(got, ref, tol):
    return abs(got - ref) <= tol * abs(ref)


def _exact_consequences(args, got):
    """(e): fixed poses keep their bytes; a point without an observation and a free pose without an edge keep theirs by value (their
    updates are H^-1 0 = 0, and exp(0) is the identity)"""
    R, t, fixed, P, ep, el = (np.asarray(args[k]) for k in (1, 2, 3, 4, 5, 6))
    fixed = fixed.astype(bool)
    R, t = R.reshape(-1, 3, 3), t.reshape(-1, 3)
    lone_points = np.flatnonzero(np.bincount(el, minlength=len(P)) == 0)
    lone_poses = np.flatnonzero(~fixed & (np.bincount(ep, minlength=len(fixed)) == 0))
    assert _same_bytes(got["pose_R"][fixed], R[fixed]) and _same_bytes(got["pose_t"][fixed], t[fixed])
    assert np.array_equal(got["points"][lone_points], P[lone_points])
    assert np.array_equal(got["pose_R"][lone_poses], R[lone_poses]) and np.array_equal(got["pose_t"][lone_poses], t[lone_poses])
    return len(lone_points), len(lone_poses)


# ----------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("name", sorted(gm.GRAPHS))
def test_linearize_against_the_longdouble_model(name):
    """Per edge (chi2, the error's row, the three rows of H_lp): the largest error relative to the row's own largest magnitude, held to 4 x
    the same figure of the float64 ba_ref.linearize -- both are float64 evaluations of the same expressions in different association
    orders.  Per entry of H_pp, b_p, H_ll, b_l: held to (m 2^-53 + the largest per-edge bar) sum_e |c_e|, derived in
    ba_graph_model.block_bars; an entry without an edge is exactly 0.0."""
    from oracle import ba_ref
    from monoorbslam3_amd import ba
    args = _args(name)
    model = gm.linearize_ld(*args, HUBER)
    ref = ba_ref.linearize(*args, HUBER)
    got = ba.linearize(*args, HUBER)
    figure = {k: (gm.row_error(got[k], model[k]), gm.row_error(ref[k], model[k])) for k in PER_EDGE}
    per_edge_bar = 4.0 * max(r for _, r in figure.values())
    bars = gm.block_bars(model, args[5], args[6], per_edge_bar)
    ratio, exact = {}, {}
    for k in BLOCKS:
        bar, m = bars[k]
        diff = np.abs(got[k].astype(np.longdouble) - model[k])
        held = bar > 0
        ratio[k] = float((diff[held] / bar[held]).max()) if held.any() else 0.0
        exact[k] = bool((diff[~held] == 0).all()) and bool((got[k][np.broadcast_to(m == 0, got[k].shape)] == 0.0).all())
    print("%s: %d edges; per edge, device / oracle against the model (bar: 4 x the oracle's): %s; blocks, error / derived bar: %s" %
          (name, len(args[5]), {k: "%.3g / %.3g" % v for k, v in figure.items()}, {k: "%.3g" % v for k, v in ratio.items()}))
    for k in PER_EDGE:
        assert figure[k][0] <= 4.0 * figure[k][1], k
    for k in BLOCKS:
        assert exact[k], k
        assert ratio[k] <= 1.0, k


# ----------------------------------------------------------------------------------------------------------------- (b)
@pytest.mark.parametrize("name", EVERY_THIRD)
def test_linearize_metamorphic_relations_are_exact(name):
    """Shuffling the edges inside the points leaves every pose's edges in their order: H_pp and b_p byte for byte, the per-edge outputs
    the same bytes after the permutation.  Renumbering the poses ("every_third" -> "first") leaves every sum in its order: H_pp and
    b_p the same blocks after the permutation, H_ll, b_l and the per-edge outputs byte for byte."""
    from monoorbslam3_amd import ba
    shuffled, ordered, first = gm.graph(name), gm.graph(name, shuffle=False), gm.graph(name, layout="first")
    a, b, c = (ba.linearize(*g["args"], HUBER) for g in (shuffled, ordered, first))
    order, new = shuffled["edge_order"], first["new_of_old"]
    moved = int((order != np.arange(len(order))).sum())
    print("%s: %d of %d edges moved by the shuffle, %d of %d poses renumbered" % (name, moved, len(order), int((new != np.arange(len(new))).sum()), len(new)))
    assert moved > len(order) // 4 and (new != np.arange(len(new))).any()
    assert np.abs(a["H_pp"]).max() > 0
    for k in ("H_pp", "b_p"):
        assert a[k].tobytes() == b[k].tobytes(), k
        assert np.ascontiguousarray(c[k][new]).tobytes() == a[k].tobytes(), k
    for k in PER_EDGE:
        assert np.ascontiguousarray(b[k][order]).tobytes() == a[k].tobytes(), k
        assert c[k].tobytes() == a[k].tobytes(), k
    for k in ("H_ll", "b_l"):
        assert c[k].tobytes() == a[k].tobytes(), k
        assert _close(b[k], a[k], 1e-12), k        # a point's sum in another order: rounding only


# ----------------------------------------------------------------------------------------------------------------- (c)
@pytest.mark.parametrize("chol", ["lds", "global"])
@pytest.mark.parametrize("name", sorted(gm.GRAPHS))
def test_one_damped_step_against_the_dense_solve(name, chol):
    """orbba_optimize with max_iterations = max_trials = 1 at user_lambda_init = the oracle's lambda0, 1.0 and 1e6 lambda0: one trial, kept.
    The stepped poses and points against the step solved on the full (6 NF + 3 NL) system without a Schur complement; the deviation
    (relative as test_ba_lm_paths._rel) is held to 4 x the larger of what the float64 oracle's Schur route deviates from the dense route
    and what the step moves under the eight jitter draws -- both measured on the CPU from the reference routes."""
    from monoorbslam3_amd import ba
    args = _args(name)
    for which in LAMBDAS:
        lam = _lambda(name, which)
        got = _with_chol(chol, lambda: ba.optimize(*args, huber_delta=HUBER, iterations=1, max_trials=1, user_lambda_init=lam))
        dense = _dense(name, which)
        route, jitter = _step_figures(name, which)
        deviation = {k: _rel(got[k], dense[k]) for k in STEP_KEYS}
        bar = 4.0 * max(route, jitter)
        print("%s %s %s: lambda %.4g, trials %d, chi2 %.6g -> %.6g; deviation from the dense step %s; Schur route %.3g, jitter %.3g, bar %.3g; "
              "worst / bar %.3g" % (name, chol, which, lam, got["trials"], got["chi2_initial"], got["chi2_final"],
                                    {k: "%.3g" % v for k, v in deviation.items()}, route, jitter, bar, max(deviation.values()) / bar))
        assert (got["iterations"], got["trials"]) == (1, 1)
        assert got["chi2_final"] < got["chi2_initial"] and not _same_bytes(got["pose_t"], args[2])       # the step is kept
        assert max(deviation.values()) <= bar, which
        _exact_consequences(args, got)


# ----------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("chol", ["lds", "global"])
@pytest.mark.parametrize("name", sorted(gm.GRAPHS))
def test_full_runs_match_the_oracle(name, chol):
    """orbba_optimize with Huber for the graph's iterations: the oracle's (iterations, trials) exactly, chi2_initial to 1e-9, estimates,
    lambda and chi2_final within max(1e-6, 100 delta), per-edge chi2 within max(1e-5, 100 delta)"""
    from monoorbslam3_amd import ba
    args, g = _args(name), gm.GRAPHS[name]
    ref = _oracle(name)
    got = _with_chol(chol, lambda: ba.optimize(*args, huber_delta=HUBER, iterations=g["iterations"]))
    tol, tol_edge = _tol(g["delta"]), _tol(g["delta"], 1e-5)
    worst = {k: _rel(got[k], ref[k]) for k in ("pose_R", "pose_t", "points", "chi2", "chi2_initial", "chi2_final", "lam")}
    print("%s %s: device %d / %d, oracle %d / %d, tol %.3g; relative differences %s" %
          (name, chol, got["iterations"], got["trials"], ref["iterations"], ref["trials"], tol, {k: "%.2g" % v for k, v in worst.items()}))
    assert (got["iterations"], got["trials"]) == (ref["iterations"], ref["trials"])
    assert _within(got["chi2_initial"], ref["chi2_initial"], 1e-9)
    assert _within(got["chi2_final"], ref["chi2_final"], tol) and _within(got["lam"], ref["lam"], tol)
    for k in STEP_KEYS:
        assert _close(got[k], ref[k], tol), k
    assert _close(got["chi2"], ref["chi2"], tol_edge)
    assert np.abs(got["pose_R"] @ got["pose_R"].transpose(0, 2, 1) - np.eye(3)).max() < 1e-12
    lone = _exact_consequences(args, got)
    print("    %d points without an observation and %d free poses without an edge kept their values" % lone)


@pytest.mark.parametrize("chol", ["lds", "global"])
@pytest.mark.parametrize("name", sorted(gm.LOCAL_BA))
def test_local_bundle_adjustment_matches_the_oracle(name, chol):
    """Optimize.cpp:892-922 on the "reference" layout and on the 23-free-pose graph: the oracle's outlier flags exactly, counts of both
    rounds, estimates within tolerance"""
    from monoorbslam3_amd import ba
    args = _args(name)
    ref = _local(name)
    got = _with_chol(chol, lambda: ba.local_bundle_adjustment(*args))
    tol, tol_edge = _tol(gm.LOCAL_BA[name]), _tol(gm.LOCAL_BA[name], 1e-5)
    print("%s local BA %s: device %d / %d, oracle %s, %d outliers (oracle %d); relative differences %s" %
          (name, chol, got["iterations"], got["trials"], _local_counts(ref), got["outlier"].sum(), ref["outlier"].sum(),
           {k: "%.2g" % _rel(got[k], ref[k]) for k in ("pose_R", "pose_t", "points", "chi2", "chi2_final", "lam")}))
    assert (got["iterations"], got["trials"]) == (ref["first_round"]["iterations"] + ref["iterations"], ref["first_round"]["trials"] + ref["trials"])
    assert np.array_equal(got["outlier"], ref["outlier"])
    assert _within(got["chi2_initial"], ref["first_round"]["chi2_initial"], 1e-9)
    assert _within(got["chi2_final"], ref["chi2_final"], tol) and _within(got["lam"], ref["lam"], tol)
    for k in STEP_KEYS:
        assert _close(got[k], ref[k], tol), k
    assert _close(got["chi2"], ref["chi2"], tol_edge)
    _exact_consequences(args, got)


# ----------------------------------------------------------------------------------------------------------------- (f)
def _as_problem(args):
    cam, R, t, fixed, P, ep, el, z, w = args
    f8 = lambda a: np.ascontiguousarray(a, np.float64)  # noqa: E731
    return dict(pose_R=f8(R).reshape(-1, 9), pose_t=f8(t), pose_fixed=np.ascontiguousarray(fixed, np.uint8), ba_points=f8(P),
                edge_pose=np.ascontiguousarray(ep, np.int32), edge_point=np.ascontiguousarray(el, np.int32), edge_z=f8(z), edge_inv_sigma2=f8(w))


@pytest.mark.parametrize("stream_kind", ["null", "explicit"])
@pytest.mark.parametrize("chol", ["lds", "global"])
@pytest.mark.parametrize("name", gm.DEVICE_FORM)
def test_the_device_form_equals_the_host_form_bit_for_bit(name, chol, stream_kind):
    """orbba_local_bundle_adjustment_device builds pose_off, pose_edges, point_off, free_pose, pose_slot and edge_of with k_lmi_* from
    shuffled edges, interleaved fixed poses, empty point ranges and poses without an edge; poses, points, chi2, outlier flags,
    iterations, trials and lambda then equal the host form's, whose index the host built, bit for bit -- on the null stream and on a
    non-blocking one"""
    import torch
    from monoorbslam3_amd import ba
    from test_local_ba_gpu import _bits_equal, _lm_outputs
    from test_triangulation_gpu import _stream, _up
    dev = torch.device("cuda", 0)
    args = _args(name)
    prob = _as_problem(args)
    n_poses, n_points, n_edges = len(prob["pose_t"]), len(prob["ba_points"]), len(prob["edge_pose"])
    host = _with_chol(chol, lambda: ba.local_bundle_adjustment(*args))
    d = {k: _up(torch, dev, v) for k, v in prob.items()}
    out = _lm_outputs(torch, dev, n_poses, n_points, n_edges)
    st = _stream(torch, dev, stream_kind)
    try:
        info = _with_chol(chol, lambda: ba.local_bundle_adjustment_device(args[0], dict(d, **out), n_poses, n_points, n_edges, stream=st))
        torch.cuda.synchronize()
    finally:
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
    print("%s %s %s stream: iterations %d trials %d lambda %.6g chi2 %.6g -> %.6g outliers %d" %
          (name, chol, stream_kind, info["iterations"], info["trials"], info["lam"], info["chi2_initial"], info["chi2_final"], int(host["outlier"].sum())))
    assert info["iterations"] >= 3 and host["outlier"].any()
    _bits_equal(out, info, host)


def _twice(prob):
    """a second edge of a free pose and a point, among that point's shuffled edges"""
    ep, el, fixed = prob["edge_pose"], prob["edge_point"], prob["pose_fixed"]
    off = np.searchsorted(el, np.arange(len(prob["ba_points"]) + 1))
    for j in range(len(off) - 1):
        mine = np.arange(off[j], off[j + 1])
        free = mine[fixed[ep[mine]] == 0]
        if len(mine) >= 3 and len(free) >= 1:
            out = ep.copy()
            out[mine[mine != free[0]][-1]] = ep[free[0]]
            return dict(prob, edge_pose=out)
    raise AssertionError("no point with three edges and a free pose")


def _out_of_order(prob):
    """a point index below its predecessor's"""
    el = prob["edge_point"].copy()
    e = len(el) // 2
    assert el[e - 1] >= 1
    el[e] = el[e - 1] - 1
    return dict(prob, edge_point=el)


@pytest.mark.parametrize("what", ["twice", "out_of_order"])
def test_both_forms_refuse_a_broken_graph_alike(what):
    """a shuffled graph with a duplicated (pose, point) edge, and one with a point index below its predecessor's: ORBX_E_ARG from both
    forms with the host form's message, every output as passed"""
    import torch
    from monoorbslam3_amd import _lib, ba
    from test_local_ba_gpu import _lm_outputs
    from test_triangulation_gpu import _up
    dev = torch.device("cuda", 0)
    args = _args("third_12x256_b1")
    prob = {"twice": _twice, "out_of_order": _out_of_order}[what](_as_problem(args))
    message = {"twice": "a point is observed twice by the same key frame", "out_of_order": "edges must be grouped by point"}[what]
    n_poses, n_points, n_edges = len(prob["pose_t"]), len(prob["ba_points"]), len(prob["edge_pose"])
    # the host form, through the C call so that its outputs are the caller's
    p, keep = ba._problem(args[0], prob["pose_R"], prob["pose_t"], prob["pose_fixed"], prob["ba_points"], prob["edge_pose"], prob["edge_point"],
                          prob["edge_z"], prob["edge_inv_sigma2"], HUBER)
    host_out, res = ba._lm_out(p)
    for v in host_out.values():
        v.fill(-3.0)
    outlier = np.full(n_edges, 9, np.uint8)
    rc = ba._L().orbba_local_bundle_adjustment(C.byref(p), C.byref(res), outlier.ctypes.data, -1)
    host_message = _lib.lib().orbx_last_error().decode("utf-8", "replace")
    # the device form
    d = {k: _up(torch, dev, v) for k, v in prob.items()}
    out = _lm_outputs(torch, dev, n_poses, n_points, n_edges)
    before = {k: v.cpu().numpy().copy() for k, v in out.items()}
    with pytest.raises(_lib.OrbxError) as err:
        ba.local_bundle_adjustment_device(args[0], dict(d, **out), n_poses, n_points, n_edges)
    torch.cuda.synchronize()
    print("%s: host form %d '%s'; device form '%s'" % (what, rc, host_message, err.value))
    assert rc != 0 and host_message == message
    assert err.value.code == rc and str(err.value) == str(_lib.OrbxError(rc, host_message))
    assert all((v == -3.0).all() for v in host_out.values()) and (outlier == 9).all()
    for k, v in out.items():
        assert v.cpu().numpy().tobytes() == before[k].tobytes(), k
