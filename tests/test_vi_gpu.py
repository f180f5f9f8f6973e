"""The visual edges on the inertial graph and the damped step on the MI355X (include/orbvi.h) against tests/vi_model.py.
Pinhole: d_err and d_chi2 equal the model BIT FOR BIT (only +, -, *, / and sqrt are involved and contraction is off); every summed
output (the pose block of H, b, the totals) within 1e-9 of the model relative to the largest entry of its own block, the bar of the
f64 BA kernels and of tests/test_factors_gpu.py.  Kannala-Brandt (atan, atan2): 1e-9 on everything.  The solve: d_dx and d_out equal
the ordered model bit for bit on identical input bytes, and the device's dx meets the backward-error bar of tests/test_vi_cpu.py.
Every output sits between guard elements.  Model outputs are computed once per scene and shared.  The largest deviation met is
printed per output."""
import numpy as np
import pytest

import factors_model as fm
import imu_model as im
import vi_model as vm
from test_factors_gpu import _Dev, _calib, _same_floats
from test_observations_gpu import _guards_intact, _padded
from test_projection_queries_gpu import _stream, _up

pytestmark = pytest.mark.gpu

BAR = 1e-9
NAN = float("nan")
_cache = {}


def _close(what, got, want):
    """within BAR of the model relative to the largest entry of the block"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    scale = np.abs(want).max() if want.size else 0.0
    rel = float(np.abs(got - want).max() / scale) if scale > 0 else float(np.abs(got).max() if got.size else 0.0)
    print("%-40s largest deviation %.3g of the block's largest entry" % (what, rel))
    assert rel <= BAR, (what, rel)


def _same(what, got, want):
    """bit for bit where the model holds a number; not a number where it does not (the payload of a NaN is not arithmetic)"""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    diff = got.view(np.uint64)[~nan] != want.view(np.uint64)[~nan]
    assert not diff.any(), (what, int(diff.sum()), "of", diff.size, "differ")


def _camera(cam):
    from monoorbslam3_amd import vi
    return vi.Camera.make(cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["model"], cam["k"])


class _Vis:
    """the device memory of one orbvi_linearize_device call: the graph, the edges and every output, padded"""

    def __init__(self, torch, dev, g, cal, cam, group_state, edge_off, cap, P, z, w, active=None, H0=None, b0=None):
        from monoorbslam3_amd import imu
        self.torch, self.dev, self.pads = torch, dev, {}
        self.n, self.ng, self.cap = g.n, len(group_state), cap
        c1 = max(cap, 1)
        self.graph_t = [_up(torch, dev, a) for a in (g.Rwb.reshape(-1), g.twb.reshape(-1), g.v.reshape(-1), g.bg.reshape(-1), g.ba.reshape(-1), g.fixed)]
        self.graph = imu.Graph.make(*self.graph_t, g.n)
        self.cal, self.cam = _calib(cal), _camera(cam)
        self.group_state, self.edge_off = _up(torch, dev, np.asarray(group_state, np.int32)), _up(torch, dev, np.asarray(edge_off, np.int32))
        room = lambda a, k: np.concatenate([np.asarray(a, np.float64).reshape(-1), np.zeros(k * c1)])[:k * c1]  # noqa: E731
        self.points, self.z, self.w = _up(torch, dev, room(P, 3)), _up(torch, dev, room(z, 2)), _up(torch, dev, room(w, 1))
        self.err, self.chi2 = self._pad("err", np.full(2 * c1, NAN), -1.5), self._pad("chi2", np.full(c1, NAN), -1.5)
        self.total = self._pad("total", np.full(2 * max(self.ng, 1), NAN), -1.5)
        self.work = self._pad("work", np.full(vm.EDGE_WORK * c1, NAN), -1.5)
        self.H_diag = self._pad("H_diag", np.full(225 * g.n, NAN) if H0 is None else H0.reshape(-1), -1.5)
        self.b = self._pad("b", np.full(15 * g.n, NAN) if b0 is None else b0.reshape(-1), -1.5)
        act = np.full(c1, 0xEE, np.uint8) if active is None else np.concatenate([np.asarray(active, np.uint8), np.zeros(c1, np.uint8)])[:c1]
        self.active = self._pad("active", act, 0xA5)
        self.n_inliers = self._pad("n_inliers", np.full(max(self.ng, 1), -9, np.int32), -7)
        self.result = self._pad("result", np.full(8, 77, np.int32), -6)

    def _pad(self, key, a, fill):
        self.pads[key] = (_padded(self.torch, self.dev, a, fill), fill)
        return self.pads[key][0][1]

    def run(self, mode, use_active=False, delta=vm.HUBER_MONO, threshold=vm.CHI2_MONO, null_Hb=False, stream=None):
        from monoorbslam3_amd import vi
        vi.linearize_device(self.graph, self.cal, self.cam, self.ng, self.cap, self.group_state, self.edge_off, self.points, self.z, self.w, self.err,
                            self.chi2, self.result, self.active if (use_active or mode == 2) else None, delta, threshold, mode,
                            None if mode == 2 else self.total, None if null_Hb else self.H_diag, None if null_Hb else self.b,
                            self.n_inliers if mode == 2 else None, self.work if mode == 0 else None, stream=stream)

    def get(self, key, shape=None):
        a = getattr(self, key).cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def finish(self):
        self.torch.cuda.synchronize()
        self.torch.cuda.set_stream(self.torch.cuda.default_stream(self.dev))
        for key, ((whole, _), fill) in self.pads.items():
            assert _guards_intact(whole, fill), key


def _start(n, seed=0):
    """what d_H_diag and d_b hold before the call: not zero, symmetric blocks"""
    rng = np.random.RandomState(90 + seed)
    H0 = rng.normal(0, 10.0, (n, 15, 15))
    return H0 + H0.transpose(0, 2, 1), rng.normal(0, 10.0, (n, 15))


def _scene(n_edges, model):
    key = ("scene", n_edges, model)
    if key not in _cache:
        sc = vm.pose_full_scene(n_edges, model=model)
        sc["H0"], sc["b0"] = _start(2)
        _cache[key] = sc
    return _cache[key]


def _model(sc, g, mode, active=None, H0=None, b0=None, group_state=None, edge_off=None, cap=None, delta=vm.HUBER_MONO):
    cap = sc["n_edges"] if cap is None else cap
    return vm.linearize(g, sc["cal"], sc["cam"], sc["group_state"] if group_state is None else group_state, sc["edge_off"] if edge_off is None else edge_off,
                        cap, sc["points"], sc["z"], sc["w"], active, delta, vm.CHI2_MONO, mode, H0, b0,
                        np.full((max(cap, 1), 2), NAN)[:cap], np.full(max(cap, 1), NAN)[:cap])


def _device(torch, sc, g, mode, active=None, H0=None, b0=None, group_state=None, edge_off=None, cap=None, delta=vm.HUBER_MONO, null_Hb=False,
            stream_kind="explicit"):
    dev = torch.device("cuda", 0)
    cap = sc["n_edges"] if cap is None else cap
    d = _Vis(torch, dev, g, sc["cal"], sc["cam"], sc["group_state"] if group_state is None else group_state, sc["edge_off"] if edge_off is None else edge_off,
             cap, sc["points"][:cap], sc["z"][:cap], sc["w"][:cap], active, H0, b0)
    d.run(mode, active is not None, delta, null_Hb=null_Hb, stream=_stream(torch, dev, stream_kind))
    d.finish()
    return d


def _assert_outputs(what, d, o, mode, exact, states=()):
    """err, chi2 (bit for bit when `exact`), the totals, and for the listed states the pose block of H and b against the model; everything
    else of H and b keeps its bytes"""
    cap = d.cap
    err, chi2 = d.get("err")[:2 * cap].reshape(cap, 2), d.get("chi2")[:cap]
    if exact:
        _same(what + ": err", err, o["err"])
        _same(what + ": chi2", chi2, o["chi2"])
    else:
        fin = np.isfinite(o["chi2"])
        assert np.array_equal(np.isfinite(chi2), fin) and np.array_equal(np.isfinite(err).all(1), fin), what
        _close(what + ": err", err[fin], o["err"][fin])
        _close(what + ": chi2", chi2[fin], o["chi2"][fin])
    assert np.array_equal(d.get("result"), o["result"]), (what, d.get("result"), o["result"])
    if mode == 2:
        assert np.array_equal(d.get("active")[:cap], o["active"]) and np.array_equal(d.get("n_inliers")[:d.ng], o["n_inliers"]), what
        return
    tot = d.get("total")[:2 * d.ng].reshape(d.ng, 2)
    for g in range(d.ng):
        _close(what + ": total", tot[g], o["total"][g])
    if mode == 0:
        H, b = d.get("H_diag", (d.n, 15, 15)), d.get("b", (d.n, 15))
        keep = np.ones((d.n, 15, 15), bool)
        for s in states:
            keep[s, :6, :6] = False
            _close(what + ": H", H[s, :6, :6], o["H_diag"][s, :6, :6])
            _close(what + ": b", b[s, :6], o["b"][s, :6])
            assert np.array_equal(H[s, :6, :6], H[s, :6, :6].T), what                 # symmetric, as what it was added to
        assert H[keep].tobytes() == o["H_diag"][keep].tobytes(), what                   # everything else keeps its bytes
        kb = keep[:, 0, :]
        assert b[kb].tobytes() == o["b"][kb].tobytes(), what


# ---- linearise --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_edges", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_one_pinhole_group_equals_the_model(n_edges):
    """the wave, the workgroup and the second- and third-trip edges; the call ADDS on top of a non-zero d_H_diag and d_b"""
    import torch
    sc = _scene(n_edges, 0)
    key = ("lin0", n_edges)
    if key not in _cache:
        _cache[key] = _model(sc, sc["graph"], 0, H0=sc["H0"], b0=sc["b0"])
    d = _device(torch, sc, sc["graph"], 0, H0=sc["H0"], b0=sc["b0"])
    _assert_outputs("pinhole %d" % n_edges, d, _cache[key], 0, True, (1,))
    if n_edges:
        assert not np.array_equal(d.get("H_diag", (2, 15, 15))[1, :6, :6], sc["H0"][1, :6, :6])


@pytest.mark.parametrize("n_edges,stream_kind", [(65, "null"), (1025, "explicit")])
def test_one_fisheye_group_equals_the_model(n_edges, stream_kind):
    import torch
    sc = _scene(n_edges, 1)
    key = ("lin1", n_edges)
    if key not in _cache:
        _cache[key] = _model(sc, sc["graph"], 0, H0=sc["H0"], b0=sc["b0"])
    d = _device(torch, sc, sc["graph"], 0, H0=sc["H0"], b0=sc["b0"], stream_kind=stream_kind)
    _assert_outputs("fisheye %d" % n_edges, d, _cache[key], 0, False, (1,))


def _three_groups():
    """three states, three groups on states 2, 0 and 1 with the middle group empty; state 1's pose fixed"""
    if "three" not in _cache:
        sc = dict(fm.make_chain(2, seed=5))
        g = sc["graph"]
        g.fixed[:] = [0, fm.FIX_POSE, fm.FIX_VELO]
        rng = np.random.RandomState(12)
        parts = [vm.make_edges(sc["cal"], vm.PINHOLE, g.Rwb[s], g.twb[s], n, rng) for s, n in ((2, 100), (1, 70))]
        sc.update(cam=vm.PINHOLE, points=np.concatenate([p[0] for p in parts]), z=np.concatenate([p[1] for p in parts]), w=np.concatenate([p[2] for p in parts]),
                  n_edges=170, group_state=np.array([2, 0, 1], np.int32), edge_off=np.array([0, 100, 100, 170], np.int32))
        sc["H0"], sc["b0"] = _start(3, 1)
        _cache["three"] = sc
    return _cache["three"]


def test_three_groups_with_the_middle_one_empty():
    """more than one workgroup: the counters are added up; the empty group writes zero totals and adds exact zeros; the group on the
    fixed pose writes its errors and totals and leaves H and b alone"""
    import torch
    sc = _three_groups()
    o = _model(sc, sc["graph"], 0, H0=sc["H0"], b0=sc["b0"])
    assert o["result"].tolist() == [3, 0, 0, 0, 0, 0, 0, 0] and not o["total"][1].any() and o["total"][2].all()
    assert np.array_equal(o["H_diag"][1], sc["H0"][1]) and np.array_equal(o["H_diag"][0], sc["H0"][0])
    d = _device(torch, sc, sc["graph"], 0, H0=sc["H0"], b0=sc["b0"])
    _assert_outputs("three groups", d, o, 0, True, (2, 0))


def test_mode_1_leaves_h_and_b_alone_also_when_they_are_null():
    import torch
    sc = _scene(400, 0)
    o = _model(sc, sc["graph"], 1)
    for null_Hb in (False, True):
        d = _device(torch, sc, sc["graph"], 1, H0=sc["H0"], b0=sc["b0"], null_Hb=null_Hb)
        _assert_outputs("mode 1", d, o, 1, True)
        assert d.get("H_diag").tobytes() == sc["H0"].tobytes() and d.get("b").tobytes() == sc["b0"].tobytes()
        assert np.isnan(d.get("work")).all()                                            # the workspace belongs to mode 0


def _odd_scene():
    """400 edges with a measurement that is not a number (its chi2 is not one either: an inlier, as in the reference) and a point on the
    camera plane Z = 0 (an infinite error: an outlier)"""
    if "odd" not in _cache:
        sc = dict(_scene(400, 0))
        sc["z"], sc["points"] = sc["z"].copy(), sc["points"].copy()
        sc["z"][17, 0] = NAN
        Rcw, tcw, _, _ = vm.derive_pose(sc["cal"], sc["graph"].Rwb[1], sc["graph"].twb[1])
        # a point (0, 0, z) with fl(r22 * z) == -t2: the products with the zeros add nothing, so Z is exactly 0 in the device's arithmetic
        z0 = -tcw[2] / Rcw[2, 2]
        cands = [z0]
        for k in range(16):
            cands += [np.nextafter(cands[-2 if k else -1], np.inf)] if k % 2 == 0 else [np.nextafter(min(cands), -np.inf)]
        hit = [c for c in cands if Rcw[2, 2] * c == -tcw[2]]
        assert hit, "no z within a few ulps puts the point on the camera plane exactly"
        sc["points"][230] = [0.0, 0.0, hit[0]]
        Pc, _, _ = vm.edge_errors(sc["cam"], Rcw, tcw, sc["points"][230:231], sc["z"][230:231], sc["w"][230:231])
        Z = Pc[2][0]
        assert Pc[0][0] != 0.0
        assert Z == 0.0
        _cache["odd"] = sc
    return _cache["odd"]


def test_mode_2_is_the_references_classification_and_feeds_the_drop():
    """d_active = !(chi2 > 5.991) with a chi2 that is not a number left an inlier; orbba_pose_drop_outliers_device then clears exactly
    those slots of the frame"""
    import torch
    from monoorbslam3_amd import ba
    sc = _odd_scene()
    o = _model(sc, sc["graph"], 2)
    assert o["active"][17] == 1 and o["active"][230] == 0 and 0 < o["n_inliers"][0] < 400 and o["result"].tolist() == [1, 0, 0, 0, 2, 0, 0, 0]
    assert np.isnan(o["chi2"][17]) and np.isinf(o["chi2"][230])
    d = _device(torch, sc, sc["graph"], 2, H0=sc["H0"], b0=sc["b0"], null_Hb=True)
    _assert_outputs("mode 2", d, o, 2, True)
    assert d.get("H_diag").tobytes() == sc["H0"].tobytes() and np.isnan(d.get("total")).all()
    dev = torch.device("cuda", 0)
    n2 = 1000
    kp = np.random.RandomState(3).permutation(n2)[:400].astype(np.int32)
    frame_mp = np.arange(n2, dtype=np.int32)
    d_mp = _padded(torch, dev, frame_mp, -3)
    ba.pose_drop_outliers_device(n2, d.edge_off, _up(torch, dev, kp), d.active, d_mp[1])
    torch.cuda.synchronize()
    want = frame_mp.copy()
    want[kp[o["active"] == 0]] = -1
    assert _guards_intact(d_mp[0], -3) and np.array_equal(d_mp[1].cpu().numpy(), want) and (want == -1).sum() == 400 - o["n_inliers"][0]


def test_masks_a_fixed_pose_and_edges_that_are_not_finite():
    """a partly active mask, no active edge at all, a fixed pose, and the two edges that are not finite: counted, left out of H, b and
    the totals, their error and chi2 written as computed"""
    import torch
    sc = _odd_scene()
    g = sc["graph"]
    part = (np.random.RandomState(8).uniform(size=400) < 0.6).astype(np.uint8)
    part[[17, 230]] = [1, 0]
    for what, active, graph, nonfinite in (("partly active", part, g, 1), ("every edge active", None, g, 2), ("no edge active", np.zeros(400, np.uint8), g, 0)):
        o = _model(sc, graph, 0, active, sc["H0"], sc["b0"])
        assert o["result"].tolist() == [1, 0, 0, 0, nonfinite, 0, 0, 0] and np.isfinite(o["H_diag"]).all() and np.isfinite(o["total"]).all()
        d = _device(torch, sc, graph, 0, active, sc["H0"], sc["b0"])
        _assert_outputs(what, d, o, 0, True, (1,))
        if active is not None:
            assert np.array_equal(d.get("active")[:400], active)                        # read, not written
    fixed = g.copy()
    fixed.fixed[1] |= fm.FIX_POSE
    o = _model(sc, fixed, 0, None, sc["H0"], sc["b0"])
    assert np.array_equal(o["H_diag"], sc["H0"]) and o["total"].all()
    d = _device(torch, sc, fixed, 0, None, sc["H0"], sc["b0"])
    _assert_outputs("fixed pose", d, o, 0, True)
    assert d.get("H_diag").tobytes() == sc["H0"].tobytes() and d.get("b").tobytes() == sc["b0"].tobytes()


def test_two_runs_of_the_2049_edge_group_give_the_same_bytes():
    import torch
    sc = _scene(2049, 0)
    runs = []
    for _ in range(2):
        d = _device(torch, sc, sc["graph"], 0, H0=sc["H0"], b0=sc["b0"])
        runs.append({k: d.get(k).tobytes() for k in ("err", "chi2", "total", "H_diag", "b", "work", "result")})
    assert runs[0] == runs[1]


# ---- distrust -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,group_state,edge_off,cap,want", [
    ("an offset above cap_edges", [2, 0, 1], [0, 100, 100, 9999], 150, [3, 0, 0]),
    ("decreasing offsets", [2, 0, 1], [0, 100, 40, 170], 170, [3, 0, 0]),
    ("negative offsets", [2, 0, 1], [-5, 100, -2147483648, 170], 170, [3, 0, 0]),
    ("offsets far past the arrays", [2, 0, 1], [2147483647, 2147483647, 2147483647, 2147483647], 170, [3, 0, 0]),
    ("a state out of range", [2, 3, 1, -1], [0, 60, 100, 150, 170], 170, [2, 2, 0]),
    ("a state named twice", [2, 0, 2, 7, 7], [0, 60, 100, 150, 160, 170], 170, [2, 2, 1]),
])
def test_distrusted_ranges_and_states(what, group_state, edge_off, cap, want):
    """the counters are the model's, the outputs are the model's, nothing is touched past cap_edges (the guards)"""
    import torch
    sc = _three_groups()
    gs, eo = np.array(group_state, np.int32), np.array(edge_off, np.int64).astype(np.int32)
    o = _model(sc, sc["graph"], 0, None, sc["H0"], sc["b0"], gs, eo, cap)
    assert o["result"][:3].tolist() == want, o["result"]
    d = _device(torch, sc, sc["graph"], 0, None, sc["H0"], sc["b0"], gs, eo, cap)
    done = [int(s) for k, s in enumerate(gs) if 0 <= s < 3 and s not in gs[:k].tolist() and not sc["graph"].fixed[s] & fm.FIX_POSE]
    _assert_outputs(what, d, o, 0, True, done)
    o2 = _model(sc, sc["graph"], 2, None, None, None, gs, eo, cap)
    d2 = _device(torch, sc, sc["graph"], 2, None, sc["H0"], sc["b0"], gs, eo, cap, null_Hb=True)
    _assert_outputs(what + ", mode 2", d2, o2, 2, True)


# ---- solve ----------------------------------------------------------------------------------------------------------------------------------------
def _systems():
    """name -> (fixed, edges, cap, H_diag, H_off, b, lambda): the tracker systems of poseInertialOptimize (12 free dof) and poseFullOptimize
    (18), a 4-state chain with walks, and two edges on one pair"""
    if "systems" in _cache:
        return _cache["systems"]
    out = {}
    sc = _scene(400, 0)
    for name, extra in (("pose full", 0), ("pose inertial", fm.FIX_POSE)):
        g = sc["graph"].copy()
        g.fixed[1] |= extra
        oi = vm.inertial_linearize(sc, g)
        ov = _model(sc, g, 0, None, oi["H_diag"], oi["b"])
        h_max = vm.solve(g.fixed, sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], 0.0)[1][1]
        out[name] = (g.fixed.copy(), sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], vm.TAU * h_max)
        out[name + ", lambda 0"] = out[name][:6] + (0.0,)
    assert [(~vm.dof_fixed(out[k][0])).sum() for k in ("pose full", "pose inertial")] == [18, 12]
    fixed, edges, cap, H, Ho, b, lam = out["pose full"]
    out["two edges on one pair"] = (fixed, np.concatenate([edges, edges]), cap, H, np.concatenate([0.5 * Ho, 0.5 * Ho]), b, lam)
    out["a dropped edge"] = (fixed, np.array([tuple(edges[0]), (0, 1, cap, 0), (1, 1, 0, 0), (0, 2, 0, 0)], fm.EDGE), cap, H, np.concatenate([Ho] * 4), b, lam)
    ch = fm.make_chain(3, seed=6)
    ch["graph"].fixed[:] = [15, 0, fm.FIX_GYRO, 0]
    info, walk, _ = fm.edge_information(ch["recs"], ch["edges"])
    oc = fm.linearize(ch["graph"], ch["recs"], ch["cal"]["gravity"], ch["edges"], info, walk, None, None, fm.HUBER_DELTA)
    h_max = vm.solve(ch["graph"].fixed, ch["edges"], len(ch["recs"]), oc["H_diag"], oc["H_off"], oc["b"], 0.0)[1][1]
    out["a 4-state chain"] = (ch["graph"].fixed.copy(), ch["edges"], len(ch["recs"]), oc["H_diag"], oc["H_off"], oc["b"], vm.TAU * h_max)
    # a free state that no edge touches, at lambda 0: refused
    out["refused"] = (np.concatenate([fixed, [0]]).astype(np.uint8), edges, cap, np.concatenate([H, np.zeros((1, 15, 15))]), Ho,
                      np.concatenate([b, np.zeros((1, 15))]), 0.0)
    for name, s in out.items():
        out[name] = s + (vm.solve(*s),)
    assert out["refused"][7][2].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and out["a dropped edge"][7][2].tolist() == [1, 3, 0, 0, 0, 0, 0, 0]
    assert all(s[7][2][vm.R_DONE] == 1 for k, s in out.items() if k != "refused")
    assert np.array_equal(out["two edges on one pair"][7][0], out["pose full"][7][0])          # 0.5 B + 0.5 B is B exactly
    _cache["systems"] = out
    return out


def _solve_on_device(torch, dev, fixed, edges, cap, H, Ho, b, lams, stream_kind="explicit"):
    """one orbvi_solve_device per lambda, each read from the SAME device double, which a device-side copy changes in between; one wait"""
    from monoorbslam3_amd import vi
    n = len(fixed)
    d_fixed, d_edges, d_H, d_Ho, d_b = (_up(torch, dev, a) for a in (fixed, edges, H.reshape(-1), Ho.reshape(-1), b.reshape(-1)))
    d_lams, d_lam = _up(torch, dev, np.asarray(lams, np.float64)), _padded(torch, dev, np.full(1, NAN), -1.5)
    pads = [(_padded(torch, dev, np.full(15 * n, NAN), -1.5), _padded(torch, dev, np.full(3, NAN), -1.5), _padded(torch, dev, np.full(8, 77, np.int32), -6)) for _ in lams]
    st = _stream(torch, dev, stream_kind)
    for k, (dx, out, res) in enumerate(pads):
        d_lam[1].copy_(d_lams[k:k + 1])                                                 # device to device on the chain's stream
        vi.solve_device(n, d_fixed, d_edges, len(edges), cap, d_H, d_Ho, d_b, d_lam[1], dx[1], out[1], res[1], stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    assert _guards_intact(d_lam[0], -1.5)
    for dx, out, res in pads:
        assert _guards_intact(dx[0], -1.5) and _guards_intact(out[0], -1.5) and _guards_intact(res[0], -6)
    return [(dx[1].cpu().numpy().reshape(n, 15), out[1].cpu().numpy(), res[1].cpu().numpy()) for dx, out, res in pads]


@pytest.mark.parametrize("name", ["pose full", "pose full, lambda 0", "pose inertial", "pose inertial, lambda 0", "a 4-state chain", "two edges on one pair",
                                  "a dropped edge", "refused"])
def test_the_solve_equals_the_ordered_model_bit_for_bit(name):
    import torch
    dev = torch.device("cuda", 0)
    fixed, edges, cap, H, Ho, b, lam, (dx_m, out_m, res_m) = _systems()[name]
    (dx, out, res), = _solve_on_device(torch, dev, fixed, edges, cap, H, Ho, b, [lam])
    print(name, "d_out", out.tolist(), "result", res.tolist())
    assert np.array_equal(res, res_m), (res, res_m)
    _same(name + ": dx", dx, dx_m)
    _same(name + ": out", out, out_m)
    fx = vm.dof_fixed(fixed)
    assert not dx.reshape(-1)[fx].any()
    if name == "refused":
        assert not dx.any() and out[0] == 0 and out[2] == 0
        return
    A, rhs, _, _, _ = vm.assemble(fixed, edges, cap, H, Ho, b, lam)
    x = dx.reshape(-1)
    L = np.longdouble
    resid, bound = float(np.abs(A.astype(L) @ x.astype(L) - rhs.astype(L)).max()), vm.backward_error_bound(A, x)
    print(name, "backward error %.3g, bound %.3g" % (resid, bound))
    assert resid <= bound


def test_lambda_is_read_from_device_memory():
    """two calls with different *d_lambda and no host change in between: a device-side copy rewrites the one double"""
    import torch
    dev = torch.device("cuda", 0)
    fixed, edges, cap, H, Ho, b, lam, _ = _systems()["pose full"]
    lams = [lam, 7.0 * lam]
    runs = _solve_on_device(torch, dev, fixed, edges, cap, H, Ho, b, lams, "null")
    for (dx, out, res), l in zip(runs, lams):
        dx_m, out_m, res_m = vm.solve(fixed, edges, cap, H, Ho, b, l)
        _same("lambda %.3g: dx" % l, dx, dx_m)
        _same("lambda %.3g: out" % l, out, out_m)
        assert np.array_equal(res, res_m)
    assert not np.array_equal(runs[0][0], runs[1][0]) and runs[0][1][1] == runs[1][1][1]


# ---- the chain ------------------------------------------------------------------------------------------------------------------------------------
def _graph_of(st):
    """a model graph holding a device stage's vertices"""
    n = len(st["fixed"])
    g = fm.Graph(n)
    g.Rwb, g.twb, g.v, g.bg, g.ba = (st[k].reshape(n, -1).copy() for k in ("Rwb", "twb", "v", "bg", "ba"))
    g.Rwb = g.Rwb.reshape(n, 3, 3)
    g.fixed, g.iter = st["fixed"].copy(), st["it"].copy()
    return g


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_one_iteration_on_one_stream_with_one_wait(stream_kind):
    """init -> edge information -> inertial linearise -> visual linearise -> solve(lambda) -> oplus -> the errors at the trial point
    (both linearisations in mode 1) -> mode 2 -> recover, all enqueued before the single wait.  Teacher-forced: the model's stage k runs
    from the device's stage k - 1, and no accept / reject decision is taken anywhere.  The edge arrays are what orbba_pose_edges_device
    leaves: floats widened, and their count as a device int behind a zero."""
    import torch
    from monoorbslam3_amd import imu, vi
    dev = torch.device("cuda", 0)
    sc = _scene(400, 0)
    cap_b, ne = len(sc["recs"]), 400
    d = _Dev(torch, dev, sc, n_priors=1, n_pjobs=1)
    d.priors.copy_(_up(torch, dev, sc["priors"]))
    v = _Vis(torch, dev, sc["graph"], sc["cal"], sc["cam"], sc["group_state"], sc["edge_off"], ne, sc["points"], sc["z"], sc["w"])
    v.graph = d.graph                                                                   # the visual edges hang on the graph the chain initialises
    src, init_jobs, pjobs = (_up(torch, dev, sc[k]) for k in ("src", "init_jobs", "pjobs"))
    lam = 4.0e9
    d_lam = _up(torch, dev, np.array([lam]))
    dx, out = _padded(torch, dev, np.full(30, NAN), -1.5), _padded(torch, dev, np.full(3, NAN), -1.5)
    rjobs = np.array([(1, 1, fm.RECOVER_POSE), (0, 0, 0)], np.int32)
    d_dst, d_bias = _padded(torch, dev, sc["src"], np.float32(-2.5)), _padded(torch, dev, np.full(12, -4.0, np.float32), np.float32(-2.5))
    snap, res = {}, {}

    def keep(stage, **tensors):
        snap[stage] = {k: t.clone() for k, t in tensors.items()}                        # device to device on the chain's stream: no wait
        res[stage] = d.result.clone() if stage not in ("visual", "visual 1", "classify") else v.result.clone()

    def vertices():
        return dict(Rwb=d.Rwb, twb=d.twb, v=d.v, bg=d.bg, ba=d.ba, fixed=d.fixed, it=d.it)

    st = _stream(torch, dev, stream_kind)
    imu.graph_init_device(d.graph, d.bank, d.cap, src, 2, init_jobs, 2, d.result, stream=st)
    keep("init", **vertices())
    imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result, stream=st)
    keep("info", info=d.info)
    d.linearize(sc, 0.0, 0, pjobs, 1, 1, st)
    keep("inertial", H_diag=d.H_diag, H_off=d.H_off, b=d.b, total=d.total)
    vi.linearize_device(d.graph, v.cal, v.cam, 1, ne, v.group_state, v.edge_off, v.points, v.z, v.w, v.err, v.chi2, v.result, mode=0, d_total=v.total,
                        d_H_diag=d.H_diag, d_b=d.b, d_work=v.work, stream=st)
    keep("visual", H_diag=d.H_diag, b=d.b, total=v.total, err=v.err, chi2=v.chi2)
    vi.solve_device(2, d.fixed, d.edges, d.ne, d.cap, d.H_diag, d.H_off, d.b, d_lam, dx[1], out[1], d.result, stream=st)
    keep("solve", dx=dx[1], out=out[1])
    imu.graph_oplus_device(d.graph, dx[1], d.it, d.result, stream=st)
    keep("oplus", **vertices())
    d.linearize(sc, 0.0, 1, pjobs, 1, 1, st)
    keep("inertial 1", total=d.total)
    vi.linearize_device(d.graph, v.cal, v.cam, 1, ne, v.group_state, v.edge_off, v.points, v.z, v.w, v.err, v.chi2, v.result, mode=1, d_total=v.total, stream=st)
    keep("visual 1", total=v.total, err=v.err, chi2=v.chi2)
    vi.linearize_device(d.graph, v.cal, v.cam, 1, ne, v.group_state, v.edge_off, v.points, v.z, v.w, v.err, v.chi2, v.result, d_active=v.active, mode=2,
                        d_n_inliers=v.n_inliers, stream=st)
    keep("classify", active=v.active, n_inliers=v.n_inliers)
    imu.graph_recover_device(d.graph, v.cal, _up(torch, dev, rjobs), 2, d_dst[1], 2, d_bias[1], d.result, stream=st)
    keep("recover")
    d.finish()                                                                          # the one wait
    v.finish()
    assert _guards_intact(dx[0], -1.5) and _guards_intact(out[0], -1.5) and _guards_intact(d_dst[0], np.float32(-2.5)) and _guards_intact(d_bias[0], np.float32(-2.5))
    S = {k: {n: t.cpu().numpy() for n, t in s.items()} for k, s in snap.items()}
    R = {k: t.cpu().numpy() for k, t in res.items()}
    # init: widening is exact
    assert R["init"].tolist() == [2, 0, 0, 0, 0, 0, 0, 0] and np.array_equal(S["init"]["Rwb"], sc["graph"].Rwb.reshape(-1)) and np.array_equal(S["init"]["v"], sc["graph"].v.reshape(-1))
    g0 = _graph_of(dict(S["init"], fixed=sc["graph"].fixed))
    # the inertial linearisation (tests/test_factors_gpu.py holds it to the model; here it is the teacher of the next stage)
    oi = vm.inertial_linearize(sc, g0)
    _close("chain: inertial H", S["inertial"]["H_diag"], oi["H_diag"].reshape(-1))
    # the visual linearisation on top of the DEVICE's inertial H and b
    ov = vm.linearize(g0, sc["cal"], sc["cam"], sc["group_state"], sc["edge_off"], ne, sc["points"], sc["z"], sc["w"], None, vm.HUBER_MONO, vm.CHI2_MONO, 0,
                      S["inertial"]["H_diag"], S["inertial"]["b"])
    assert R["visual"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0]
    _same("chain: err", S["visual"]["err"].reshape(ne, 2), ov["err"])
    _same("chain: chi2", S["visual"]["chi2"], ov["chi2"])
    _close("chain: H", S["visual"]["H_diag"].reshape(2, 15, 15)[1, :6, :6], ov["H_diag"][1, :6, :6])
    _close("chain: b", S["visual"]["b"].reshape(2, 15)[1, :6], ov["b"][1, :6])
    _close("chain: total", S["visual"]["total"], ov["total"].reshape(-1))
    keep_mask = np.ones((2, 15, 15), bool)
    keep_mask[1, :6, :6] = False
    assert S["visual"]["H_diag"].reshape(2, 15, 15)[keep_mask].tobytes() == S["inertial"]["H_diag"].reshape(2, 15, 15)[keep_mask].tobytes()
    # the solve on the DEVICE's system: bit for bit
    dx_m, out_m, res_m = vm.solve(sc["graph"].fixed, sc["edges"], cap_b, S["visual"]["H_diag"], S["inertial"]["H_off"], S["visual"]["b"], lam)
    assert np.array_equal(R["solve"], res_m) and res_m[vm.R_DONE] == 1
    _same("chain: dx", S["solve"]["dx"].reshape(2, 15), dx_m)
    _same("chain: out", S["solve"]["out"], out_m)
    # oplus with the DEVICE's dx
    g1 = g0.copy()
    ores = fm.oplus(g1, S["solve"]["dx"])
    assert np.array_equal(R["oplus"], ores) and np.array_equal(S["oplus"]["it"], g1.iter)
    _close("chain: oplus Rwb", S["oplus"]["Rwb"], g1.Rwb.reshape(-1))
    for k in ("twb", "v", "bg", "ba"):
        _close("chain: oplus " + k, S["oplus"][k], getattr(g1, k).reshape(-1))
    assert np.array_equal(S["oplus"]["Rwb"][:9], S["init"]["Rwb"][:9]) and not np.array_equal(S["oplus"]["Rwb"][9:], S["init"]["Rwb"][9:])
    # the errors at the trial point, from the DEVICE's updated vertices: the two scalars a caller reads are the totals and d_out[0]
    g1d = _graph_of(dict(S["oplus"], fixed=sc["graph"].fixed))
    _close("chain: inertial total at the trial", S["inertial 1"]["total"], vm.inertial_linearize(sc, g1d, 1)["total"])
    o1 = vm.linearize(g1d, sc["cal"], sc["cam"], sc["group_state"], sc["edge_off"], ne, sc["points"], sc["z"], sc["w"], None, vm.HUBER_MONO, vm.CHI2_MONO, 1)
    _same("chain: err at the trial", S["visual 1"]["err"].reshape(ne, 2), o1["err"])
    _same("chain: chi2 at the trial", S["visual 1"]["chi2"], o1["chi2"])
    _close("chain: total at the trial", S["visual 1"]["total"], o1["total"].reshape(-1))
    before = S["inertial"]["total"][1] + S["visual"]["total"][1]
    after = S["inertial 1"]["total"][1] + S["visual 1"]["total"][1]
    print("chain: robust total %.6g -> %.6g, scale %.3g" % (before, after, S["solve"]["out"][0]))
    assert after < before
    o2 = vm.linearize(g1d, sc["cal"], sc["cam"], sc["group_state"], sc["edge_off"], ne, sc["points"], sc["z"], sc["w"], None, vm.HUBER_MONO, vm.CHI2_MONO, 2)
    assert np.array_equal(S["classify"]["active"], o2["active"]) and S["classify"]["n_inliers"][0] == o2["n_inliers"][0] and R["classify"].tolist() == o2["result"].tolist()
    # recover from the DEVICE's vertices
    dst = sc["src"].copy()
    bias, _, _, rres = fm.recover(g1d, sc["cal"], rjobs, dst, with_pose=False)
    assert np.array_equal(R["recover"], rres) and rres[0] == 2
    _same_floats("chain: recover dst", d_dst[1].cpu().numpy().reshape(2, 15), dst)
    _same_floats("chain: recover bias", d_bias[1].cpu().numpy().reshape(2, 6), bias)
