"""The visual window of the inertial local bundle adjustment on the MI355X (include/orbvw.h) against tests/vw_model.py.  Every stage is
teacher-forced: it gets uploaded inputs and is compared with the model on those same inputs.  d_point_off and every counter are exact;
every double output within 1e-9 of the model relative to the largest entry of the output's own block, the bar of the f64 BA kernels;
the solve equals the model's ordered Cholesky BIT FOR BIT and, for N <= 60, orbvi_solve_device.  Every output sits between guard
elements.  Model outputs are computed once per scene and shared.  The largest deviation met is printed per output."""
import numpy as np
import pytest

import factors_model as fm
import vi_model as vm
import vw_model as wm
from test_factors_gpu import _Dev, _calib
from test_observations_gpu import _guards_intact, _padded
from test_projection_queries_gpu import _stream, _up
from test_vi_gpu import _camera, _same

pytestmark = pytest.mark.gpu

BAR = 1e-9
NAN = float("nan")
_cache = {}


def _close(what, got, want, block=None):
    """within BAR of the model relative to the largest entry of the block (the trailing `block` axes; None: the whole array)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    if not got.size:
        return
    ax = tuple(range(got.ndim - (got.ndim if block is None else block), got.ndim))
    scale = np.abs(want).max(ax, keepdims=True)
    diff = np.abs(got - want)
    assert not diff[np.broadcast_to(scale == 0, diff.shape)].any(), what
    rel = float((diff / np.where(scale > 0, scale, 1.0)).max())
    print("%-44s largest deviation %.3g of the block's largest entry" % (what, rel))
    assert rel <= BAR, (what, rel)


def _scene(n_solve, n_fixed, n_points, model=0):
    key = ("scene", n_solve, n_fixed, n_points, model)
    if key not in _cache:
        sc = wm.window_scene(n_solve, n_fixed, n_points, 1, model)
        rng = np.random.RandomState(90 + n_points)
        H0 = rng.normal(0, 10.0, (sc["graph"].n, 15, 15))
        sc["H0"], sc["b0"] = H0 + H0.transpose(0, 2, 1), rng.normal(0, 10.0, (sc["graph"].n, 15))
        _cache[key] = sc
    return _cache[key]


class _Win:
    """the device memory of a window: the graph, the points, the edges and every output of the four calls, padded"""

    def __init__(self, torch, dev, sc, g=None, **over):
        from monoorbslam3_amd import imu
        self.torch, self.dev, self.pads = torch, dev, {}
        g = sc["graph"] if g is None else g
        a = {k: over.get(k, sc[k]) for k in ("points", "edge_state", "edge_point", "z", "w")}
        self.n, self.ns, self.np_, self.ne = g.n, sc["n_solve"], len(a["points"]), len(a["edge_state"])
        e1, N = max(self.ne, 1), 15 * self.ns
        self.graph_t = [_up(torch, dev, x) for x in (g.Rwb.reshape(-1), g.twb.reshape(-1), g.v.reshape(-1), g.bg.reshape(-1), g.ba.reshape(-1), g.fixed)]
        self.fixed = self.graph_t[5]
        self.graph = imu.Graph.make(*self.graph_t, g.n)
        self.cal, self.cam = _calib(sc["cal"]), _camera(sc["cam"])
        room = lambda x, k, t: np.concatenate([np.asarray(x, t).reshape(-1), np.zeros(k, t)])[:max(k * self.ne, k)]  # noqa: E731
        self.points = self._pad("points", np.asarray(a["points"], np.float64).reshape(-1), -1.5)
        self.edge_state, self.edge_point = _up(torch, dev, room(a["edge_state"], 1, np.int32)), _up(torch, dev, room(a["edge_point"], 1, np.int32))
        self.z, self.w = _up(torch, dev, room(a["z"], 2, np.float64)), _up(torch, dev, room(a["w"], 1, np.float64))
        act = over.get("active")
        self.active = None if act is None else _up(torch, dev, np.asarray(act, np.uint8))
        f64 = lambda k, n: self._pad(k, np.full(n, NAN), -1.5)  # noqa: E731
        self.point_off = self._pad("point_off", np.full(self.np_ + 1, -77, np.int32), -3)
        self.err, self.chi2, self.total, self.work = f64("err", 2 * e1), f64("chi2", e1), f64("total", 2), f64("work", wm.EDGE_WORK * e1)
        self.H_diag = self._pad("H_diag", over["H0"].reshape(-1) if "H0" in over else np.full(225 * g.n, NAN), -1.5)
        self.b = self._pad("b", over["b0"].reshape(-1) if "b0" in over else np.full(15 * g.n, NAN), -1.5)
        self.Hll, self.bl, self.Hlp = f64("Hll", 9 * self.np_), f64("bl", 3 * self.np_), f64("Hlp", 18 * e1)
        self.outlier = self._pad("outlier", np.full(e1, 0xEE, np.uint8), 0xA5)
        self.result = self._pad("result", np.full(8, 77, np.int32), -6)
        self.S, self.rhs, self.Hll_inv, self.tl, self.out = f64("S", N * N), f64("rhs", N), f64("Hll_inv", 9 * self.np_), f64("tl", 3 * self.np_), f64("out", 3)
        self.dx = self._pad("dx", np.zeros(15 * g.n), -1.5)
        self.xl, self.points_out, self.out_points = f64("xl", 3 * self.np_), f64("points_out", 3 * self.np_), f64("out_points", 1)
        self.lam = self._pad("lam", np.full(1, NAN), -1.5)
        self.H_off = _up(torch, dev, np.zeros(225 * max(len(sc["edges"]), 1)))
        self.edges = _up(torch, dev, sc["edges"] if len(sc["edges"]) else np.zeros(1, fm.EDGE))
        self.n_iedges, self.cap = len(sc["edges"]), len(sc["recs"])

    def _pad(self, key, a, fill):
        self.pads[key] = (_padded(self.torch, self.dev, a, fill), fill)
        return self.pads[key][0][1]

    def put(self, **arrays):
        for k, a in arrays.items():
            t = getattr(self, k)
            t.copy_(self.torch.from_numpy(np.ascontiguousarray(a).reshape(-1).astype(t.cpu().numpy().dtype)).to(self.dev))

    def linearize(self, mode, null=False, points=None, H_diag=None, b=None, stream=None):
        from monoorbslam3_amd import vw
        z = mode != 0 or null
        vw.linearize_device(self.graph, self.cal, self.cam, self.ns, self.np_, self.ne, self.points if points is None else points, self.edge_state,
                            self.edge_point, self.z, self.w, self.point_off, self.err, self.chi2, self.result, self.active, mode=mode,
                            d_total=None if mode == 2 else self.total, d_work=None if z else self.work, d_H_diag=None if z else (self.H_diag if H_diag is None else H_diag),
                            d_b=None if z else (self.b if b is None else b), d_Hll=None if z else self.Hll, d_bl=None if z else self.bl,
                            d_Hlp=None if z else self.Hlp, d_outlier=self.outlier if mode == 2 else None, stream=stream)

    def reduce(self, fixed=None, H_diag=None, H_off=None, b=None, stream=None):
        from monoorbslam3_amd import vw
        vw.reduce_device(self.ns, self.fixed if fixed is None else fixed, self.edges, self.n_iedges, self.cap, self.H_diag if H_diag is None else H_diag,
                         self.H_off if H_off is None else H_off, self.b if b is None else b, self.lam, self.np_, self.ne, self.point_off, self.edge_state, self.Hll, self.bl,
                         self.Hlp, self.S, self.rhs, self.Hll_inv, self.tl, self.out, self.result, stream=stream)

    def solve(self, b=None, stream=None):
        from monoorbslam3_amd import vw
        vw.solve_device(self.ns, self.S, self.rhs, self.b if b is None else b, self.lam, self.dx, self.out, self.result, stream=stream)

    def backsub(self, stream=None):
        from monoorbslam3_amd import vw
        vw.backsub_device(self.ns, self.np_, self.ne, self.point_off, self.edge_state, self.Hlp, self.Hll_inv, self.bl, self.dx, self.lam, self.points, self.xl,
                          self.points_out, self.out_points, self.result, stream=stream)

    def get(self, key, shape=None):
        a = getattr(self, key).cpu().numpy().copy()
        return a if shape is None else a.reshape(shape)

    def finish(self):
        self.torch.cuda.synchronize()
        self.torch.cuda.set_stream(self.torch.cuda.default_stream(self.dev))
        for key, ((whole, _), fill) in self.pads.items():
            assert _guards_intact(whole, fill), key


def _model_lin(sc, mode, g=None, **over):
    a = {k: over.get(k, sc[k]) for k in ("points", "edge_state", "edge_point", "z", "w")}
    return wm.linearize(sc["graph"] if g is None else g, sc["cal"], sc["cam"], sc["n_solve"], a["points"], a["edge_state"], a["edge_point"], a["z"], a["w"],
                        over.get("active"), mode=mode, H_diag=over.get("H0"), b=over.get("b0"))


def _assert_lin(what, d, o, mode, sc, g=None, H0=None, b0=None):
    g = sc["graph"] if g is None else g
    ne, npt = d.ne, d.np_
    assert np.array_equal(d.get("point_off"), o["point_off"]), what
    assert np.array_equal(d.get("result"), o["result"]), (what, d.get("result"), o["result"])
    err, chi2 = d.get("err")[:2 * ne].reshape(ne, 2), d.get("chi2")[:ne]
    fin = np.isfinite(o["chi2"]) & np.isfinite(o["err"]).all(1)
    assert np.array_equal(np.isfinite(chi2) & np.isfinite(err).all(1), fin), what
    _close(what + ": err", err[fin], o["err"][fin])
    _close(what + ": chi2", chi2[fin], o["chi2"][fin])
    print(what, "err equal bit for bit:", err[fin].tobytes() == o["err"][fin].tobytes())
    if mode == 2:
        assert np.array_equal(d.get("outlier")[:ne], o["outlier"]), what
        return
    _close(what + ": total", d.get("total"), o["total"])
    if mode == 1:
        return
    _close(what + ": Hlp", d.get("Hlp")[:18 * ne].reshape(ne, 18), o["Hlp"], 1)
    _close(what + ": Hll", d.get("Hll", (npt, 9)), o["Hll"], 1)
    _close(what + ": bl", d.get("bl", (npt, 3)), o["bl"], 1)
    H, b = d.get("H_diag", (g.n, 15, 15)), d.get("b", (g.n, 15))
    keep = np.ones((g.n, 15, 15), bool)
    for s in range(sc["n_solve"]):
        if int(g.fixed[s]) & fm.FIX_POSE:
            continue
        keep[s, :6, :6] = False
        _close(what + ": H", H[s, :6, :6], o["H_diag"][s, :6, :6])
        _close(what + ": b", b[s, :6], o["b"][s, :6])
        assert np.array_equal(H[s, :6, :6], H[s, :6, :6].T), what
    assert H[keep].tobytes() == H0[keep].tobytes() and b[keep[:, 0, :]].tobytes() == b0[keep[:, 0, :]].tobytes(), what   # everything else keeps its bytes


# ---- linearise --------------------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 0, 1, 0), (2, 1, 63, 0), (5, 3, 65, 0), (3, 2, 1025, 0), (2, 1, 65, 1)]


@pytest.mark.parametrize("n_solve,n_fixed,n_points,model", SHAPES)
def test_linearise_equals_the_model(n_solve, n_fixed, n_points, model):
    """mode 0 on top of a non-zero d_H_diag and d_b: one point, fewer and more than a wave and a workgroup of points and edges"""
    import torch
    sc = _scene(n_solve, n_fixed, n_points, model)
    key = ("lin0", n_solve, n_fixed, n_points, model)
    if key not in _cache:
        _cache[key] = _model_lin(sc, 0, H0=sc["H0"], b0=sc["b0"])
    d = _Win(torch, torch.device("cuda", 0), sc, H0=sc["H0"], b0=sc["b0"])
    d.linearize(0)
    d.finish()
    _assert_lin("%d+%d states, %d points, model %d" % (n_solve, n_fixed, n_points, model), d, _cache[key], 0, sc, H0=sc["H0"], b0=sc["b0"])
    assert not np.array_equal(d.get("H_diag", (-1, 15, 15))[0, :6, :6], sc["H0"][0, :6, :6])


def test_modes_1_and_2_with_null_optionals_and_an_inactive_mask():
    import torch
    dev = torch.device("cuda", 0)
    sc = _scene(2, 1, 63)
    ne = len(sc["w"])
    o2 = _model_lin(sc, 2)
    assert 0 < o2["result"][wm.R_OUTLIER] < ne
    for mode, o in ((1, _model_lin(sc, 1)), (2, o2)):
        d = _Win(torch, dev, sc, H0=sc["H0"], b0=sc["b0"])
        d.linearize(mode, stream=_stream(torch, dev, "explicit"))
        d.finish()
        _assert_lin("mode %d" % mode, d, o, mode, sc)
        assert d.get("H_diag").tobytes() == sc["H0"].tobytes() and d.get("b").tobytes() == sc["b0"].tobytes()
        assert np.isnan(d.get("work")).all() and np.isnan(d.get("Hll")).all() and np.isnan(d.get("Hlp")).all()
        assert np.isnan(d.get("total")).all() == (mode == 2)
    active = (np.random.RandomState(8).uniform(size=ne) < 0.6).astype(np.uint8)
    for act in (active, np.zeros(ne, np.uint8)):
        o = _model_lin(sc, 0, active=act, H0=sc["H0"], b0=sc["b0"])
        d = _Win(torch, dev, sc, active=act, H0=sc["H0"], b0=sc["b0"])
        d.linearize(0)
        d.finish()
        _assert_lin("a mask with %d active" % act.sum(), d, o, 0, sc, H0=sc["H0"], b0=sc["b0"])
        assert not o["Hlp"][act == 0].any() and np.array_equal(d.active.cpu().numpy(), act)


def _on_the_camera_plane(sc):
    """point 0 (one observation) moved to (0, 0, z) with fl(r22 * z) == -t2: the products with the zeros add nothing, so Z is exactly 0"""
    s = int(sc["edge_state"][0])
    assert sc["edge_point"][0] == 0 and sc["edge_point"][1] == 1
    Rcw, tcw, _, _ = vm.derive_pose(sc["cal"], sc["graph"].Rwb[s], sc["graph"].twb[s])
    cands = [-tcw[2] / Rcw[2, 2]]
    for k in range(16):
        cands += [np.nextafter(cands[-2 if k else -1], np.inf)] if k % 2 == 0 else [np.nextafter(min(cands), -np.inf)]
    hit = [c for c in cands if Rcw[2, 2] * c == -tcw[2]]
    assert hit, "no z within a few ulps puts the point on the camera plane exactly"
    P = sc["points"].copy()
    P[0] = [0.0, 0.0, hit[0]]
    return P


def test_an_edge_on_the_camera_plane_is_counted_and_adds_nothing():
    import torch
    sc = _scene(2, 1, 63)
    P = _on_the_camera_plane(sc)
    o = _model_lin(sc, 0, points=P, H0=sc["H0"], b0=sc["b0"])
    assert o["result"][vm.R_NONFINITE] == 1 and not np.isfinite(o["chi2"][0]) and not o["Hll"][0].any() and np.isfinite(o["H_diag"]).all()
    d = _Win(torch, torch.device("cuda", 0), sc, points=P, H0=sc["H0"], b0=sc["b0"])
    d.linearize(0)
    d.finish()
    _assert_lin("Z = 0", d, o, 0, sc, H0=sc["H0"], b0=sc["b0"])
    assert not np.isfinite(d.get("chi2")[0])


def _distrusted(what):
    sc = _scene(2, 1, 63)
    es, ep, z, w = (sc[k].copy() for k in ("edge_state", "edge_point", "z", "w"))
    if what == "unsorted":
        ep[[10, 40]] = ep[[40, 10]]
        ep[5], ep[-1] = -7, 1 << 30
    elif what == "range":
        es[[3, 50]] = [3, -1]
        es[51] = -1
    elif what == "duplicate":
        k = int(np.nonzero(ep[1:] == ep[:-1])[0][0])
        es[k + 1] = es[k]
    else:
        extra = 257 - int((ep == 62).sum())
        es = np.concatenate([es, np.arange(extra, dtype=np.int32) % 3])
        ep = np.concatenate([ep, np.full(extra, 62, np.int32)])
        z, w = np.concatenate([z, np.tile(z[-1:], (extra, 1))]), np.concatenate([w, np.tile(w[-1:], extra)])
    return sc, dict(edge_state=es, edge_point=ep, z=z, w=w)


@pytest.mark.parametrize("what,slot", [("unsorted", None), ("range", wm.R_RANGE), ("duplicate", wm.R_DUPLICATE), ("257 edges", wm.R_REFUSED)])
def test_distrusted_edge_lists(what, slot):
    """an unsorted d_edge_point with entries outside its range, states out of range, a state named twice by one point, a point with
    257 edges: the ranges, the counters and every output are the model's, in modes 0 and 2"""
    import torch
    sc, over = _distrusted(what)
    o = _model_lin(sc, 0, H0=sc["H0"], b0=sc["b0"], **over)
    ne = len(over["w"])
    assert o["result"][wm.R_DONE] + o["result"][wm.R_RANGE] + o["result"][wm.R_DUPLICATE] + (257 if what == "257 edges" else 0) == ne
    if slot is not None:
        assert o["result"][slot] == {"range": 3, "duplicate": 1, "257 edges": 1}[what], o["result"]
        assert not o["Hlp"][o["status"] != 0].any() and not o["err"][o["status"] != 0].any()
    else:
        assert not np.array_equal(o["point_off"], wm.point_ranges(sc["edge_point"], 63)[0]) and (np.diff(o["point_off"]) >= 0).all()
    if what == "257 edges":
        assert not o["Hll"][62].any() and (np.diff(o["point_off"]) == 257).sum() == 1
    dev = torch.device("cuda", 0)
    d = _Win(torch, dev, sc, H0=sc["H0"], b0=sc["b0"], **over)
    d.linearize(0)
    d.finish()
    _assert_lin(what, d, o, 0, sc, H0=sc["H0"], b0=sc["b0"])
    d2 = _Win(torch, dev, sc, **over)
    d2.linearize(2)
    d2.finish()
    _assert_lin(what + ", mode 2", d2, _model_lin(sc, 2, **over), 2, sc)


# ---- reduce -------------------------------------------------------------------------------------------------------------------------------------
def _linear(sc, fixed=None):
    """the model's two linearisations of a scene, with other fixed masks on demand: the teacher of reduce"""
    key = ("linear", id(sc), None if fixed is None else tuple(fixed))
    if key not in _cache:
        g = sc["graph"].copy()
        if fixed is not None:
            g.fixed[:len(fixed)] = fixed
        oi = vm.inertial_linearize(sc, g)
        _cache[key] = (g, oi, wm.linearize(g, sc["cal"], sc["cam"], sc["n_solve"], sc["points"], sc["edge_state"], sc["edge_point"], sc["z"], sc["w"], mode=0,
                                           H_diag=oi["H_diag"], b=oi["b"]))
    return _cache[key]


def _model_reduce(sc, g, oi, ov, lam):
    return wm.reduce(sc["n_solve"], g.fixed, sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], lam, ov["point_off"], sc["edge_state"], ov["Hll"],
                     ov["bl"], ov["Hlp"], len(sc["w"]))


def _upload_linear(d, oi, ov, lam):
    d.put(H_diag=ov["H_diag"], b=ov["b"], Hll=ov["Hll"], bl=ov["bl"], Hlp=ov["Hlp"], point_off=ov["point_off"], lam=np.array([lam]))
    if d.n_iedges:
        d.put(H_off=oi["H_off"])


@pytest.mark.parametrize("shape,fixed,lam", [((1, 0, 1), None, 1.0), ((2, 1, 63), None, 1.0), ((5, 3, 65), [fm.FIX_GYRO, fm.FIX_POSE, 0, fm.FIX_VELO | fm.FIX_ACC, 0], 3.5),
                                             ((3, 2, 1025), None, 1e3), ((2, 1, 63), [0, 15], 0.0)])
def test_reduce_equals_the_model(shape, fixed, lam):
    """the base, the points' inverses and the Schur complement on the model's linearisation; fixed masks; at lambda 0 the point with one
    observation is singular and skipped"""
    import torch
    sc = _scene(*shape)
    g, oi, ov = _linear(sc, fixed)
    r = _model_reduce(sc, g, oi, ov, lam)
    single = np.bincount(sc["edge_point"], minlength=sc["n_points"]) == 1
    # a point with one observation has a determinant of 0 up to rounding: skipped are those whose rounding leaves it <= 0
    assert r["result"][wm.R_POINT_SINGULAR] == r["skipped"].sum() and (r["skipped"].any() and single[r["skipped"]].all() if not lam else not r["skipped"].any())
    d = _Win(torch, torch.device("cuda", 0), sc, g)
    _upload_linear(d, oi, ov, lam)
    d.reduce()
    d.finish()
    N, what = 15 * sc["n_solve"], "reduce %s lambda %g" % (shape, lam)
    assert np.array_equal(d.get("result"), r["result"]), (d.get("result"), r["result"])
    blocks = lambda A: A.reshape(N // 15, 15, N // 15, 15).transpose(0, 2, 1, 3)  # noqa: E731
    _close(what + ": S", blocks(d.get("S", (N, N))), blocks(r["S"]), 2)
    _close(what + ": rhs", d.get("rhs", (N // 15, 15)), r["rhs"].reshape(-1, 15), 1)
    _close(what + ": Hll_inv", d.get("Hll_inv", (-1, 9)), r["Hll_inv"], 1)
    _close(what + ": tl", d.get("tl", (-1, 3)), r["tl"], 1)
    out = d.get("out")
    assert out[1] == r["h_max"] and np.isnan(out[0]) and np.isnan(out[2])
    S = d.get("S", (N, N))
    fx = vm.dof_fixed(g.fixed[:sc["n_solve"]])
    assert np.array_equal(S[fx][:, fx], np.eye(int(fx.sum()))) and not S[fx][:, ~fx].any() and not d.get("rhs")[fx].any()
    if not lam:
        assert not d.get("Hll_inv", (-1, 9))[r["skipped"]].any()


# ---- solve ----------------------------------------------------------------------------------------------------------------------------------------
def _systems():
    """name -> (S, rhs, b, lambda): the model's reduced systems of three scenes (N = 15, 60, 75) and a synthetic SPD system of N = 480"""
    if "systems" not in _cache:
        out = {}
        for shape in ((1, 0, 1), (4, 1, 20), (5, 3, 65)):
            sc = _scene(*shape)
            g, oi, ov = _linear(sc)
            r = _model_reduce(sc, g, oi, ov, 1.0)
            out[15 * shape[0]] = (r["S"], r["rhs"], ov["b"][:shape[0]].reshape(-1), 1.0)
        rng = np.random.RandomState(480)
        M = rng.normal(0, 1.0, (480, 480))
        out[480] = (M @ M.T + 480.0 * np.eye(480), rng.normal(0, 1.0, 480), rng.normal(0, 1.0, 480), 0.25)
        _cache["systems"] = {k: v + (wm.solve(*v),) for k, v in out.items()}
    return _cache["systems"]


def _solve_on_device(torch, dev, S, rhs, b, lams, stream_kind="explicit"):
    """one orbvw_solve_device per lambda, each read from the SAME device double, which a device-side copy changes in between"""
    from monoorbslam3_amd import vw
    n = len(rhs) // 15
    d_rhs, d_b, d_lams = _up(torch, dev, rhs), _up(torch, dev, b), _up(torch, dev, np.asarray(lams, np.float64))
    d_lam = _padded(torch, dev, np.full(1, NAN), -1.5)
    pads = [(_padded(torch, dev, S.reshape(-1), -1.5), _padded(torch, dev, np.full(15 * n, NAN), -1.5), _padded(torch, dev, np.full(3, NAN), -1.5),
             _padded(torch, dev, np.full(8, 77, np.int32), -6)) for _ in lams]
    st = _stream(torch, dev, stream_kind)
    for k, (dS, dx, out, res) in enumerate(pads):
        d_lam[1].copy_(d_lams[k:k + 1])
        vw.solve_device(n, dS[1], d_rhs, d_b, d_lam[1], dx[1], out[1], res[1], stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for dS, dx, out, res in pads:
        assert _guards_intact(dS[0], -1.5) and _guards_intact(dx[0], -1.5) and _guards_intact(out[0], -1.5) and _guards_intact(res[0], -6)
    return [(dx[1].cpu().numpy().reshape(n, 15), out[1].cpu().numpy(), res[1].cpu().numpy()) for _, dx, out, res in pads]


@pytest.mark.parametrize("N", [15, 60, 75, 480])
def test_the_solve_equals_the_ordered_model_bit_for_bit(N):
    import torch
    dev = torch.device("cuda", 0)
    S, rhs, b, lam, (dx_m, (scale_m, pivot_m), res_m) = _systems()[N]
    (dx, out, res), = _solve_on_device(torch, dev, S, rhs, b, [lam])
    print("N", N, "d_out", out.tolist(), "result", res.tolist())
    assert np.array_equal(res, res_m) and res[wm.R_DONE] == 1
    _same("N %d: dx" % N, dx, dx_m)
    _same("N %d: out" % N, out[[0, 2]], np.array([scale_m, pivot_m]))
    assert np.isnan(out[1])
    x, L = dx.reshape(-1), np.longdouble
    A = np.tril(S) + np.tril(S, -1).T                                                   # the lower triangle is the system
    resid, bound = float(np.abs(A.astype(L) @ x.astype(L) - rhs.astype(L)).max()), vm.backward_error_bound(A, x)
    print("N %d: backward error %.3g, bound %.3g" % (N, resid, bound))
    assert resid <= bound
    if N > 60:
        return
    # the same system through orbvi_solve_device: the diagonal blocks as d_H_diag, every pair's block as an edge's d_H_off, lambda 0
    from monoorbslam3_amd import vi
    n = N // 15
    pairs = [(i, j) for i in range(n) for j in range(i + 1, n)]
    edges = np.array([(i, j, 0, 0) for i, j in pairs], fm.EDGE) if pairs else np.zeros(1, fm.EDGE)
    B = S.reshape(n, 15, n, 15)
    H_off = np.stack([B[i, :, j, :] for i, j in pairs]) if pairs else np.zeros((1, 15, 15))
    assert all(np.array_equal(B[i, :, j, :], B[j, :, i, :].T) for i, j in pairs)
    t = [_up(torch, dev, a) for a in (np.zeros(n, np.uint8), edges, np.stack([B[i, :, i, :] for i in range(n)]).reshape(-1), H_off.reshape(-1), rhs, np.zeros(1))]
    dx_v, out_v, res_v = _up(torch, dev, np.full(N, NAN)), _up(torch, dev, np.full(3, NAN)), _up(torch, dev, np.full(8, 77, np.int32))
    vi.solve_device(n, t[0], t[1], len(pairs), 1, t[2], t[3], t[4], t[5], dx_v, out_v, res_v)
    (dx0, out0, _), = _solve_on_device(torch, dev, S, rhs, rhs, [0.0], "null")
    torch.cuda.synchronize()
    assert res_v.cpu().numpy()[wm.R_DONE] == 1
    _same("N %d: dx against orbvi_solve_device" % N, dx0.reshape(-1), dx_v.cpu().numpy())
    _same("N %d: out against orbvi_solve_device" % N, out0[[0, 2]], out_v.cpu().numpy()[[0, 2]])
    _same("N %d: dx" % N, dx0, dx_m)


def test_a_refused_pivot_and_lambda_from_device_memory():
    import torch
    dev = torch.device("cuda", 0)
    S, rhs, b, lam, _ = _systems()[75]
    bad = S.copy()
    bad[40, 40] = -1.0
    dx_m, (scale_m, pivot_m), res_m = wm.solve(bad, rhs, b, lam)
    assert res_m[wm.R_REFUSED] == 1 and not res_m[wm.R_DONE] and pivot_m < 0
    (dx, out, res), = _solve_on_device(torch, dev, bad, rhs, b, [lam])
    assert np.array_equal(res, res_m) and not dx.any() and out[0] == 0.0 and out[2] == pivot_m
    lams = [lam, 7.0 * lam]
    runs = _solve_on_device(torch, dev, S, rhs, b, lams, "null")
    for (dx, out, res), l in zip(runs, lams):
        dx_m, (scale_m, pivot_m), res_m = wm.solve(S, rhs, b, l)
        _same("lambda %g: dx" % l, dx, dx_m)
        _same("lambda %g: out" % l, out[[0, 2]], np.array([scale_m, pivot_m]))
    assert runs[0][1][0] != runs[1][1][0] and np.array_equal(runs[0][0], runs[1][0])


# ---- back-substitution ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,lam", [((1, 0, 1), 1.0), ((5, 3, 65), 1.0), ((3, 2, 1025), 1.0), ((2, 1, 63), 0.0)])
def test_backsub_equals_the_model_and_leaves_the_points_alone(shape, lam):
    import torch
    sc = _scene(*shape)
    g, oi, ov = _linear(sc)
    r = _model_reduce(sc, g, oi, ov, lam)
    ns = sc["n_solve"]
    dx = wm.solve(r["S"], r["rhs"], ov["b"][:ns], lam)[0] if lam else np.random.RandomState(5).normal(0, 1e-3, (ns, 15))
    m = wm.backsub(ns, ov["point_off"], sc["edge_state"], ov["Hlp"], r["Hll_inv"], ov["bl"], dx, lam, sc["points"], len(sc["w"]))
    d = _Win(torch, torch.device("cuda", 0), sc, g)
    full = np.zeros((g.n, 15))
    full[:ns] = dx
    d.put(Hlp=ov["Hlp"], Hll_inv=r["Hll_inv"], bl=ov["bl"], point_off=ov["point_off"], lam=np.array([lam]), dx=full)
    d.backsub()
    d.finish()
    what = "backsub %s" % (shape,)
    assert np.array_equal(d.get("result"), m["result"]), (d.get("result"), m["result"])
    _close(what + ": xl", d.get("xl", (-1, 3)), m["xl"], 1)
    _close(what + ": points_out", d.get("points_out", (-1, 3)), m["points_out"], 1)
    _close(what + ": scale", d.get("out_points"), np.array([m["scale"]]))
    assert d.get("points").tobytes() == sc["points"].tobytes()
    if not lam:
        sk = r["skipped"]
        assert sk.any() and d.get("points_out", (-1, 3))[sk].tobytes() == sc["points"][sk].tobytes() and not d.get("xl", (-1, 3))[sk].any()
    else:
        assert m["xl"].any()


# ---- determinism and the chain -----------------------------------------------------------------------------------------------------------------
OUTPUTS = ("point_off", "err", "chi2", "total", "H_diag", "b", "Hll", "bl", "Hlp", "S", "rhs", "Hll_inv", "tl", "out", "dx", "xl", "points_out", "out_points")


def test_two_runs_of_the_1025_point_window_give_the_same_bytes():
    import torch
    sc = _scene(3, 2, 1025)
    g, oi, ov = _linear(sc)
    runs = []
    for _ in range(2):
        d = _Win(torch, torch.device("cuda", 0), sc, H0=oi["H_diag"], b0=oi["b"])
        d.put(H_off=oi["H_off"], lam=np.array([1.0]))
        d.linearize(0), d.reduce(), d.solve(), d.backsub()
        d.finish()
        runs.append({k: d.get(k).tobytes() for k in OUTPUTS + ("result",)})
        assert d.get("result").tolist() == [1025, 0, 0, 0, 0, 0, 0, 0] and np.isfinite(d.get("dx")).all() and d.get("dx").any()
    assert runs[0] == runs[1]


def _chain(torch, dev, sc, stream_kind, staged):
    """one whole iteration: graph init -> edge information -> orbi_linearize_device -> orbvw_linearize_device -> reduce -> solve -> backsub ->
    orbi_graph_oplus_device -> both linearisations in mode 1 on d_points_out.  Staged: a wait behind every call; otherwise one wait."""
    from monoorbslam3_amd import imu
    g = sc["graph"]
    i = _Dev(torch, dev, sc, g, n_priors=1, n_pjobs=1)
    i.priors.copy_(_up(torch, dev, sc["priors"]))
    w = _Win(torch, dev, sc)
    w.graph, w.fixed = i.graph, i.fixed
    w.put(lam=np.array([1.0]))
    src, init_jobs, pjobs = (_up(torch, dev, sc[k]) for k in ("src", "init_jobs", "pjobs"))
    st = _stream(torch, dev, stream_kind)
    snap = {}

    def step(name, call, **keep):
        call()
        if staged:
            torch.cuda.synchronize()
        snap[name] = {k: t.clone() for k, t in keep.items()}                            # device to device on the chain's stream: no wait

    ns = sc["n_solve"]
    step("init", lambda: imu.graph_init_device(i.graph, i.bank, i.cap, src, len(sc["src"]), init_jobs, ns, i.result, stream=st), Rwb=i.Rwb, res=i.result)
    step("info", lambda: imu.edge_information_device(i.bank, i.cap, i.edges, i.ne, i.info, i.walk, i.result, stream=st), info=i.info)
    step("inertial", lambda: i.linearize(sc, 0.0, 0, pjobs, 1, 1, st), H_diag=i.H_diag, H_off=i.H_off, b=i.b, total=i.total)
    step("visual", lambda: w.linearize(0, H_diag=i.H_diag, b=i.b, stream=st), H_diag=i.H_diag, b=i.b, total=w.total, Hll=w.Hll, bl=w.bl, Hlp=w.Hlp, res=w.result)
    step("reduce", lambda: w.reduce(H_diag=i.H_diag, H_off=i.H_off, b=i.b, stream=st), S=w.S, rhs=w.rhs, Hll_inv=w.Hll_inv, out=w.out, res=w.result)
    step("solve", lambda: w.solve(b=i.b, stream=st), dx=w.dx, out=w.out, res=w.result)
    step("backsub", lambda: w.backsub(stream=st), xl=w.xl, points_out=w.points_out, out_points=w.out_points, res=w.result)
    step("oplus", lambda: imu.graph_oplus_device(i.graph, w.dx, i.it, i.result, stream=st), Rwb=i.Rwb, twb=i.twb, v=i.v, bg=i.bg, ba=i.ba)
    step("inertial 1", lambda: i.linearize(sc, 0.0, 1, pjobs, 1, 1, st), total=i.total)
    step("visual 1", lambda: w.linearize(1, points=w.points_out, stream=st), total=w.total, chi2=w.chi2, res=w.result)
    i.finish()                                                                          # the one wait
    w.finish()
    return {k: {n: t.cpu().numpy() for n, t in s.items()} for k, s in snap.items()}


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_one_iteration_on_one_stream_with_one_wait(stream_kind):
    """the chain of include/orbvw.h enqueued before a single wait gives the bytes of the same calls with a wait behind each; the solve is
    not refused, the points move, and the robustified total at the trial point is lower"""
    import torch
    dev = torch.device("cuda", 0)
    sc = _scene(2, 1, 63)
    if "staged" not in _cache:
        _cache["staged"] = _chain(torch, dev, sc, "explicit", True)
    staged, once = _cache["staged"], _chain(torch, dev, sc, stream_kind, False)
    for stage, outs in staged.items():
        for k, a in outs.items():
            assert once[stage][k].tobytes() == a.tobytes(), (stage, k)
    assert once["init"]["res"][0] == 2 and once["solve"]["res"].tolist() == [1, 0, 0, 0, 0, 0, 0, 0] and once["backsub"]["res"][0] == 63
    assert once["visual"]["res"][0] == len(sc["w"]) and once["visual 1"]["res"][0] == len(sc["w"])
    before = once["inertial"]["total"][1] + once["visual"]["total"][1]
    after = once["inertial 1"]["total"][1] + once["visual 1"]["total"][1]
    it = sc["first"]
    print("chain: robust total %.6g -> %.6g (model %.6g -> %.6g), scale %.6g + %.6g" % (before, after, it["before"], it["after"], once["solve"]["out"][0],
                                                                                   once["backsub"]["out_points"][0]))
    assert after < before and once["backsub"]["xl"].any()
    _close("chain: total before", np.array([before]), np.array([it["before"]]))
