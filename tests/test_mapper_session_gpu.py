"""A whole mapper session on the MI355X: key frame K + 1 runs on what key frame K's step left in device memory, every call through the
wrappers of monoorbslam3_amd.matcher / .ba on one stream, and after every key frame the device holds, byte for byte, what
tests/mapper_session.py's composition of the array models holds (the refreshed normals by value, as the per-call tests compare them).

tests/mapper_session.py's step() is written once over a backend, so the device and the models cannot be composed differently; _Device
below is the device's backend.  The read-backs inside a step are the two INTEGRATION.md names: the fuse targets and the BA problem's 32
bytes; the step's one wait is at its end, where Map::eraseKeyFrame is replayed from d_code.

Two float answers of the model session come from the library's host entry points, not from numpy: the local BA's estimate
(orbba_local_bundle_adjustment on the model's problem, which tests/test_local_ba_gpu.py holds bit-equal to the device form, and which is
compared here with oracle/ba_ref.py's at tests/test_ba.py's tolerance at every key frame) and the triangulated rows' floats
(orbm_triangulate_matches, which tests/test_triangulation_gpu.py holds byte-equal to the device form and, inside its stated band, to
the float64 model -- that comparison is repeated here on every pair): the device's triangulation solver is not LAPACK's, so no numpy
restatement has its bits, and a session needs the bits, because every later call reads them."""
import time

import numpy as np
import pytest

import graph_model as gm
import local_ba_model as lbm
import mapper_session as ms
import projection_model as pm
import refresh_model as rm
import triangulation_model as tm
from test_ba import LM_TOL, _close   # the LM tolerance is test_ba.py's, not a copy
from test_keyframe_gpu import _fill
from test_local_ba_gpu import OUT_TYPES, WIDTH, _host_ba
from test_observations_gpu import GUARD, _guards_intact, _padded  # noqa: F401
from test_triangulation_gpu import _exclusions, _stream, _up

pytestmark = pytest.mark.gpu

BY_VALUE = ("normals",)                # -0 equals +0, as tests/test_local_ba_gpu.py and tests/test_fuse_gpu.py compare the refresh
_models = {}


# ---- the model session beside the device ---------------------------------------------------------------------------------------------------
def _ba_host(checks):
    def solve(cam, prob):
        from monoorbslam3_amd import ba
        from oracle import ba_ref
        host = _host_ba(cam, prob)
        ref = ba_ref.local_bundle_adjustment(cam, prob["pose_R"].reshape(-1, 3, 3), prob["pose_t"], prob["pose_fixed"], prob["ba_points"], prob["edge_pose"],
                                             prob["edge_point"], prob["edge_z"], prob["edge_inv_sigma2"], ba.HUBER_MONO)
        checks.append(dict(outlier=np.array_equal(host["outlier"], ref["outlier"]), n_outliers=int(host["outlier"].sum()),
                           close={k: bool(_close(host[k], ref[k], LM_TOL)) for k in ("pose_R", "pose_t", "points")},
                           err={k: float(np.abs(host[k] - ref[k]).max() / max(np.abs(ref[k]).max(), 1e-30)) for k in ("pose_R", "pose_t", "points")}))
        return host["pose_R"].reshape(-1, 9), host["pose_t"], host["points"], host["outlier"].astype(np.uint8)
    return solve


def _triangulate_twin(checks):
    def triangulate(s, nb, K, m12):
        """orbm_triangulate_matches on copies of the model's arrays -> what triangulation_model.evaluate returns, with the library's bits"""
        from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
        t = s["table"]
        kps1, kps2, desc2 = s["rec_kps"][nb], s["rec_kps"][K], s["rec_desc"][K]
        n0 = s["n_points"]
        a = dict(n_points=np.array([n0], np.int32), mp1=t["slots"][nb, :len(kps1)].copy(), mp2=t["slots"][K, :len(kps2)].copy(),
                 has_mp1=np.zeros(len(kps1), np.uint8), has_mp2=np.zeros(len(kps2), np.uint8),
                 **{k: s[k].copy() for k in ("points", "valid", "normals", "min_dist", "max_dist", "desc", "obs")})
        code, result = ORBMatcher().TriangulateMatches(ProjCamera.make(s["cam"], s["bounds"]), a, kps1, kps2, desc2, m12, (t["pose_R"][nb], t["pose_t"][nb]),
                                                       (t["pose_R"][K], t["pose_t"][K]), tm.SIGMA2, float(tm.MAX_SCALE_FACTOR), float(tm.RATIO_FACTOR),
                                                       fisheye_scale=s["scale_table"])
        cloud = dict(cam=s["cam"], scale_table=s["scale_table"], R1=t["pose_R"][nb], t1=t["pose_t"][nb], R2=t["pose_R"][K], t2=t["pose_t"][K], kps1=kps1,
                     kps2=kps2, desc2=desc2, matches12=m12, n_points=n0)
        e32, e64 = tm.run_model(cloud), tm.run_model(cloud, np.float64)
        _, excluded = _exclusions(cloud, e32, e64)
        checks.append(dict(K=K, nb=nb, matches=int((m12 >= 0).sum()), excluded=int(excluded.sum()), equal=bool(np.array_equal(code[~excluded], e64["code"][~excluded]))))
        feat1 = np.flatnonzero(code == 0)
        rows = n0 + np.arange(len(feat1))
        if result[1]:
            return dict(code=code, result=result, overflow=True, index=np.zeros(len(m12), np.int64), feat1=feat1[:0])
        index = np.full(len(m12), -1, np.int64)
        index[feat1] = rows
        return dict(code=code, result=result, index=index, feat1=feat1, feat2=m12[feat1], points=a["points"][rows], normals=a["normals"][rows],
                    min_dist=a["min_dist"][rows], max_dist=a["max_dist"][rows], desc=a["desc"][rows], obs=a["obs"][rows])
    return triangulate


def _model(name):
    """the session on the array models with the library's two float answers, once per name, shared, never changed:
    per key frame the frame, the state before and after and the calls' outputs"""
    if name not in _models:
        steps, ba_checks, tri_checks = [], [], []
        t0 = time.time()
        out = ms.run_session(name, ba=_ba_host(ba_checks), triangulate=_triangulate_twin(tri_checks),
                             each=lambda K, frame, before, s, log: steps.append(dict(K=K, frame=frame, before=before, after=ms.copy_state(s), log=log)))
        world = out["world"]
        _models[name] = dict(out, steps=steps, ba_checks=ba_checks, tri_checks=tri_checks, initial=ms.initial_state(world), seconds=time.time() - t0)
    return _models[name]


# ---- the device's backend ---------------------------------------------------------------------------------------------------------------------
class _Device:
    """the session's tables in padded device arrays with guards, and every call of mapper_session.step through the wrappers"""

    def __init__(self, torch, dev, world, state, stream_kind, records=None):
        from monoorbslam3_amd.frame import FramePost
        from monoorbslam3_amd.matcher import CovisGraph, ORBMatcher, ProjCamera
        self.torch, self.dev, self.world = torch, dev, world
        cfg = self.cfg = world.cfg
        ck, st, cp, co = cfg["cap_kf"], cfg["stride"], cfg["cap_points"], cfg["cap_obs"]
        self.s = dict(cfg=cfg, n_kf=state["n_kf"], dead_kfs=list(state["dead_kfs"]))
        self.m = ORBMatcher(0.6, False)                                   # LocalMapping.cpp:151
        self.cam = ProjCamera.make(world.cam, world.bounds)
        post = FramePost(pm.W, pm.H, *world.cam[:4], undistort=False)
        self.grid = (post.cols, post.rows)
        assert all(len(f["cell_start"]) == post.cols * post.rows + 1 for f in world.features)   # the oracle's grid is the library's
        self.records = records or self._upload_records()
        host = {{"kps": "kf_kps", "desc": "kf_desc"}.get(k, k): v.copy() for k, v in state["table"].items()}   # `desc` is the points' here
        for k in range(state["n_kf"]):
            host["kf_kps"][k], host["kf_desc"][k] = self.addr(k)
        host.update({k: state[k] for k in ms.STATE_ARRAYS})
        host.update({k: np.array([state[k]], np.int32) for k in ms.STATE_INTS})
        host.update({"g_" + k: state["graph"][k] for k in ms.GRAPH_KEYS})
        z = lambda n, dt=np.int32, fill=None: np.full(n, (205 if dt == np.uint8 else -51) if fill is None else fill, dt)  # noqa: E731
        scratch = dict(frame_mp=z(st), frame_pose_R=z(9, np.float64), frame_pose_t=z(3, np.float64), d_found=z(cp), d_visible=z(cp), has_mp=z(ck * st, np.uint8, 0),
                       matches12=z(st), search_result=z(8), tri_code=z(ms.N_NEIGHBOURS * st), q_xy=z(2 * cp, np.float32, 0), q_radius=z(cp, np.float32, 0),
                       q_level=z(cp), q_ok=z(cp, np.uint8), mask=z(cp + 1, np.uint8), q_valid=z(cp, np.uint8), best_idx=z(cp), best_dist=z(cp), best_sel=z(cp),
                       q_result=z(8), work_q=z(cp), sigma2=tm.SIGMA2.copy(), targets=z(ck), rows=z(cp), work_rows=z(cp), work_kf=z(ck), local=z(ck + 1),
                       n_local=z(1), work=z(cp + ck), est_pose_R=z(9 * ck, np.float64), est_pose_t=z(3 * ck, np.float64), est_points=z(3 * cp, np.float64),
                       chi2=z(co, np.float64), outlier=z(co, np.uint8), kf_code=z(ck), num_mp=z(ck), num_redundant=z(ck),
                       fuse_code=z((ck + 1) * cp), fuse_sel=z((ck + 1) * cp))
        sizes = dict(pose_R=9 * ck, pose_t=3 * ck, pose_fixed=ck, pose_kf=ck, ba_points=3 * cp, point_row=cp, edge_off=cp + 1)
        for k, dt in OUT_TYPES.items():
            scratch["ba_" + k] = z(sizes.get(k, co * WIDTH.get(k, 1)), dt, 91 if dt == np.uint8 else -91)
        names = ["insert", "build", "refresh", "update", "cull_map_points", "register", "build2", "fuse_targets", "build3", "refresh2", "update2", "ba_problem",
                 "ba_apply", "build4", "refresh3", "cull_keyframes", "erase"] + ["triangulate_%d" % k for k in range(ck)]
        names += ["fuse_%d" % j for j in range(ck + 1)] + ["build_fuse_%d" % j for j in range(ck + 1)]
        scratch.update({"r_" + n: z(16) for n in names})
        host.update(scratch)
        self.host0 = {k: np.ascontiguousarray(a) for k, a in host.items()}
        self.pads = {k: _padded(torch, dev, a, _fill(a)) for k, a in self.host0.items()}
        self.d = {k: v[1] for k, v in self.pads.items()}
        self.graph = CovisGraph.make(*(self.d["g_" + k] for k in ms.GRAPH_KEYS))
        self.st = _stream(torch, dev, stream_kind)

    def _upload_records(self):
        torch, dev, st = self.torch, self.dev, self.cfg["stride"]
        rec = []
        for f in self.world.features:
            n2 = len(f["kps"])
            kps, desc = np.zeros(st, pm.KP_DTYPE), np.zeros((st, 32), np.uint8)
            kps[:n2], desc[:n2] = f["kps"], f["desc"]
            nodes, off, idx = f["fv"]
            rec.append(dict(n2=n2, kps=_up(torch, dev, kps), desc=_up(torch, dev, desc), cell_start=_up(torch, dev, f["cell_start"]),
                            cell_items=_up(torch, dev, np.concatenate([f["cell_items"], np.zeros(1, np.int32)])),
                            fv=(_up(torch, dev, nodes.view(np.int32)), _up(torch, dev, off), _up(torch, dev, np.concatenate([idx.view(np.int32), np.zeros(1, np.int32)])),
                                _up(torch, dev, np.array([len(nodes)], np.int32)))))
        return rec

    def addr(self, k):
        return self.records[k]["kps"].data_ptr(), self.records[k]["desc"].data_ptr()

    def close(self):
        self.torch.cuda.synchronize()
        self.torch.cuda.set_stream(self.torch.cuda.default_stream(self.dev))

    def host(self, a):
        """the step's ONE wait"""
        self.torch.cuda.synchronize()
        return a.cpu().numpy()

    def guards_intact(self):
        for k, (whole, _) in self.pads.items():
            assert _guards_intact(whole, _fill(self.host0[k])), k

    # -- views ------------------------------------------------------------------------------------------------------------------------------------
    def _kft(self):
        from monoorbslam3_amd.matcher import KfTable
        nk, d = self.s["n_kf"], self.d
        return KfTable.make(d["pose_R"][:9 * nk], d["pose_t"][:3 * nk], d["bad"][:nk], d["kf_kps"][:nk], d["kf_desc"][:nk], d["n"][:nk])

    def _row(self, key, k, width):
        return self.d[key][k * width:(k + 1) * width]

    def _with(self, name, **more):
        return dict(self.d, result=self.d["r_" + name], **more)

    # -- the calls ----------------------------------------------------------------------------------------------------------------------------------
    def track(self, frame):
        d, st = self.d, self.cfg["stride"]
        mp = np.full(st, -1, np.int32)
        mp[:frame.n2] = frame.mp
        for key, a in (("frame_mp", mp), ("frame_pose_R", frame.R), ("frame_pose_t", frame.t), ("d_found", frame.d_found), ("d_visible", frame.d_visible)):
            d[key].copy_(self.torch.from_numpy(np.ascontiguousarray(a)))   # the tracker's hand-over: the step's input
        self.torch.cuda.synchronize()
        d["found"] += d["d_found"]
        d["visible"] += d["d_visible"]
        d["ba_point_row"].fill_(-1)
        self.n2 = frame.n2

    def insert(self, frame):
        K, rec = frame.K, self.records[frame.K]
        self.m.InsertKeyFrameDevice(self._with("insert", kps=self.d["kf_kps"], desc=self.d["kf_desc"]), K, self.cfg["stride"], self.cfg["cap_points"], frame.n2, rec["kps"], rec["desc"], stream=self.st)
        self.s["n_kf"] = K + 1
        return self.d["r_insert"]

    def build(self, name):
        self.m.BuildObservationsDevice(self._with(name), self.s["n_kf"], self.cfg["stride"], self.cfg["cap_points"], self.cfg["cap_obs"], stream=self.st)
        return self.d["r_" + name]

    def refresh(self, name, sel, kf_self=-1):
        if sel[0] == "slots":
            rows, n_sel = self._row("slots", sel[1], self.cfg["stride"]), self.records[sel[1]]["n2"]
        else:
            rows, n_sel = self.d["ba_point_row"], self.cfg["cap_points"]
        self.m.RefreshPointsDevice(self._kft(), self._with(name, sel=rows), n_sel, self.cfg["cap_points"], self.cfg["cap_obs"], float(rm.MAX_SCALE_FACTOR),
                                   kf_self=kf_self, stream=self.st)
        return self.d["r_" + name]

    def update(self, name, K):
        self.m.UpdateConnectionsDevice(self.graph, self._with(name, work=self.d["work_kf"]), self.s["n_kf"], K, first_kf=ms.FIRST_KF, stream=self.st)
        return self.d["r_" + name]

    def cull_map_points(self, K):
        self.m.CullMapPointsDevice(self._with("cull_map_points", code=self.d["mp_code"]), K, self.s["n_kf"], self.cfg["stride"], self.cfg["cap_points"],
                                   self.cfg["cap_obs"], stream=self.st)
        return self.d["r_cull_map_points"]

    def has_mp(self, k):
        """d_has_mp of key frame k: its slot names a row.  Nothing in the library keeps it between steps; torch, on the chain's stream"""
        st = self.cfg["stride"]
        flags = self._row("has_mp", k, st)
        flags.copy_(self._row("slots", k, st) >= 0)
        return flags

    def triangulate_pair(self, name, nb, K, has2):
        d, st, rec1, rec2 = self.d, self.cfg["stride"], self.records[nb], self.records[K]
        self.n_tri = getattr(self, "n_tri", 0) + 1
        code = self._row("tri_code", self.n_tri % ms.N_NEIGHBOURS, st)
        has1 = self.has_mp(nb)
        call = dict(d, desc1=rec1["desc"], kps1=rec1["kps"], has_mp1=has1, fv1=rec1["fv"], desc2=rec2["desc"], kps2=rec2["kps"], has_mp2=has2, fv2=rec2["fv"],
                    result=d["search_result"])
        self.m.SearchForTriangulationDevice(call, rec1["n2"], rec2["n2"], stream=self.st)
        call.update(pose_R1=self._row("pose_R", nb, 9), pose_t1=self._row("pose_t", nb, 3), pose_R2=self._row("pose_R", K, 9), pose_t2=self._row("pose_t", K, 3),
                    mp1=self._row("slots", nb, st), mp2=self._row("slots", K, st), code=code, result=d["r_triangulate_%d" % nb])
        if self.world.scale_table is not None:
            if not hasattr(self, "scale"):
                self.scale = _up(self.torch, self.dev, self.world.scale_table)
            call["fisheye_scale"] = self.scale
        self.m.TriangulateMatchesDevice(self.cam, call, rec1["n2"], rec2["n2"], self.cfg["cap_points"], tm.SIGMA2, float(tm.MAX_SCALE_FACTOR),
                                        float(tm.RATIO_FACTOR), stream=self.st)
        return code[:rec1["n2"]], d["r_triangulate_%d" % nb]

    def register(self, K):
        self.m.RegisterNewPointsDevice(self._with("register"), K, K, self.cfg["cap_points"], stream=self.st)
        return self.d["r_register"]

    def fuse_targets(self, K):
        d, cfg = self.d, self.cfg
        self.m.FuseTargetsDevice(self.graph, self._with("fuse_targets", work=d["work_rows"]), self.s["n_kf"], cfg["stride"], cfg["cap_points"], K, cfg["cap_kf"],
                                 cfg["cap_points"], stream=self.st)
        self.torch.cuda.synchronize()                                      # the fuse's read-back: d_result and the targets
        res = d["r_fuse_targets"].cpu().numpy()[:8].copy()
        n_t, self.n_rows = min(int(res[gm.T_TARGETS]), cfg["cap_kf"]), min(int(res[gm.T_ROWS]), cfg["cap_points"])
        return d["targets"].cpu().numpy()[:n_t].copy(), d["rows"][:self.n_rows], res

    def fuse(self, name, K, target, into_current):
        torch, d, cfg = self.torch, self.d, self.cfg
        cap, st = cfg["cap_points"], cfg["stride"]
        j = int(name.split("_")[1])
        cand = (d["rows"][:self.n_rows] if into_current else self._row("slots", K, st)).long()
        d["mask"].zero_()                                                  # the candidates as a mask over the table: torch, on the chain's stream
        d["mask"].index_fill_(0, torch.where(cand >= 0, cand, torch.full_like(cand, cap)), 1)
        torch.mul(d["mask"][:cap], (d["valid"] != 0).to(torch.uint8), out=d["q_valid"])
        rec = self.records[target]
        q = dict(d, pose_R=self._row("pose_R", target, 9), pose_t=self._row("pose_t", target, 3), valid=d["q_valid"], q_desc=d["desc"], kps=rec["kps"],
                 desc=rec["desc"], cell_start=rec["cell_start"], cell_items=rec["cell_items"], result=d["q_result"])
        self.m.ProjectFuseDevice(self.cam, q, cap, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), ms.FUSE_TH, stream=self.st)
        self.m.SearchFuseDevice(q, cap, self.grid[0], self.grid[1], list_cap=48, stream=self.st)
        code, sel = self._row("fuse_code", j, cap), self._row("fuse_sel", j, cap)
        if into_current:
            nq = self.n_rows
            d["best_sel"][:nq].copy_(d["best_idx"][cand])
            call = self._with("fuse_%d" % j, best_idx=d["best_sel"], rows=d["rows"], work=d["work_q"], code=code, refresh_sel=sel)
        else:
            nq = cap
            call = self._with("fuse_%d" % j, best_idx=d["best_idx"], rows=None, work=d["work_q"], code=code, refresh_sel=sel)
        self.m.FuseApplyDevice(call, nq, self.s["n_kf"], target, st, cap, cfg["cap_obs"], stream=self.st)
        return code[:nq], sel[:nq], d["r_fuse_%d" % j]

    def connected(self, K):
        self.m.ConnectedKeyFramesDevice(self.graph, dict(out=self.d["local"], n_out=self.d["n_local"]), self.s["n_kf"], K, include_self=True, stream=self.st)
        return self.d["local"], self.d["n_local"]

    def ba_problem(self):
        from monoorbslam3_amd import matcher
        d, cfg = self.d, self.cfg
        self.ba_d = dict(d, **{k: d["ba_" + k] for k in OUT_TYPES})
        self.ba_d.update(kf_pose_R=d["pose_R"], kf_pose_t=d["pose_t"], pose_R=d["ba_pose_R"], pose_t=d["ba_pose_t"])
        matcher.local_ba_problem_device(self.m, self._kft(), dict(self.ba_d, result=d["r_ba_problem"]), cfg["stride"], cfg["cap_points"], cfg["cap_obs"],
                                        cfg["cap_kf"] + 1, ms.FIRST_KF, cfg["cap_kf"], cfg["cap_points"], cfg["cap_obs"], stream=self.st)
        self.head = d["r_ba_problem"][:8].cpu().numpy()                    # the 32-byte read-back
        return self.head

    def ba_solve(self):
        from monoorbslam3_amd import ba
        n_poses, n_points, n_edges = (int(v) for v in self.head[:3])
        self.info = ba.local_bundle_adjustment_device(self.world.cam, self.ba_d, n_poses, n_points, n_edges, stream=self.st)
        d = self.d
        return d["est_pose_R"][:9 * n_poses], d["est_pose_t"][:3 * n_poses], d["est_points"][:3 * n_points], d["outlier"][:n_edges]

    def ba_apply(self):
        from monoorbslam3_amd import matcher
        cfg = self.cfg
        matcher.local_ba_apply_device(self.m, dict(self.ba_d, result=self.d["r_ba_apply"]), self.s["n_kf"], cfg["stride"], cfg["cap_points"], cfg["cap_obs"],
                                      int(self.head[lbm.P_LOCAL]), int(self.head[lbm.P_POINTS]), int(self.head[lbm.P_EDGES]), stream=self.st)
        return self.d["r_ba_apply"]

    def cull_keyframes(self, recent, timestamps):
        d, cfg = self.d, self.cfg
        n = len(recent)
        call = self._with("cull_keyframes", code=d["kf_code"], num_mp=d["num_mp"], num_redundant=d["num_redundant"])
        self.m.CullKeyFramesDevice(self._kft(), call, cfg["stride"], cfg["cap_points"], cfg["cap_obs"], recent, timestamps, first_kf=ms.FIRST_KF, stream=self.st)
        return d["kf_code"][:n], d["num_mp"][:n], d["num_redundant"][:n], d["r_cull_keyframes"]

    def erase(self, recent, code):
        self.m.EraseConnectionsDevice(self.graph, dict(code=self.d["kf_code"], work=self.d["work_kf"], result=self.d["r_erase"]), self.s["n_kf"], recent, stream=self.st)
        return self.d["r_erase"]

    # -- what the device holds ------------------------------------------------------------------------------------------------------------------------
    def download(self):
        return {k: v.cpu().numpy() for k, v in self.d.items() if k in self.host_keys()}

    def host_keys(self):
        return set(ms.STATE_ARRAYS) | set(ms.STATE_INTS) | {"g_" + k for k in ms.GRAPH_KEYS} | {"pose_R", "pose_t", "bad", "kf_kps", "kf_desc", "n", "slots"}


# ---- the comparison ---------------------------------------------------------------------------------------------------------------------------------
def _state_differences(be, want):
    """-> the arrays in which the device differs from the model state `want`"""
    got = be.download()
    nk = want["n_kf"]
    bad = []

    def same(key, a, b):
        a, b = np.ascontiguousarray(a).reshape(-1), np.ascontiguousarray(b).reshape(-1)
        ok = np.array_equal(a, b) if key in BY_VALUE else a.tobytes() == b.astype(a.dtype).tobytes()
        if not ok:
            where = np.flatnonzero(a != b.astype(a.dtype))
            bad.append("%s (%d entries, the first at %s: device %s, model %s)" % (key, len(where), where[:1].tolist(), a[where[:1]].tolist(), b[where[:1]].tolist()))

    for key in ("pose_R", "pose_t", "bad", "n", "slots"):
        same("table." + key, got[key], want["table"][key])
    for k in range(nk):
        same("table.kps[%d]" % k, got["kf_kps"][k:k + 1], np.array([be.addr(k)[0]]))
        same("table.desc[%d]" % k, got["kf_desc"][k:k + 1], np.array([be.addr(k)[1]]))
    for key in ms.STATE_ARRAYS:
        same(key, got[key], want[key])
    for key in ms.STATE_INTS:
        same(key, got[key], np.array([want[key]], np.int32))
    for key in ms.GRAPH_KEYS:
        same("graph." + key, got["g_" + key], want["graph"][key])
    return bad


def _output_differences(be, name, got, want):
    bad = []
    for key, w in want.items():
        if w is None:
            continue
        g = be.d["r_ba_problem"] if name == "ba_problem" else got[key]     # the step read 32 bytes of it back; all 16 counters are compared
        g = g.cpu().numpy() if hasattr(g, "cpu") else np.asarray(g)
        w = np.ascontiguousarray(w).reshape(-1)
        g = g.reshape(-1)[:len(w)]
        if len(g) != len(w):
            bad.append("%s.%s (device %d entries, model %d)" % (name, key, len(g), len(w)))
        elif g.tobytes() != w.astype(g.dtype).tobytes():
            where = np.flatnonzero(g != w.astype(g.dtype))
            bad.append("%s.%s (%d entries, the first at %s: device %s, model %s)" % (name, key, len(where), where[:1].tolist(), g[where[:1]].tolist(), w[where[:1]].tolist()))
    return bad


def _first_difference(torch, dev, world, step, stream_kind, records):
    """key frame K once more from the model's state before it, with a wait and a comparison behind every call -> a description of the
    first call behind which the device differs from the model's intermediate state, and of the arrays that differ"""
    snaps = []
    s = ms.copy_state(step["before"])
    ms.step_arrays(s, step["frame"], world, ba=_ba_host([]), triangulate=_triangulate_twin([]),
                   after=lambda name, out: snaps.append((name, ms.copy_state(s), out)))
    be = _Device(torch, dev, world, step["before"], stream_kind, records)
    found, at = [], [0]

    def after(name, out):
        if found:
            return
        torch.cuda.synchronize()
        want_name, want_state, want_out = snaps[at[0]]
        at[0] += 1
        assert name == want_name, (name, want_name)
        bad = _output_differences(be, name, out, want_out) + _state_differences(be, dict(want_state, n_kf=be.s["n_kf"]))
        if bad:
            found.append("the first difference is behind `%s`: %s" % (name, "; ".join(bad)))

    ms.step(be, step["frame"], world, after=after)
    be.close()
    return found[0] if found else "the key frame run again call by call shows no difference: the step's calls overlap differently without the waits"


def _run_device_session(name, stream_kind):
    """-> (bytes of the device's state after every key frame, seconds on the device side)"""
    import torch
    dev = torch.device("cuda", 0)
    model = _model(name)
    world = model["world"]
    be = _Device(torch, dev, world, model["initial"], stream_kind)
    assert not _state_differences(be, model["initial"])
    trail, t0 = [], time.time()
    try:
        for step in model["steps"]:
            K = step["K"]
            log = ms.step(be, step["frame"], world)                        # one wait at its end: be.host(d_code)
            be.guards_intact()
            bad = _state_differences(be, step["after"])
            assert [n for n, _ in log] == [n for n, _ in step["log"]], (K, [n for n, _ in log], [n for n, _ in step["log"]])
            for (n, got), (_, want) in zip(log, step["log"]):
                bad += _output_differences(be, n, got, want)
            if bad:
                be.close()
                where = _first_difference(torch, dev, world, step, stream_kind, be.records)
                raise AssertionError("session %s, key frame %d: %s.  After the whole step: %s" % (name, K, where, "; ".join(bad)))
            got = be.download()
            trail.append(b"".join(got[k].tobytes() for k in sorted(got) if k not in ("kf_kps", "kf_desc")))
    finally:
        be.close()
    return trail, time.time() - t0


def _admit(name):
    """the model session the device is compared with holds every event it was designed for, and the library's two float answers agree
    with their references at every key frame"""
    model = _model(name)
    tags = model["tags"]
    print("session %s: model %.2f s, events %s" % (name, model["seconds"], tags))
    if name == "main":
        assert set(tags) >= ms.ALL_TAGS and not set(tags) & ms.OVERFLOW_TAGS, (ms.ALL_TAGS - set(tags), set(tags) & ms.OVERFLOW_TAGS)
    if name in ms.OVERFLOW_TAGS:
        assert name in tags and tags[name] < model["world"].cfg["n_kf"] - 1, tags          # and the session goes on behind it
        later = {"csr_overflow"} if name == "csr_overflow_late" else set()      # key frame 3 of that session opens with an overflow of its own
        assert not (ms.OVERFLOW_TAGS - {name} - later) & set(tags)
    for c in model["ba_checks"]:
        print("  local BA against ba_ref: outliers %d, equal %s, relative error %s" % (c["n_outliers"], c["outlier"], c["err"]))
        assert c["outlier"] and all(c["close"].values()), c
    for c in model["tri_checks"]:
        assert c["equal"] and c["excluded"] <= max(1, c["matches"] // 20), c
    print("  triangulated pairs %d, matches excluded from the float64 comparison %d of %d" % (
        len(model["tri_checks"]), sum(c["excluded"] for c in model["tri_checks"]), sum(c["matches"] for c in model["tri_checks"])))
    return model


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_the_main_session_equals_the_models_after_every_key_frame(stream_kind):
    """ten key frames behind a two-view map, Pinhole: 96 slots a key frame, 330 world points, a table of 1400 rows.  Every event of
    mapper_session.ALL_TAGS occurs and neither capacity is reached; after every key frame every table, d_result, code array, list, the
    graph, the whole of the CSR arrays and the refreshed rows equal the composed models'."""
    _admit("main")
    trail, seconds = _run_device_session("main", stream_kind)
    print("device session: %.2f s for %d key frames" % (seconds, len(trail)))


def test_the_kannala_brandt_session_equals_the_models():
    """four key frames behind a two-view map through the Fisheye camera: the triangulation's scale table, the fuse builder's atanf and
    the BA's Kannala-Brandt Jacobians in the chain"""
    _admit("kb")
    trail, seconds = _run_device_session("kb", "explicit")
    print("device session: %.2f s for %d key frames" % (seconds, len(trail)))


@pytest.mark.parametrize("name", sorted(ms.OVERFLOW_TAGS))
def test_a_session_goes_on_behind_a_full_table_and_a_full_csr(name):
    """the point table runs full inside a triangulation (reported, nothing written, the later neighbours of that key frame refused too);
    cap_obs overflows at the first build of a step (the refresh, the graph update and MapPointCulling behind empty lists) and, in the
    third session, at the builds behind the fuse (fuse applies, the second refresh and update, the BA assembly -- refused with "no
    edge", so the LM, the apply, build4 and refresh3 are skipped --, KeyFrameCulling and the erase behind empty lists).  What each call
    does there is mapper_session.py's docstring and the headers'.  Every session goes on for at least one more key frame, and the device
    still equals the models after each."""
    _admit(name)
    _run_device_session(name, "explicit")


def test_the_main_session_twice_from_fresh_tables_gives_the_same_bytes():
    """every table, the graph, the CSR arrays and the counters after every key frame (the two columns of record addresses left out)"""
    a, _ = _run_device_session("main", "explicit")
    b, _ = _run_device_session("main", "explicit")
    assert len(a) == len(b) and all(x == y for x, y in zip(a, b))
