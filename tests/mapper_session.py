"""A whole mapper session on the device-resident map, stated three times on one small deterministic world.

  World                 a few hundred 3D points with a 32-byte descriptor each, a camera path of key frames with overlapping views (Pinhole,
                        or Kannala-Brandt), and per key frame the tracked frame the tracker would hand over: key points with octaves,
                        descriptors in which every observation flips a few bits of its point's, the pose, and frame_mp from the ground-truth
                        association with the table AS THE TRACKER LAST SAW IT (one step behind), with some entries wrong and some missing.
                        The grid and the feature vector the two searches read are built when the frame is made, by the oracle: inputs.
  step(backend, frame)  ONE mapper step in the order of INTEGRATION.md, "One mapper step as a chain on one stream", written once over a
                        backend: which calls, in which order, on which host decisions (the neighbours, the fuse targets read back, the 32
                        bytes of the BA problem).  ArrayBackend below composes the array models of tests/*_model.py; the GPU test's backend
                        makes the same calls through monoorbslam3_amd.matcher / .ba, so the two cannot be composed differently.
  step_arrays           step() on ArrayBackend: the model the device is compared with, call by call and byte for byte.
  step_objects          the same step on Python KeyFrame / MapPoint objects, following LocalMapping.cpp:47-372 call by call.  It knows
                        nothing of slots, CSR offsets or tombstones, and is the reference the array session is judged by on the CPU.

Two estimates are parameters of a session, so that a CPU and a GPU session can supply different ones: the local BA's (oracle/ba_ref.py's
LM on the CPU; the library's host entry point beside the device) and the triangulation's floats (triangulation_model.evaluate in
float32 on the CPU; the library's host twin beside the device -- the device's solver is not LAPACK's, tests/test_triangulation_gpu.py
holds it to the float64 model inside a stated band, and a session needs the bits).

What a session settles between the calls (each is a sentence of INTEGRATION.md or include/orbm.h now):
  * d_has_mp of a key frame is `its slot names a table row` at the moment a search reads it; no call maintains it between steps.
  * the fuse runs orbm_build_observations_device in front of EVERY orbm_fuse_apply_device: the apply finds a row's slots through the
    CSR, and the apply of the target before it added and moved slots the old CSR does not list.
  * the CSR arrays keep what an earlier build wrote behind the entries of the last one; n_obs is passed as cap_obs throughout and the
    offsets bound the lists.
  * behind a build that overflowed every list is empty: the refresh writes no row and counts every selected valid row under "no
    observation", d_covis is all zero and the graph update has nothing to do; MapPointCulling sees getNumObs() == 0 and sets every listed
    row of age >= 2 bad without clearing a slot (no list names one), and the next build skips those slots as invalid.  A map is lost that
    way, so the header now tells a chain that cannot read d_result[1] back to size cap_obs to n_kf x stride.
    Where the overflow falls on the build behind the fuse instead (session csr_overflow_late), the second refresh writes no row, the
    second graph update has nothing to do, the BA assembly keeps its local key frames, drops every row for having no edge and refuses
    with "no edge" -- the step then runs neither the LM, the apply, the build behind it nor the third refresh --, KeyFrameCulling counts
    numMP from the slots and no redundant point, keeps every candidate, and the erase finds no code 3.
No kernel of the library runs here: the searches are the oracle's, and monoorbslam3_amd.synth only draws the vocabulary."""
import numpy as np

import fuse_model as fm
import graph_model as gm
import keyframe_model as km
import local_ba_model as lbm
import observations_model as om
import projection_model as pm
import refresh_model as rm
import triangulation_model as tm

W, H = pm.W, pm.H
FIRST_KF = 0
FRAMES_PER_KF = 3                      # ordinary frames the tracker sees per key frame: what found / visible advance by
N_NEIGHBOURS = 3                       # key frames createNewMapPoints triangulates against
FUSE_TH = 3.0                          # LocalMapping.cpp:282
SIGMA2 = tm.SIGMA2

SESSIONS = {
    "main": dict(seed=5, fisheye=False, n_kf=12, n_points=330, stride=96, cap_kf=14, cap_points=1400, cap_obs=6000, cap_recent=700),
    "kb": dict(seed=9, fisheye=True, n_kf=6, n_points=260, stride=96, cap_kf=8, cap_points=900, cap_obs=4000, cap_recent=500),
    "table_full": dict(seed=5, fisheye=False, n_kf=5, n_points=330, stride=96, cap_kf=6, cap_points=112, cap_obs=3000, cap_recent=200),
    "csr_overflow": dict(seed=5, fisheye=False, n_kf=5, n_points=330, stride=96, cap_kf=6, cap_points=600, cap_obs=225, cap_recent=400),
    # cap_obs between what key frame 2's builds count ahead of the fuse (178, 202) and behind it (212): the overflow falls on the fuse's
    # later builds and on build3, so the second refresh, the BA assembly and KeyFrameCulling run behind empty lists
    "csr_overflow_late": dict(seed=5, fisheye=False, n_kf=5, n_points=330, stride=96, cap_kf=6, cap_points=600, cap_obs=210, cap_recent=400),
}

# ---- the events a session is admitted by -------------------------------------------------------------------------------------------------
ALL_TAGS = {
    "fused_row_meets_the_culling",      # a row a fuse hit replaced while listed in recent is met by the NEXT cull_map_points as already bad
    "ba_outlier_kills_recent_row",      # a row goes bad in the local BA's outlier handling while still listed in recent
    "fuse_replaces_recent_row",         # the fuse replaces a row that recent lists
    "kf_cull_cascade",                  # a culled key frame's cascade moves another row's ref_kf AND clears slots of other key frames
    "reconnect_after_erase",            # a key frame whose list an erase rebuilt has it rebuilt again by the SECOND update of a later step:
                                        # an edge between two key frames that both existed changes weight behind the erase
    "has_mp_suppresses_match",          # a later neighbour's search gives other matches than it would without the flags an earlier one set
    "two_triangulations_one_register",  # n_registered < n_points across two triangulations that both accepted rows, before the register
    "second_target_hits_changed_row",   # a fuse apply REPLACES (code 5 / 6) where the list row or the occupant is a row that an earlier
                                        # target's apply of the same step added or merged: its getNumObs() counts slots the old CSR lacks
    "frame_names_dead_row",             # the tracked frame's frame_mp names a row that went bad since the tracker saw the table
}
OVERFLOW_TAGS = {"table_full", "csr_overflow", "csr_overflow_late"}   # csr_overflow: a build of the step's opening; _late: build3


class Frame(dict):
    __getattr__ = dict.__getitem__


class World:
    """the points, the path and the frames of one session; frame(K, seen) needs the table as the tracker last saw it"""

    def __init__(self, name):
        from monoorbslam3_amd import synth
        from oracle import orb_ref_py as oracle
        cfg = dict(SESSIONS[name])
        self.name, self.cfg = name, cfg
        rng = np.random.RandomState(cfg["seed"])
        camd = pm.FISHEYE if cfg["fisheye"] else pm.PINHOLE
        self.cam, self.bounds = camd["cam"], camd["bounds"]
        self.scale_table = tm.fisheye_scale_table(self.cam) if cfg["fisheye"] else None
        n_pts, n_kf = cfg["n_points"], cfg["n_kf"]
        # a slab 6 - 12 m in front of a camera that walks along +x and turns a little: neighbours share most of their view
        self.P = np.stack([rng.uniform(-9.0, 15.0, n_pts), rng.uniform(-2.2, 2.2, n_pts), rng.uniform(6.0, 12.0, n_pts)], 1)
        self.desc = rng.randint(0, 256, (n_pts, 32)).astype(np.uint8)
        self.angle = rng.uniform(0, 360, n_pts).astype(np.float32)
        self.strength = rng.rand(n_pts)                                   # the extractor keeps the strongest corners in view
        self.hard = rng.rand(n_pts) < 0.12                               # points the tracker never finds again
        x = np.cumsum(np.r_[0.0, rng.uniform(0.45, 0.6, n_kf - 1)])
        if n_kf > 8:
            x[6] = x[5] + 0.04                                           # key frames 5 and 6 stand almost on one spot: one grows redundant
            x[7:] -= 0.35
        self.poses = []
        for k in range(n_kf):
            R = pm._rodrigues(np.array([0.004 * k + 1e-3, 0.012 * (k % 3) + 1e-3, -0.003 * k + 1e-3]))
            C = np.array([x[k], 0.03 * (k % 2), 0.05 * (k % 3)])
            self.poses.append((R, -R @ C))
        self.timestamps = 0.2 * np.arange(cfg["cap_kf"])
        self.voc = oracle.Vocabulary(synth.make_vocabulary(10, 3, seed=7, p_early_leaf=0.0, p_stop=0.0))
        self.oracle = oracle
        self.features = [self._features(k, np.random.RandomState(cfg["seed"] * 100 + k)) for k in range(n_kf)]

    def _project(self, Pc):
        return tm._project(np.float64, self.cam, Pc[:, 0], Pc[:, 1], Pc[:, 2])

    def _features(self, k, rng):
        """key points (orbx_kp records, as the frame post-processing leaves them: no distortion to remove), descriptors, the point behind
        each feature (-1 = clutter), the grid and the feature vector"""
        R, t = self.poses[k]
        stride = self.cfg["stride"]
        Pc = self.P @ R.T + t
        with np.errstate(all="ignore"):
            u, v = self._project(Pc)
        b = self.bounds
        vis = np.flatnonzero((Pc[:, 2] > 0.5) & (u > b[0] + 12) & (u < b[1] - 12) & (v > b[2] + 12) & (v < b[3] - 12))
        vis = vis[np.argsort(-(self.strength[vis] + 0.3 * rng.rand(len(vis))), kind="stable")][:stride - 8 - int(rng.randint(0, 6))]
        n_clutter = 4
        n2 = len(vis) + n_clutter
        kp = np.zeros(n2, pm.KP_DTYPE)
        depth = Pc[vis, 2]
        octave = np.clip(np.floor(np.log(12.5 / depth) / np.log(1.2)), 0, pm.N_LEVELS - 1).astype(np.int32)
        noise = 0.35 * pm.SCALE_FACTORS[octave].astype(np.float64)
        kp["x"][:len(vis)], kp["y"][:len(vis)] = u[vis] + rng.normal(size=len(vis)) * noise, v[vis] + rng.normal(size=len(vis)) * noise
        kp["octave"][:len(vis)] = octave
        kp["angle"][:len(vis)] = self.angle[vis]
        kp["x"][len(vis):], kp["y"][len(vis):] = rng.uniform(20, W - 20, n_clutter), rng.uniform(20, H - 20, n_clutter)
        kp["octave"][len(vis):], kp["angle"][len(vis):] = rng.randint(0, 4, n_clutter), rng.uniform(0, 360, n_clutter)
        kp["size"], kp["response"], kp["class_id"] = pm.SCALE_FACTORS[kp["octave"]], 50.0, -1   # the level's scale factor, as the frame post-processing leaves it
        desc = rng.randint(0, 256, (n2, 32)).astype(np.uint8)
        d = self.desc[vis].copy()
        for j in range(len(vis)):                                         # every observation flips a few bits, chosen per observation
            for bit in rng.choice(256, rng.randint(2, 7), replace=False):
                d[j, bit >> 3] ^= np.uint8(1 << (bit & 7))
        desc[:len(vis)] = d
        point = np.r_[vis, np.full(n_clutter, -1)]
        order = rng.permutation(n2)
        kp, desc, point = kp[order], np.ascontiguousarray(desc[order]), point[order]
        fx, fy, cx, cy = self.cam[:4]
        _, un, start, items = self.oracle.frame_post(W, H, fx, fy, cx, cy, [], kp, undistort=False)
        assert un.tobytes() == kp.tobytes()
        fv = self.voc.transform(desc)[2]
        return dict(kps=kp, desc=desc, point=point, cell_start=start.astype(np.int32), cell_items=items.astype(np.int32), fv=fv)

    def row_points(self, seen):
        """the world point behind every valid row of a table: the point most of the slots naming the row belong to"""
        votes = {}
        t = seen["table"]
        for k in range(seen["n_kf"]):
            if t["bad"][k]:
                continue
            for i in range(int(t["n"][k])):
                p = int(t["slots"][k, i])
                if p >= 0 and seen["valid"][p]:
                    votes.setdefault(p, []).append(int(self.features[k]["point"][i]))
        return {p: (max(set(v), key=lambda q: (v.count(q), -q)), len(v)) for p, v in votes.items()}

    def frame(self, K, seen):
        """the tracked frame that becomes key frame K.  seen: the session state when the tracker last read the table"""
        f = self.features[K]
        rng = np.random.RandomState(self.cfg["seed"] * 1000 + K)
        rows = self.row_points(seen)
        best = {}
        for p, (q, n) in rows.items():
            if q >= 0 and (q not in best or (n, -p) > (best[q][1], -best[q][0])):
                best[q] = (p, n)
        n2 = len(f["point"])
        mp = np.full(n2, -1, np.int32)
        d_found, d_visible = np.zeros(self.cfg["cap_points"], np.int32), np.zeros(self.cfg["cap_points"], np.int32)
        used = set()
        for i in rng.permutation(n2):
            q = int(f["point"][i])
            if q < 0 or q not in best:
                continue
            p = best[q][0]
            d_visible[p] += FRAMES_PER_KF                                 # in the frustum of every frame since the last key frame
            if self.hard[q] or rng.rand() < 0.22:
                continue                                                  # a missing entry
            mp[i] = p
            used.add(p)
            d_found[p] += FRAMES_PER_KF
        young = sorted((p for p in rows if p not in used), reverse=True)  # wrong entries name rows made lately, which recent still lists
        for i in rng.permutation(n2)[:5]:
            if mp[i] == -1 and f["point"][i] >= 0 and young:
                p = young.pop(0)
                if rows[p][0] != f["point"][i]:
                    mp[i] = p
                    used.add(p)
        R, t = self.poses[K]
        dR = pm._rodrigues(rng.normal(0, 2e-3, 3) + 1e-9)
        return Frame(K=K, mp=mp, R=(dR @ R).reshape(9), t=t + rng.normal(0, 4e-3, 3), kps=f["kps"], desc=f["desc"], cell_start=f["cell_start"],
                     cell_items=f["cell_items"], fv=f["fv"], d_found=d_found, d_visible=d_visible, n2=n2)


# ---- the session state as arrays ------------------------------------------------------------------------------------------------------------
STATE_ARRAYS = ("points", "valid", "normals", "min_dist", "max_dist", "desc", "obs", "ref_kf", "first_kf", "found", "visible", "recent", "mp_code",
                "obs_off", "obs_kf", "obs_kp", "covis")
STATE_INTS = ("n_points", "n_registered", "n_recent")
GRAPH_KEYS = ("weight", "ord_kf", "ord_n", "parent")


def empty_state(cfg, cam, bounds, scale_table):
    ck, st, cp, co, cr = cfg["cap_kf"], cfg["stride"], cfg["cap_points"], cfg["cap_obs"], cfg["cap_recent"]
    z = lambda shape, dt, fill=0: np.full(shape, fill, dt)  # noqa: E731
    return dict(
        cfg=cfg, cam=cam, bounds=bounds, scale_table=scale_table, n_kf=0, dead_kfs=[],
        table=dict(pose_R=z((ck, 9), np.float64), pose_t=z((ck, 3), np.float64), bad=z(ck, np.uint8), kps=z(ck, np.int64), desc=z(ck, np.int64),
                   n=z(ck, np.int32), slots=z((ck, st), np.int32, -1)),
        rec_kps=[], rec_desc=[], rec_grid=[], rec_fv=[],
        points=z((cp, 3), np.float32), valid=z(cp, np.uint8), normals=z((cp, 3), np.float32), min_dist=z(cp, np.float32), max_dist=z(cp, np.float32),
        desc=z((cp, 32), np.uint8), obs=z((cp, 2), np.int32, -1), ref_kf=z(cp, np.int32, -1), first_kf=z(cp, np.int32, -1), found=z(cp, np.int32),
        visible=z(cp, np.int32), recent=z(cr, np.int32, -3), mp_code=z(cr, np.int32, -9), n_points=0, n_registered=0, n_recent=0,
        graph=gm.new_graph(ck), obs_off=z(cp + 1, np.int32), obs_kf=z(co, np.int32), obs_kp=z(co, np.int32), covis=z(ck, np.int32))


def copy_state(s):
    out = dict(s)
    out["table"] = {k: v.copy() for k, v in s["table"].items()}
    out["graph"] = gm.copy_graph(s["graph"])
    for k in STATE_ARRAYS:
        out[k] = s[k].copy()
    for k in ("rec_kps", "rec_desc", "rec_grid", "rec_fv", "dead_kfs"):
        out[k] = list(s[k])
    return out


def state_bytes(s):
    """every byte a session holds, for `twice gives the same bytes`"""
    parts = [s["table"][k].tobytes() for k in km.TABLE_KEYS] + [s[k].tobytes() for k in STATE_ARRAYS] + [s["graph"][k].tobytes() for k in GRAPH_KEYS]
    return b"".join(parts) + repr([s[k] for k in STATE_INTS + ("n_kf",)]).encode()


def _view(s):
    """the dict the models read: the tables cut to the key frames that exist"""
    nk, t = s["n_kf"], s["table"]
    return dict(n_kf=nk, n=t["n"][:nk], bad=t["bad"][:nk], slots=t["slots"][:nk], pose_R=t["pose_R"][:nk], pose_t=t["pose_t"][:nk], stride=s["cfg"]["stride"],
                cap_points=s["cfg"]["cap_points"], valid=s["valid"], points=s["points"], ref_kf=s["ref_kf"], kps=s["rec_kps"], kf_desc=s["rec_desc"],
                normals=s["normals"], min_dist=s["min_dist"], max_dist=s["max_dist"], desc=s["desc"], obs_off=s["obs_off"], obs_kf=s["obs_kf"],
                obs_kp=s["obs_kp"], found=s["found"], visible=s["visible"], first_kf=FIRST_KF)


def _csr(s):
    return s["obs_off"], s["obs_kf"], s["obs_kp"]


def triangulate_float32(s, nb, K, m12):
    """the triangulation's answer from the numpy model in float32: what a CPU session uses"""
    t = s["table"]
    return tm.evaluate(s["cam"], s["scale_table"], t["pose_R"][nb], t["pose_t"][nb], t["pose_R"][K], t["pose_t"][K], s["rec_kps"][nb], s["rec_kps"][K],
                       s["rec_desc"][K], m12, n_points=s["n_points"])


def ba_reference(cam, prob):
    """the local BA's answer from oracle/ba_ref.py's LM: what a CPU session uses"""
    from oracle import ba_ref
    out = ba_ref.local_bundle_adjustment(cam, prob["pose_R"].reshape(-1, 3, 3), prob["pose_t"], prob["pose_fixed"], prob["ba_points"], prob["edge_pose"],
                                         prob["edge_point"], prob["edge_z"], prob["edge_inv_sigma2"], float(np.sqrt(np.float32(5.991))))
    return out["pose_R"].reshape(-1, 9), out["pose_t"], out["points"], out["outlier"].astype(np.uint8)


class ArrayBackend:
    """every call of the step as the array model of its header section, on the session state `s` (changed in place)"""

    def __init__(self, s, ba=ba_reference, triangulate=triangulate_float32, addr=None):
        """addr(k) -> the (d_kps, d_desc) addresses the key-frame table holds for key frame k (a device session's are real ones)"""
        from oracle import orb_ref_py
        self.s, self.ba, self.triangulate, self.oracle, self.addr = s, ba, triangulate, orb_ref_py, addr or (lambda k: (0, 0))
        self.notes = {}                                                   # what the event detectors need beyond d_result
        self.replays = []                                                 # (call, the rows Map::eraseMapPoint is replayed for, in order)

    # -- the frame arrives ----------------------------------------------------------------------------------------------------------------------
    def track(self, frame):
        self.s["found"] += frame.d_found
        self.s["visible"] += frame.d_visible

    def host(self, a):
        return a

    def insert(self, frame):
        s, K = self.s, frame.K
        out = km.insert_keyframe(s["table"], K, s["valid"], s["cfg"]["cap_points"], frame.mp, frame.R, frame.t, *self.addr(K))
        for k in km.TABLE_KEYS:
            s["table"][k] = out[k]
        s["n_kf"] = K + 1
        for key, val in (("rec_kps", frame.kps), ("rec_desc", frame.desc), ("rec_grid", (frame.cell_start, frame.cell_items)), ("rec_fv", frame.fv)):
            s[key].append(val)
        return out["result"]

    def build(self, name="build"):
        """name: the step's name of this call (a build, a refresh, an update and a fuse occur several times in a step)"""
        s, v = self.s, _view(self.s)
        off, kf, kp, res = om.build(v["n"], v["bad"], v["slots"], v["stride"], v["valid"], v["cap_points"], s["cfg"]["cap_obs"])
        s["obs_off"] = off
        s["obs_kf"][:len(kf)], s["obs_kp"][:len(kp)] = kf, kp            # entries at and past n_obs are not written
        return res

    def refresh(self, name, sel, kf_self=-1):
        """sel: ("slots", K) | ("point_row",) -- on the device a pointer into an array the chain already holds"""
        s, v = self.s, _view(self.s)
        rows = v["slots"][sel[1], :int(v["n"][sel[1]])] if sel[0] == "slots" else self.point_row
        out = rm.refresh(v, rows, v["cap_points"], kf_self=kf_self)
        for k in ("normals", "min_dist", "max_dist", "desc"):
            s[k] = out[k]
        s["covis"][:] = 0
        s["covis"][:v["n_kf"]] = out["covis"]
        return out["result"]

    def update(self, name, K):
        v = _view(self.s)
        before = self.s["graph"]["weight"].copy()
        res = gm.update(self.s["graph"], v["n_kf"], v["bad"], self.s["covis"][:v["n_kf"]], K, FIRST_KF)
        w = self.s["graph"]["weight"]
        self.notes["rebuilt_now"] = {int(j) for j in np.flatnonzero(w[:, K] != before[:, K])}   # the key frames whose edge to K changed
        return res

    def cull_map_points(self, K):
        s, v = self.s, _view(self.s)
        out = km.cull_map_points(dict(v, obs_off=s["obs_off"], obs_kf=s["obs_kf"], obs_kp=s["obs_kp"]), s["recent"], s["n_recent"], K, s["first_kf"],
                                 s["found"], s["visible"], code=s["mp_code"])
        self.notes["culled_rows"] = {int(p): int(c) for p, c in zip(s["recent"][:s["n_recent"]], out["code"])}
        self.replays.append(("cull_map_points", [int(p) for p, c in zip(s["recent"][:s["n_recent"]], out["code"]) if c in (2, 3)]))   # Map::eraseMapPoint from d_code
        s["recent"], s["n_recent"], s["valid"], s["mp_code"] = out["recent"], out["n_recent"], out["valid"], out["code"]
        s["table"]["slots"][:v["n_kf"]] = out["slots"]
        return out["result"]

    # -- createNewMapPoints -----------------------------------------------------------------------------------------------------------------------
    def has_mp(self, k):
        v = _view(self.s)
        return (v["slots"][k, :int(v["n"][k])] >= 0).astype(np.uint8)

    def search_for_triangulation(self, nb, K, has1, has2):
        s = self.s
        _, m12 = self.oracle.search_for_triangulation(False, s["rec_desc"][nb], s["rec_kps"][nb]["angle"], has1, s["rec_fv"][nb], s["rec_desc"][K],
                                                      s["rec_kps"][K]["angle"], has2, s["rec_fv"][K])
        return m12

    def triangulate_pair(self, name, nb, K, has2):
        """search + triangulation of one neighbour; has2: the current key frame's flags, carried from neighbour to neighbour (changed in place)
        -> (d_code [n1], d_result)"""
        s, cap = self.s, self.s["cfg"]["cap_points"]
        m12 = self.search_for_triangulation(nb, K, self.has_mp(nb), has2)
        self.notes["m12"] = m12
        e = self.triangulate(s, nb, K, m12)
        res, rows, n0 = e["result"].astype(np.int32).copy(), e["index"][e["feat1"]], s["n_points"]
        if e.get("overflow") or n0 + len(rows) > cap:                                          # a full table: reported, and nothing changes
            res[0], res[1] = 0, 1
            return e["code"], res
        s["points"][rows], s["valid"][rows], s["normals"][rows] = e["points"], 1, e["normals"]
        s["min_dist"][rows], s["max_dist"][rows], s["desc"][rows], s["obs"][rows] = e["min_dist"], e["max_dist"], e["desc"], e["obs"]
        s["table"]["slots"][nb, e["feat1"]], s["table"]["slots"][K, e["feat2"]] = rows, rows
        has2[e["feat2"]] = 1
        s["n_points"] = n0 + len(rows)
        return e["code"], res

    def register(self, K):
        s = self.s
        out = km.register_new_points(s["n_points"], s["n_registered"], s["n_recent"], K, K, s["cfg"]["cap_points"], s["ref_kf"], s["first_kf"], s["found"],
                                     s["visible"], s["recent"])
        for k in ("ref_kf", "first_kf", "found", "visible", "recent", "n_registered", "n_recent"):
            s[k] = out[k]
        return out["result"]

    # -- searchInNeighbors --------------------------------------------------------------------------------------------------------------------------
    def fuse_targets(self, K):
        """-> (targets, rows: what the caller reads back, d_result)"""
        s, v = self.s, _view(self.s)
        targets, rows, res = gm.fuse_targets(s["graph"], v["n_kf"], v["n"], v["bad"], v["slots"], v["stride"], v["valid"], v["cap_points"], K,
                                             cap_targets=s["cfg"]["cap_kf"], cap_rows=v["cap_points"])
        self.fuse_rows = rows
        return targets, rows, res

    def _queries(self, kf, mask):
        s, t = self.s, self.s["table"]
        return fuse_queries(self.oracle, s["cam"], s["bounds"], t["pose_R"][kf], t["pose_t"][kf], s, mask, s["rec_kps"][kf], s["rec_desc"][kf])

    def fuse(self, name, K, target, into_current):
        """one direction of the fuse: the current key frame's points into `target`, or the targets' points (d_rows) into the current one.
        The candidates reach the builder as a mask over the table; the apply takes entry j as row j, or d_rows with the hits gathered.
        -> (d_code, d_refresh_sel, d_result)"""
        s, v = self.s, _view(self.s)
        cap = v["cap_points"]
        mask = np.zeros(cap, np.uint8)
        cand = self.fuse_rows if into_current else v["slots"][K, :int(v["n"][K])]
        cand = cand[(cand >= 0) & (cand < cap)]
        mask[cand] = s["valid"][cand] != 0
        best = self._queries(target, mask)
        sc = dict(n=v["n"], bad=v["bad"], slots=v["slots"], stride=v["stride"], valid=s["valid"], cap_points=cap, K=target, found=s["found"],
                  visible=s["visible"], best_idx=best[self.fuse_rows] if into_current else best, rows=self.fuse_rows if into_current else None)
        out = fm.apply(sc, _csr(s))
        self.notes["fuse_in"] = sc
        if out["code"] is None:
            return None, None, out["result"]
        held, losers, pairs = {}, [], []                                  # the replay from d_code: 3 fills the slot, 5 loses the list row, 6 the occupant
        for p, sl, c in zip(fm._rows(sc).tolist(), sc["best_idx"].tolist(), out["code"].tolist()):
            o = held.get(sl, int(v["slots"][target, sl])) if c >= fm.ADDED else -1
            if c in (fm.ADDED, fm.OCCUPANT_REPLACED):
                held[sl] = p
            if c in (fm.LIST_REPLACED, fm.OCCUPANT_REPLACED):
                losers.append(p if c == fm.LIST_REPLACED else o)
                pairs.append((p, o))
        self.replays.append((name, losers))
        self.notes["replace_pairs"] = pairs
        s["table"]["slots"][:v["n_kf"]], s["valid"], s["found"] = out["slots"], out["valid"], out["found"]
        return out["code"], out["refresh_sel"], out["result"]

    def connected(self, K):
        s = self.s
        self.local, n = gm.connected(s["graph"], s["n_kf"], K, True, s["n_kf"], s["cfg"]["cap_kf"] + 1)
        return self.local, np.array([n], np.int32)

    # -- the local BA --------------------------------------------------------------------------------------------------------------------------------
    def ba_problem(self):
        """-> the first eight counters of d_result: the step's 32-byte read-back"""
        s, v = self.s, _view(self.s)
        cfg = s["cfg"]
        self.prob = lbm.problem(dict(v, local=self.local), _csr(s), cap_poses=cfg["cap_kf"], cap_local_points=cfg["cap_points"], cap_edges=cfg["cap_obs"])
        self.point_row = np.full(cfg["cap_points"], -1, np.int32)
        if self.prob["point_row"] is not None:
            self.point_row[:len(self.prob["point_row"])] = self.prob["point_row"]
        return self.prob["result"]

    def ba_solve(self):
        self.est = self.ba(self.s["cam"], self.prob)
        return self.est

    def ba_apply(self):
        s, v = self.s, _view(self.s)
        before = s["valid"].copy()
        out = lbm.apply(v, _csr(s), self.prob, *self.est)
        s["table"]["slots"][:v["n_kf"]], s["valid"], s["ref_kf"], s["points"] = out["slots"], out["valid"], out["ref_kf"], out["points"]
        s["table"]["pose_R"][:v["n_kf"]], s["table"]["pose_t"][:v["n_kf"]] = out["pose_R"], out["pose_t"]
        self.notes["ba_killed"] = set(np.flatnonzero((before != 0) & (out["valid"] == 0)).tolist())
        self.replays.append(("ba_apply", self.notes["ba_killed"]))        # no per-row code: the rows d_valid lost
        return out["result"]

    # -- KeyFrameCulling -----------------------------------------------------------------------------------------------------------------------------
    def cull_keyframes(self, recent, timestamps):
        s, v = self.s, _view(self.s)
        before, valid0 = (s["ref_kf"].copy(), v["slots"].copy()), s["valid"].copy()
        out = om.cull(dict(v, recent=np.asarray(recent, np.int32), timestamps=np.asarray(timestamps, np.float64)), *_csr(s))
        s["table"]["bad"][:v["n_kf"]], s["table"]["slots"][:v["n_kf"]], s["valid"], s["ref_kf"] = out["bad"], out["slots"], out["valid"], out["ref_kf"]
        self.notes["kf_cull"] = (before, out)
        self.replays.append(("cull_keyframes", set(np.flatnonzero((valid0 != 0) & (out["valid"] == 0)).tolist())))   # the cascade: no per-row code
        return out["code"], out["num_mp"], out["num_redundant"], out["result"]

    def erase(self, recent, code):
        s = self.s
        before = s["graph"]["weight"].copy()
        res = gm.erase(s["graph"], s["n_kf"], np.asarray(recent, np.int32), code)
        w = s["graph"]["weight"]
        self.notes["lost_connection"] = {int(j) for j in np.flatnonzero(((before > 0) & (w == 0)).any(1))} - {int(c) for c, x in zip(recent, code) if x == 3}
        return res


# ---- one mapper step, written once ----------------------------------------------------------------------------------------------------------------
def neighbours(s, K):
    """the key frames createNewMapPoints triangulates against: the most recent ones the host knows to be alive (it replays
    Map::eraseKeyFrame from d_code after every step's one wait), newest first"""
    return [k for k in range(K - 1, -1, -1) if k not in s["dead_kfs"]][:N_NEIGHBOURS]


def step(be, frame, world, after=None, tags=None, memo=None):
    """LocalMapping::run's body for one key frame (LocalMapping.cpp:47-91) on a backend.  after(name, outputs): called behind every call
    with what the call wrote beside the state (d_result, code arrays, lists).  tags: the event record of a model session, memo: what its detectors carry from key frame to key frame.
    -> the list of (name, outputs)"""
    s, K = be.s, frame.K
    log = []
    notes = getattr(be, "notes", None)
    tags = tags if tags is not None and notes is not None else None
    memo = memo if memo is not None else {}
    lost, fused = memo.setdefault("lost", set()), memo.setdefault("fused_while_recent", set())

    def did(name, **out):
        log.append((name, out))
        if after is not None:
            after(name, out)
        return out

    be.track(frame)                                                        # the tracker's counters since the last key frame
    r = did("insert", result=be.insert(frame))["result"]                  # processNewKeyFrame, LocalMapping.cpp:93-105
    if tags is not None and r[km.I_INVALID]:
        tags.setdefault("frame_names_dead_row", K)
    did("build", result=be.build("build"))
    did("refresh", result=be.refresh("refresh", ("slots", K), kf_self=K))
    did("update", result=be.update("update", K))
    did("cull_map_points", result=be.cull_map_points(K))                   # MapPointCulling, :117-144
    if tags is not None:
        for p, c in notes["culled_rows"].items():
            if c == 1 and p in fused:
                tags.setdefault("fused_row_meets_the_culling", K)
    has2 = be.has_mp(K)                                                    # createNewMapPoints, :146-259
    accepted, has2_start = 0, (has2.copy() if tags is not None else None)
    for nb in neighbours(s, K):
        if tags is not None:                                               # the same search with the flags as they were when the step began
            plain = be.search_for_triangulation(nb, K, be.has_mp(nb), has2_start)
        code, res = be.triangulate_pair("triangulate_%d" % nb, nb, K, has2)
        did("triangulate_%d" % nb, code=code, result=res)
        if tags is not None:
            if accepted and res[0]:
                tags.setdefault("two_triangulations_one_register", K)
            if accepted and not np.array_equal(plain, notes["m12"]):
                tags.setdefault("has_mp_suppresses_match", K)
            if res[1]:
                tags.setdefault("table_full", K)
            accepted += int(res[0])
    did("register", result=be.register(K))
    did("build2", result=be.build("build2"))
    targets, rows, res = be.fuse_targets(K)                                # searchInNeighbors, :261-316; the one read-back of the fuse
    did("fuse_targets", targets=targets, rows=rows, result=res)
    changed = set()
    fused.clear()
    for j, (target, into) in enumerate([(int(t), False) for t in targets] + [(K, True)]):
        if res[gm.T_REFUSED]:
            break
        if j:
            did("build_fuse_%d" % j, result=be.build("build_fuse_%d" % j))                   # the apply before this one moved slots: the CSR is rebuilt
        code, sel, fres = be.fuse("fuse_%d" % j, K, target, into)
        did("fuse_%d" % j, code=code, refresh_sel=sel, result=fres)
        if tags is not None and code is not None:
            sc = notes["fuse_in"]
            if j and any(p in changed or o in changed for p, o in notes["replace_pairs"]):
                tags.setdefault("second_target_hits_changed_row", K)
            changed |= {int(x) for x in sel if x >= 0}
            gone = set(np.flatnonzero((sc["valid"] != 0) & (s["valid"] == 0)).tolist())
            now_recent = set(s["recent"][:s["n_recent"]].tolist())
            if gone & now_recent:
                tags.setdefault("fuse_replaces_recent_row", K)
                fused |= gone & now_recent
    did("build3", result=be.build("build3"))
    did("refresh2", result=be.refresh("refresh2", ("slots", K), kf_self=K))            # :304-315
    did("update2", result=be.update("update2", K))
    if tags is not None and notes["rebuilt_now"] & lost:                   # K and j both existed before this update
        tags.setdefault("reconnect_after_erase", K)
    local, n_local = be.connected(K)
    did("connected", local=local, n_local=n_local)
    head = did("ba_problem", result=be.ba_problem())["result"]            # Optimize::localBundleAdjustment; the 32-byte read-back
    if not head[lbm.P_REFUSED]:
        est = be.ba_solve()
        did("ba_solve", est_pose_R=est[0], est_pose_t=est[1], est_points=est[2], outlier=est[3])
        did("ba_apply", result=be.ba_apply())
        if tags is not None and notes["ba_killed"] & set(s["recent"][:s["n_recent"]].tolist()):
            tags.setdefault("ba_outlier_kills_recent_row", K)
        did("build4", result=be.build("build4"))
        did("refresh3", result=be.refresh("refresh3", ("point_row",)))
    if tags is not None:
        for name, tag in (("build", "csr_overflow"), ("build2", "csr_overflow"), ("build3", "csr_overflow_late")):
            if dict(log)[name]["result"][om.OVERFLOW]:
                tags.setdefault(tag, K)
    alive = [k for k in range(K + 1) if k not in s["dead_kfs"]]            # KeyFrameCulling, :318-372: getRecentKeyFrames(25), oldest first
    ts = [float(world.timestamps[k]) for k in alive]
    code, num_mp, num_red, cres = be.cull_keyframes(alive, ts)
    did("cull_keyframes", code=code, num_mp=num_mp, num_redundant=num_red, result=cres)
    if tags is not None and cres[om.CULLED]:
        (ref0, slots0), out = notes["kf_cull"]
        culled = [c for c, x in zip(alive, code) if x == 3]
        others = [k for k in range(s["n_kf"]) if k not in culled]
        if cres[om.REASSIGNED] and cres[om.CLEARED] and (out["slots"][others] != slots0[others]).any() and (out["ref_kf"] != ref0).any():
            tags.setdefault("kf_cull_cascade", K)
    did("erase", result=be.erase(alive, code))
    if notes is not None:
        lost |= notes["lost_connection"]
    s["dead_kfs"] = s["dead_kfs"] + [c for c, x in zip(alive, be.host(code)) if x == 3]   # Map::eraseKeyFrame, replayed from d_code behind the wait
    return log


def step_arrays(s, frame, world, ba=ba_reference, triangulate=triangulate_float32, addr=None, **kw):
    """one mapper step as the composition of the array models; s is changed in place.  -> the list of (call, outputs)"""
    return step(ArrayBackend(s, ba, triangulate, addr), frame, world, **kw)


# ---- the map a session starts from ------------------------------------------------------------------------------------------------------------------
def initial_frames(world):
    """-> (the two frames that become key frames 0 and 1, the world points both see, their table positions: true places plus 2 cm)"""
    rng = np.random.RandomState(world.cfg["seed"] + 77)
    f0, f1 = world.features[0], world.features[1]
    in1 = set(f1["point"].tolist())
    common = [int(q) for q in f0["point"] if q >= 0 and q in in1][:min(70, world.cfg["cap_points"] - 8)]
    m = len(common)
    frames = []
    for k, f in ((0, f0), (1, f1)):
        where = {int(q): i for i, q in enumerate(f["point"])}
        mp = np.full(len(f["point"]), -1, np.int32)
        mp[[where[q] for q in common]] = np.arange(m)
        R, t = world.poses[k]
        frames.append(Frame(K=k, mp=mp, R=R.reshape(9), t=t.copy(), kps=f["kps"], desc=f["desc"], cell_start=f["cell_start"], cell_items=f["cell_items"],
                            fv=f["fv"], n2=len(mp)))
    return frames, common, (world.P[common] + rng.normal(0, 0.02, (m, 3))).astype(np.float32)


def initial_state(world, addr=None):
    """Tracking::createInitialMap's outcome, stated with the models: key frames 0 and 1 observe the points both see, every such row
    valid, registered and listed in recent; the lists built, the rows refreshed, the two key frames connected."""
    s = empty_state(world.cfg, world.cam, world.bounds, world.scale_table)
    frames, common, positions = initial_frames(world)
    m = len(common)
    s["points"][:m], s["valid"][:m] = positions, 1
    be = ArrayBackend(s, addr=addr)
    for fr in frames:
        be.insert(fr)
    s["ref_kf"][:m], s["first_kf"][:m], s["found"][:m], s["visible"][:m] = 0, 0, 1, 1
    s["recent"][:m], s["n_recent"], s["n_points"], s["n_registered"] = np.arange(m), m, m, m
    be.build()
    for k in (0, 1):
        be.refresh("refresh", ("slots", k), kf_self=k)
        be.update("update", k)
    return s


def run_session(name, ba=ba_reference, triangulate=triangulate_float32, world=None, each=None):
    """the whole session on the array models.  each(K, frame, before, state, log): called behind every key frame.
    -> dict(world, state, tags: event -> key frame, logs)"""
    world = world or World(name)
    s = initial_state(world)
    seen = [copy_state(s), copy_state(s)]                                  # the table as the tracker saw it: one step behind
    tags, memo, logs = {}, {}, []
    for K in range(2, world.cfg["n_kf"]):
        frame = world.frame(K, seen[-2])
        before = copy_state(s) if each else None
        log = step_arrays(s, frame, world, ba, triangulate, tags=tags, memo=memo)
        logs.append(log)
        seen.append(copy_state(s))
        if each:
            each(K, frame, before, s, log)
    return dict(world=world, state=s, tags=tags, logs=logs)


# ---- the same session on objects ------------------------------------------------------------------------------------------------------------------
# LocalMapping::run (LocalMapping.cpp:47-91) on KeyFrame / MapPoint objects: who observes whom, who is bad, who refers to whom, who is
# connected to whom.  The objects own the STRUCTURE of the map.  The numbers -- a point's position, normal, range and descriptor where
# the fuse projects it, and the bundle adjustment's estimate -- are handed over by identity (row, key frame) from the array session's
# call of the same name: a restatement of their float arithmetic exists already (refresh_model, oracle/ba_ref.py) and is not repeated.
# The objects PERSIST from key frame to key frame: that is the point of a session.  The models' own object twins (fuse_model.apply_objects,
# local_ba_model.problem_objects / apply_objects, observations_model.cull_objects) build their objects afresh from the slot arrays at
# every call, so composing them would carry the map from call to call in the arrays and test nothing the array session does not.  What
# composes without that is used as it is: keyframe_model's MapPoint, process_new_key_frame and map_point_culling, graph_model's KeyFrame
# (updateConnections, setBad's graph and tree) and search_in_neighbors; the fuse loop, the BA's structure and tail and KeyFrameCulling are
# stated here on the persistent objects, each a few lines beside the reference lines it cites.
class ObjectMap:
    def __init__(self):
        self.erased_points, self.erased_kfs = [], []

    def erase_map_point(self, mp):                                         # Map::eraseMapPoint
        self.erased_points.append(mp.row)

    def erase_key_frame(self, kf):                                         # Map::eraseKeyFrame
        self.erased_kfs.append(kf.id)


class SessionPoint(km.MapPoint):
    def __getitem__(self, i):
        """(table row, not bad): the shape graph_model.search_in_neighbors reads a key frame's map points in"""
        return (self.row, int(not self.is_bad))[i]

    def observes(self, kf):
        return kf in self.observations

    def erase_observation(self, kf):                                       # MapPoint.cpp:190-208
        if kf not in self.observations:
            return
        del self.observations[kf]
        if self.reference_kf is kf and self.observations:
            self.reference_kf = min(self.observations, key=lambda k: k.slot)   # observations.begin(), in the header's order
        if self.get_num_obs() <= 2:
            self.set_bad()

    def replace(self, other):                                              # MapPoint.cpp:233-264
        if other is self:
            return
        obs, self.observations, self.is_bad = self.observations, {}, True
        for kf in sorted(obs, key=lambda k: k.slot):
            if not other.observes(kf):
                kf.map_points[obs[kf]] = other                             # KeyFrame::addMapPoint
                other.add_observation(kf, obs[kf])
            else:
                kf.map_points[obs[kf]] = None                              # KeyFrame::eraseMapPoint
        other.num_found += self.num_found                                  # increaseFound(numFound)
        other.num_found += self.num_visible                                # increaseFound(numVisible): the reference's text
        self.point_map.erase_map_point(self)


class SessionKeyFrame(gm.KeyFrame):
    def __init__(self, k, frame, mps):                                     # KeyFrame.cpp:15-25
        gm.KeyFrame.__init__(self, k)
        self.slot, self.num_kps = k, len(frame.mp)
        self.kps, self.descriptors, self.fv = frame.kps, frame.desc, frame.fv
        self.R, self.t = np.array(frame.R, np.float64).reshape(9), np.array(frame.t, np.float64)
        self.map_points = [mps[p] if 0 <= p < len(mps) else None for p in frame.mp.tolist()]

    def erase_map_point(self, i):
        self.map_points[i] = None

    def set_bad_all(self, object_map):                                     # KeyFrame.cpp:402-467
        for mp in list(self.map_points):
            if mp is not None:
                mp.erase_observation(self)
        gm.KeyFrame.set_bad(self)                                          # the graph and the spanning tree
        self.map_points = [None] * self.num_kps
        object_map.erase_key_frame(self)


def _update_connections(kf):
    """KeyFrame.cpp:225-242: the counting loop, then graph_model's restatement of the rest"""
    counter = {}
    for mp in kf.map_points:
        if mp is None or mp.is_bad:
            continue
        for other in mp.observations:
            if other is not kf:
                counter[other] = counter.get(other, 0) + 1
    kf.update_connections(counter, FIRST_KF)


def initial_objects(world):
    """the objects of initial_state's map"""
    frames, common, _ = initial_frames(world)
    ow = dict(world=world, kfs=[], mps=[], recent=[], map=ObjectMap(), dead=[])
    ow["mps"] = [SessionPoint(p, False, ow["map"]) for p in range(len(common))]
    for fr in frames:
        kf = SessionKeyFrame(fr.K, fr, ow["mps"])
        ow["kfs"].append(kf)
        km.process_new_key_frame(kf)
    for mp in ow["mps"]:
        mp.reference_kf, mp.first_kf_id, mp.num_found, mp.num_visible = ow["kfs"][0], 0, 1, 1
        ow["recent"].append(mp)
    for kf in ow["kfs"]:
        _update_connections(kf)
    return ow


def fuse_queries(oracle, cam, bounds, R, t, floats, mask, kps, desc):
    """ORBMatcher.cpp:536-575 for the rows of `mask`: the builder's gates and the window search -> the hit key point per table row"""
    q = pm.evaluate(pm.FUSE, cam, bounds, R, t, floats["points"], mask, normals=floats["normals"], min_dist=floats["min_dist"], max_dist=floats["max_dist"],
                    th=FUSE_TH)
    return oracle.search_fuse(floats["desc"], q["q_xy"], q["q_radius"], q["q_level"], q["q_ok"], kps, desc, W, H, SIGMA2)[0]


def _fuse_objects(ow, target, plist, floats):
    """the static SearchByProjection(keyFrame, mapPoints, Map*, th), ORBMatcher.cpp:524-592, over plist in its order"""
    world = ow["world"]
    mask = np.zeros(world.cfg["cap_points"], np.uint8)
    mask[[mp.row for mp in plist if not mp.is_bad]] = 1
    best = fuse_queries(world.oracle, world.cam, world.bounds, target.R, target.t, floats, mask, target.kps, target.descriptors)
    for mp in plist:
        s = int(best[mp.row])
        if s < 0 or mp.is_bad or mp.observes(target):                      # :534
            continue
        held = target.map_points[s]
        if held is None:                                                   # :576-578
            mp.add_observation(target, s)
            target.map_points[s] = mp
        elif not held.is_bad:                                              # :579-586
            if held.get_num_obs() > mp.get_num_obs():
                mp.replace(held)
            else:
                held.replace(mp)


def step_objects(ow, frame, numbers):
    """one mapper step on the objects.  numbers: dict(floats: the table's float columns and descriptors as the array session holds them
    when the fuse begins; prob, est: the array session's BA problem and estimate, None when the assembly refused).
    -> dict(local, points, fixed, edges: the BA's structure as the objects see it, None when there is no edge)"""
    world, kfs, mps, recent, omap = ow["world"], ow["kfs"], ow["mps"], ow["recent"], ow["map"]
    K = frame.K
    for row in np.flatnonzero(frame.d_visible):                            # the tracker since the last key frame: increaseVisible / increaseFound
        mps[row].num_visible += int(frame.d_visible[row])
        mps[row].num_found += int(frame.d_found[row])
    kf = SessionKeyFrame(K, frame, mps)                                    # processNewKeyFrame, LocalMapping.cpp:93-105
    kfs.append(kf)
    km.process_new_key_frame(kf)
    _update_connections(kf)
    km.map_point_culling(recent, kf)                                       # :117-144
    for nb in [kfs[k] for k in range(K - 1, -1, -1) if k not in ow["dead"]][:N_NEIGHBOURS]:   # createNewMapPoints, :146-259
        has1 = np.array([mp is not None for mp in nb.map_points], np.uint8)
        has2 = np.array([mp is not None for mp in kf.map_points], np.uint8)
        _, m12 = world.oracle.search_for_triangulation(False, nb.descriptors, nb.kps["angle"], has1, nb.fv, kf.descriptors, kf.kps["angle"], has2, kf.fv)
        e = tm.evaluate(world.cam, world.scale_table, nb.R, nb.t, kf.R, kf.t, nb.kps, kf.kps, kf.descriptors, m12, n_points=len(mps))
        for i, m in zip(e["feat1"].tolist(), e["feat2"].tolist()):         # :243-248
            mp = SessionPoint.construct(len(mps), nb, kf, (i, m), omap)
            nb.map_points[i] = kf.map_points[m] = mp
            recent.append(mp)
            mps.append(mp)
    marks = [len(omap.erased_points)]                                      # Map::eraseMapPoint so far: MapPointCulling's part ends here
    target_ids, candidate_rows = gm.search_in_neighbors(kfs, kf, K)       # searchInNeighbors, :261-300
    targets, candidates = [kfs[k] for k in target_ids], [mps[p] for p in candidate_rows]
    floats = numbers["floats"]
    for target in targets:                                                 # the builder numbers its queries by table row: ascending rows
        _fuse_objects(ow, target, sorted((mp for mp in kf.map_points if mp is not None), key=lambda mp: mp.row), floats)
        marks.append(len(omap.erased_points))
    _fuse_objects(ow, kf, candidates, floats)
    marks.append(len(omap.erased_points))
    _update_connections(kf)
    local = [kf] + [k2 for k2 in kf.ordered_connected_kfs if not k2.is_bad]   # Optimize::localBundleAdjustment, Optimize.cpp:766-806
    points, marked = [], set()
    for lk in local:
        for mp in lk.map_points:
            if mp is not None and not mp.is_bad and mp.row not in marked:
                marked.add(mp.row)
                points.append(mp)
    fixed = {k2.id for mp in points for k2 in mp.observations if k2 not in local and not k2.is_bad}
    edges = {(k2.id, mp.row, i) for mp in points for k2, i in mp.observations.items() if not k2.is_bad}
    structure = dict(local=[k2.id for k2 in local], points=[mp.row for mp in points], fixed=fixed, edges=edges) if edges else None   # `erased` joins it below
    prob, est = numbers["prob"], numbers["est"]
    if est is not None:                                                    # the tail, :914-950, with the estimate handed over by identity
        for j in np.flatnonzero(est[3]):
            k2, mp = kfs[int(prob["edge_kf"][j])], mps[int(prob["point_row"][prob["edge_point"][j]])]
            if mp.is_bad:
                continue
            k2.erase_map_point(mp.observations[k2])
            mp.erase_observation(k2)
        for q in range(int(prob["result"][lbm.P_LOCAL])):
            k2 = kfs[int(prob["pose_kf"][q])]
            k2.R, k2.t = est[0][q].reshape(9).astype(np.float32).astype(np.float64), est[1][q].astype(np.float32).astype(np.float64)
    marks.append(len(omap.erased_points))
    alive = [kfs[k] for k in range(K + 1) if k not in ow["dead"]]          # KeyFrameCulling, :318-372
    last = 0
    for idx in range(1, len(alive) - 1):
        c = alive[idx]
        if c.id == FIRST_KF or world.timestamps[alive[idx + 1].id] - world.timestamps[alive[last].id] > om.MAX_GAP:
            continue
        count = redundant = 0
        for i, mp in enumerate(c.map_points):
            if mp is None or mp.is_bad:
                continue
            count += 1
            if mp.get_num_obs() > om.TH_OBS:
                level, seen_by = int(c.kps["octave"][i]), 0
                for k2 in sorted(mp.observations, key=lambda k: k.slot):
                    if k2 is not c and int(k2.kps["octave"][mp.observations[k2]]) <= level + 1:
                        seen_by += 1
                        if seen_by >= om.TH_OBS:
                            break
                redundant += seen_by >= om.TH_OBS
        if redundant > om.RATIO * count:
            c.set_bad_all(omap)
            ow["dead"].append(c.id)
        else:
            last = idx
    marks.append(len(omap.erased_points))
    erased, start = [], ow.get("erased_before", 0)
    for name, end in zip(["cull_map_points"] + ["fuse_%d" % j for j in range(len(targets) + 1)] + ["ba_apply", "cull_keyframes"], marks):
        erased.append((name, omap.erased_points[start:end]))
        start = end
    ow["erased_before"] = start
    if structure is not None:
        structure["erased"] = erased
    return structure if structure is not None else dict(erased=erased, edges=None)


def replays_differ(erased, replays):
    """Map::eraseMapPoint as the objects made the calls, against its replay from the array session's codes: call by call and IN ORDER where
    the call has a code per row (MapPointCulling's d_code 2 / 3, the fuse's 5 / 6 with its loser); as sets where it has none (the BA
    apply's outlier handling and the key-frame cull's cascade: d_valid before and after is all the caller has)"""
    want, bad = dict(replays), []
    for name, rows in erased:
        w = want.pop(name, [] if name.startswith(("cull_map", "fuse")) else set())
        if (set(rows) != w or len(set(rows)) != len(rows)) if isinstance(w, set) else (rows != w):
            bad.append("Map::eraseMapPoint behind %s: the objects %s, the codes %s" % (name, rows, sorted(w) if isinstance(w, set) else w))
    return bad + ["a replay without a call of the objects: %s" % n for n, w in want.items() if len(w)]


def objects_describe_the_arrays(ow, s, prob=None, structure=None, replays=None):
    """-> the list of differences between the map the objects hold and the map the arrays hold (empty: the same map)"""
    kfs, mps, t, bad = ow["kfs"], ow["mps"], s["table"], []
    if len(kfs) != s["n_kf"] or len(mps) != s["n_points"]:
        return ["%d key frames and %d points against %d and %d" % (len(kfs), len(mps), s["n_kf"], s["n_points"])]
    for k, kf in enumerate(kfs):
        if bool(kf.is_bad) != bool(t["bad"][k]):
            bad.append("key frame %d bad: %s against %d" % (k, kf.is_bad, t["bad"][k]))
        want = [mp.row if mp is not None else -1 for mp in kf.map_points]
        if want != t["slots"][k, :kf.num_kps].tolist():
            bad.append("the slots of key frame %d" % k)
    observed = {}
    for k in range(s["n_kf"]):
        if not t["bad"][k]:
            for i in range(int(t["n"][k])):
                if t["slots"][k, i] >= 0:
                    observed.setdefault(int(t["slots"][k, i]), set()).add((k, i))
    for p, mp in enumerate(mps):
        if bool(mp.is_bad) == bool(s["valid"][p]):
            bad.append("row %d bad: %s against valid %d" % (p, mp.is_bad, s["valid"][p]))
        elif not mp.is_bad:
            if {(kf.id, i) for kf, i in mp.observations.items()} != observed.get(p, set()):
                bad.append("the observations of row %d" % p)
            if mp.reference_kf.id != s["ref_kf"][p]:
                bad.append("ref_kf of row %d: %d against %d" % (p, mp.reference_kf.id, s["ref_kf"][p]))
            if (mp.first_kf_id, mp.num_found, mp.num_visible) != (s["first_kf"][p], s["found"][p], s["visible"][p]):
                bad.append("first_kf / found / visible of row %d" % p)
    if [mp.row for mp in ow["recent"]] != s["recent"][:s["n_recent"]].tolist():
        bad.append("the recent list")
    try:
        gm.objects_equal_arrays(kfs, s["graph"], s["n_kf"], t["bad"])
    except AssertionError as e:
        bad.append("the covisibility graph at key frame %s" % (e.args,))
    if sorted(ow["dead"]) != sorted(s["dead_kfs"]) or ow["map"].erased_kfs != s["dead_kfs"]:
        bad.append("Map::eraseKeyFrame: %s against %s" % (ow["map"].erased_kfs, s["dead_kfs"]))
    if sorted(set(ow["map"].erased_points)) != np.flatnonzero(s["valid"][:s["n_points"]] == 0).tolist() or len(set(ow["map"].erased_points)) != len(ow["map"].erased_points):
        bad.append("Map::eraseMapPoint")
    if replays is not None:
        bad += replays_differ(structure["erased"], replays)
    if structure is not None and structure.get("edges") is not None and prob is not None and prob["point_row"] is not None:
        n_local = int(prob["result"][lbm.P_LOCAL])
        edges = {(int(k), int(prob["point_row"][x]), int(i)) for k, x, i in zip(prob["edge_kf"], prob["edge_point"], prob["edge_kp"])}
        if structure["local"] != prob["pose_kf"][:n_local].tolist() or structure["fixed"] != set(prob["pose_kf"][n_local:].tolist()):
            bad.append("the local BA's key frames")
        if structure["points"] != prob["point_row"].tolist() or structure["edges"] != edges:
            bad.append("the local BA's points and edges")
    return bad
