"""Plain numpy / Python restatement of include/orbm.h, "The inertial local BA window on the device-resident map", twice:
  problem          the ARRAY form the header states (slot arrays, CSR, liveness, first[] and the inclusive X of the cap), the model the
                   device is compared with, built on the helpers of observations_model / local_ba_model
  problem_objects  an independent OBJECT-style restatement of the reference: steps 1 and 3 of Optimize::localFullBundleAdjustment
                   (Optimize.cpp:1073-1108, :1129-1244) with BA_local_for_kf / BA_fixed_for_kf marks on MapPoint / KeyFrame objects, the
                   `break` at maxNumFixed, and step 7's chaining (:1274-1299); a point's observations iterated in ascending key-frame slot
velocity_prior, the remainder of step 7, and the seeded scenes the test files use.  No part of the library is used here."""
import numpy as np

import local_ba_model as lm
import observations_model as om
from projection_model import KP_DTYPE, SCALE_FACTORS

MAX_SOLVE, MAX_FIXED_DEFAULT, MAX_OBS = 32, 150, 256
(W_STATES, W_POINTS, W_EDGES, W_SOLVE, W_FIXED, W_REFUSED, W_WINDOW_UNUSABLE, W_IMU_RANGE, W_NO_EDGE, W_SECOND, W_CSR_DROPPED, W_CAPPED, W_LONG,
 W_CANDIDATES) = range(14)
REFUSE_STATES, REFUSE_POINTS, REFUSE_EDGES, REFUSE_WINDOW, REFUSE_NO_EDGE, REFUSE_IMU = 1, 2, 4, 8, 16, 32
FIX_ALL, EDGE_WALKS, PRIOR_ALL, RECOVER_POSE = 15, 1, 15, 1             # orbi_factors.h: ORBI_FIX_* | .., ORBI_EDGE_WALKS, ORBI_PRIOR_* | .., ORBI_RECOVER_POSE
VISUAL_OUT = ("ba_points", "point_row", "edge_off", "edge_state", "edge_point", "edge_z", "edge_inv_sigma2", "edge_kf", "edge_kp", "state_kf")
INERTIAL_OUT = ("init_jobs", "fixed", "inertial_edges", "prior_jobs", "recover_jobs", "bias_ids", "prior_info_jobs")
OUT = VISUAL_OUT + INERTIAL_OUT


# ---- the array form -----------------------------------------------------------------------------------------------------------
def problem(sc, csr, cap_states=1 << 20, cap_local_points=1 << 20, cap_edges=1 << 20, inclusive=True):
    """sc: the scene of local_ba_model (n, bad, slots, stride, valid, points, cap_points, kps) with window i32 [n_window] (oldest first),
    kf_imu i32 [n_kf, 3], n_src, cap_bank, n_priors, max_fixed.  -> dict of the output arrays cut to the counts (None when refused),
    result i32 [16], and `first`: first[f] per key frame that could be fixed, by point order (not an output).  inclusive=False: the WRONG cap, with
    X exclusive, for the test that shows the scenes tell the two apart."""
    n_kf, cap = len(sc["n"]), sc["cap_points"]
    window, imu = [int(k) for k in sc["window"]], np.asarray(sc["kf_imu"]).reshape(-1, 3)
    st = lm._state(sc, csr)
    result = np.zeros(16, np.int32)
    out = dict(result=result, **{k: None for k in OUT})
    unusable = [pos for pos, k in enumerate(window) if not 0 <= k < n_kf or sc["bad"][k] or k in window[:pos]]
    result[W_STATES] = result[W_SOLVE] = len(window)
    if unusable:
        result[W_REFUSED], result[W_WINDOW_UNUSABLE] = REFUSE_WINDOW, len(unusable)
        return out
    result[W_CSR_DROPPED] = lm._csr_dropped(st)

    def imu_ok(k, fields):
        return all(0 <= imu[k][c] < (sc["n_src"], sc["cap_bank"], sc["n_priors"])[c] for c in fields)

    imu_range = sum(not imu_ok(k, (0, 1, 2)) for k in window)
    # local rows at their first occurrence, with their live entries
    seen, local = set(), []
    for k in window:
        for i in range(lm._n_slots(sc, k)):
            p = int(sc["slots"][k, i])
            if p < 0 or p >= cap or not sc["valid"][p] or p in seen:
                continue
            seen.add(p)
            local.append((p, lm._live_entries(st, p)))
    # first[f]: the smallest number (here: the position in `local`, which orders the rows as every numbering does) observing f
    first = {}
    for number, (p, entries) in enumerate(local):
        for k, _ in entries:
            if k not in window:
                first.setdefault(k, number)
    result[W_CANDIDATES] = len(first)
    if len(first) >= sc["max_fixed"]:
        X = sorted(first.values())[sc["max_fixed"] - 1]              # the smallest X with #{f : first[f] <= X} >= max_fixed
        fixed = sorted(f for f, x in first.items() if (x <= X if inclusive else x < X))
    else:
        fixed = sorted(first)
    imu_range += sum(not imu_ok(k, (0,)) for k in fixed)
    state_kf = window + fixed
    state_of = {k: q for q, k in enumerate(state_kf)}
    rows, edges = [], []
    for p, entries in local:
        mine, have = [], set()
        for k, i in entries:
            if k in have:
                result[W_SECOND] += 1
                continue
            have.add(k)
            if k not in state_of:
                result[W_CAPPED] += 1
                continue
            mine.append((k, i))
        if not mine:
            result[W_NO_EDGE] += 1
            continue
        result[W_LONG] += len(mine) > MAX_OBS
        rows.append(p)
        edges.append(mine)
    n_edges, n_solve = sum(len(m) for m in edges), len(window)
    result[[W_STATES, W_POINTS, W_EDGES, W_FIXED, W_IMU_RANGE]] = len(state_kf), len(rows), n_edges, len(fixed), imu_range
    result[W_REFUSED] = (REFUSE_STATES * (len(state_kf) > cap_states) | REFUSE_POINTS * (len(rows) > cap_local_points)
                         | REFUSE_EDGES * (n_edges > cap_edges) | REFUSE_NO_EDGE * (n_edges < 1) | REFUSE_IMU * (imu_range > 0))
    out["first"] = first
    if result[W_REFUSED]:
        return out
    flat = [(k, i, x) for x, mine in enumerate(edges) for k, i in mine]
    kp = [sc["kps"][k][i] for k, i, _ in flat]
    size, one = np.array([r["size"] for r in kp], np.float32), np.float32(1)
    i32 = lambda v, shape=(-1,): np.array(v, np.int32).reshape(shape)  # noqa: E731
    row, rec, prior = (lambda k: int(imu[k][0])), (lambda k: int(imu[k][1])), (lambda k: int(imu[k][2]))
    out.update(
        ba_points=sc["points"][rows].astype(np.float64), point_row=i32(rows),
        edge_off=np.concatenate([[0], np.cumsum([len(m) for m in edges])]).astype(np.int32),
        edge_state=i32([state_of[e[0]] for e in flat]), edge_point=i32([e[2] for e in flat]),
        edge_z=np.array([[r["x"], r["y"]] for r in kp], np.float32).astype(np.float64).reshape(-1, 2),
        edge_inv_sigma2=((one / size) / size).astype(np.float64), edge_kf=i32([e[0] for e in flat]), edge_kp=i32([e[1] for e in flat]),
        state_kf=i32(state_kf),
        init_jobs=i32([(q, row(k), rec(k) if q < n_solve else -1) for q, k in enumerate(state_kf)], (-1, 3)),
        fixed=np.array([0 if q < n_solve else FIX_ALL for q in range(len(state_kf))], np.uint8),
        inertial_edges=i32([(s, s + 1, rec(window[s]), EDGE_WALKS) for s in range(n_solve - 1)], (-1, 4)),
        prior_jobs=i32([(0, prior(window[0]), PRIOR_ALL)], (-1, 3)),
        recover_jobs=i32([(s, row(window[s]), RECOVER_POSE) for s in range(n_solve)], (-1, 3)),
        bias_ids=i32([rec(k) for k in window]),
        prior_info_jobs=i32([(prior(window[s]), rec(window[s - 1]), row(window[s])) for s in range(1, n_solve)], (-1, 3)))
    return out


def velocity_prior(priors, src, recover_jobs, prior_jobs):
    """orbm_inertial_window_velocity_prior_device: priors f32 [n_priors, 36] (orbi_prior), src f32 [n_src, 15] -> (priors after, result i32 [8])"""
    priors, result = priors.copy(), np.zeros(8, np.int32)
    row, slot = int(np.asarray(recover_jobs).reshape(-1)[1]), int(np.asarray(prior_jobs).reshape(-1)[1])
    if 0 <= row < len(src) and 0 <= slot < len(priors):
        priors[slot, 0:3] = src[row, 12:15]
        result[0] = 1
    else:
        result[1] = 1
    return priors, result


# ---- the object form ----------------------------------------------------------------------------------------------------------
def problem_objects(sc):
    """Optimize.cpp:1073-1108, :1129-1244 and the chaining of :1274-1299 on objects; for scenes whose CSR is fresh and whose window is
    usable.  -> dict(solve, fixed (in the order the reference meets them), rows, edges (per row its (key frame, feature)), null (edges
    the reference hands a null vertex), and the inertial side as the reference builds it: inertial (i, j, key frame whose pre-integrator),
    priors (key frame), chain (key frame, key frame whose C and new bias))"""
    world = lm._objects(sc)
    kfs, max_fixed = world["kfs"], sc["max_fixed"]
    optimize = [kfs[int(k)] for k in sc["window"]]                        # getRecentKeyFrames(numOpt)
    for kf in optimize:
        kf.ba_local = True
    points = []
    for kf in optimize:
        for mp in kf.map_points:
            if mp is not None and not mp.is_bad and not mp.ba_local:
                points.append(mp)
                mp.ba_local = True
    fixed = []
    for mp in points:
        for k in sorted(mp.observations):
            kf = kfs[k]
            if not kf.is_bad and not kf.ba_local and not kf.ba_fixed:
                fixed.append(kf)
                kf.ba_fixed = True
        if len(fixed) >= max_fixed:
            break
    num_opt = len(optimize)
    vertex = {}                                                            # optimizer.vertex(kf->id)
    inertial, priors = [], []
    for i in range(num_opt - 1, -1, -1):
        kf = optimize[i]
        vertex[kf.k] = i
        if i < num_opt - 1:
            inertial.append((i, i + 1, kf.k))                              # EdgeInertial(kf->pre_integrator), vertices of kf and of vPose2
        if i == 0:
            priors.append(kf.k)
    for q, kf in enumerate(fixed):
        vertex[kf.k] = num_opt + q
    rows, edges, null = [], [], 0
    for mp in points:
        mine = []
        for k in sorted(mp.observations):
            if kfs[k].is_bad:
                continue
            if k not in vertex:                                            # optimizer.vertex() == nullptr: g2o takes no such edge
                null += 1
                continue
            mine.append((k, mp.observations[k][0]))
        if mine:                                                           # a vertex without an edge is not part of the optimisation
            rows.append(mp.row)
            edges.append(mine)
    chain = [(optimize[i].k, optimize[i - 1].k) for i in range(1, num_opt)]   # :1293-1296
    return dict(solve=[kf.k for kf in optimize], fixed=[kf.k for kf in fixed], rows=rows, edges=edges, null=null, inertial=sorted(inertial),
                priors=priors, chain=chain)


# ---- a loop scene laid out as a map, and the tail behind the loop ------------------------------------------------------------------
def map_from_window_scene(ws, seed=3):
    """vw_model.window_scene (states, points, edges) laid out as what the assembly reads: key frames in shuffled slots (the fixed states'
    ascending, as the assembly orders them) with two more that see nothing, a slot and an orbx_kp record per edge, table rows in shuffled
    order, state rows, records and prior slots behind d_kf_imu.  The fixed states' poses become the float rows' values widened, as
    orbi_graph_init_device would leave them.  -> the map scene; ["ws"] is the window scene with that graph, ["kf_of_state"],
    ["row_of_point"], ["src"] f32 [n_src, 15], ["priors"] (factors_model.PRIOR [n_priors]) say where everything went."""
    import factors_model as fm
    rng = np.random.RandomState(seed)
    ns, nf, n_points, ne = ws["n_solve"], ws["n_fixed"], ws["n_points"], len(ws["edge_state"])
    n_states, n_kf = ns + nf, ns + nf + 2
    order = [int(k) for k in rng.permutation(n_kf)]
    kf_of_state = order[:ns] + sorted(order[ns:n_states])
    stride, cap = n_points + 8, n_points + 10
    row_of_point = rng.permutation(cap)[:n_points]
    slots = np.full((n_kf, stride), -1, np.int32)
    free = [[int(i) for i in rng.permutation(stride)] for _ in range(n_kf)]
    sizes = [np.float32(31.0) * np.float32(1.2) ** np.float32(r) for r in range(8)]
    kps = [np.zeros(stride, KP_DTYPE) for _ in range(n_kf)]
    for kp in kps:
        kp["size"], kp["class_id"] = sizes[0], -1
    for e in range(ne):
        k, i = kf_of_state[int(ws["edge_state"][e])], None
        i = free[k].pop()
        slots[k, i] = row_of_point[int(ws["edge_point"][e])]
        octave = [r for r, size in enumerate(sizes) if np.float64((np.float32(1) / size) / size) == ws["w"][e]]
        assert octave, "the scene's weight is 1 / size^2 of one of its eight sizes"
        kps[k]["x"][i], kps[k]["y"][i], kps[k]["size"][i], kps[k]["octave"][i] = ws["z"][e, 0], ws["z"][e, 1], sizes[octave[0]], octave[0]
        assert np.float64(kps[k]["x"][i]) == ws["z"][e, 0] and np.float64(kps[k]["y"][i]) == ws["z"][e, 1]
    points = rng.uniform(-9, 9, (cap + 4, 3)).astype(np.float32)
    points[row_of_point] = ws["points"].astype(np.float32)
    assert (points[row_of_point].astype(np.float64) == ws["points"]).all()
    valid = np.zeros(cap + 4, np.uint8)
    valid[row_of_point] = 1
    ref_kf = np.zeros(cap + 4, np.int32)
    for e in range(ne - 1, -1, -1):
        ref_kf[row_of_point[int(ws["edge_point"][e])]] = kf_of_state[int(ws["edge_state"][e])]
    g = ws["graph"].copy()
    n_src, n_priors = n_states + 1, ns + 1
    row_of_state, prior_of_state = rng.permutation(n_src)[:n_states], rng.permutation(n_priors)[:ns]
    src = rng.uniform(-1, 1, (n_src, 15)).astype(np.float32)
    for q in range(n_states):
        if q < ns:
            src[row_of_state[q]] = ws["src"][q]
        else:
            src[row_of_state[q]] = np.concatenate([g.Rwb[q].reshape(9), g.twb[q], np.zeros(3)]).astype(np.float32)
            g.Rwb[q], g.twb[q] = src[row_of_state[q], :9].astype(np.float64).reshape(3, 3), src[row_of_state[q], 9:12].astype(np.float64)
    kf_imu = np.full((n_kf, 3), -1, np.int32)
    for q in range(n_states):
        kf_imu[kf_of_state[q]] = (row_of_state[q], q, prior_of_state[q]) if q < ns else (row_of_state[q], -1, -1)
    priors = np.frombuffer(rng.randint(0, 255, n_priors * fm.PRIOR.itemsize).astype(np.uint8).tobytes(), fm.PRIOR).copy()
    for name in fm.PRIOR.names:                                          # floats a model can copy: no NaN among them
        priors[name] = rng.uniform(-1, 1, priors[name].shape)
    priors[prior_of_state[0]] = ws["priors"][0]
    import vi_model as vm
    pose_R, pose_t = np.tile(np.eye(3).reshape(9), (n_kf, 1)), np.zeros((n_kf, 3))     # T_cw of the table, floats widened as KeyFrame holds them
    for q in range(n_states):
        Rcw, tcw = vm.derive_pose(ws["cal"], g.Rwb[q], g.twb[q])[:2]
        pose_R[kf_of_state[q]], pose_t[kf_of_state[q]] = Rcw.reshape(9).astype(np.float32), np.asarray(tcw).astype(np.float32)
    return dict(n=np.full(n_kf, stride, np.int32), bad=np.zeros(n_kf, np.uint8), slots=slots, stride=stride, valid=valid, points=points, cap_points=cap,
                kps=kps, ref_kf=ref_kf, pose_R=pose_R, pose_t=pose_t, window=np.array(kf_of_state[:ns], np.int32), kf_imu=kf_imu, n_src=n_src,
                cap_bank=len(ws["recs"]), n_priors=n_priors, max_fixed=MAX_FIXED_DEFAULT, src=src, priors=priors, ws=dict(ws, graph=g),
                kf_of_state=kf_of_state, row_of_point=row_of_point)


def window_scene_of(sc, a):
    """the window scene the assembly `a` of the map `sc` describes, for the model back-ends of tests/inertial_loop.py: the laid-out scene
    with points and edges in the assembly's order and the inertial side from its job lists"""
    import factors_model as fm
    ws = {k: v for k, v in sc["ws"].items() if k not in ("info", "walk", "first")}
    edges = np.zeros(len(a["inertial_edges"]), fm.EDGE)
    for c, name in enumerate(("i", "j", "rec", "flags")):
        edges[name] = a["inertial_edges"][:, c]
    pjobs = np.zeros(1, fm.PRIOR_JOB)
    pjobs["state"], pjobs["prior"], pjobs["mask"] = a["prior_jobs"][0]
    ws.update(points=a["ba_points"], edge_state=a["edge_state"], edge_point=a["edge_point"], z=a["edge_z"], w=a["edge_inv_sigma2"], edges=edges, pjobs=pjobs,
              priors=sc["priors"], init_jobs=a["init_jobs"], n_points=len(a["ba_points"]))
    return ws


def reproduces(sc, a):
    """the assembly of a laid-out scene IS the scene up to the stated point order: states in place, every point and every edge once"""
    ws, res = sc["ws"], a["result"]
    assert res[W_REFUSED] == 0 and res[W_SOLVE] == ws["n_solve"] and res[W_FIXED] == ws["n_fixed"] and res[W_POINTS] == ws["n_points"]
    assert res[W_EDGES] == len(ws["edge_state"]) and not res[6:13].any()
    assert a["state_kf"].tolist() == sc["kf_of_state"] and a["fixed"].tolist() == ws["graph"].fixed.tolist()
    point_of_row = {int(r): l for l, r in enumerate(sc["row_of_point"])}
    perm = [point_of_row[int(r)] for r in a["point_row"]]
    assert sorted(perm) == list(range(ws["n_points"])) and (a["ba_points"] == ws["points"][perm]).all()
    theirs = sorted((int(s), int(l), float(z[0]), float(z[1]), float(w)) for s, l, z, w in zip(ws["edge_state"], ws["edge_point"], ws["z"], ws["w"]))
    mine = sorted((int(s), perm[int(x)], float(z[0]), float(z[1]), float(w))
                  for s, x, z, w in zip(a["edge_state"], a["edge_point"], a["edge_z"], a["edge_inv_sigma2"]))
    assert mine == theirs
    ns = ws["n_solve"]
    assert a["inertial_edges"].tolist() == [[e["i"], e["j"], e["rec"], e["flags"]] for e in ws["edges"]]
    assert a["prior_jobs"][0, 0] == 0 and (sc["priors"][a["prior_jobs"][0, 1]] == ws["priors"][0]) and a["prior_jobs"][0, 2] == ws["pjobs"]["mask"][0]
    assert (sc["src"][a["init_jobs"][:ns, 1]] == ws["src"][:ns]).all() and a["init_jobs"][:ns, 2].tolist() == list(range(ns))
    return perm


def tail(sc, csr, a, est, outlier, recs):
    """everything behind the loop (include/orbm.h, the section's chain) in the models, applied to an estimate `est` (the dict a back-end's
    estimate() gives; the device's own): orbi_graph_recover_device, orbm_local_ba_apply_device, orbi_set_bias_device,
    orbi_prior_information_device, the velocity prior.  recs: the records (changed in place by set_bias).  -> dict of every array the
    tail writes"""
    import factors_model as fm
    import imu_model as im
    ws = sc["ws"]
    g = ws["graph"].copy()
    for k in ("Rwb", "twb", "v", "bg", "ba"):
        setattr(g, k, np.array(est[k], np.float64))
    src = sc["src"].copy()
    bias, pose_R, pose_t, rres = fm.recover(g, ws["cal"], a["recover_jobs"], src)
    prob = dict(a, pose_kf=a["state_kf"], result=np.array([a["result"][W_STATES], a["result"][W_POINTS], a["result"][W_EDGES], a["result"][W_SOLVE]] + [0] * 12, np.int32))
    applied = lm.apply(sc, csr, prob, pose_R, pose_t, np.asarray(est["points"], np.float64), outlier)
    bank = im.Bank(len(recs), max(max(len(r.meas) for r in recs), 1))
    bank.recs = recs
    bres = im.run_set_bias(ws["cal"], bank, a["bias_ids"], bias)
    priors = sc["priors"].copy()
    pres, _ = fm.prior_information(priors, bank.recs, src, a["prior_info_jobs"])
    flat, vres = velocity_prior(np.frombuffer(priors.tobytes(), np.float32).reshape(-1, 36), src, a["recover_jobs"], a["prior_jobs"])
    return dict(applied, src=src, bias=bias, est_pose_R=pose_R, est_pose_t=pose_t, bank=bank, priors=np.frombuffer(flat.tobytes(), fm.PRIOR).copy(),
                results=dict(recover=rres, apply=applied["result"], set_bias=bres, prior_information=pres, velocity_prior=vres))


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------
def with_imu(sc, window, max_fixed=MAX_FIXED_DEFAULT, seed=7):
    """a local_ba_model scene extended with d_window and d_kf_imu: state rows, records and prior slots are three different permutations
    into arrays longer than the key-frame table"""
    rng = np.random.RandomState(seed)
    n_kf = len(sc["n"])
    n_src, cap_bank, n_priors = n_kf + 2, n_kf + 3, n_kf + 1
    kf_imu = np.stack([rng.permutation(n_src)[:n_kf], rng.permutation(cap_bank)[:n_kf], rng.permutation(n_priors)[:n_kf]], 1).astype(np.int32)
    return dict(sc, window=np.array(window, np.int32), kf_imu=kf_imu, n_src=n_src, cap_bank=cap_bank, n_priors=n_priors, max_fixed=max_fixed)


def _base(seed=41, **kw):
    return lm.make_scene(seed, True, **kw)


def _window3(sc):
    r = sc["roles"]
    return [r["conn"][0], r["conn"][1], r["cur"]]


def forged_csr(sc, csr):
    """the fresh CSR with the offset of a local row forged past the arrays (two lists become empty) and entries out of range put into two
    other lists"""
    off, kf, kp = [np.asarray(a).copy() for a in csr]
    lists = om.lists_of(off, kf, kp)
    lists[3].insert(1, (len(sc["n"]) + 5, 0))
    lists[9].insert(0, (-3, 2))
    lists[11].append((int(sc["window"][0]), sc["stride"] + 1))
    off = np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32)
    flat = [e for v in lists for e in v]
    kf, kp = np.array([a for a, _ in flat], np.int32), np.array([b for _, b in flat], np.int32)
    off[20] = len(kf) + 7
    return (off, kf, kp), 3


def long_scene(n_obs=257):
    """one row seen by n_obs + 3 key frames of 8 slots, three of them the window: a point with more than 256 kept edges; a second row
    seen by the window alone"""
    n_kf, stride, cap = n_obs + 3, 8, 16
    rng = np.random.RandomState(5)
    slots = np.full((n_kf, stride), -1, np.int32)
    slots[:, 2] = 0
    slots[:3, 5] = 1
    kps = []
    for k in range(n_kf):
        kp = np.zeros(stride, KP_DTYPE)
        kp["x"], kp["y"] = rng.uniform(0, 752, stride), rng.uniform(0, 480, stride)
        kp["octave"] = rng.randint(0, 8, stride)
        kp["size"] = SCALE_FACTORS[kp["octave"]]
        kps.append(kp)
    valid = np.zeros(cap + 4, np.uint8)
    valid[:2] = 1
    sc = dict(n=np.full(n_kf, stride, np.int32), bad=np.zeros(n_kf, np.uint8), slots=slots, stride=stride, valid=valid,
              points=rng.uniform(-3, 3, (cap + 4, 3)).astype(np.float32), cap_points=cap, kps=kps, ref_kf=np.zeros(cap + 4, np.int32),
              pose_R=np.tile(np.eye(3).reshape(9), (n_kf, 1)), pose_t=np.zeros((n_kf, 3)))
    return with_imu(sc, [2, 0, 1], max_fixed=n_kf)


CAP_SCENES = ("cap1", "cap2", "cap3")                                  # max_fixed = 1, 2, 3 against four key frames that could be fixed


def make(name):
    """-> (scene, CSR).  The cap scenes' max_fixed is below the number of key frames that could be fixed, the others' is not
    (test_inertial_window_cpu.py asserts it)."""
    if name == "long":
        sc = long_scene()
        return sc, lm.fresh_csr(sc)
    if name == "tiles":                                                    # 2 window key frames x 600 slots: numbering crosses a tile of 1024
        base = _base(seed=43, stride=600, cap_points=700, n_rows=640)
        r = base["roles"]
        sc = with_imu(base, [r["conn"][1], r["cur"]])
        return sc, lm.fresh_csr(sc)
    base = _base()
    csr = lm.fresh_csr(base)
    if name == "window3":
        return with_imu(base, _window3(base)), csr
    if name == "window1":
        return with_imu(base, [base["roles"]["cur"]]), csr
    if name == "stale":
        stale, spoilt, _ = lm.stale_scene(base, csr)
        return with_imu(stale, _window3(base)), spoilt
    if name == "forged":
        sc = with_imu(base, _window3(base))
        return sc, forged_csr(sc, csr)[0]
    if name in CAP_SCENES:
        return with_imu(base, _window3(base), max_fixed=int(name[3:])), csr
    raise KeyError(name)


SCENES = ("window3", "window1", "stale", "cap1", "cap2", "cap3", "forged", "tiles", "long")
