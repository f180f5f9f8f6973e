"""Plain numpy restatement of include/orbfi.h: fullInertialOptimize's shared-bias graph (reference modules/Backend/Optimize.cpp:239-442,
the beInit branch) -- EdgeInertial (G2oTypes.cpp:377-445) with its bias vertices in a carrier state, the two EdgePriori3D on it, the
gather, the step-4 recovery and the job lists of this graph shape.  The edge's error and raw Jacobian, Huber, the ordered sums, the graph
and oplus are factors_model's; the visual side, the reduce, the solve and the back-substitution are vw_model's and vi_model's.  float64
behind the cast, no `@` below the scene builder, every sum written out in the header's order.  No part of the library is used here."""
import numpy as np

import factors_model as fm
import vi_model as vm
import vw_model as wm

F64 = np.float64
MAX_KEYFRAMES, EDGE_WORK, HUBER_DELTA = 31, 482, fm.HUBER_DELTA
PRIOR_G, PRIOR_A = 1e6, 1e12                                   # LocalMapping.cpp:59
USER_LAMBDA_INIT, ITERATIONS = 1e-5, 100                       # Optimize.cpp:250, LocalMapping.cpp:447
R_DONE, R_RANGE, R_DUPLICATE, R_REFUSED, R_PRIOR_DONE, R_PRIOR_RANGE = 0, 1, 2, 3, 4, 5
KF_FIXED, CARRIER_FIXED, FIRST_FIXED = fm.FIX_GYRO | fm.FIX_ACC, fm.FIX_POSE | fm.FIX_VELO, fm.FIX_POSE | fm.FIX_VELO


# ---- orbfi_jobs_device --------------------------------------------------------------------------------------------------------------------
def jobs(init_jobs, edges, recover_jobs, n_kf, fix_first, n_src, cap):
    """a dict of fixed [n_kf + 1], init [n_kf + 1, 3], edges [n_kf - 1], recover [n_kf, 3], prior_rec, result"""
    init_jobs = np.asarray(init_jobs, np.int32).reshape(-1, 3)
    res = np.zeros(8, np.int32)
    fixed = np.full(n_kf + 1, KF_FIXED, np.uint8)
    fixed[n_kf] = CARRIER_FIXED
    if fix_first:
        fixed[0] |= FIRST_FIXED
    init = np.zeros((n_kf + 1, 3), np.int32)
    for k in range(n_kf + 1):
        row, rec = (int(v) for v in init_jobs[min(k, n_kf - 1), 1:])
        row = row if 0 <= row < n_src else -1
        rec = rec if 0 <= rec < cap else -1
        init[k] = (k, row, -1) if k < n_kf else (k, row, rec if rec >= 0 else -2)
        res[R_RANGE if row < 0 or (k == n_kf and rec < 0) else R_DONE] += 1
        prior = rec
    out = np.zeros(n_kf - 1, fm.EDGE)
    for e in range(n_kf - 1):
        i, j, rec = (int(edges[e][k]) for k in ("i", "j", "rec"))
        if 0 <= i < n_kf and 0 <= j < n_kf and i != j and 0 <= rec < cap:
            out[e] = (i, j, rec, 0)
        else:
            out[e] = (-1, -1, -1, 0)
            res[R_RANGE] += 1
    return dict(fixed=fixed, init=init, edges=out, recover=np.array(recover_jobs, np.int32).reshape(-1, 3)[:n_kf].copy(), prior_rec=np.int32(prior),
                result=res)


# ---- orbfi_linearize_device -----------------------------------------------------------------------------------------------------------------
class _SharedBias:
    """a graph whose every state reads the bias pair of state b: what factors_model.inertial_edge looks up as the bias of state i"""

    def __init__(self, graph, b):
        self.Rwb, self.twb, self.v = graph.Rwb, graph.twb, graph.v
        self.bg, self.ba = np.tile(graph.bg[b], (graph.n, 1)), np.tile(graph.ba[b], (graph.n, 1))


def column_mask(graph, i, j, b):
    """bool [30]: the fixed columns of an edge's Jacobian -- 0..8 state i's, 9..14 the carrier's, 15..29 state j's"""
    fi, fb, fj = fm.dof_fixed(graph.fixed[i]), fm.dof_fixed(graph.fixed[b]), fm.dof_fixed(graph.fixed[j])
    return np.concatenate([fi[:9], fb[9:], fj])


def linearize(graph, recs, gravity, edges, info, bias_state, prior_rec, prior_g=PRIOR_G, prior_a=PRIOR_A, delta=HUBER_DELTA, mode=0):
    """a dict of err, chi2, chi2_prior, total, result, flt, status and, in mode 0, H_diag, b, off_edges, H_off, J (raw), M (the 30 x 30 forms)"""
    ne, n, b = len(edges), graph.n, int(bias_state)
    assert 0 <= b < n
    p = (F64(np.float32(prior_g)), F64(np.float32(prior_a)))
    o = dict(err=np.zeros((ne, 9)), chi2=np.zeros(ne), chi2_prior=np.zeros(2), flt=np.zeros((ne, 15), np.float32), result=np.zeros(8, np.int32),
             status=np.zeros(ne, np.int32))
    if mode == 0:
        o.update(H_diag=np.zeros((n, 15, 15)), b=np.zeros((n, 15)), off_edges=np.zeros(3 * ne, fm.EDGE), H_off=np.zeros((3 * ne, 15, 15)), J=np.zeros((ne, 9, 30)),
                 M=np.zeros((ne, 30, 30)))
    view, part = _SharedBias(graph, b), {}
    for e, ed in enumerate(edges):
        i, j, rec = (int(ed[k]) for k in ("i", "j", "rec"))
        if not (0 <= i < n and 0 <= j < n and i != j and 0 <= rec < len(recs)) or b in (i, j):
            o["status"][e] = R_RANGE
        elif info[e, 0] == 0:
            o["status"][e] = R_REFUSED
        o["result"][o["status"][e]] += 1
        if o["status"][e]:
            continue
        err, J, flt = fm.inertial_edge(recs[rec], view, i, j, gravity, mode == 0)
        Om = info[e].reshape(9, 9)
        We = fm._ordered(Om, err[:, None])[:, 0]
        chi = float(fm._ordered(err[None, :], We[:, None])[0, 0])
        rho1 = fm.huber(chi, delta)[1]
        o["err"][e], o["chi2"][e], o["flt"][e] = err, chi, flt
        if mode != 0:
            continue
        o["J"][e] = J
        Jm = np.where(column_mask(graph, i, j, b)[None, :], 0.0, J)
        WJ = rho1 * fm._ordered(Om, Jm)
        M = fm._ordered(Jm.T, WJ)
        m = -fm._ordered(Jm.T, (rho1 * We)[:, None])[:, 0]
        o["M"][e], part[e] = M, (M, m)
        o["off_edges"][3 * e:3 * e + 3] = [(i, j, rec, 0), (i, b, rec, 0), (j, b, rec, 0)]
        o["H_off"][3 * e, :9, :9], o["H_off"][3 * e + 1, :9, 9:], o["H_off"][3 * e + 2, :9, 9:] = M[:9, 15:24], M[:9, 9:15], M[15:24, 9:15]
    ok = 0 <= prior_rec < len(recs)
    o["result"][R_PRIOR_DONE if ok else R_PRIOR_RANGE] = 2
    ep = [np.zeros(3), np.zeros(3)]
    if ok:
        meas = recs[prior_rec].updated_bias.astype(F64)
        ep = [meas[:3] - graph.bg[b], meas[3:] - graph.ba[b]]
        for v in range(2):
            o["chi2_prior"][v] = (ep[v][0] * (p[v] * ep[v][0]) + ep[v][1] * (p[v] * ep[v][1])) + ep[v][2] * (p[v] * ep[v][2])
    plain = robust = 0.0
    for e in range(ne):
        plain, robust = plain + o["chi2"][e], robust + fm.huber(o["chi2"][e], delta)[0]
    o["total"] = np.array([(plain + o["chi2_prior"][0]) + o["chi2_prior"][1], (robust + o["chi2_prior"][0]) + o["chi2_prior"][1]])
    if mode != 0:
        return o
    for s in range(n):                                          # a state at a time, its edges ascending from zero, the priors last
        H, bb = np.zeros((15, 15)), np.zeros(15)
        for e in sorted(part):
            M, m = part[e]
            i, j = int(edges[e]["i"]), int(edges[e]["j"])
            if s == b:
                H[9:, 9:], bb[9:] = H[9:, 9:] + M[9:15, 9:15], bb[9:] + m[9:15]
            elif s == i:
                H[:9, :9], bb[:9] = H[:9, :9] + M[:9, :9], bb[:9] + m[:9]
            elif s == j:
                H[:9, :9], bb[:9] = H[:9, :9] + M[15:24, 15:24], bb[:9] + m[15:24]
        if s == b and ok:
            fx = fm.dof_fixed(graph.fixed[b])
            for v in range(2):
                sl = slice(9 + 3 * v, 12 + 3 * v)
                if not fx[9 + 3 * v]:
                    H[sl, sl] = H[sl, sl] + p[v] * np.eye(3)
                    bb[sl] = bb[sl] + p[v] * ep[v]
        o["H_diag"][s], o["b"][s] = H, bb
    return o


# ---- orbfi_recover_device -------------------------------------------------------------------------------------------------------------------
def recover(graph, cal, bias_state, jobs_, dst):
    """factors_model.recover with ORBI_RECOVER_POSE in every job and the carrier's bias in every kept job's row"""
    jobs_ = np.array(jobs_, np.int32).reshape(-1, 3)
    forced = jobs_.copy()
    forced[:, 2] = fm.RECOVER_POSE
    bias, pose_R, pose_t, res = fm.recover(graph, cal, forced, dst)
    dup = fm._dups([int(j[1]) for j in jobs_])
    for k, (st, to, _) in enumerate(jobs_):
        if 0 <= st < graph.n and 0 <= to < len(dst) and not dup[k]:
            bias[k] = np.concatenate([graph.bg[bias_state], graph.ba[bias_state]]).astype(np.float32)
    return bias, pose_R, pose_t, res


# ---- the dense system and one iteration ------------------------------------------------------------------------------------------------------
def dense(o, fixed, cap, lam=0.0):
    """vi_model.assemble on a linearisation's blocks: what orbvw_reduce_device builds as its base.  (A, rhs, fixed dof mask, h_max, dropped)"""
    return vm.assemble(fixed, o["off_edges"], cap, o["H_diag"], o["H_off"], o["b"], lam)


def inertial_linearize(sc, graph, mode=0):
    if "info" not in sc:
        sc["info"], sc["walk"], _ = fm.edge_information(sc["recs"], sc["edges"])
    if sc.get("per_state"):                                     # the !beInit branch: existing calls only
        return fm.linearize(graph, sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], None, None, HUBER_DELTA, mode)
    return linearize(graph, sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["bias_state"], sc["prior_rec"], sc["prior_g"], sc["prior_a"],
                     HUBER_DELTA, mode)


def reduce_edges(sc, oi):
    return (sc["edges"], oi["H_off"]) if sc.get("per_state") else (oi["off_edges"], oi["H_off"])


def iterate(sc, lam, graph=None, points=None):
    """one model iteration of the chain of include/orbfi.h from (graph, points), vw_model.iterate with this header's inertial side"""
    g = sc["graph"] if graph is None else graph
    P = sc["points"] if points is None else points
    ns, ne = sc["n_solve"], len(sc["edge_state"])
    vis = lambda gr, pts, mode, **kw: wm.linearize(gr, sc["cal"], sc["cam"], ns, pts, sc["edge_state"], sc["edge_point"], sc["z"], sc["w"], mode=mode, **kw)  # noqa: E731
    oi = inertial_linearize(sc, g)
    ov = vis(g, P, 0, H_diag=oi["H_diag"], b=oi["b"])
    ed, Hoff = reduce_edges(sc, oi)
    rd = wm.reduce(ns, g.fixed, ed, len(sc["recs"]), ov["H_diag"], Hoff, ov["b"], lam, ov["point_off"], sc["edge_state"], ov["Hll"], ov["bl"], ov["Hlp"], ne)
    dx, (scale, pivot), sres = wm.solve(rd["S"], rd["rhs"], ov["b"][:ns], lam)
    bs = wm.backsub(ns, ov["point_off"], sc["edge_state"], ov["Hlp"], rd["Hll_inv"], ov["bl"], dx, lam, P, ne)
    g1 = g.copy()
    fm.oplus(g1, dx)
    oi1, ov1 = inertial_linearize(sc, g1, 1), vis(g1, bs["points_out"], 1)
    return dict(inertial=oi, visual=ov, reduce=rd, dx=dx, scale=scale, pivot=pivot, solve_result=sres, backsub=bs, graph=g1, inertial1=oi1, visual1=ov1,
                before=oi["total"][1] + ov["total"][1], after=oi1["total"][1] + ov1["total"][1])


# ---- the scene ---------------------------------------------------------------------------------------------------------------------------------
def shared_graph(chain, recs, n_kf, fix_first, last_rec):
    """the n_kf + 1 states of orbfi.h from a chain's: the key frames without bias vertices, the carrier with the last record's updated_bias"""
    g = fm.Graph(n_kf + 1)
    for k in ("Rwb", "twb", "v"):
        getattr(g, k)[:n_kf] = getattr(chain, k)[:n_kf]
        getattr(g, k)[n_kf] = getattr(chain, k)[n_kf - 1]
    ub = recs[last_rec].updated_bias.astype(F64)
    g.bg[n_kf], g.ba[n_kf] = ub[:3], ub[3:]
    g.fixed[:n_kf], g.fixed[n_kf] = KF_FIXED, CARRIER_FIXED
    if fix_first:
        g.fixed[0] |= FIRST_FIXED
    return g


def scene(n_kf, n_points, seed=1, fix_first=True, per_state=False, common_bias=False, **kw):
    """fullInertialOptimize's graph on vw_model.window_scene(n_kf, 0, n_points): its chain of n_kf key frames, records and observations;
    every key frame a solve state, nothing fixed besides key frame 0 (fix_first).  per_state=False is the beInit branch: the carrier state
    behind the key frames, the edges without walks, the two priors from the last key frame's record.  per_state=True is the other branch:
    the window's own graph with walks and no priors, key frame 0 fixed whole.  common_bias: the records as inertialOptimize leaves them, all with
    one updated_bias -- the state this optimiser starts from, and what a closed loop needs (tests/full_inertial_loop.py)."""
    sc = wm.window_scene(n_kf, 0, n_points, seed=seed, **kw)
    return of_window_scene(with_common_bias(sc) if common_bias else sc, fix_first, per_state)


def with_common_bias(ws):
    """a window scene as inertialOptimize leaves it (Optimize.cpp:196-201 sets ONE bias for every key frame): every record's updated_bias is
    the last key frame's, its linearisation point moved along so that its delta_bias -- and with it its residual at that bias -- stays what
    it was; every state's bias is that one"""
    sc = dict(ws)
    shared = sc["recs"][sc["n_solve"] - 1].updated_bias.copy()
    sc["recs"] = [r.copy() for r in sc["recs"]]
    for r in sc["recs"]:
        r.updated_bias, r.bias = shared.copy(), (shared - r.delta_bias).astype(np.float32)
        r.delta_bias = r.updated_bias - r.bias
    g = sc["graph"].copy()
    g.bg[:], g.ba[:] = shared[:3].astype(F64), shared[3:].astype(F64)
    sc["graph"] = g
    return sc


def of_window_scene(ws, fix_first=True, per_state=False):
    """fullInertialOptimize's graph on a window scene of vw_model without fixed key frames (scene() says what the two branches are)"""
    sc = dict(ws)
    n_kf = sc["n_solve"]
    assert sc["n_fixed"] == 0
    sc.pop("first", None), sc.pop("info", None), sc.pop("walk", None)
    sc["n_kf"], sc["fix_first"], sc["per_state"] = n_kf, bool(fix_first), bool(per_state)
    if per_state:
        g = sc["graph"].copy()
        g.fixed[0] = 15 if fix_first else 0
        sc.update(graph=g, priors=None, pjobs=np.zeros(0, fm.PRIOR_JOB))
    else:
        last = n_kf - 1                                          # make_chain: record k is key frame k's, the last one the chain's spare
        edges = sc["edges"].copy()
        edges["flags"] = 0
        init = np.stack([np.arange(n_kf + 1), np.minimum(np.arange(n_kf + 1), n_kf - 1), np.full(n_kf + 1, -1)], 1).astype(np.int32)
        init[n_kf, 2] = last
        sc.update(graph=shared_graph(sc["graph"], sc["recs"], n_kf, fix_first, last), edges=edges, init_jobs=init, n_solve=n_kf + 1, bias_state=n_kf,
                  prior_rec=last, prior_g=PRIOR_G, prior_a=PRIOR_A)
        chk = fm.Graph(n_kf + 1)
        assert fm.graph_init(chk, sc["recs"], sc["src"], init)[R_DONE] == n_kf + 1
        for k in ("Rwb", "twb", "v", "bg", "ba"):
            assert np.array_equal(getattr(chk, k), getattr(sc["graph"], k)), k
    sc["recover_jobs"] = np.stack([np.arange(n_kf), np.arange(n_kf), np.full(n_kf, fm.RECOVER_POSE)], 1).astype(np.int32)
    sc["first"] = iterate(sc, 1.0)
    assert sc["first"]["solve_result"][R_DONE] == 1 and sc["first"]["pivot"] > 0
    return sc


STAGE_POINTS = 40               # fewer than a wave: the visual side's shapes are tests/test_vw_gpu.py's, the shapes here are the inertial side's
STAGE_COMMON_BIAS = (5, 31)     # the key-frame counts whose stage scene has one bias for all records, so that chi2 lies on both sides of Huber


def stage_scene(n_kf, fix_first=True):
    """the scene of the teacher-forced stage tests, CPU and GPU: random biases per record (every chi2 far above the Huber threshold, large bias
    deltas through the float part) at 2 and 3 key frames, one bias for all at 5 and 31"""
    return scene(n_kf, STAGE_POINTS, fix_first=fix_first, common_bias=n_kf in STAGE_COMMON_BIAS)
