"""The Levenberg-Marquardt loops of the reference's inertial optimisers, closed: TEST CODE ONLY.  include/orbi_factors.h, orbvi.h and
orbvw.h ship the stages of one iteration and leave the loop to the caller; this file is such a caller, written once, so that the
stages can be run from the first iteration to the last on their own outputs.

The policy is g2o's OptimizationAlgorithmLevenberg::solve / SparseOptimizer::optimize (g2o 20201223, not vendored) exactly as
oracle/ba_ref.py:175-229 (lm_optimize) restates it -- tests/test_inertial_loop_cpu.py drives it with a dense back-end built from
ba_ref.linearize and holds its trace to lm_optimize's.  A back-end carries the estimate and has seven methods:
  linearize()          both linearisations at the estimate; returns the robustified total (g2o's activeRobustChi2)
  largest_diagonal()   the largest free diagonal entry of H before damping, what computeLambdaInit multiplies by tau (the window
                       back-ends have none: localFullBundleAdjustment always sets a user lambda init)
  trial(lam)           push, the damped solve, the update: returns (the solve was not refused, the pose side of computeScale, the points' side)
  totals()             the robustified totals (inertial, visual) at the trial point
  accept()             keep the trial: the points' buffers swap
  reject()             pop: the graph, the update counters and the points go back
  classify()           mode 2 at the estimate
Two kinds: the model back-ends (numpy, over factors_model / vi_model / vw_model) and the device back-ends (the library on an MI355X;
the estimate never leaves device memory).  Three drivers follow Optimize.cpp with the lines cited: pose_inertial, pose_full, local_full.
Every loop is bounded by iterations x max_trials.  The scenes a loop can be judged on are at the bottom; why the stage scenes cannot
carry a loop is in DESIGN.md ("The inertial optimisers, closed-loop")."""
import hashlib

import numpy as np

import factors_model as fm
import imu_model as im
import vi_model as vm
import vw_model as wm

DBL_MAX = float(np.finfo(np.float64).max)
TAU, MAX_TRIALS, LOWER, UPPER = vm.TAU, 10, 1.0 / 3.0, 2.0 / 3.0         # g2o's defaults, as ba_ref.lm_optimize has them
BAR = 1e-9                                                               # the stage bar of the teacher-forced tests
NAN = float("nan")
STATE = ("Rwb", "twb", "v", "bg", "ba")
# a trial of the trace: ba_ref.lm_optimize's tuple, then what the device reads back
FIELDS = ("iteration", "trial", "lam", "current", "temp", "scale", "rho", "ok", "total_inertial", "total_visual", "scale_pose", "scale_points", "accepted")


# ---- the policy ------------------------------------------------------------------------------------------------------------------------------
def optimize(be, iterations, user_lambda_init=0.0, tau=TAU, max_trials=MAX_TRIALS, lower=LOWER, upper=UPPER, forced_lambda_init=None):
    """one optimizer.optimize(iterations): oracle/ba_ref.py:175-229 line by line, the arithmetic behind a back-end.  Returns a dict of
    iterations (run), lam (the last), trace (one FIELDS tuple per trial), accepted (their count).  forced_lambda_init is no part of the
    policy: it puts a value g2o would never start from (0) into lambda, for the refused-solve scene."""
    lam, ni, its, trace = 0.0, 2.0, 0, []
    for it in range(iterations):
        current = be.linearize()                                         # :178-180 computeActiveErrors, activeRobustChi2, buildSystem
        if it == 0:                                                      # :181-183 computeLambdaInit, at iteration 0 of every optimize()
            lam, ni = user_lambda_init if user_lambda_init > 0 else tau * be.largest_diagonal(), 2.0
            if forced_lambda_init is not None:
                lam = forced_lambda_init
        rho, qmax = 0.0, 0
        for _ in range(max_trials):                                      # :185 do { ... } while (rho < 0 && qmax < max_trials)
            ok, scale_pose, scale_points = be.trial(lam)                 # :186-203 push, setLambda, solve, update
            ti, tv = be.totals()
            temp = ti + tv if ok else DBL_MAX                            # :204 a refused solve
            scale = float(scale_pose + scale_points) + 1e-3              # :205 computeScale + 1e-3
            with np.errstate(over="ignore"):
                rho = (current - temp) / scale                           # :206 (DBL_MAX over a small scale is -inf, as in g2o)
            accepted = bool(rho > 0 and np.isfinite(temp))               # :209
            trace.append((it, qmax, lam, current, temp, scale, rho, bool(ok), ti, tv, scale_pose, scale_points, accepted))
            if accepted:
                lam *= max(lower, min(1.0 - (2 * rho - 1) ** 3, upper))  # :210-211
                ni = 2.0
                current = temp
                be.accept()                                              # discardTop
            else:
                lam *= ni                                                # :215-216
                ni *= 2
                be.reject()                                              # :217 pop
                if not np.isfinite(lam):
                    break
            qmax += 1
            if not (rho < 0 and qmax < max_trials):                      # :221
                break
        its += 1
        if qmax == max_trials or rho == 0 or not np.isfinite(lam):       # :224 Terminate
            break
    return dict(iterations=its, lam=lam, trace=trace, accepted=sum(t[-1] for t in trace))


def decisions(rounds):
    """the accept / reject sequence of a run, one string per optimize()"""
    return ["".join("a" if t[-1] else "r" for t in r["trace"]) for r in rounds]


# ---- the drivers ----------------------------------------------------------------------------------------------------------------------------
def pose_inertial(be, forced_lambda_init=None):
    """Optimize::poseInertialOptimize (Optimize.cpp:547-608): two states with both poses fixed (:578 builds EdgeInertialOnly from the
    two poses as constants; the listing sets its four vertices and never passes it to addEdge -- the chain of include/orbvi.h has the
    edge in, and so has this driver), the three priors (:584-597), initializeOptimization and optimize(10) with the default lambda init
    (:600-601)"""
    return [optimize(be, 10, forced_lambda_init=forced_lambda_init)]


def pose_full(be, forced_lambda_init=None):
    """Optimize::poseFullOptimize (Optimize.cpp:610-764): four rounds (:713-716); before each only the frame's POSE goes back to its
    initial value (:717 setEstimate(initialPose); velocity and biases keep what the last round left); optimize(10) on the level-0 edges
    (:719-720); then every edge is classified against 5.991 (:722-735) and the classification is the next round's level.  Huber stays
    (:736 never fires).  forced_lambda_init reaches the FIRST round only (the refused-solve scene)."""
    rounds = []
    for k in range(4):
        be.reset_pose()
        r = optimize(be, 10, forced_lambda_init=forced_lambda_init if k == 0 else None)
        r["classification"] = be.classify()
        rounds.append(r)
    return rounds


def local_full(be, iterations=10, be_large=False):
    """Optimize::localFullBundleAdjustment (Optimize.cpp:1064-1310): the user lambda init 1e-2 (beLarge) or 1e0 (:1120-1122),
    optimize(iterations) (:1245-1246), then every EdgeMono against chi2Mono (:1255-1261)"""
    r = optimize(be, iterations, user_lambda_init=1e-2 if be_large else 1e0)
    r["classification"] = be.classify()
    return [r]


# ---- the model back-ends -----------------------------------------------------------------------------------------------------------------------
class Noise:
    """every trial output times 1 + sigma * N(0, 1), elementwise: a stage error of the size the stage tests allow"""

    def __init__(self, seed, sigma=BAR):
        self.rng, self.sigma = np.random.RandomState(seed), sigma

    def __call__(self, x):
        x = np.asarray(x, np.float64)
        return x * (1.0 + self.sigma * self.rng.normal(0.0, 1.0, x.shape))


def _exact(x):
    return x


def _noisy_graph(noise, g1, g):
    """the updated vertices through `noise`; what is fixed keeps the bytes of g"""
    if noise is _exact:
        return
    for k, bit in zip(STATE, (fm.FIX_POSE, fm.FIX_POSE, fm.FIX_VELO, fm.FIX_GYRO, fm.FIX_ACC)):
        free = (g.fixed & bit) == 0
        getattr(g1, k)[free] = noise(getattr(g1, k)[free])


class ModelWindow:
    """the chain of include/orbvw.h in numpy: vw_model.iterate cut at the trial, so that a rejected trial does not linearise again"""

    def __init__(self, sc, noise=None):
        self.sc, self.g, self.P, self.noise = sc, sc["graph"].copy(), sc["points"].copy(), noise or _exact
        self.refused = 0

    def _vis(self, g, P, mode, **kw):
        sc = self.sc
        return wm.linearize(g, sc["cal"], sc["cam"], sc["n_solve"], P, sc["edge_state"], sc["edge_point"], sc["z"], sc["w"], mode=mode, **kw)

    def linearize(self):
        self.oi = vm.inertial_linearize(self.sc, self.g)
        self.ov = self._vis(self.g, self.P, 0, H_diag=self.oi["H_diag"], b=self.oi["b"])
        return self.oi["total"][1] + self.ov["total"][1]

    def _reduce(self, lam):
        sc, g, oi, ov = self.sc, self.g, self.oi, self.ov
        return wm.reduce(sc["n_solve"], g.fixed, sc["edges"], len(sc["recs"]), ov["H_diag"], oi["H_off"], ov["b"], lam, ov["point_off"], sc["edge_state"],
                         ov["Hll"], ov["bl"], ov["Hlp"], len(sc["w"]))

    def trial(self, lam):
        sc, g, ov, noise = self.sc, self.g, self.ov, self.noise
        ns, ne = sc["n_solve"], len(sc["w"])
        rd = self._reduce(lam)
        dx, (scale, _), res = wm.solve(rd["S"], rd["rhs"], ov["b"][:ns], lam)
        dx = noise(dx)
        bs = wm.backsub(ns, ov["point_off"], sc["edge_state"], ov["Hlp"], rd["Hll_inv"], ov["bl"], dx, lam, self.P, ne)
        g1, full = g.copy(), np.zeros((g.n, 15))
        full[:ns] = dx
        fm.oplus(g1, full)
        _noisy_graph(noise, g1, g)
        P1 = noise(bs["points_out"])
        ok = bool(res[wm.R_DONE] == 1)
        self.refused += not ok
        self.t = dict(g=g1, P=P1, dx=dx, ok=ok, totals=(float(noise(vm.inertial_linearize(sc, g1, 1)["total"][1])), float(noise(self._vis(g1, P1, 1)["total"][1]))))
        return ok, float(noise(scale)), float(noise(bs["scale"]))

    def totals(self):
        return self.t["totals"]

    def accept(self):
        self.g, self.P = self.t["g"], self.t["P"]

    def reject(self):
        pass                                                             # the trial lived on copies

    def classify(self):
        o = self._vis(self.g, self.P, 2)
        return dict(outlier=o["outlier"], n_outliers=int(o["result"][wm.R_OUTLIER]), chi2=o["chi2"])

    def estimate(self):
        return dict({k: getattr(self.g, k).copy() for k in STATE}, points=self.P.copy(), iter=self.g.iter.copy())


class ModelPose:
    """the chain of include/orbvi.h in numpy; visual=False is poseInertialOptimize's graph, without a group of EdgeMonoOnlyPose"""

    def __init__(self, sc, graph=None, visual=True, noise=None):
        self.sc, self.g, self.visual, self.noise = sc, (sc["graph"] if graph is None else graph).copy(), visual, noise or _exact
        self.start = self.g.copy()
        self.active = np.ones(sc["n_edges"], np.uint8) if visual else None
        self.refused = 0

    def _vis(self, g, mode, **kw):
        sc = self.sc
        return vm.linearize(g, sc["cal"], sc["cam"], sc["group_state"], sc["edge_off"], sc["n_edges"], sc["points"], sc["z"], sc["w"], self.active, vm.HUBER_MONO,
                            vm.CHI2_MONO, mode, **kw)

    def reset_pose(self):
        s = int(self.sc["group_state"][0])
        self.g.Rwb[s], self.g.twb[s], self.g.iter[s] = self.start.Rwb[s], self.start.twb[s], 0

    def linearize(self):
        self.oi = vm.inertial_linearize(self.sc, self.g)
        self.H, self.b, total = self.oi["H_diag"], self.oi["b"], self.oi["total"][1]
        if self.visual:
            ov = self._vis(self.g, 0, H_diag=self.H, b=self.b)
            self.H, self.b, total = ov["H_diag"], ov["b"], total + ov["total"][0, 1]
        return total

    def _solve(self, lam):
        return vm.solve(self.g.fixed, self.sc["edges"], len(self.sc["recs"]), self.H, self.oi["H_off"], self.b, lam)

    def largest_diagonal(self):
        return float(self.noise(self._solve(0.0)[1][1]))                 # a solve whose step is discarded, as on the device

    def trial(self, lam):
        noise = self.noise
        dx, out, res = self._solve(lam)
        dx = noise(dx)
        g1 = self.g.copy()
        fm.oplus(g1, dx)
        _noisy_graph(noise, g1, self.g)
        ok = bool(res[vm.R_DONE] == 1)
        self.refused += not ok
        tv = float(noise(self._vis(g1, 1)["total"][0, 1])) if self.visual else 0.0
        self.t = dict(g=g1, dx=dx, ok=ok, totals=(float(noise(vm.inertial_linearize(self.sc, g1, 1)["total"][1])), tv))
        return ok, float(noise(out[0])), 0.0

    def totals(self):
        return self.t["totals"]

    def accept(self):
        self.g = self.t["g"]

    def reject(self):
        pass

    def classify(self):
        if not self.visual:
            return None
        o = self._vis(self.g, 2)
        self.active = o["active"].copy()
        return dict(active=o["active"].copy(), n_inliers=int(o["n_inliers"][0]), chi2=o["chi2"])

    def estimate(self):
        return dict({k: getattr(self.g, k).copy() for k in STATE}, iter=self.g.iter.copy())


# ---- the device back-ends ---------------------------------------------------------------------------------------------------------------------
class _Device:
    """what both device back-ends share: the vertices' push / pop, the audit of a pop and the read-back of the estimate.  PUSH AND POP ARE
    DEVICE-TO-DEVICE COPIES OF Rwb, twb, v, bg, ba AND d_iter: CameraImuPose's update counter is part of the estimate g2o pushes.  With
    audit=True the estimate is also read back around every trial, to hold a pop to the bytes before the push; otherwise nothing but
    the scalars the headers name (and the solve's d_result) leaves the device before estimate()."""

    def _init_state(self, d, audit):
        self.d, self.audit, self.n_trials, self.refused, self.dx_zero = d, audit, 0, 0, []
        d.it = d._pad("it", np.zeros(d.n, np.int32), -3)
        self.live = [d.Rwb, d.twb, d.v, d.bg, d.ba, d.it]
        self.saved = [d._pad("saved " + k, np.full(len(t), NAN), -1.5) for k, t in zip(STATE, self.live)] + [d._pad("saved it", np.full(d.n, -9, np.int32), -3)]

    def _push(self):
        if self.audit:
            self.before = self._bytes()
        for s, t in zip(self.saved, self.live):
            s.copy_(t)

    def _pop(self):
        for s, t in zip(self.saved, self.live):
            t.copy_(s)
        if self.audit:
            after = self._bytes()
            for k in after:
                assert after[k] == self.before[k], "trial %d was rejected and %s does not hold the bytes it held before it" % (self.n_trials - 1, k)

    def _bytes(self):
        return {k: v.tobytes() for k, v in self.estimate().items()}

    def _graph_arrays(self):
        d, n = self.d, self.d.n
        return dict(Rwb=d.get("Rwb").reshape(n, 3, 3).copy(), twb=d.get("twb").reshape(n, 3).copy(), v=d.get("v").reshape(n, 3).copy(),
                    bg=d.get("bg").reshape(n, 3).copy(), ba=d.get("ba").reshape(n, 3).copy(), iter=d.get("it").copy())

    def totals(self):
        return self.t

    def accept(self):
        pass                                                             # the graph was updated in place

    def reject(self):
        self._pop()


def _chain_stream(torch, dev, kind):
    """the stream of a device loop.  "null": stream 0 itself, made torch's current stream first -- an explicit-stream test before this one
    in the process leaves its own stream current, and stream=None follows the current one"""
    from test_projection_queries_gpu import _stream
    if kind == "null":
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        assert torch.cuda.current_stream(dev).cuda_stream == 0
    return _stream(torch, dev, kind)


class DeviceWindow(_Device):
    """the chain of include/orbvw.h on the device, per trial
      *d_lambda <- lam; orbvw_reduce_device; orbvw_solve_device; orbvw_backsub_device (live points -> the other buffer); push;
      orbi_graph_oplus_device; orbi_linearize_device (mode 1); orbvw_linearize_device (mode 1, on the other buffer)
    and ONE read-back: the two robustified totals, d_out[0], d_out_points[0] and the solve's d_result.  The points ping-pong between two
    buffers (the back-substitution refuses d_points_out == d_points): an accepted trial swaps which one is live, a rejected one leaves
    the live one as it is."""

    def __init__(self, torch, dev, sc, stream_kind="explicit", audit=False):
        from monoorbslam3_amd import imu, vw
        from test_factors_gpu import _Dev
        from test_projection_queries_gpu import _up
        from test_vw_gpu import _Win
        self.torch, self.sc, self.imu, self.vw = torch, sc, imu, vw
        i = _Dev(torch, dev, sc, sc["graph"], n_priors=1, n_pjobs=1)
        i.priors.copy_(_up(torch, dev, sc["priors"]))
        w = _Win(torch, dev, sc)
        w.graph, w.fixed = i.graph, i.fixed
        self.w, self.pjobs = w, _up(torch, dev, sc["pjobs"])
        self._init_state(i, audit)
        self.pts, self.cur = [w.points, w.points_out], 0
        self.st = _chain_stream(torch, dev, stream_kind)
        imu.edge_information_device(i.bank, i.cap, i.edges, i.ne, i.info, i.walk, i.result, stream=self.st)

    def linearize(self):
        i, w = self.d, self.w
        i.linearize(self.sc, 0.0, 0, self.pjobs, 1, 1, self.st)
        w.linearize(0, points=self.pts[self.cur], H_diag=i.H_diag, b=i.b, stream=self.st)
        t = self.torch.cat([i.total[1:2], w.total[1:2]]).cpu().numpy()
        return t[0] + t[1]

    def trial(self, lam):
        i, w, st, torch = self.d, self.w, self.st, self.torch
        a, b = self.pts[self.cur], self.pts[1 - self.cur]
        w.lam.fill_(lam)
        w.reduce(H_diag=i.H_diag, H_off=i.H_off, b=i.b, stream=st)
        w.solve(b=i.b, stream=st)
        res = w.result.clone()
        self.vw.backsub_device(w.ns, w.np_, w.ne, w.point_off, w.edge_state, w.Hlp, w.Hll_inv, w.bl, w.dx, w.lam, a, w.xl, b, w.out_points, w.result, stream=st)
        self._push()
        self.imu.graph_oplus_device(i.graph, w.dx, i.it, i.result, stream=st)
        i.linearize(self.sc, 0.0, 1, self.pjobs, 1, 1, st)
        w.linearize(1, points=b, stream=st)
        s = torch.cat([i.total[1:2], w.total[1:2], w.out[0:1], w.out_points[0:1]]).cpu().numpy()       # the four scalars
        res = res.cpu().numpy()
        ok = bool(res[wm.R_DONE] == 1 and res[wm.R_REFUSED] == 0)
        assert ok or res[wm.R_REFUSED] == 1, res
        self.n_trials, self.refused, self.t = self.n_trials + 1, self.refused + (not ok), (float(s[0]), float(s[1]))
        if self.audit:
            self.dx_zero.append(not w.get("dx").any())
        return ok, float(s[2]), float(s[3])

    def accept(self):
        self.cur = 1 - self.cur

    def classify(self):
        self.w.linearize(2, points=self.pts[self.cur], stream=self.st)
        out, res = self.w.get("outlier")[:self.w.ne], self.w.get("result")
        return dict(outlier=out, n_outliers=int(res[wm.R_OUTLIER]), chi2=self.w.get("chi2")[:self.w.ne])

    def estimate(self):
        return dict(self._graph_arrays(), points=self.pts[self.cur].cpu().numpy().reshape(-1, 3).copy())

    def finish(self):
        self.d.finish()
        self.w.finish()


class DevicePose(_Device):
    """the chain of include/orbvi.h on the device, per trial
      *d_lambda <- lam; orbvi_solve_device; push; orbi_graph_oplus_device; orbi_linearize_device (mode 1); orbvi_linearize_device (mode 1)
    and ONE read-back: the two robustified totals, d_out[0] and the solve's d_result.  THE LAMBDA INIT NEEDS d_out[1] BEFORE THE FIRST
    TRIAL, AND ONLY THE SOLVE WRITES IT: largest_diagonal() runs orbvi_solve_device once at lambda 0 and discards its step.  reset_pose and
    the d_active of mode 2 stay on the device from round to round."""

    def __init__(self, torch, dev, sc, graph=None, visual=True, stream_kind="explicit", audit=False):
        from monoorbslam3_amd import imu, vi
        from test_factors_gpu import _Dev
        from test_projection_queries_gpu import _up
        from test_vi_gpu import _Vis
        self.torch, self.sc, self.imu, self.vi, self.visual = torch, sc, imu, vi, visual
        g = sc["graph"] if graph is None else graph
        d = _Dev(torch, dev, sc, g, n_priors=1, n_pjobs=1)
        d.priors.copy_(_up(torch, dev, sc["priors"]))
        self.pjobs = _up(torch, dev, sc["pjobs"])
        self._init_state(d, audit)
        self.lam, self.dx, self.out = d._pad("lam", np.full(1, NAN), -1.5), d._pad("dx", np.full(15 * d.n, NAN), -1.5), d._pad("out", np.full(3, NAN), -1.5)
        self.v = None
        if visual:
            ne = sc["n_edges"]
            self.v = _Vis(torch, dev, g, sc["cal"], sc["cam"], sc["group_state"], sc["edge_off"], ne, sc["points"], sc["z"], sc["w"], active=np.ones(ne, np.uint8))
            self.v.graph = d.graph
            s = int(sc["group_state"][0])
            self.pose = (d.Rwb[9 * s:9 * s + 9], d.twb[3 * s:3 * s + 3], d.it[s:s + 1])
            self.pose0 = [t.clone() for t in self.pose]
        self.st = _chain_stream(torch, dev, stream_kind)
        imu.edge_information_device(d.bank, d.cap, d.edges, d.ne, d.info, d.walk, d.result, stream=self.st)

    def _vis(self, mode):
        v, d, ne = self.v, self.d, self.sc["n_edges"]
        self.vi.linearize_device(d.graph, v.cal, v.cam, 1, ne, v.group_state, v.edge_off, v.points, v.z, v.w, v.err, v.chi2, v.result, d_active=v.active, mode=mode,
                                 d_total=None if mode == 2 else v.total, d_H_diag=None if mode else d.H_diag, d_b=None if mode else d.b,
                                 d_n_inliers=v.n_inliers if mode == 2 else None, d_work=None if mode else v.work, stream=self.st)

    def reset_pose(self):
        for t, t0 in zip(self.pose, self.pose0):
            t.copy_(t0)

    def linearize(self):
        d = self.d
        d.linearize(self.sc, 0.0, 0, self.pjobs, 1, 1, self.st)
        if not self.visual:
            return float(d.total[1:2].cpu().numpy()[0])
        self._vis(0)
        t = self.torch.cat([d.total[1:2], self.v.total[1:2]]).cpu().numpy()
        return t[0] + t[1]

    def _solve(self, lam):
        d = self.d
        self.lam.fill_(lam)
        self.vi.solve_device(d.n, d.fixed, d.edges, d.ne, d.cap, d.H_diag, d.H_off, d.b, self.lam, self.dx, self.out, d.result, stream=self.st)

    def largest_diagonal(self):
        self._solve(0.0)
        return float(self.out[1:2].cpu().numpy()[0])

    def trial(self, lam):
        d, st, torch = self.d, self.st, self.torch
        self._solve(lam)
        res = d.result.clone()
        self._push()
        self.imu.graph_oplus_device(d.graph, self.dx, d.it, d.result, stream=st)
        d.linearize(self.sc, 0.0, 1, self.pjobs, 1, 1, st)
        if self.visual:
            self._vis(1)
        s = torch.cat([d.total[1:2], self.v.total[1:2] if self.visual else torch.zeros_like(d.total[1:2]), self.out[0:1]]).cpu().numpy()
        res = res.cpu().numpy()
        ok = bool(res[vm.R_DONE] == 1 and res[vm.R_REFUSED] == 0)
        assert ok or res[vm.R_REFUSED] == 1, res
        self.n_trials, self.refused, self.t = self.n_trials + 1, self.refused + (not ok), (float(s[0]), float(s[1]))
        if self.audit:
            self.dx_zero.append(not self.dx.cpu().numpy().any())
        return ok, float(s[2]), 0.0

    def classify(self):
        if not self.visual:
            return None
        self._vis(2)
        ne = self.sc["n_edges"]
        return dict(active=self.v.get("active")[:ne].copy(), n_inliers=int(self.v.get("n_inliers")[0]), chi2=self.v.get("chi2")[:ne].copy())

    def estimate(self):
        return self._graph_arrays()

    def finish(self):
        self.d.finish()
        if self.v is not None:
            self.v.finish()


# ---- the gradient of the whole system -------------------------------------------------------------------------------------------------------
def window_gradient(sc, est):
    """b of both linearisations at an estimate (a dict as estimate() gives), the free dof of the solve states and every point: the
    negative gradient of half the robustified cost the loop minimises"""
    g = sc["graph"].copy()
    for k in STATE:
        setattr(g, k, np.array(est[k], np.float64))
    be = ModelWindow(dict(sc, graph=g, points=np.array(est["points"], np.float64)))
    be.linearize()
    ns = sc["n_solve"]
    free = ~vm.dof_fixed(g.fixed[:ns])
    return np.concatenate([be.ov["b"][:ns].reshape(-1)[free], be.ov["bl"].reshape(-1)])


# ---- the scenes ----------------------------------------------------------------------------------------------------------------------------------
LOOP_WINDOW = dict(sample_counts=(100,) * 5, depth=(2.0, 6.0), min_obs=3, fixed_offset=1.0)
# name -> (driver, how the scene is built, the driver's keywords).  The shapes are the smallest that still cross the kernels' edges: fewer
# points than a wave, one more than a wave, more than a workgroup of points and edges; both camera models; both lambda inits.
SCENES = {
    "window 3+2 63": ("local_full", dict(shape=(3, 2, 63), seed=1), dict(iterations=10)),
    "window 4+3 65 large": ("local_full", dict(shape=(4, 3, 65), seed=1, outlier_share=0.1), dict(iterations=25, be_large=True)),
    "window 3+2 65 fisheye": ("local_full", dict(shape=(3, 2, 65), seed=1, model=1), dict(iterations=25)),
    "window 3+2 1025": ("local_full", dict(shape=(3, 2, 1025), seed=1), dict(iterations=10)),
    "window 3+2 63 converging": ("local_full", dict(shape=(3, 2, 63), seed=1, pixel_noise=0.05), dict(iterations=25)),
    "pose full 65": ("pose_full", dict(n_edges=65, model=0, seed=10), {}),
    "pose full 1025": ("pose_full", dict(n_edges=1025, model=0, seed=4), {}),
    "pose full 65 fisheye": ("pose_full", dict(n_edges=65, model=1, seed=11), {}),
    "pose inertial": ("pose_inertial", dict(n_edges=0, model=0), {}),
    # the refused solve and the recovery from it: poseFullOptimize's graph with the frame's bias vertices free, which no edge touches (the
    # "refused" system of tests/test_vi_gpu.py as a graph), and lambda forced to 0 in the FIRST round: every solve of it is refused, every
    # trial rejected (lambda * nu stays 0) and the round ends through max_trials with the estimate untouched; the second round's default
    # lambda init, tau * d_out[1], is positive -- a refused solve writes d_out[1] too -- and its solves succeed on the same buffers
    "pose refused": ("pose_full", dict(n_edges=65, model=0, seed=5, fixed=(fm.FIX_POSE, 0)), dict(forced_lambda_init=0.0)),
}
CONVERGING = "window 3+2 63 converging"
_scenes, _runs = {}, {}


def scene(name):
    if name not in _scenes:
        driver, how, _ = SCENES[name]
        if driver == "local_full":
            how = dict(how)
            shape = how.pop("shape")
            _scenes[name] = wm.window_scene(*shape, **dict(LOOP_WINDOW, **how))
        else:
            sc = vm.pose_full_scene(how["n_edges"], seed=how.get("seed", 3), model=how["model"], sample_counts=LOOP_WINDOW["sample_counts"])
            if driver == "pose_inertial" or "fixed" in how:              # poseInertialOptimize: both poses fixed, the frame without bias vertices
                sc["graph"] = sc["graph"].copy()
                sc["graph"].fixed[:] = how.get("fixed", (fm.FIX_POSE, fm.FIX_POSE | fm.FIX_GYRO | fm.FIX_ACC))
            _scenes[name] = sc
    return _scenes[name]


def model_backend(name, noise=None):
    driver = SCENES[name][0]
    sc = scene(name)
    return ModelWindow(sc, noise) if driver == "local_full" else ModelPose(sc, visual=driver == "pose_full", noise=noise)


def device_backend(torch, dev, name, stream_kind="explicit", audit=False):
    driver = SCENES[name][0]
    sc = scene(name)
    if driver == "local_full":
        return DeviceWindow(torch, dev, sc, stream_kind, audit)
    return DevicePose(torch, dev, sc, visual=driver == "pose_full", stream_kind=stream_kind, audit=audit)


def run(name, be):
    driver, _, kw = SCENES[name]
    return dict(rounds=globals()[driver](be, **kw), estimate=be.estimate(), refused=be.refused)


def model_run(name):
    """the unperturbed model loop of a scene, computed once and shared: nobody changes it"""
    if name not in _runs:
        _runs[name] = run(name, model_backend(name))
    return _runs[name]


RHO_MIN = 1e-3
# the scenes that reach their minimum: behind flat_from() their sequence is rounding and only the estimate is compared
CONVERGED = (CONVERGING, "pose inertial")


def flat_from(trace):
    """the first trial with |rho| < RHO_MIN; len(trace) when none.  From there the totals are flat: current and trial total differ by
    less than a thousandth of computeScale + 1e-3, and the sign of rho, with it the decision, is a matter of rounding."""
    for k, t in enumerate(trace):
        if abs(t[6]) < RHO_MIN:
            return k
    return len(trace)


def digest(sc):
    """a hash over every array of a scene: the records, the source states, the graph, the edges, the priors and what the scene observes"""
    h = hashlib.sha256()
    for r in sc["recs"]:
        for k in im.FIELDS:
            h.update(np.ascontiguousarray(getattr(r, k)).tobytes())
        h.update(str(len(r.meas)).encode())
    g = sc["graph"]
    for a in [sc["src"], sc["edges"], sc["init_jobs"]] + [getattr(g, k) for k in STATE + ("fixed",)]:
        h.update(np.ascontiguousarray(a).tobytes())
    for k in ("priors", "pjobs", "points", "z", "w", "edge_state", "edge_point", "group_state", "edge_off"):
        if k in sc:
            h.update(np.ascontiguousarray(sc[k]).tobytes())
    return h.hexdigest()
