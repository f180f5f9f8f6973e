"""The model of the inertial factors (tests/factors_model.py) judged without a GPU: its analytic Jacobian against central differences,
the whole model against an independent object-style restatement (dense `@` products, np.linalg.inv, eigh with the clamp, one dense
Hessian for the whole graph), the information clamps, the fixed masks, symmetry and both branches of the Huber kernel."""
import math

import numpy as np
import pytest

import factors_model as fm
import imu_model as im

_cache = {}


def _chain(n, **kw):
    key = (n, tuple(sorted(kw.items())))
    if key not in _cache:
        sc = fm.make_chain(n, **kw)
        sc["info"], sc["walk"], res = fm.edge_information(sc["recs"], sc["edges"])
        assert res[fm.R_DONE] == n
        _cache[key] = sc
    return _cache[key]


# ---- the analytic Jacobian against central differences ---------------------------------------------------------------------------------
# measured with this file (largest |analytic - numeric| over the largest |entry| of the 9 x 30 Jacobian; steps 1e-6, 1e-3 for the
# bias dof, which pass through a cast to float): 2 samples 3.3e-06, 8 samples 1.3e-05, 40 samples 2.9e-05.  The bar is 4 x that.
MEASURED_FD = {2: 3.3e-06, 8: 1.3e-05, 40: 2.9e-05}


def _perturbed_error(sc, e, dof, h):
    g = sc["graph"].copy()
    g.fixed[:] = 0
    i, j = int(sc["edges"][e]["i"]), int(sc["edges"][e]["j"])
    dx = np.zeros((g.n, 15))
    dx[i if dof < 15 else j, dof % 15] = h
    fm.oplus(g, dx)
    return fm.inertial_edge(sc["recs"][e], g, i, j, sc["cal"]["gravity"], False)[0]


@pytest.mark.parametrize("n_samples", [2, 8, 40])
def test_the_analytic_jacobian_agrees_with_central_differences(n_samples):
    sc = _chain(5)
    e = fm.SAMPLE_COUNTS.index(n_samples)
    assert len(sc["recs"][e].meas) == n_samples
    i, j = int(sc["edges"][e]["i"]), int(sc["edges"][e]["j"])
    _, J, _ = fm.inertial_edge(sc["recs"][e], sc["graph"], i, j, sc["cal"]["gravity"])
    num = np.zeros((9, 30))
    for dof in range(30):
        if dof >= 24:
            continue                                  # the edge reads no bias vertex of its second state
        h = 1e-3 if 9 <= dof < 15 else 1e-6
        num[:, dof] = (_perturbed_error(sc, e, dof, h) - _perturbed_error(sc, e, dof, -h)) / (2 * h)
    assert not J[:, 24:].any()
    worst = np.abs(J - num).max() / np.abs(J).max()
    print("samples %d: analytic vs central differences %.3g of the largest entry" % (n_samples, worst))
    assert worst <= 4 * MEASURED_FD[n_samples]


# ---- an independent object-style restatement ----------------------------------------------------------------------------------------------
def _hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], float)


def _log(R):
    tr = np.trace(R)
    if tr == 3:
        return np.zeros(3)
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(w)
    th = math.atan2(s, 0.5 * (tr - 1))
    return w if abs(th) < 1e-6 else th * w / s


def _jr(v, inverse=False):
    d = np.linalg.norm(v)
    if d < 1e-6:
        return np.eye(3)
    W = _hat(v)
    if inverse:
        return np.eye(3) + W / 2 + (1 / d ** 2 - (1 + math.cos(d)) / (2 * d * math.sin(d))) * W @ W
    return np.eye(3) - (1 - math.cos(d)) / d ** 2 * W + (d - math.sin(d)) / d ** 3 * W @ W


class _Edge:
    """a g2o-style edge: vertex offsets into the graph's dense state, error, Jacobian blocks, information"""

    def __init__(self, offsets, err, blocks, info, robust_delta=0.0):
        self.offsets, self.err, self.blocks, self.info, self.delta = offsets, err, blocks, info, robust_delta

    def chi2(self):
        return float(self.err @ self.info @ self.err)

    def add_to(self, H, b, fixed):
        chi = self.chi2()
        w = self.delta / math.sqrt(chi) if self.delta > 0 and chi > self.delta ** 2 else 1.0
        for oa, Ja in zip(self.offsets, self.blocks):
            if fixed[oa]:
                continue
            b[oa:oa + Ja.shape[1]] -= Ja.T @ (w * self.info) @ self.err
            for ob, Jb in zip(self.offsets, self.blocks):
                if not fixed[ob]:
                    H[oa:oa + Ja.shape[1], ob:ob + Jb.shape[1]] += Ja.T @ (w * self.info) @ Jb


def _objects(sc, pjobs, priors, delta):
    g, cal = sc["graph"], sc["cal"]
    fixed = np.concatenate([fm.dof_fixed(f) for f in g.fixed])
    inertial, walks, pri = [], [], []
    G = np.array([0, 0, -float(np.float32(cal["gravity"]))])
    for e, ed in enumerate(sc["edges"]):
        i, j, r = int(ed["i"]), int(ed["j"]), sc["recs"][int(ed["rec"])]
        dRf, dVf, dPf, dbgf = fm.float_deltas(r, g.bg[i], g.ba[i])
        dR, dV, dP, dbg = (x.astype(float) for x in (dRf, dVf, dPf, dbgf))
        JRg, JVg, JVa, JPg, JPa = (getattr(r, k).astype(float) for k in ("JRg", "JVg", "JVa", "JPg", "JPa"))
        dt = float(r.delta_t)
        R1, R2 = g.Rwb[i], g.Rwb[j]
        eR = dR.T @ R1.T @ R2
        er = _log(eR)
        a = R1.T @ (g.v[j] - g.v[i] - G * dt)
        c = R1.T @ (g.twb[j] - g.twb[i] - g.v[i] * dt - 0.5 * G * dt * dt)
        invJ = _jr(er, True)
        Z = np.zeros((3, 3))
        blocks = [np.block([[-invJ @ R2.T @ R1, Z], [_hat(a), Z], [_hat(c), -np.eye(3)]]),          # pose 1
                  np.vstack([Z, -R1.T, -R1.T * dt]),                                             # velocity 1
                  np.vstack([-invJ @ eR.T @ _jr(JRg @ dbg) @ JRg, -JVg, -JPg]),                  # gyro bias
                  np.vstack([Z, -JVa, -JPa]),                                                    # acc bias
                  np.block([[invJ, Z], [Z, Z], [Z, R1.T @ R2]]),                                 # pose 2
                  np.vstack([Z, R1.T, Z])]                                                       # velocity 2
        C = r.C.astype(float)
        info = np.linalg.inv(C[:9, :9])
        info = (info + info.T) / 2
        lam, V = np.linalg.eigh(info)
        info = V @ np.diag(np.where(lam < 1e-12, 0, lam)) @ V.T
        inertial.append(_Edge([15 * i, 15 * i + 6, 15 * i + 9, 15 * i + 12, 15 * j, 15 * j + 6], np.concatenate([er, a - dV, c - dP]), blocks, info, delta))
        if int(ed["flags"]) & fm.EDGE_WALKS:
            for k, est in enumerate((g.bg, g.ba)):
                walks.append((e, _Edge([15 * i + 9 + 3 * k, 15 * j + 9 + 3 * k], est[j] - est[i], [-np.eye(3), np.eye(3)],
                                       np.linalg.inv(C[9 + 3 * k:12 + 3 * k, 9 + 3 * k:12 + 3 * k]))))
    for pj in pjobs:
        s, p, mask = int(pj["state"]), priors[int(pj["prior"])], int(pj["mask"])
        est = (g.v[s], g.bg[s], g.ba[s])
        meas = (p["velo_priori"], p["bias_priori"][:3], p["bias_priori"][3:])
        infos = (p["velo_info"], p["gyro_info"], p["gyro_info"] if mask & fm.PRIOR_ACC_GYRO_INFO else p["acc_info"])
        for v in range(3):
            if mask >> v & 1:
                pri.append(_Edge([15 * s + 6 + 3 * v], meas[v].astype(float) - est[v], [-np.eye(3)], infos[v].astype(float).reshape(3, 3)))
    return fixed, inertial, walks, pri


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(b).max(), 1e-300)


@pytest.mark.parametrize("delta", [0.0, fm.HUBER_DELTA])
def test_the_model_agrees_with_an_object_style_restatement(delta):
    sc = _chain(5)
    g = sc["graph"].copy()
    g.fixed[:] = [fm.FIX_POSE | fm.FIX_VELO | fm.FIX_GYRO | fm.FIX_ACC, 0, fm.FIX_POSE, fm.FIX_GYRO, fm.FIX_VELO | fm.FIX_ACC, 0]
    sc = dict(sc, graph=g)
    priors, _, _ = fm.make_priors(sc, [2, 4])                  # from the states behind: the priors' errors are not zero
    pjobs = np.array([(1, 0, 7), (3, 1, 7 | fm.PRIOR_ACC_GYRO_INFO), (1, 1, fm.PRIOR_GYRO)], fm.PRIOR_JOB)   # two jobs name state 1's gyro bias
    o = fm.linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], priors, pjobs, delta)
    fixed, inertial, walks, pri = _objects(sc, pjobs, priors, delta)
    n = g.n
    H, b = np.zeros((15 * n, 15 * n)), np.zeros(15 * n)
    for ed in inertial + [w for _, w in walks] + pri:
        ed.add_to(H, b, fixed)
    worst = {}
    worst["info"] = max(_rel(sc["info"][e].reshape(9, 9), ed.info) for e, ed in enumerate(inertial))
    worst["walk"] = max(_rel(sc["walk"][e].reshape(2, 3, 3)[k % 2], w.info) for k, (e, w) in enumerate(walks))
    worst["err"] = _rel(o["err"], np.stack([ed.err for ed in inertial]))
    worst["chi2"] = _rel(o["chi2"][:, 0], [ed.chi2() for ed in inertial])
    worst["chi2_walk"] = _rel(o["chi2"][:, 1:].reshape(-1), [w.chi2() for _, w in walks])
    want = np.zeros((len(pjobs), 3))
    want[np.array([[m >> v & 1 for v in range(3)] for m in pjobs["mask"]], bool)] = [p.chi2() for p in pri]
    assert len(pri) == 7 and (want != 0).sum() == 7
    worst["chi2_prior"] = _rel(o["chi2_prior"], want)
    worst["J"] = max(_rel(o["J"][e], np.concatenate([np.hstack(ed.blocks[:4]), np.hstack(ed.blocks[4:] + [np.zeros((9, 6))])], 1)) for e, ed in enumerate(inertial))
    worst["H_diag"] = _rel(o["H_diag"], np.stack([H[15 * s:15 * s + 15, 15 * s:15 * s + 15] for s in range(n)]))
    worst["H_off"] = _rel(o["H_off"], np.stack([H[15 * e:15 * e + 15, 15 * e + 15:15 * e + 30] for e in range(n - 1)]))
    worst["b"] = _rel(o["b"], b.reshape(n, 15))
    everything = inertial + [w for _, w in walks] + pri
    rob = [(2 * math.sqrt(c) * delta - delta ** 2 if delta > 0 and c > delta ** 2 else c) for c in (ed.chi2() for ed in inertial)]
    worst["total"] = _rel(o["total"], [sum(ed.chi2() for ed in everything), sum(rob) + sum(ed.chi2() for ed in everything[len(inertial):])])
    print({k: "%.2g" % v for k, v in worst.items()})
    assert max(worst.values()) <= 1e-12, worst
    # the Hessian of the whole graph is symmetric, and so is every diagonal block of the model
    assert _rel(H, H.T) <= 1e-12 and _rel(o["H_diag"], np.transpose(o["H_diag"], (0, 2, 1))) <= 1e-12
    # both branches of the Huber kernel
    inside = o["chi2"][:, 0] <= fm.HUBER_DELTA ** 2
    print("inertial chi2", o["chi2"][:, 0])
    assert inside.any() and (~inside).any()
    if delta > 0:
        assert o["total"][1] < o["total"][0]
    else:
        assert o["total"][1] == o["total"][0]


def test_fixed_masks_zero_exactly_their_rows_and_columns():
    sc = _chain(2)
    priors, _, _ = fm.make_priors(sc, [0, 1, 2])
    pjobs = np.array([(s, s, 7) for s in range(3)], fm.PRIOR_JOB)
    free = fm.linearize(sc["graph"], sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], priors, pjobs)
    assert all((free["H_diag"][s] != 0).any(0).all() for s in range(3)) and (free["b"] != 0).all()
    for bit in (fm.FIX_POSE, fm.FIX_VELO, fm.FIX_GYRO, fm.FIX_ACC, 15):
        g = sc["graph"].copy()
        g.fixed[1] = bit                                   # the middle state: both edges meet it
        o = fm.linearize(g, sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], priors, pjobs)
        fx = fm.dof_fixed(bit)
        assert not o["H_diag"][1][fx].any() and not o["H_diag"][1][:, fx].any() and not o["b"][1][fx].any()
        assert not o["H_off"][0][:, fx].any() and not o["H_off"][1][fx].any()
        keep = ~fx
        # everything else is what it was: the mask removes rows and columns and changes nothing beside them
        assert np.array_equal(o["H_diag"][1][np.ix_(keep, keep)], free["H_diag"][1][np.ix_(keep, keep)]) and np.array_equal(o["b"][1][keep], free["b"][1][keep])
        assert np.array_equal(o["H_diag"][[0, 2]], free["H_diag"][[0, 2]]) and np.array_equal(o["H_off"][0][:, keep], free["H_off"][0][:, keep])
        assert np.array_equal(o["chi2"], free["chi2"]) and np.array_equal(o["total"], free["total"]) and np.array_equal(o["J"], free["J"])


def test_mode_1_is_the_error_part_of_mode_0():
    sc = _chain(5)
    a = fm.linearize(sc["graph"], sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], delta=fm.HUBER_DELTA)
    b = fm.linearize(sc["graph"], sc["recs"], sc["cal"]["gravity"], sc["edges"], sc["info"], sc["walk"], delta=fm.HUBER_DELTA, mode=1)
    assert all(np.array_equal(a[k], b[k]) for k in ("err", "chi2", "total", "flt", "result")) and "H_diag" not in b


# ---- the information clamps ----------------------------------------------------------------------------------------------------------------
def test_the_edge_information_clamp_is_a_no_op_on_every_test_record():
    """The device omits the eigenvalue clamp of G2oTypes.cpp:368-372: on every record the tests use the smallest eigenvalue of the
    information is many orders above 1e-12, and clamping changes nothing beyond eigh's own rounding."""
    recs = list(_chain(33)["recs"][:33]) + [fm.make_record(im.calib(), 400, 77)]
    edges = np.zeros(len(recs), fm.EDGE)
    edges["rec"] = np.arange(len(recs))
    info, _, res = fm.edge_information(recs, edges)
    assert res[fm.R_DONE] == len(recs)
    low = []
    for e in range(len(recs)):
        M = info[e].reshape(9, 9)
        clamped, count, lam_min = fm.clamp_information(M)
        low.append(lam_min)
        assert count == 0 and _rel(clamped, M) <= 1e-12 and np.array_equal(M, M.T)
    print("smallest information eigenvalue over %d records: %.3g .. %.3g" % (len(recs), min(low), max(low)))
    assert min(low) > 1e3


@pytest.mark.parametrize("noise_acc,n_samples,want", [(2.0e-3, 10, 0), (1e-7, 10, 3), (2e-7, 10, 3), (2e-7, 20, 1)])
def test_the_prior_information_clamp_off_all_and_mixed(noise_acc, n_samples, want):
    """setPrioriInformation's clamp three ways: the default calibration (off), noise_acc = 1e-7 with 10 samples (all three eigenvalues
    of C[3:6,3:6] below 1e-12: 4e-18, 7e-13, 7e-13) and the mixed case.  noise_acc = 2e-7 with 10 samples is NOT mixed: the two large
    eigenvalues are the gyro noise carried into the velocity by the accelerometer reading, and the accelerometer noise only moves the
    small one (1.3e-17, 7e-13, 7e-13: all clamped again).  They grow with the cube of the integration time, so 20 samples give
    6e-17, 5e-12, 5e-12: one clamped, two kept.  The Jacobi decomposition agrees with eigh."""
    cal, rec = fm.make_clamp_record(noise_acc, n_samples)
    A = rec.C[3:6, 3:6].astype(float)
    A = (A + A.T) / 2
    lam_ref, V_ref = np.linalg.eigh(A)
    print("noise_acc %g: eigenvalues" % noise_acc, lam_ref)
    lam, V = fm.jacobi_eigen(A)
    assert _rel(np.sort(lam), lam_ref) <= 1e-12 and _rel(V @ np.diag(lam) @ V.T, A) <= 1e-12 and _rel(V.T @ V, np.eye(3)) <= 1e-14
    pri = np.zeros(1, fm.PRIOR)
    res, clamped = fm.prior_information(pri, [rec], None, np.array([[0, 0, -1]], np.int32))
    assert res[fm.R_DONE] == 1 and clamped == [want] and int((lam_ref < 1e-12).sum()) == want
    ref = (V_ref * np.where(lam_ref < 1e-12, 0, lam_ref)) @ V_ref.T
    got = pri["velo_info"][0].reshape(3, 3).astype(float)
    if want == 3:
        assert not got.any()
    else:
        assert _rel(got, ref) <= 2 ** -23                     # the slot holds floats
    if want == 1:
        assert np.linalg.matrix_rank(got, tol=1e-20) == 2
    assert _rel(pri["gyro_info"][0].reshape(3, 3), np.linalg.inv(rec.C[9:12, 9:12].astype(float))) <= 2 ** -23
    assert _rel(pri["acc_info"][0].reshape(3, 3), np.linalg.inv(rec.C[12:15, 12:15].astype(float))) <= 2 ** -23
    assert np.array_equal(pri["bias_priori"][0], rec.updated_bias)


def test_a_record_without_samples_is_refused_everywhere():
    cal = im.calib()
    recs = [fm.make_record(cal, 0, 1), fm.make_record(cal, 3, 2)]
    edges = np.array([(0, 1, 0, 1), (0, 1, 1, 1), (0, 1, 2, 0)], fm.EDGE)
    info, walk, res = fm.edge_information(recs, edges)
    assert res.tolist()[:4] == [1, 1, 0, 1] and not info[0].any() and not walk[0].any() and info[1].any() and not info[2].any()
    pri = np.full(1, 7, np.uint8).view(np.uint8).repeat(144).view(fm.PRIOR)
    before = pri.copy()
    res, _ = fm.prior_information(pri, recs, None, np.array([[0, 0, -1]], np.int32))
    assert res[fm.R_REFUSED] == 1 and pri.tobytes() == before.tobytes()
