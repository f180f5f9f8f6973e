"""The IMU preintegration and pose prediction (include/orbi.h) without a GPU: the numpy model of tests/imu_model.py judged against an
independent object-style restatement of Imu.cpp and against its own float64 run, the two pose directions composed, and the ABI
(exports, argument checks before the device is looked for, no CPU path)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import imu_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- an independent restatement of Imu.cpp: objects, dense products, an SVD -------------------------------------------------------
def _hat(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def _exp(v):
    d = np.linalg.norm(v)
    W = _hat(v)
    return np.eye(3) + W + 0.5 * W @ W if d < 1e-6 else np.eye(3) + np.sin(d) / d * W + (1 - np.cos(d)) / d ** 2 * W @ W


def _right_jacobian(v):
    d = np.linalg.norm(v)
    W = _hat(v)
    return np.eye(3) if d < 1e-6 else np.eye(3) - (1 - np.cos(d)) / d ** 2 * W + (d - np.sin(d)) / d ** 3 * W @ W


def _normalize(R):
    U, _, Vt = np.linalg.svd(R)
    return U @ Vt


class PreIntegrator:
    """Imu.cpp:76-204 in float64, written from the reference alone"""

    def __init__(self, cal, bias):
        self.noise, self.walk = np.diag(cal["cov_noise"].astype(np.float64)), np.diag(cal["cov_walk"].astype(np.float64))
        self.bias = np.asarray(bias, np.float64).copy()
        self.measurements = []
        self._reset()

    def _reset(self):
        self.delta_t, self.C = 0.0, np.zeros((15, 15))
        self.dR, self.dV, self.dP = np.eye(3), np.zeros(3), np.zeros(3)
        self.JRg, self.JVg, self.JVa, self.JPg, self.JPa = (np.zeros((3, 3)) for _ in range(5))
        self.updated_bias, self.delta_bias = self.bias.copy(), np.zeros(6)

    def Reset(self, bias):
        self.bias = np.asarray(bias, np.float64).copy()
        self._reset()
        self.measurements = []

    def IntegrateNewMeasurement(self, gyro, acc, dt):
        gyro, acc, dt = np.asarray(gyro, np.float64), np.asarray(acc, np.float64), float(dt)
        self.measurements.append((gyro, acc, dt))
        A, B = np.eye(9), np.zeros((9, 6))
        w, a = gyro - self.bias[:3], acc - self.bias[3:]
        dR = self.dR
        self.dP = self.dP + self.dV * dt + 0.5 * dR @ a * dt * dt
        self.dV = self.dV + dR @ a * dt
        aHat = _hat(a)
        A[3:6, 0:3] = -dR @ aHat * dt
        A[6:9, 0:3] = -0.5 * dR @ aHat * dt * dt
        A[6:9, 3:6] = dt * np.eye(3)
        B[3:6, 3:6] = dR * dt
        B[6:9, 3:6] = 0.5 * dR * dt * dt
        self.JPg = self.JPg + self.JVg * dt - 0.5 * dR @ aHat @ self.JRg * dt * dt
        self.JPa = self.JPa + self.JVa * dt - 0.5 * dR * dt * dt
        self.JVg = self.JVg - dR @ aHat @ self.JRg * dt
        self.JVa = self.JVa - dR * dt
        deltaR, rightJ = _exp(w * dt), _right_jacobian(w * dt)
        self.dR = _normalize(dR @ deltaR)
        A[0:3, 0:3] = deltaR.T
        B[0:3, 0:3] = rightJ * dt
        self.C[:9, :9] = A @ self.C[:9, :9] @ A.T + B @ self.noise @ B.T
        self.C[9:, 9:] += self.walk
        self.JRg = deltaR.T @ self.JRg - rightJ * dt
        self.delta_t += dt

    def ReIntegrate(self):
        copy = self.measurements
        self.Reset(self.updated_bias)
        for w, a, dt in copy:
            self.IntegrateNewMeasurement(w, a, dt)

    def MergeNext(self, other):
        if other is self:
            return
        m1, m2 = list(self.measurements), list(other.measurements)
        if np.linalg.norm(self.delta_bias[:3]) > 1e-5:
            self.Reset(self.updated_bias)
            for m in m1:
                self.IntegrateNewMeasurement(*m)
        for m in m2:
            self.IntegrateNewMeasurement(*m)

    def setNewBias(self, bias):
        self.updated_bias = np.asarray(bias, np.float64).copy()
        self.delta_bias = self.updated_bias - self.bias
        if np.linalg.norm(self.delta_bias[:3]) > 0.01:
            self.ReIntegrate()

    def computePreIntegration(self, samples, timestamp, end_time):
        start = timestamp + self.delta_t
        n, t = len(samples), samples["t"]
        if n == 1:
            return self.IntegrateNewMeasurement(samples["w"][0], samples["a"][0], np.float32(end_time - start))
        for i in range(n):
            dt = t[i + 1] - start if i == 0 else end_time - t[i] if i == n - 1 else t[i + 1] - t[i]
            self.IntegrateNewMeasurement(samples["w"][i], samples["a"][i], np.float32(dt))


def _rel(a, b):
    """largest deviation relative to the quantity's largest entry"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max()
    return float(np.abs(a - b).max() / scale) if scale > 0 else float(np.abs(a).max())


def _compare(rec, obj, what, bound):
    worst = max(_rel(getattr(rec, k), getattr(obj, k)) for k in im.FIELDS)
    assert len(rec.meas) == len(obj.measurements), what
    assert worst <= bound, (what, {k: _rel(getattr(rec, k), getattr(obj, k)) for k in im.FIELDS})
    return worst


def test_model_float64_equals_the_object_restatement_after_every_operation():
    """A scripted life of two key frames' integrators: reset, integrate (12, 1 and 0 samples; a second batch into the same record), a
    bias step below and one above 0.01, a merge with delta_bias.bg below and one above 1e-5, a merge with itself.  After EVERY
    operation every field of the model's float64 run equals the restatement's within 1e-10 of the field's largest entry: both are
    float64 (eps 2.2e-16), the only differences are summation order and Newton against SVD on a matrix that is orthogonal to a few
    eps, over fewer than 100 samples; measured 1.9e-15."""
    cal = im.calib()
    rng = np.random.RandomState(7)
    b0, b1 = im.random_bias(rng), im.random_bias(rng)
    s = im.make_stream(60, 5)
    recs = [im.Rec(np.float64), im.Rec(np.float64)]
    objs = [PreIntegrator(cal, np.zeros(6)), PreIntegrator(cal, np.zeros(6))]
    worst = [0.0]

    def both(what, f_model, f_obj):
        f_model(), f_obj()
        for r, o in zip(recs, objs):
            worst[0] = max(worst[0], _compare(r, o, what, 1e-10))

    T = lambda a, b: (s["t"][a] - 0.4 / im.RATE, s["t"][b - 1] + 0.6 / im.RATE)  # noqa: E731
    both("reset", lambda: [recs[0].reset(b0), recs[1].reset(b1)], lambda: [objs[0].Reset(b0), objs[1].Reset(b1)])
    t0, t1 = T(0, 12)
    both("integrate 12", lambda: recs[0].compute_preintegration(cal, s[0:12], t0, t1), lambda: objs[0].computePreIntegration(s[0:12], t0, t1))
    both("integrate 1", lambda: recs[0].compute_preintegration(cal, s[12:13], t0, s["t"][13]), lambda: objs[0].computePreIntegration(s[12:13], t0, s["t"][13]))
    both("integrate 0", lambda: recs[0].compute_preintegration(cal, s[13:13], t0, s["t"][13]), lambda: objs[0].computePreIntegration(s[13:13], t0, s["t"][13]))
    t2, t3 = T(13, 30)
    both("integrate next", lambda: recs[1].compute_preintegration(cal, s[13:30], t2, t3), lambda: objs[1].computePreIntegration(s[13:30], t2, t3))
    small, big = b0 + np.array([0.004, 0, 0, 0.01, 0, 0], np.float32), b0 + np.array([0.008, -0.007, 0.002, 0.01, 0, 0.02], np.float32)
    both("bias below 0.01", lambda: recs[0].set_new_bias(cal, small), lambda: objs[0].setNewBias(small))
    assert recs[0].delta_bias.any() and not np.array_equal(recs[0].bias, recs[0].updated_bias)
    both("bias above 0.01", lambda: recs[0].set_new_bias(cal, big), lambda: objs[0].setNewBias(big))
    assert not recs[0].delta_bias.any() and np.array_equal(recs[0].bias, big.astype(np.float64))
    tiny = big + np.array([4e-6, 0, 0, 0, 0, 0], np.float32)
    both("bias step of 4e-6", lambda: recs[0].set_new_bias(cal, tiny), lambda: objs[0].setNewBias(tiny))
    n0 = len(recs[0].meas)
    both("merge below 1e-5", lambda: recs[0].merge_next(cal, recs[1].copy()), lambda: objs[0].MergeNext(objs[1]))
    assert 0 < np.linalg.norm(recs[0].delta_bias[:3]) < 1e-5 and len(recs[0].meas) == n0 + 17
    step = b1 + np.array([0, 5e-5, 0, 0, 0, 0], np.float32)
    both("bias step of 5e-5", lambda: recs[1].set_new_bias(cal, step), lambda: objs[1].setNewBias(step))
    both("merge above 1e-5", lambda: recs[1].merge_next(cal, recs[0].copy()), lambda: objs[1].MergeNext(objs[0]))
    assert not recs[1].delta_bias.any() and len(recs[1].meas) == 17 + n0 + 17
    both("merge with itself", lambda: None, lambda: objs[1].MergeNext(objs[1]))   # the model's entry point counts it and does nothing
    print("largest relative deviation over the script: %.3g" % worst[0])


_long = {}


def _long_run(n):
    """one record through n samples of the committed stream in float32 and in float64 (cached)"""
    if n not in _long:
        cal, s = im.calib(), im.make_stream(n, 9)
        bias = im.random_bias(np.random.RandomState(11))
        out = []
        for D in (np.float32, np.float64):
            r = im.Rec(D, bias)
            r.compute_preintegration(cal, s, s["t"][0] - 0.4 / im.RATE, s["t"][-1] + 0.6 / im.RATE)
            out.append(r)
        _long[n] = out
    return _long[n]


# measured on the committed stream (make_stream(n, 9)): the largest deviation of the float32 run from the float64 run, relative to the
# quantity's largest entry, per field; the assertion is at 4 x these, DESIGN.md section 5's bar for the triangulation
MEASURED = {
    200: dict(delta_t=8.39e-8, dR=2.00e-7, dV=1.66e-7, dP=1.08e-7, JRg=8.34e-7, JVg=1.78e-6, JVa=1.43e-7, JPg=2.60e-6, JPa=3.56e-7, C=2.06e-6),
    1000: dict(delta_t=3.22e-7, dR=6.34e-7, dV=4.61e-7, dP=1.71e-7, JRg=3.00e-6, JVg=7.09e-7, JVa=6.17e-7, JPg=1.12e-6, JPa=1.17e-6, C=2.35e-6),
}


@pytest.mark.parametrize("n", [200, 1000])
def test_model_float32_against_its_float64_run(n):
    """One record through 200 and through 1000 samples (1 s and 5 s at 200 Hz: a frame's and a long key frame's integration) of the
    committed stream, in float32 and in float64.  Measured, relative to each quantity's largest entry: at 200 samples delta_t 8.4e-8,
    dR 2.0e-7, dV 1.7e-7, dP 1.1e-7, JRg 8.3e-7, JVg 1.8e-6, JVa 1.4e-7, JPg 2.6e-6, JPa 3.6e-7, C 2.1e-6; at 1000 samples delta_t
    3.2e-7, dR 6.3e-7, dV 4.6e-7, dP 1.7e-7, JRg 3.0e-6, JVg 7.1e-7, JVa 6.2e-7, JPg 1.1e-6, JPa 1.2e-6, C 2.4e-6 -- a few float32 eps
    (6e-8) times the square root of the sample count; |R^T R - I| of dR 7.3e-8 and 8.5e-8.  Asserted at 4 x the measured values."""
    r32, r64 = _long_run(n)
    got = {k: _rel(getattr(r32, k), getattr(r64, k)) for k in MEASURED[n]}
    print(n, {k: "%.3g" % v for k, v in got.items()})
    ortho = np.abs(r32.dR.astype(np.float64).T @ r32.dR.astype(np.float64) - np.eye(3)).max()
    print("|R^T R - I| = %.3g" % ortho)
    assert ortho <= 4 * 1.2e-7           # include/orbi.h: two Newton steps keep dR orthogonal
    for k, v in got.items():
        assert v <= 4 * MEASURED[n][k], (k, v, MEASURED[n][k])


# measured: the largest deviation of imu_pose(predict(...)) from predict's own (Rwb2, twb2), relative to the largest entry
MEASURED_ROUND_TRIP = dict(R=1.20e-7, t=1.11e-7)


def test_the_two_pose_directions_compose_to_the_identity():
    """T_wb -> T_cw = T_cb * T_wb^-1 (orbi_predict_device) -> T_wb = T_cw^-1 * T_cb (orbi_imu_pose_device) on the three states of the
    prediction scene, float32: back at the start within 4 x the measured deviation (MEASURED_ROUND_TRIP: a few float32 eps of the
    largest entry -- two 3x3 products and two translations by vectors of a few metres).  The float64 run closes to 1e-14."""
    sc = im.make_predict_scene()
    worst = dict(R=0.0, t=0.0)
    for i, src in enumerate(sc["src"]):
        for D in (np.float32, np.float64):
            r = sc["bank"].recs[i].copy()
            if D is np.float64:
                r64 = im.Rec(np.float64)
                for k in im.FIELDS:
                    setattr(r64, k, np.asarray(getattr(r, k), np.float64))
                r = r64
            dst, Rcw, tcw = im.predict(sc["cal"], r, src)
            Rwb, twb = im.imu_pose(sc["cal"], Rcw, tcw, D)
            dR, dt = _rel(Rwb, dst[:9].reshape(3, 3)), _rel(twb, dst[9:12])
            if D is np.float64:      # (the float64 pose passes through imu_pose's rounding to float: float32 eps)
                assert dR <= 2e-7 and dt <= 2e-7
            else:
                worst["R"], worst["t"] = max(worst["R"], dR), max(worst["t"], dt)
    print({k: "%.3g" % v for k, v in worst.items()})
    assert worst["R"] <= 4 * MEASURED_ROUND_TRIP["R"] and worst["t"] <= 4 * MEASURED_ROUND_TRIP["t"]


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def imu():
    import __graft_entry__ as g
    g.build()
    from monoorbslam3_amd import imu
    return imu


def _declared():
    txt = open(os.path.join(ROOT, "include", "orbi.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(orbi_[a-z0-9_]+)\s*\(", txt)))


ENTRY_POINTS = ["orbi_imu_pose_device", "orbi_integrate_device", "orbi_merge_next_device", "orbi_predict_device", "orbi_reset_device",
                "orbi_set_bias_device"]


def test_every_declared_entry_point_is_exported_and_mirrored(imu):
    from monoorbslam3_amd import _lib
    assert _declared() == ENTRY_POINTS
    L = C.CDLL(_lib.LIB_PATH)
    for n in ENTRY_POINTS:
        assert hasattr(L, n), "liborbx.so does not export %s" % n
        assert callable(getattr(imu, n[len("orbi_"):])), n
    assert C.sizeof(imu.Calib) == 100 and imu.RECORD.itemsize == imu.RECORD_BYTES == im.RECORD.itemsize
    assert imu.RECORD == im.RECORD and imu.SAMPLE == im.SAMPLE and imu.JOB == im.JOB
    header = open(os.path.join(ROOT, "include", "orbi.h")).read()
    assert "#define ORBI_RECORD_BYTES %d" % imu.RECORD_BYTES in header and "#define ORBI_MAX_JOBS %d" % imu.MAX_JOBS in header


def _calib(imu):
    c = im.calib()
    return imu.Calib.make(c["Rcb"], c["tcb"], c["cov_noise"], c["cov_walk"], c["gravity"])


def _calls(imu, **over):
    """every wrapper with valid arguments (fake device addresses, never dereferenced) except for `over`"""
    a = dict(bank=0x1000, pool=0x1000, cap=8, cap_meas=16, ids=0x1000, second=0x1000, bias=0x1000, n=2, jobs=0x1000, samples=0x1000,
             n_samples=10, result=0x1000, rec_id=3, src=0x1000, dst=0x1000, pose_R=0x1000, pose_t=0x1000)
    a.update(over)
    cal = _calib(imu)
    return dict(
        reset=lambda: imu.reset_device(a["bank"], a["cap"], a["ids"], a["n"], a["result"], a["second"], a["bias"]),
        integrate=lambda: imu.integrate_device(cal, a["bank"], a["pool"], a["cap"], a["cap_meas"], a["jobs"], a["n"], a["samples"], a["n_samples"], a["result"]),
        set_bias=lambda: imu.set_bias_device(cal, a["bank"], a["pool"], a["cap"], a["cap_meas"], a["ids"], a["bias"], a["n"], a["result"]),
        merge_next=lambda: imu.merge_next_device(cal, a["bank"], a["pool"], a["cap"], a["cap_meas"], a["ids"], a["second"], a["n"], a["result"]),
        predict=lambda: imu.predict_device(cal, a["bank"], a["cap"], a["rec_id"], a["src"], a["dst"], a["pose_R"], a["pose_t"]),
        imu_pose=lambda: imu.imu_pose_device(cal, a["pose_R"], a["pose_t"], a["dst"]))


def _code(call):
    from monoorbslam3_amd._lib import OrbxError
    with pytest.raises(OrbxError) as e:
        call()
    return e.value.code


def test_argument_errors_are_reported_before_the_device_is_looked_for(imu):
    E_ARG, E_UNSUPPORTED = -1, -4
    jobs = ("reset", "integrate", "set_bias", "merge_next")
    cases = [(dict(bank=None), jobs + ("predict",)), (dict(cap=0), jobs + ("predict",)), (dict(n=-1), jobs), (dict(result=None), jobs),
             (dict(ids=None), ("reset", "set_bias", "merge_next")), (dict(pool=None), jobs[1:]), (dict(cap_meas=0), jobs[1:]),
             (dict(jobs=None), ("integrate",)), (dict(samples=None), ("integrate",)), (dict(n_samples=-1), ("integrate",)),
             (dict(bias=None), ("set_bias",)), (dict(second=None), ("merge_next",)), (dict(rec_id=-1), ("predict",)),
             (dict(rec_id=8), ("predict",)), (dict(src=None), ("predict",)), (dict(dst=None), ("predict", "imu_pose")),
             (dict(pose_R=None), ("predict", "imu_pose")), (dict(pose_t=None), ("predict", "imu_pose"))]
    for over, names in cases:
        for name in names:
            assert _code(_calls(imu, **over)[name]) == E_ARG, (over, name)
    for name in jobs:
        assert _code(_calls(imu, n=imu.MAX_JOBS + 1)[name]) == E_UNSUPPORTED, name


def test_every_wrapper_fails_loudly_without_a_gpu(imu):
    import torch
    if torch.cuda.is_available():
        pytest.skip("needs a machine without a GPU")
    from monoorbslam3_amd import _lib
    for name, call in _calls(imu).items():
        assert _code(call) == -2, name
        assert b"no HIP device" in _lib.lib().orbx_last_error(), name
    # the optional arguments are optional: still the device that is missing, not an argument
    assert _code(_calls(imu, second=None, bias=None)["reset"]) == -2 and _code(_calls(imu, pose_R=None, pose_t=None)["predict"]) == -2
    assert _code(_calls(imu, n=0)["integrate"]) == -2
