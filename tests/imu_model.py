"""Plain numpy restatement of include/orbi.h: the IMU preintegration (reference modules/Sensor/Imu.cpp:76-204), the dt rule of
Frame.cpp:73-88, the prediction of Tracking.cpp:185-243 and the two pose directions of Frame.cpp:57-71, in the evaluation orders the
header fixes.  Parametrised by dtype: the float32 run is the model the device is compared with bit for bit, the float64 run is the
yardstick the float32 run is judged by.  No `@`, no BLAS: every sum over k is written as elementwise operations in ascending k.
sinf / cosf of the float32 run come from the host libm through ctypes.  The seeded scenes of both test files live here too; each
asserts that it holds the cases it is meant to hold.  No part of the library is used here."""
import ctypes
import ctypes.util
import math

import numpy as np

R_DONE, R_RANGE, R_DUPLICATE, R_REFUSED, R_NEED, R_REINTEGRATED, R_NOOP = range(7)

RECORD = np.dtype([("bias", "<f4", 6), ("updated_bias", "<f4", 6), ("delta_bias", "<f4", 6), ("delta_t", "<f4"), ("dR", "<f4", 9),
                   ("dV", "<f4", 3), ("dP", "<f4", 3), ("JRg", "<f4", 9), ("JVg", "<f4", 9), ("JVa", "<f4", 9), ("JPg", "<f4", 9),
                   ("JPa", "<f4", 9), ("C", "<f4", 225), ("n_meas", "<i4"), ("pad", "<i4", 3)])
SAMPLE = np.dtype([("w", "<f4", 3), ("a", "<f4", 3), ("t", "<f8")])
JOB = np.dtype([("id", "<i4"), ("first", "<i4"), ("count", "<i4"), ("pad", "<i4"), ("timestamp", "<f8"), ("end_time", "<f8")])
assert RECORD.itemsize == 1232 and SAMPLE.itemsize == 32 and JOB.itemsize == 32
MATS = ("dR", "JRg", "JVg", "JVa", "JPg", "JPa")
FIELDS = ("bias", "updated_bias", "delta_bias", "delta_t", "dR", "dV", "dP") + MATS[1:] + ("C",)

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = _libm.cosf.restype = ctypes.c_float
_libm.sinf.argtypes = _libm.cosf.argtypes = [ctypes.c_float]


def calib(Rcb=None, tcb=(0.0148, -0.0650, 0.0069), noise_gyro=1.7e-4, noise_acc=2.0e-3, walk_gyro=1.9393e-5, walk_acc=3.0e-3, gravity=9.8):
    """ImuCalib as orbi_calib holds it: float32 values (EuRoC-like defaults)"""
    f = np.float32
    if Rcb is None:
        Rcb = rodrigues(np.array([0.02, -1.55, 0.03]))
    ng, na, wg, wa = f(noise_gyro) * f(noise_gyro), f(noise_acc) * f(noise_acc), f(walk_gyro) * f(walk_gyro), f(walk_acc) * f(walk_acc)
    return dict(Rcb=np.asarray(Rcb, np.float32).reshape(3, 3), tcb=np.asarray(tcb, np.float32), cov_noise=np.array([ng] * 3 + [na] * 3, np.float32),
                cov_walk=np.array([wg] * 3 + [wa] * 3, np.float32), gravity=f(gravity))


def rodrigues(w):
    """a float64 rotation for building scenes (not part of the model)"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    return np.eye(3) if th < 1e-12 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


# ---- the arithmetic, header order ----------------------------------------------------------------------------------------------
def mm(A, B):
    """A (n x 3) * B (3 x m): (a_i0*b_0j + a_i1*b_1j) + a_i2*b_2j"""
    return (A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :]) + A[:, 2:3] * B[2:3, :]


def mv(A, x):
    return (A[:, 0] * x[0] + A[:, 1] * x[1]) + A[:, 2] * x[2]


def hat(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], v.dtype)


def norm3(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def _sincos(d):
    if d.dtype == np.float32:
        return np.float32(_libm.sinf(float(d))), np.float32(_libm.cosf(float(d)))
    return np.float64(math.sin(float(d))), np.float64(math.cos(float(d)))


def exp_and_right_jacobian(v):
    """ExpSO3f(v), RightJacobianSO3f(v) (LieAlgeBra.cpp:47-58, 94-102); the branch compares in double"""
    D = v.dtype.type
    I, W = np.eye(3, dtype=D), hat(v)
    d2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
    d = np.sqrt(d2)
    if float(d) < 1e-6:
        return (I + W) + mm(D(0.5) * W, W), I
    sn, cs = _sincos(d)
    s1, s2, s3 = sn / d, (D(1) - cs) / d2, (d - sn) / (d2 * d)
    return (I + s1 * W) + mm(s2 * W, W), (I - s2 * W) + mm(s3 * W, W)


def newton(X):
    """one step X <- 0.5*(X + cof(X)/det(X))"""
    D = X.dtype.type
    r = lambda a, b: np.roll(X, (-a, -b), (0, 1))  # noqa: E731   r(a, b)[i, j] = X[(i+a)%3, (j+b)%3]
    cof = r(1, 1) * r(2, 2) - r(1, 2) * r(2, 1)
    det = (X[0, 0] * cof[0, 0] + X[0, 1] * cof[0, 1]) + X[0, 2] * cof[0, 2]
    return D(0.5) * (X + cof / det)


def normalize_rotation(X):
    return newton(newton(X))


class Rec:
    """one PreIntegrator in dtype D; `meas` is the pool row (list of (w, a, dt))"""

    def __init__(self, D, bias=None):
        self.D = D
        self.bias = np.zeros(6, D) if bias is None else np.asarray(bias, D).copy()
        self.meas = []
        self._reset()

    def _reset(self):
        D = self.D
        self.delta_t = D(0)
        self.C = np.zeros((15, 15), D)
        self.dR, self.dV, self.dP = np.eye(3, dtype=D), np.zeros(3, D), np.zeros(3, D)
        self.JRg, self.JVg, self.JVa, self.JPg, self.JPa = (np.zeros((3, 3), D) for _ in range(5))
        self.updated_bias, self.delta_bias = self.bias.copy(), np.zeros(6, D)

    def reset(self, bias):
        self.bias = np.asarray(bias, self.D).copy()
        self._reset()
        self.meas = []

    def copy(self):
        o = Rec(self.D)
        for k in FIELDS:
            setattr(o, k, np.array(getattr(self, k), self.D, copy=True) if np.ndim(getattr(self, k)) else getattr(self, k))
        o.meas = list(self.meas)
        return o

    def integrate(self, cal, gyro, acc, dt):
        """IntegrateNewMeasurement (Imu.cpp:101-148)"""
        D = self.D
        gyro, acc, dt = np.asarray(gyro, np.float32).astype(D), np.asarray(acc, np.float32).astype(D), D(np.float32(dt))
        self.meas.append((gyro.astype(np.float32), acc.astype(np.float32), np.float32(dt)))
        h = D(0.5)
        w, a = gyro - self.bias[:3], acc - self.bias[3:]
        dt2 = dt * dt
        dR = self.dR
        Ra = mv(dR, a)
        RA = mm(dR, hat(a))
        RAJ = mm(RA, self.JRg)
        dP = (self.dP + self.dV * dt) + (h * Ra) * dt2
        dV = self.dV + Ra * dt
        JPg = (self.JPg + self.JVg * dt) - (h * RAJ) * dt2
        JVg = self.JVg - RAJ * dt
        JPa = (self.JPa + self.JVa * dt) - (h * dR) * dt2
        JVa = self.JVa - dR * dt
        A10, A20 = (-RA) * dt, (-(h * RA)) * dt2
        B11, B21 = dR * dt, (h * dR) * dt2
        dE, Jr = exp_and_right_jacobian(w * dt)
        self.dR = normalize_rotation(mm(dR, dE))
        A00, B00 = dE.T, Jr * dt
        C = self.C[:9, :9]
        T = np.empty((9, 9), D)
        T[0:3] = mm(A00, C[0:3])
        T[3:6] = mm(A10, C[0:3]) + C[3:6]
        T[6:9] = (mm(A20, C[0:3]) + dt * C[3:6]) + C[6:9]
        S = np.empty((9, 9), D)
        S[:, 0:3] = mm(T[:, 0:3], A00.T)
        S[:, 3:6] = mm(T[:, 0:3], A10.T) + T[:, 3:6]
        S[:, 6:9] = (mm(T[:, 0:3], A20.T) + T[:, 3:6] * dt) + T[:, 6:9]
        ng, na = cal["cov_noise"][:3].astype(D), cal["cov_noise"][3:].astype(D)
        q = lambda X, Y, n: mm(X * n[None, :], Y.T)  # noqa: E731   ((x_i0*n_0)*y_j0 + (x_i1*n_1)*y_j1) + (x_i2*n_2)*y_j2
        S[0:3, 0:3] = S[0:3, 0:3] + q(B00, B00, ng)
        S[3:6, 3:6] = S[3:6, 3:6] + q(B11, B11, na)
        S[3:6, 6:9] = S[3:6, 6:9] + q(B11, B21, na)
        S[6:9, 3:6] = S[6:9, 3:6] + q(B21, B11, na)
        S[6:9, 6:9] = S[6:9, 6:9] + q(B21, B21, na)
        self.C[:9, :9] = S
        for i in range(6):
            self.C[9 + i, 9 + i] = self.C[9 + i, 9 + i] + cal["cov_walk"][i].astype(D)
        self.JRg = mm(A00, self.JRg) - Jr * dt
        self.dP, self.dV, self.JPg, self.JVg, self.JPa, self.JVa = dP, dV, JPg, JVg, JPa, JVa
        self.delta_t = self.delta_t + dt

    def compute_preintegration(self, cal, samples, timestamp, end_time):
        """Frame::computePreIntegration (Frame.cpp:73-88): doubles, each dt rounded to float once"""
        start = np.float64(timestamp) + np.float64(self.delta_t)
        n, t = len(samples), samples["t"]
        for i in range(n):
            if n == 1:
                dt = end_time - start
            elif i == 0:
                dt = t[1] - start
            elif i == n - 1:
                dt = end_time - t[i]
            else:
                dt = t[i + 1] - t[i]
            self.integrate(cal, samples["w"][i], samples["a"][i], np.float32(np.float64(dt)))

    def reintegrate(self, cal):
        meas = self.meas
        self.reset(self.updated_bias)
        for w, a, dt in meas:
            self.integrate(cal, w, a, dt)

    def set_new_bias(self, cal, bias):
        """setNewBias (Imu.cpp:174-180); True when it re-integrated"""
        self.updated_bias = np.asarray(bias, np.float32).astype(self.D)
        self.delta_bias = self.updated_bias - self.bias
        if float(norm3(self.delta_bias[:3])) > 0.01:
            self.reintegrate(cal)
            return True
        return False

    def merge_next(self, cal, nxt):
        """MergeNext (Imu.cpp:157-172) for nxt is not self; True when it took the Reset branch"""
        m1, m2 = list(self.meas), list(nxt.meas)
        redo = float(norm3(self.delta_bias[:3])) > 1e-5
        if redo:
            self.reset(self.updated_bias)
            for w, a, dt in m1:
                self.integrate(cal, w, a, dt)
        for w, a, dt in m2:
            self.integrate(cal, w, a, dt)
        return redo

    def updated_deltas(self):
        """getUpdatedDeltaRotation / Velocity / Position (Imu.cpp:194-204)"""
        dbg, dba = self.delta_bias[:3], self.delta_bias[3:]
        dE, _ = exp_and_right_jacobian(mv(self.JRg, dbg))
        return (normalize_rotation(mm(self.dR, dE)), (self.dV + mv(self.JVg, dbg)) + mv(self.JVa, dba),
                (self.dP + mv(self.JPg, dbg)) + mv(self.JPa, dba))


def predict(cal, rec, src):
    """Tracking.cpp:211-243 + Frame.cpp:65-71.  src: 15 floats (Rwb, twb, v).  Returns (dst 15, Rcw 3x3, tcw 3) in rec.D."""
    D = rec.D
    src = np.asarray(src, np.float32).astype(D)
    Rwb, twb, v = src[:9].reshape(3, 3), src[9:12], src[12:15]
    dRu, dVu, dPu = rec.updated_deltas()
    dt = rec.delta_t
    g = np.array([0, 0, -cal["gravity"]], np.float32).astype(D)
    Rwb2 = normalize_rotation(mm(Rwb, dRu))
    twb2 = ((twb + v * dt) + ((D(0.5) * g) * dt) * dt) + mv(Rwb, dPu)
    v2 = (v + g * dt) + mv(Rwb, dVu)
    Rcb, tcb = cal["Rcb"].astype(D), cal["tcb"].astype(D)
    Rbw = Rwb2.T
    tbw = mv(-Rbw, twb2)
    return np.concatenate([Rwb2.reshape(9), twb2, v2]), mm(Rcb, Rbw), mv(Rcb, tbw) + tcb


def imu_pose(cal, pose_R, pose_t, D=np.float32):
    """Frame.cpp:57-63 from the doubles poseOptimize leaves, rounded to float first.  Returns (Rwb 3x3, twb 3)."""
    R = np.asarray(pose_R, np.float64).reshape(3, 3).astype(np.float32).astype(D)
    t = np.asarray(pose_t, np.float64).reshape(3).astype(np.float32).astype(D)
    Rcb, tcb = cal["Rcb"].astype(D), cal["tcb"].astype(D)
    Rwc = R.T
    twc = mv(-Rwc, t)
    return mm(Rwc, Rcb), mv(Rwc, tcb) + twc


# ---- the bank, the pool and the entry points' job rules --------------------------------------------------------------------------
class Bank:
    """`cap` records and their pool rows; pack() gives the bytes the device must hold (float32 runs only)"""

    def __init__(self, cap, cap_meas, D=np.float32, fill=None):
        self.cap, self.cap_meas, self.D = cap, cap_meas, D
        self.recs = [Rec(D) for _ in range(cap)]
        self.pool_fill = np.float32(-7.25) if fill is None else np.float32(fill)
        # what a pool row holds behind its measurements: whatever was there before (the device never clears a row)
        self.stale = np.full((cap, cap_meas, 7), self.pool_fill, np.float32)

    def copy(self):
        o = Bank(self.cap, self.cap_meas, self.D, self.pool_fill)
        o.recs, o.stale = [r.copy() for r in self.recs], self.stale.copy()
        return o

    def pack(self):
        bank = np.zeros(self.cap, RECORD)
        pool = self.stale.copy()
        for i, r in enumerate(self.recs):
            for k in FIELDS:
                bank[k][i] = np.asarray(getattr(r, k), np.float32).reshape(-1) if np.ndim(getattr(r, k)) else np.float32(getattr(r, k))
            bank["n_meas"][i] = len(r.meas)
            for m, (w, a, dt) in enumerate(r.meas):
                pool[i, m, :3], pool[i, m, 3:6], pool[i, m, 6] = w, a, dt
        self.stale = pool.copy()      # a later reset leaves these values in the row
        return bank, pool


def _conflicts(ids, second):
    """job j is a duplicate when an earlier job j' has id_j == id_j', id_j == second_j' or second_j == id_j' (second >= 0 only)"""
    out = np.zeros(len(ids), bool)
    for j in range(len(ids)):
        for k in range(j):
            if ids[j] == ids[k] or (second[j] >= 0 and second[j] == ids[k]) or (second[k] >= 0 and ids[j] == second[k]):
                out[j] = True
                break
    return out


def _result():
    return np.zeros(8, np.int32)


def run_reset(bank, ids, src=None, bias=None):
    ids = np.asarray(ids, np.int64)
    second = np.full(len(ids), -1, np.int64) if src is None else np.asarray(src, np.int64)
    res, dup = _result(), _conflicts(ids, second)
    bank.pack()                                     # the rows keep what they hold
    new = {}
    for j, (i, s) in enumerate(zip(ids, second)):
        if not (0 <= i < bank.cap) or not (-1 <= s < bank.cap):
            res[R_RANGE] += 1
        elif dup[j]:
            res[R_DUPLICATE] += 1
        else:
            b = bank.recs[s].updated_bias if s >= 0 else (np.zeros(6, np.float32) if bias is None else np.asarray(bias, np.float32).reshape(-1, 6)[j])
            new[i] = Rec(bank.D, np.asarray(b).astype(bank.D))
            res[R_DONE] += 1
    for i, r in new.items():
        bank.recs[i] = r
    return res


def run_integrate(cal, bank, jobs, samples):
    ids = jobs["id"].astype(np.int64)
    res, dup = _result(), _conflicts(ids, np.full(len(ids), -1))
    for j, job in enumerate(jobs):
        i, first, count = int(job["id"]), int(job["first"]), int(job["count"])
        if not (0 <= i < bank.cap) or first < 0 or count < 0 or first > len(samples) or count > len(samples) - first:
            res[R_RANGE] += 1
        elif dup[j]:
            res[R_DUPLICATE] += 1
        elif len(bank.recs[i].meas) + count > bank.cap_meas:
            res[R_REFUSED] += 1
            res[R_NEED] = max(res[R_NEED], len(bank.recs[i].meas) + count)
        else:
            bank.recs[i].compute_preintegration(cal, samples[first:first + count], job["timestamp"], job["end_time"])
            res[R_DONE] += 1
    return res


def run_set_bias(cal, bank, ids, bias):
    ids = np.asarray(ids, np.int64)
    res, dup = _result(), _conflicts(ids, np.full(len(ids), -1))
    for j, i in enumerate(ids):
        if not (0 <= i < bank.cap):
            res[R_RANGE] += 1
        elif dup[j]:
            res[R_DUPLICATE] += 1
        else:
            res[R_REINTEGRATED] += bool(bank.recs[i].set_new_bias(cal, np.asarray(bias, np.float32).reshape(-1, 6)[j]))
            res[R_DONE] += 1
    return res


def run_merge(cal, bank, ids, nxt):
    ids, nxt = np.asarray(ids, np.int64), np.asarray(nxt, np.int64)
    res, dup = _result(), _conflicts(ids, nxt)
    before = [r.copy() for r in bank.recs]          # a `next` is never a record another kept job writes: the state as passed
    for j, (i, k) in enumerate(zip(ids, nxt)):
        if not (0 <= i < bank.cap) or not (0 <= k < bank.cap):
            res[R_RANGE] += 1
        elif dup[j]:
            res[R_DUPLICATE] += 1
        elif i == k:
            res[R_DONE] += 1
            res[R_NOOP] += 1
        elif len(before[i].meas) + len(before[k].meas) > bank.cap_meas:
            res[R_REFUSED] += 1
            res[R_NEED] = max(res[R_NEED], len(before[i].meas) + len(before[k].meas))
        else:
            res[R_REINTEGRATED] += bool(bank.recs[i].merge_next(cal, before[k]))
            res[R_DONE] += 1
    return res


# ---- scenes ------------------------------------------------------------------------------------------------------------------------
RATE = 200.0      # Hz


def make_stream(n, seed, t0=100.0):
    """n samples at 200 Hz with time jitter: a hand-held motion's gyro (rad/s) and accelerometer (m/s^2, gravity included)"""
    rng = np.random.RandomState(seed)
    s = np.zeros(n, SAMPLE)
    k = np.arange(n)
    ph = rng.uniform(0, 2 * np.pi, 6)
    s["w"] = np.stack([0.4 * np.sin(0.031 * k + ph[0]), 0.25 * np.sin(0.017 * k + ph[1]), 0.6 * np.sin(0.023 * k + ph[2])], 1) + rng.normal(0, 0.01, (n, 3)) + 0.01
    s["a"] = np.stack([1.5 * np.sin(0.029 * k + ph[3]), 9.8 + 0.8 * np.sin(0.013 * k + ph[4]), 1.1 * np.sin(0.019 * k + ph[5])], 1) + rng.normal(0, 0.05, (n, 3))
    s["t"] = t0 + (k + rng.uniform(-0.1, 0.1, n)) / RATE
    return s


def random_bias(rng):
    return np.concatenate([rng.normal(0, 0.01, 3), rng.normal(0, 0.05, 3)]).astype(np.float32)


def prefill(cal, bank, rec_id, n, seed):
    """n measurements integrated into record rec_id (a job of its own: timestamps before the scene's)"""
    s = make_stream(n, seed, t0=50.0)
    r = bank.recs[rec_id]
    r.compute_preintegration(cal, s, 50.0 - 0.5 / RATE, s["t"][-1] + 1.0 / RATE if n else 50.0)


INTEGRATE_COUNTS = (65, 0, 1, 2, 3)
CAP_MEAS = 70


def make_integrate_scene(n_jobs, seed=1):
    """n_jobs jobs over n_jobs + 3 records; sample counts 65, 0, 1, 2, 3 in turn (65 every fortieth job in the large scene).  With
    n_jobs >= 32 also: jobs 9 / 10 sharing one sample range, job 11 with gyro == bias.bg (the d < 1e-6 branch), job 12 filling its pool
    row exactly, job 13 one sample over (refused), jobs 14 / 15 with ids -1 and cap, job 16 repeating job 3's id, job 17 with a sample
    range past the array."""
    rng = np.random.RandomState(seed)
    cal = calib()
    cap = n_jobs + 3
    bank = Bank(cap, CAP_MEAS)
    for r in bank.recs:
        r.reset(random_bias(rng))
    jobs = np.zeros(n_jobs, JOB)
    perm = rng.permutation(cap)[:n_jobs]
    counts = [INTEGRATE_COUNTS[j % 5] if n_jobs < 32 or j % 5 else (65 if j % 40 == 0 else 4) for j in range(n_jobs)]
    special = n_jobs >= 32
    if special:
        counts[9], counts[10], counts[11], counts[12], counts[13] = 7, 7, 3, 65, 65
        prefill(cal, bank, perm[12], CAP_MEAS - 65, 21)
        prefill(cal, bank, perm[13], CAP_MEAS - 64, 22)
    total = sum(counts)
    samples = make_stream(total + 4, seed + 100)
    first = 0
    for j in range(n_jobs):
        # the frame's time stamp: what the record has integrated so far ends 0.4 sample periods before the first new sample
        jobs[j] = (perm[j], first, counts[j], 0, samples["t"][first] - 0.4 / RATE - float(bank.recs[perm[j]].delta_t),
                   samples["t"][first + max(counts[j] - 1, 0)] + 0.6 / RATE)
        first += counts[j]
    if special:
        jobs[10]["first"], jobs[10]["timestamp"], jobs[10]["end_time"] = jobs[9]["first"], jobs[9]["timestamp"], jobs[9]["end_time"]
        f11 = int(jobs[11]["first"])
        samples["w"][f11:f11 + 3] = bank.recs[perm[11]].bias[:3]
        jobs[14]["id"], jobs[15]["id"], jobs[16]["id"] = -1, cap, jobs[3]["id"]
        jobs[17]["first"], jobs[17]["count"] = len(samples) - 1, 2
        assert len(bank.recs[perm[12]].meas) + 65 == CAP_MEAS and len(bank.recs[perm[13]].meas) + 65 == CAP_MEAS + 1
        w11 = samples["w"][f11] - bank.recs[perm[11]].bias[:3]
        assert not w11.any() and jobs[16]["id"] in jobs["id"][:16] and jobs[9]["first"] == jobs[10]["first"]
    assert {0, 1, 2, 3, 65} <= set(counts) or n_jobs < 5
    return dict(cal=cal, bank=bank, jobs=jobs, samples=samples, special=special)


def make_bias_scene(seed=2):
    """set_bias jobs on records with 0 .. CAP_MEAS measurements: bg steps whose norm lies 3 .. 12 ulps below and above 0.01 (two of
    each), a step of 0.05 on a FULL row, small steps, a record without measurements, ids -1 and cap, a repeated id."""
    rng = np.random.RandomState(seed)
    cal = calib()
    cap = 12
    bank = Bank(cap, CAP_MEAS)
    fills = [10, 10, 10, 10, CAP_MEAS, 3, 0, 17, 5, 5, 1, 2]
    for i, r in enumerate(bank.recs):
        r.reset(random_bias(rng))
        prefill(cal, bank, i, fills[i], 30 + i)
    ids = np.array([0, 1, 2, 3, 4, 5, 6, -1, cap, 7, 1, 8], np.int32)
    bias = np.zeros((len(ids), 6), np.float32)
    ulp = np.spacing(np.float32(0.01))
    sides = {}
    for j, i in enumerate(ids):
        if not 0 <= i < cap:
            continue
        old = bank.recs[i].bias
        if j < 4:                                    # just below (j = 0, 1) and just above (j = 2, 3) the threshold
            want = -1 if j < 2 else 1
            d = rng.normal(0, 1, 3)
            d /= np.linalg.norm(d)
            for m in range(1, 400):
                nb = (old[:3].astype(np.float64) + d * 0.01 * (1 + want * m * 2e-7)).astype(np.float32)
                nrm = norm3(nb - old[:3])
                off = (float(nrm) - 0.01) / float(ulp)
                if 3 <= want * off <= 12:
                    break
            else:
                raise AssertionError("no step found")
            sides[j] = off
            bias[j, :3], bias[j, 3:] = nb, old[3:] + np.float32(0.02)
        elif j == 4:
            bias[j] = old + np.array([0.03, -0.03, 0.02, 0.1, 0, -0.1], np.float32)
        else:
            bias[j] = old + rng.normal(0, 0.001, 6).astype(np.float32)
    assert all(-12 <= sides[j] <= -3 for j in (0, 1)) and all(3 <= sides[j] <= 12 for j in (2, 3)), sides
    assert len(bank.recs[4].meas) == CAP_MEAS
    return dict(cal=cal, bank=bank, ids=ids, bias=bias)


def make_merge_scene(seed=3):
    """merge jobs: delta_bias.bg norms of 5e-6 and 2e-5 (both sides of 1e-5), equal ids, a sum that overflows the row, a sum that
    fills it exactly, an empty next, ids out of range, a job whose next an earlier job writes, a next shared by two jobs."""
    rng = np.random.RandomState(seed)
    cal = calib()
    cap = 16
    bank = Bank(cap, CAP_MEAS)
    fills = [12, 9, 12, 9, 40, 31, 40, 30, 6, 0, 6, 6, 6, 6, 6, 6]
    steps = {0: 5e-6, 2: 2e-5, 4: 2e-5, 6: 2e-5, 8: 0.0, 10: 3e-5, 12: 0.0}
    for i, r in enumerate(bank.recs):
        r.reset(random_bias(rng))
        prefill(cal, bank, i, fills[i], 60 + i)
        if steps.get(i):
            nb = r.bias.copy()
            nb[0] += np.float32(steps[i])
            assert not r.set_new_bias(cal, nb)
    ids = np.array([0, 2, 4, 6, 8, 10, 12, -1, 13, 1, 14, 15, 7], np.int32)
    nxt = np.array([1, 3, 5, 7, 9, 10, 11, 3, cap, 13, 11, 11, 2], np.int32)
    n = lambda i: float(norm3(bank.recs[i].delta_bias[:3]))  # noqa: E731
    assert 0 < n(0) < 1e-5 < n(2) and fills[4] + fills[5] > CAP_MEAS and fills[6] + fills[7] == CAP_MEAS and n(6) > 1e-5
    return dict(cal=cal, bank=bank, ids=ids, nxt=nxt)


def make_predict_scene(seed=4):
    """three (record, source state) pairs: no bias change, a small one (below setNewBias's threshold, so delta_bias != 0 and the
    Jacobians act), and a key frame's long integration with a bias change"""
    rng = np.random.RandomState(seed)
    cal = calib()
    bank = Bank(3, 400)
    out = []
    for i, (n, step) in enumerate([(10, 0.0), (10, 0.004), (300, 0.002)]):
        r = bank.recs[i]
        r.reset(random_bias(rng))
        prefill(cal, bank, i, n, 80 + i)
        if step:
            assert not r.set_new_bias(cal, r.bias + np.array([step, -step, step / 2, 0.05, -0.02, 0.03], np.float32))
        src = np.concatenate([rodrigues(rng.normal(0, 0.8, 3)).reshape(9), rng.normal(0, 2.0, 3), rng.normal(0, 0.7, 3)]).astype(np.float32)
        out.append(src)
    assert not bank.recs[0].delta_bias.any() and bank.recs[1].delta_bias.all() and bank.recs[2].delta_bias.all()
    return dict(cal=cal, bank=bank, src=out)
