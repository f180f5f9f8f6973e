"""Plain numpy / Python restatement of include/orbm.h, "Observations built and key frames culled on the device", twice:
  build / cull              the ARRAY form the header states (slot arrays, CSR, liveness), the model the device is compared with
  build_objects / cull_objects   an independent OBJECT-style restatement of the reference: MapPoint objects whose `observations` are
                            dicts keyed by key frame and iterated in ascending key-frame slot (the header's order; the reference's
                            std::map iterates by heap address), KeyFrame objects with a map_points list; MapPoint::addObservation /
                            eraseObservation / setBad (MapPoint.cpp:182-226), KeyFrame::setBad (KeyFrame.cpp:402-418) and
                            LocalMapping::KeyFrameCulling (LocalMapping.cpp:318-372), with the observations constructed from the
                            slots the way processNewKeyFrame adds them (LocalMapping.cpp:93-105)
and the seeded scenes both test files use.  No part of the library is used here."""
import numpy as np

from projection_model import KP_DTYPE, N_LEVELS

MAX_STRIDE, MAX_KF, MAX_POINTS, LONG = 8192, 262143, 524288, 1024
NOBS, OVERFLOW, SKIP_INVALID, SKIP_BAD_KF, LONGEST, TWICE, N_LONG = range(7)
CULLED, KEPT, SKIPPED, POINTS_BAD, CLEARED, REASSIGNED, DROPPED = range(7)
TH_OBS, RATIO, MAX_GAP = 3, 0.9, 1.5


# ---- the array form -----------------------------------------------------------------------------------------------------------
def build(n, bad, slots, stride, valid, cap_points, cap_obs):
    """-> (obs_off i32 [cap_points + 1], obs_kf, obs_kp i32 [n_obs] (empty on overflow), result i32 [8])"""
    n_kf = len(n)
    slots = np.asarray(slots, np.int32).reshape(n_kf, stride) if n_kf else np.zeros((0, stride), np.int32)
    have = np.arange(stride)[None, :] < np.minimum(np.asarray(n, np.int64), stride)[:, None]
    k, i = np.nonzero(have)                                              # ascending (k, i)
    p = slots[k, i].astype(np.int64)
    in_range = (p >= 0) & (p < cap_points)
    k, i, p = k[in_range], i[in_range], p[in_range]
    invalid = np.asarray(valid)[p] == 0
    bad_kf = ~invalid & (np.asarray(bad)[k] != 0)
    ok = ~invalid & ~bad_kf
    k, i, p = k[ok], i[ok], p[ok]
    order = np.argsort(p, kind="stable")                                 # rows ascending, (k, i) ascending inside a row
    obs_kf, obs_kp, row = k[order].astype(np.int32), i[order].astype(np.int32), p[order]
    counts = np.bincount(p, minlength=cap_points)[:cap_points] if cap_points else np.zeros(0, np.int64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    result = np.zeros(8, np.int32)
    result[NOBS], result[SKIP_INVALID], result[SKIP_BAD_KF] = len(p), invalid.sum(), bad_kf.sum()
    result[LONGEST], result[N_LONG] = counts.max() if cap_points else 0, (counts > LONG).sum()
    if len(p) > cap_obs:
        result[OVERFLOW] = 1
        return np.zeros(cap_points + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), result
    same = (obs_kf[1:] == obs_kf[:-1]) & (row[1:] == row[:-1])
    result[TWICE] = len(np.unique(row[1:][same]))
    return off, obs_kf, obs_kp, result


def _entry_ok(st, k, i):
    return 0 <= k < len(st["n"]) and 0 <= i < min(int(st["n"][k]), st["stride"])


def _live(st, k, i, p):
    return st["slots"][k, i] == p and st["bad"][k] == 0


def _list(st, p):
    b, e = int(st["obs_off"][p]), int(st["obs_off"][p + 1])
    if b < 0 or e < b or e > len(st["obs_kf"]):
        return range(0)
    return range(b, e)


def _evaluate(st, c, th_obs):
    """(numMP, numRedundant) of candidate c on the state as it is"""
    cap = st["cap_points"]
    num_mp = num_red = 0
    for i in range(min(max(int(st["n"][c]), 0), st["stride"])):
        p = int(st["slots"][c, i])
        if p < 0 or p >= cap or not st["valid"][p]:
            continue
        num_mp += 1
        level = int(st["kps"][c]["octave"][i])
        live = others = 0
        for j in _list(st, p):
            k2, i2 = int(st["obs_kf"][j]), int(st["obs_kp"][j])
            if not _entry_ok(st, k2, i2) or not _live(st, k2, i2, p):
                continue
            live += 1
            others += k2 != c and int(st["kps"][k2]["octave"][i2]) <= level + 1
        num_red += live > th_obs and others >= th_obs
    return num_mp, num_red


def cull(sc, obs_off, obs_kf, obs_kp, th_obs=TH_OBS, ratio=RATIO, max_gap=MAX_GAP, trace=None):
    """sc: a culling scene (make_cull_scene).  -> dict(bad, slots, valid, ref_kf, code, num_mp, num_redundant, result): the arrays
    after the call.  trace (a list) receives (idx, numMP, numRedundant on the INITIAL state) for every evaluated candidate."""
    st = dict(n=sc["n"], stride=sc["stride"], cap_points=sc["cap_points"], kps=sc["kps"], bad=sc["bad"].copy(), slots=sc["slots"].copy(),
              valid=sc["valid"].copy(), obs_off=obs_off, obs_kf=obs_kf, obs_kp=obs_kp)
    st0 = dict(st, bad=sc["bad"], slots=sc["slots"], valid=sc["valid"])
    ref_kf = sc["ref_kf"].copy()
    recent, ts = sc["recent"], sc["timestamps"]
    nr, cap = len(recent), sc["cap_points"]
    code, num_mp, num_red, result = np.full(nr, -1, np.int32), np.zeros(nr, np.int32), np.zeros(nr, np.int32), np.zeros(8, np.int32)
    result[DROPPED] = sum(not _entry_ok(st, int(k), int(i)) for k, i in zip(obs_kf, obs_kp))
    last = 0
    for idx in range(1, nr - 1):
        c = int(recent[idx])
        if c == sc["first_kf"]:
            code[idx] = 1
        elif ts[idx + 1] - ts[last] > max_gap:
            code[idx] = 2
        if code[idx] > 0:
            result[SKIPPED] += 1
            continue
        num_mp[idx], num_red[idx] = _evaluate(st, c, th_obs)
        if trace is not None:
            trace.append((idx,) + _evaluate(st0, c, th_obs))
        if not float(num_red[idx]) > ratio * float(num_mp[idx]):
            code[idx], last = 0, idx
            result[KEPT] += 1
            continue
        code[idx] = 3
        result[CULLED] += 1
        st["bad"][c] = 1
        n_c = min(max(int(st["n"][c]), 0), st["stride"])
        done = set()
        for i in range(n_c):
            p = int(st["slots"][c, i])
            if p < 0 or p >= cap or not st["valid"][p] or p in done:
                continue
            done.add(p)
            left = []
            for j in _list(st, p):
                k2, i2 = int(obs_kf[j]), int(obs_kp[j])
                if _entry_ok(st, k2, i2) and k2 != c and _live(st, k2, i2, p):
                    left.append((k2, i2))
            if ref_kf[p] == c and left:
                ref_kf[p] = left[0][0]
                result[REASSIGNED] += 1
            if len(left) <= 2:
                st["valid"][p] = 0
                result[POINTS_BAD] += 1
                for k2, i2 in left:
                    if _live(st, k2, i2, p):                          # an entry listed twice clears its slot once
                        st["slots"][k2, i2] = -1
                        result[CLEARED] += 1
        st["slots"][c, :n_c] = -1
    return dict(bad=st["bad"], slots=st["slots"], valid=st["valid"], ref_kf=ref_kf, code=code, num_mp=num_mp, num_redundant=num_red,
                result=result)


# ---- the object form ----------------------------------------------------------------------------------------------------------
class _MapPoint:
    def __init__(self, row, bad, ref):
        self.row, self.is_bad, self.ref, self.observations = row, bool(bad), int(ref), {}   # key frame slot -> [feature, ...]

    def num_obs(self):
        return sum(len(v) for v in self.observations.values())

    def add_observation(self, k, i):
        """MapPoint.cpp:182-188; a second slot of the same key frame (which the reference refuses) is kept beside the first"""
        self.observations.setdefault(k, []).append(i)

    def erase_observation(self, k, world):
        """MapPoint.cpp:190-208"""
        if k not in self.observations:
            return
        del self.observations[k]
        if self.ref == k and self.observations:
            self.ref = min(self.observations)                         # observations.begin()
            world["reassigned"] += 1
        if self.num_obs() <= 2:
            self.set_bad(world)

    def set_bad(self, world):
        """MapPoint.cpp:210-226"""
        obs, self.observations, self.is_bad = self.observations, {}, True
        world["points_bad"] += 1
        for k in sorted(obs):
            for i in obs[k]:
                world["kfs"][k].map_points[i] = None                  # KeyFrame::eraseMapPoint
                world["cleared"] += 1


class _KeyFrame:
    def __init__(self, k, bad, octaves):
        self.k, self.is_bad, self.octaves, self.map_points = k, bool(bad), octaves, []

    def set_bad(self, world):
        """KeyFrame.cpp:402-418, without the graph"""
        for mp in list(self.map_points):
            if mp is not None:
                mp.erase_observation(self.k, world)
        self.map_points = [None] * len(self.map_points)
        self.is_bad = True


def _world(n, bad, slots, stride, valid, cap_points, ref_kf=None, kps=None):
    """the objects a mapper would hold whose slot arrays are `slots`: every slot of a key frame that is not bad naming a point that
    is not bad adds an observation, key frames ascending, slots ascending (LocalMapping.cpp:93-105)"""
    n_kf = len(n)
    slots = np.asarray(slots).reshape(n_kf, stride)
    mps = [_MapPoint(p, not valid[p], ref_kf[p] if ref_kf is not None else -1) for p in range(cap_points)]
    kfs = [_KeyFrame(k, bad[k], kps[k]["octave"] if kps is not None else None) for k in range(n_kf)]
    world = dict(kfs=kfs, mps=mps, points_bad=0, cleared=0, reassigned=0, skip_invalid=0, skip_bad_kf=0)
    for k, kf in enumerate(kfs):
        for i in range(min(max(int(n[k]), 0), stride)):
            p = int(slots[k, i])
            mp = mps[p] if 0 <= p < cap_points else None
            kf.map_points.append(mp)
            if mp is None:
                continue
            if mp.is_bad:
                world["skip_invalid"] += 1
            elif kf.is_bad:
                world["skip_bad_kf"] += 1
            else:
                mp.add_observation(k, i)
    return world


def _observation_lists(world):
    """[(k, i), ...] per row, key frames ascending"""
    return [[(k, i) for k in sorted(mp.observations) for i in mp.observations[k]] for mp in world["mps"]]


def build_objects(n, bad, slots, stride, valid, cap_points, cap_obs):
    world = _world(n, bad, slots, stride, valid, cap_points)
    lists = _observation_lists(world)
    lengths = [len(v) for v in lists]
    result = np.zeros(8, np.int32)
    result[NOBS], result[SKIP_INVALID], result[SKIP_BAD_KF] = sum(lengths), world["skip_invalid"], world["skip_bad_kf"]
    result[LONGEST], result[N_LONG] = max(lengths + [0]), sum(v > LONG for v in lengths)
    if sum(lengths) > cap_obs:
        result[OVERFLOW] = 1
        return np.zeros(cap_points + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32), result
    result[TWICE] = sum(any(len(v) > 1 for v in mp.observations.values()) for mp in world["mps"])
    flat = [e for v in lists for e in v]
    return (np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32), np.array([k for k, _ in flat], np.int32).reshape(-1),
            np.array([i for _, i in flat], np.int32).reshape(-1), result)


def cull_objects(sc, th_obs=TH_OBS, ratio=RATIO, max_gap=MAX_GAP):
    """LocalMapping::KeyFrameCulling on the objects; returns what `cull` returns plus `lists`, the observation sets afterwards"""
    n, stride, cap = sc["n"], sc["stride"], sc["cap_points"]
    world = _world(n, sc["bad"], sc["slots"], stride, sc["valid"], cap, sc["ref_kf"], sc["kps"])
    kfs = world["kfs"]
    recent, ts = [kfs[k] for k in sc["recent"]], sc["timestamps"]
    nr = len(recent)
    code, num_mp, num_red, result = np.full(nr, -1, np.int32), np.zeros(nr, np.int32), np.zeros(nr, np.int32), np.zeros(8, np.int32)
    culled = []
    last = 0
    for idx in range(1, nr - 1):
        kf = recent[idx]
        if kf.k == sc["first_kf"] or ts[idx + 1] - ts[last] > max_gap:
            code[idx] = 1 if kf.k == sc["first_kf"] else 2
            result[SKIPPED] += 1
            continue
        redundant = count = 0
        for i, mp in enumerate(kf.map_points):
            if mp is None or mp.is_bad:
                continue
            count += 1
            if mp.num_obs() > th_obs:
                level, seen = int(kf.octaves[i]), 0
                for k2 in sorted(mp.observations):
                    if k2 == kf.k:
                        continue
                    for i2 in mp.observations[k2]:
                        if int(kfs[k2].octaves[i2]) <= level + 1:
                            seen += 1
                    if seen >= th_obs:
                        break
                if seen >= th_obs:
                    redundant += 1
        num_mp[idx], num_red[idx] = count, redundant
        if redundant > ratio * count:
            kf.set_bad(world)
            culled.append(kf.k)
            code[idx] = 3
            result[CULLED] += 1
        else:
            code[idx], last = 0, idx
            result[KEPT] += 1
    result[POINTS_BAD], result[REASSIGNED] = world["points_bad"], world["reassigned"]
    result[CLEARED] = world["cleared"]
    slots = sc["slots"].copy()
    for k, kf in enumerate(kfs):
        for i, mp in enumerate(kf.map_points):
            if mp is None and 0 <= slots[k, i] < cap:
                slots[k, i] = -1
        if k in culled:
            slots[k, :len(kf.map_points)] = -1
    bad, valid, ref_kf = sc["bad"].copy(), sc["valid"].copy(), sc["ref_kf"].copy()
    bad[culled] = 1
    valid[:cap][[mp.is_bad for mp in world["mps"]]] = 0
    ref_kf[:cap] = [mp.ref for mp in world["mps"]]
    return dict(bad=bad, slots=slots, valid=valid, ref_kf=ref_kf, code=code, num_mp=num_mp, num_redundant=num_red, result=result,
                lists=_observation_lists(world))


def lists_of(obs_off, obs_kf, obs_kp):
    return [list(zip(obs_kf[b:e].tolist(), obs_kp[b:e].tolist())) for b, e in zip(obs_off[:-1], obs_off[1:])]


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------
BUILD_SCENES = {
    "small": dict(seed=11, n_kf=3, stride=64, cap_points=200, lengths=(0, 1, 2, 2, 1, 0), n_bad=1, typical=(1, 3)),
    "mid": dict(seed=12, n_kf=12, stride=256, cap_points=1000, lengths=(0, 1, 2, 3, 4, 7), n_bad=2, typical=(2, 8)),
    "long": dict(seed=13, n_kf=1100, stride=8, cap_points=700, lengths=(1025, 1024, 65, 64, 63, 4, 3, 2, 1, 0), n_bad=40, typical=(2, 15)),
}


def make_build_scene(seed, n_kf, stride, cap_points, lengths, n_bad, typical):
    """Slot arrays whose valid rows 0 .. len(lengths) - 1 get EXACTLY `lengths` observations (in key frames that are not bad), the
    other rows draw from `typical` over all key frames; then -1 and out-of-range slots, rows named behind d_n[k], d_n[k] > stride, a
    key frame without slots, invalid rows, one row twice in one key frame.  valid / slots carry spare rows past cap_points."""
    rng = np.random.RandomState(seed)
    bad = np.zeros(n_kf, np.uint8)
    bad[rng.permutation(n_kf)[:n_bad]] = rng.randint(1, 200, n_bad)
    n = rng.randint(stride // 2, stride + 1, n_kf).astype(np.int32)
    good = np.flatnonzero(bad == 0)
    n[good[0]], n[good[1]] = stride + 3, stride                        # d_n[k] > stride: clamped
    n[good[-1]] = 0 if n_kf > 8 else n[good[-1]]                       # a key frame without slots
    if n_kf > 8:
        n[good[-2]] = -4
    slots = np.full((n_kf, stride), -1, np.int32)
    free = [list(rng.permutation(min(max(int(n[k]), 0), stride))) for k in range(n_kf)]
    valid = (rng.uniform(size=cap_points + 8) < 0.9).astype(np.uint8) * rng.randint(1, 200, cap_points + 8).astype(np.uint8)
    valid[:len(lengths) + 1] = 1
    want = np.full(cap_points, -1, np.int64)
    twice = len(lengths)                                                 # row `twice`: two slots of one key frame, and no other
    for p in range(cap_points):
        exact = p < len(lengths)
        if p == twice:
            k2 = next(k for k in good if len(free[k]) >= 2)
            slots[k2, free[k2].pop()] = twice
            slots[k2, free[k2].pop()] = twice
            spare = [[free[k].pop() for _ in range((len(free[k]) + 5) // 6)] for k in range(n_kf)]   # kept for the junk below
            continue
        length = lengths[p] if exact else rng.randint(typical[0], typical[1] + 1)
        pool = [k for k in (good if exact else range(n_kf)) if free[k]]
        ks = rng.permutation(pool)[:length] if len(pool) else []
        assert not exact or len(ks) == length, "the scene has too few slots for the stated lengths"
        for k in ks:
            slots[k, free[k].pop()] = p
        if exact:
            want[p] = length
    junk = [cap_points, cap_points + 7, -5, 2 ** 31 - 1, -2 ** 31, -1]
    for k in range(n_kf):                                                # what is left: mostly -1, some out of range
        for i in free[k] + spare[k]:
            slots[k, i] = junk[rng.randint(len(junk))]
        slots[k, min(max(int(n[k]), 0), stride):] = rng.randint(0, cap_points, stride - min(max(int(n[k]), 0), stride))   # behind d_n: ignored
    return dict(n=n, bad=bad, slots=slots, stride=stride, valid=valid, cap_points=cap_points, want=want, twice=twice)


def make_cull_scene(seed, n_kf=12, stride=256, cap_points=1000, noise=120):
    """An engineered mapper state (seed permutes the key-frame numbering and draws the noise).  Roles, by position in `recent`:
    0 and 9 never candidates; 1 the first key frame (code 1); 2 = C, culled: 20 redundant rows, one named by two of its slots, and
    two rows W shared with D and an old key frame only, which the cull sets bad; 3 = D: 18 redundant rows plus the two W rows: kept on
    the initial state (18 of 20), culled after C's cascade (18 of 18); 4 kept; 5 numMP == 0; 6 the boundary, 9 redundant of 10: kept;
    7 and 8 behind a gap in the timestamps (code 2).  Two more key frames are not recent, one of them bad from the start."""
    assert n_kf >= 12
    rng = np.random.RandomState(seed)
    role = rng.permutation(n_kf)                                         # role r is key frame role[r]
    recent = role[:10].astype(np.int32)
    old, old_bad = int(role[10]), int(role[11])
    r = [int(x) for x in role]
    C, D, E, F, G = r[2], r[3], r[4], r[5], r[6]
    anchors = [r[0], r[9], old]                                          # never culled
    slots = np.full((n_kf, stride), -1, np.int32)
    used = np.zeros(n_kf, np.int64)
    octave = rng.randint(0, N_LEVELS, (n_kf, stride)).astype(np.int32)
    ref_kf = rng.randint(0, n_kf, cap_points + 4).astype(np.int32)
    rows = [0]

    def point(observers, ref=None):
        p = rows[0]
        rows[0] += 1
        for k, level in observers:
            slots[k, used[k]] = p
            octave[k, used[k]] = level
            used[k] += 1
        ref_kf[p] = observers[0][0] if ref is None else ref
        return p

    seen3 = lambda level: [(k, level) for k in anchors]  # noqa: E731
    for j in range(20):                                                  # C's redundant rows; every other one refers to C
        p = point([(C, 2)] + seen3(rng.randint(0, 4)), ref=C if j % 2 else anchors[0])
    slots[C, used[C]], octave[C, used[C]] = p, 2                          # the last of them twice in C
    used[C] += 1
    w = [point([(C, 1), (D, 1), (old, 1), (old_bad, 0)], ref=C), point([(D, 3), (C, 3), (old, 3)], ref=D)]
    for j in range(18):
        point([(D, 4)] + seen3(rng.randint(0, 6)), ref=D if j % 3 == 0 else anchors[1])
    for j in range(15):                                                  # E: two or three observers only
        point([(E, 0), (anchors[j % 3], 0)] + ([(anchors[(j + 1) % 3], 0)] if j % 2 else []))
    for j in range(9):                                                   # G: octave exactly one above: redundant
        point([(G, 0)] + seen3(1))
    point([(G, 0)] + seen3(2))                                           # ... and two above: four observers, none counts
    invalid = [point([(F, 0), (anchors[0], 0), (anchors[1], 0), (old, 0)]) for _ in range(3)]
    slots[F, used[F]:used[F] + 3] = [cap_points, -7, cap_points + 2]      # F: invalid rows and no map point: numMP == 0
    used[F] += 3
    pool = anchors + [old_bad, E, r[7], r[8], r[1]]
    for _ in range(noise):
        ks = rng.permutation(pool)[:rng.randint(2, 7)]
        point([(int(k), int(rng.randint(0, N_LEVELS))) for k in ks])
    assert rows[0] <= cap_points and used.max() + 8 <= stride
    n = (used + rng.randint(0, 8, n_kf)).astype(np.int32)
    valid = np.zeros(cap_points + 4, np.uint8)
    valid[:rows[0]] = rng.randint(1, 200, rows[0])
    valid[invalid] = 0
    bad = np.zeros(n_kf, np.uint8)
    bad[old_bad] = 1
    kps = []
    for k in range(n_kf):
        kp = np.zeros(n[k], KP_DTYPE)
        kp["octave"], kp["class_id"], kp["size"] = octave[k, :n[k]], -1, 31.0
        kp["x"], kp["y"] = rng.uniform(0, 752, n[k]), rng.uniform(0, 480, n[k])
        kps.append(kp)
    ts = 10.0 + 0.1 * np.arange(10)
    ts[8:] += 2.0                                                        # candidates 7 and 8 look across the gap
    return dict(n=n, bad=bad, slots=slots, stride=stride, valid=valid, cap_points=cap_points, kps=kps, ref_kf=ref_kf, recent=recent,
                timestamps=ts, first_kf=r[1], roles=dict(C=C, D=D, E=E, F=F, G=G, W=w, old=old, old_bad=old_bad), n_rows=rows[0])


def make_small_cull_scene(seed, n_kf=3, stride=64, cap_points=200):
    """three key frames that all see the same 40 rows, the middle one of `recent` the only candidate: kept with th_obs = 3 (three
    observations are not more than three), culled with th_obs = 2, after which every row is left with two observations and goes bad"""
    rng = np.random.RandomState(seed)
    slots = np.full((n_kf, stride), -1, np.int32)
    for k in range(n_kf):
        slots[k, rng.permutation(stride)[:40]] = rng.permutation(40) + 5
    n = np.full(n_kf, stride, np.int32)
    kps = []
    for k in range(n_kf):
        kp = np.zeros(stride, KP_DTYPE)
        kp["octave"], kp["class_id"] = 3, -1
        kps.append(kp)
    valid = np.ones(cap_points + 4, np.uint8)
    return dict(n=n, bad=np.zeros(n_kf, np.uint8), slots=slots, stride=stride, valid=valid, cap_points=cap_points, kps=kps,
                ref_kf=rng.randint(0, n_kf, cap_points + 4).astype(np.int32), recent=np.array([2, 0, 1], np.int32),
                timestamps=np.array([1.0, 1.1, 1.2]), first_kf=-1, n_rows=45)


def check_cull_scene(sc, out, trace):
    """the properties the mid culling scene was built for; `out` = cull(...), `trace` its trace"""
    ro = sc["roles"]
    pos = {int(k): i for i, k in enumerate(sc["recent"])}
    code = out["code"].tolist()
    assert code == [-1, 1, 3, 3, 0, 0, 0, 2, 2, -1], code
    initial = {idx: (mp, red) for idx, mp, red in trace}
    d = pos[ro["D"]]
    assert initial[d] == (20, 18) and (out["num_mp"][d], out["num_redundant"][d]) == (18, 18)       # the cascade decides D
    assert not 18 > 0.9 * 20 and 18 > 0.9 * 18
    assert (out["num_mp"][pos[ro["C"]]], out["num_redundant"][pos[ro["C"]]]) == (23, 21)
    assert out["num_mp"][pos[ro["F"]]] == 0 and out["num_redundant"][pos[ro["F"]]] == 0
    g = pos[ro["G"]]
    assert (out["num_mp"][g], out["num_redundant"][g]) == (10, 9) and float(9) == 0.9 * float(10)   # the exact boundary: kept
    assert not out["valid"][ro["W"]].any() and sc["valid"][ro["W"]].all()
    res = out["result"]
    assert res[CULLED] == 2 and res[KEPT] == 3 and res[SKIPPED] == 3 and res[POINTS_BAD] == 2 and res[CLEARED] >= 3
    assert res[REASSIGNED] >= 10 and (out["ref_kf"][:sc["n_rows"]] != sc["ref_kf"][:sc["n_rows"]]).sum() == res[REASSIGNED]
    assert (out["slots"][ro["D"]] == -1).all() and (out["slots"][ro["C"]][:sc["n"][ro["C"]]] == -1).all()
