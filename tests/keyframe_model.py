"""Two restatements of include/orbm.h, "Key frames inserted and recent map points culled on the device", and the seeded scenes.

The ARRAY form states the three calls on the header's arrays, exactly as the header does: it is the model the device is compared with,
every output and d_result.  The OBJECT form follows the reference line by line -- the KeyFrame constructor behind
Tracking::createNewKeyFrame (modules/BasicObject/KeyFrame.cpp:15-25) with the loop of LocalMapping::processNewKeyFrame
(modules/Frontend/LocalMapping.cpp:93-105), the bookkeeping of a created point (:243-248, MapPoint.cpp:16-30) and
LocalMapping::MapPointCulling (:117-144) with MapPoint::setBad (MapPoint.cpp:210-226) -- on KeyFrame / MapPoint objects with an
`observations` map and recent_map_points as a list; the reference's map order is taken as ascending (key frame, slot), the header's
order.  A scene is a seeded world (slot arrays and the CSR observations_model.build left from them, then aged: slots cleared and a key
frame gone bad behind it, stale entries forged) and lists of calls of the three kinds.  No part of the library is used here."""
import numpy as np

import observations_model as om

I_HELD, I_INVALID, I_RANGE, I_TWICE, I_CUT = 0, 2, 3, 4, 5
G_ROWS, G_REFUSED, G_FROM, G_TO, G_RECENT = range(5)
P_KEPT, P_REFUSED, P_BAD, P_RATIO, P_FEW, P_AGED, P_CLEARED, P_DROPPED = range(8)
TABLE_KEYS = ("pose_R", "pose_t", "bad", "kps", "desc", "n", "slots")
QUARTER = np.float32(0.25)


def _clamp(x, hi):
    return min(max(int(x), 0), hi)


# ---- the array form ---------------------------------------------------------------------------------------------------------------
def insert_keyframe(table, K, valid, cap_points, frame_mp, frame_R, frame_t, frame_kps, frame_desc):
    """table: pose_R f64 [cap_kf, 9], pose_t f64 [cap_kf, 3], bad u8, kps, desc i64 (addresses), n i32 [cap_kf], slots i32 [cap_kf, stride]
    -> dict of the seven arrays as the call leaves them, and result i32 [8]"""
    t = {k: np.array(table[k]) for k in TABLE_KEYS}
    stride, n2 = t["slots"].shape[1], len(frame_mp)
    res = np.zeros(8, np.int32)
    t["pose_R"][K].view(np.uint64)[:] = np.asarray(frame_R, np.float64).view(np.uint64)      # bit for bit
    t["pose_t"][K].view(np.uint64)[:] = np.asarray(frame_t, np.float64).view(np.uint64)
    t["bad"][K], t["n"][K], t["kps"][K], t["desc"][K] = 0, n2, frame_kps, frame_desc
    t["slots"][K] = -1
    seen = set()
    for i in range(min(n2, stride)):
        p = int(frame_mp[i])
        if p == -1:
            continue
        if not 0 <= p < cap_points:
            res[I_RANGE] += 1
        elif not valid[p]:
            res[I_INVALID] += 1                                    # eraseMapPoint (:98)
        else:
            t["slots"][K, i] = p                                   # the slot IS the observation (:100)
            res[I_HELD] += 1
            seen.add(p)
    res[I_TWICE] = res[I_HELD] - len(seen)
    res[I_CUT] = max(n2 - stride, 0)
    t["result"] = res
    return t


def register_new_points(n_points, n_registered, n_recent, K, kf_id, cap_points, ref_kf, first_kf, found, visible, recent):
    """-> dict(n_registered, n_recent: the device ints afterwards; ref_kf, first_kf, found, visible, recent: as the call leaves them;
    result i32 [8])"""
    out = dict(ref_kf=np.array(ref_kf), first_kf=np.array(first_kf), found=np.array(found), visible=np.array(visible), recent=np.array(recent),
               n_registered=int(n_registered), n_recent=int(n_recent))
    cap_recent = len(recent)
    a, b, r = _clamp(n_registered, cap_points), _clamp(n_points, cap_points), _clamp(n_recent, cap_recent)
    res = np.zeros(8, np.int32)
    res[G_FROM], res[G_TO], res[G_RECENT] = a, b, r
    res[G_REFUSED] = 2 if a > b else (1 if r + (b - a) > cap_recent else 0)
    if not res[G_REFUSED]:
        rows = np.arange(a, b, dtype=np.int32)
        out["ref_kf"][a:b], out["first_kf"][a:b], out["found"][a:b], out["visible"][a:b] = K, kf_id, 1, 1
        out["recent"][r:r + b - a] = rows                          # creation order
        out["n_recent"], out["n_registered"] = r + b - a, b
        res[G_ROWS], res[G_RECENT] = b - a, r + b - a
    out["result"] = res
    return out


def _row_list(w, p):
    b, e = int(w["obs_off"][p]), int(w["obs_off"][p + 1])
    return range(b, e) if 0 <= b <= e <= len(w["obs_kf"]) else range(0)


def _entry_ok(w, j):
    k, i = int(w["obs_kf"][j]), int(w["obs_kp"][j])
    return 0 <= k < w["n_kf"] and 0 <= i < min(max(int(w["n"][k]), 0), w["stride"])


def entry_state(w, slots, j, p):
    """CSR entry j of row p: 1 live, 0 stale (the slot names another row now), -2 its key frame is bad, -1 an index out of range"""
    if not _entry_ok(w, j):
        return -1
    k, i = int(w["obs_kf"][j]), int(w["obs_kp"][j])
    if slots[k, i] != p:
        return 0
    return -2 if w["bad"][k] else 1


def _live(w, slots, p):
    return [(int(w["obs_kf"][j]), int(w["obs_kp"][j])) for j in _row_list(w, p) if entry_state(w, slots, j, p) == 1]


def found_ratio_low(found, visible):
    """(float) found / (float) visible < 0.25f, literally: int32 -> float rounds to nearest even, the division is IEEE"""
    with np.errstate(all="ignore"):
        return bool(np.float32(np.int32(found)) / np.float32(np.int32(visible)) < QUARTER)


def age(cur_kf_id, first):
    return (int(cur_kf_id) - int(first)) & 0xFFFFFFFF


def _classify(w, valid, slots, p, cur_kf_id, first_kf, found, visible):
    if not 0 <= p < w["cap_points"]:
        return -1
    if not valid[p]:
        return 1
    if found_ratio_low(found[p], visible[p]):
        return 2
    d = age(cur_kf_id, first_kf[p])
    if d >= 2 and len(_live(w, slots, p)) <= 2:
        return 3
    return 4 if d > 2 else 0


def cull_map_points(w, recent, n_recent, cur_kf_id, first_kf, found, visible, code=None, sequential=True):
    """w: the world (n_kf, stride, cap_points, n, bad, slots [n_kf, stride], valid, obs_off, obs_kf, obs_kp).  sequential: entry by entry,
    each on what the ones before it left, as the reference's loop runs; else every entry classified on the arrays AS PASSED and the
    setBads applied afterwards, as the device's threads run.  -> dict(recent, n_recent, valid, slots, code, result)"""
    cap_recent = len(recent)
    out = dict(recent=np.array(recent), n_recent=int(n_recent), valid=np.array(w["valid"]), slots=np.array(w["slots"]),
               code=np.array(code) if code is not None else np.full(cap_recent, -9, np.int32))
    res = np.zeros(8, np.int32)
    out["result"] = res
    n = _clamp(n_recent, cap_recent)
    rows = [int(p) for p in recent[:n]]
    in_range = [p for p in rows if 0 <= p < w["cap_points"]]
    if len(set(in_range)) != len(in_range):                        # the premise, before anything is written
        res[P_REFUSED] = 1
        return out
    k, i = np.asarray(w["obs_kf"], np.int64), np.asarray(w["obs_kp"], np.int64)     # once each over all of [0, n_obs)
    have = np.minimum(np.maximum(np.asarray(w["n"], np.int64), 0), w["stride"])
    in_kf = (k >= 0) & (k < w["n_kf"])
    res[P_DROPPED] = len(k) - (in_kf & (i >= 0) & (i < have[np.where(in_kf, k, 0)] if w["n_kf"] else False)).sum()
    args = (cur_kf_id, first_kf, found, visible)

    def set_bad(p):
        out["valid"][p] = 0
        for j in _row_list(w, p):                                  # entry by entry: a slot a forged CSR lists twice is cleared, and counted, once
            if entry_state(w, out["slots"], j, p) == 1:
                out["slots"][int(w["obs_kf"][j]), int(w["obs_kp"][j])] = -1
                res[P_CLEARED] += 1

    if sequential:
        codes = []
        for p in rows:
            codes.append(_classify(w, out["valid"], out["slots"], p, *args))
            if codes[-1] in (2, 3):
                set_bad(p)
    else:
        codes = [_classify(w, w["valid"], w["slots"], p, *args) for p in rows]
        for p, c in zip(rows, codes):
            if c in (2, 3):
                set_bad(p)
    out["code"][:n] = codes
    kept = [p for p, c in zip(rows, codes) if c == 0]
    out["recent"][:len(kept)] = kept                               # in place: what lies at and past the new length is as passed
    out["n_recent"] = len(kept)
    for c, slot in ((-1, P_DROPPED), (0, P_KEPT), (1, P_BAD), (2, P_RATIO), (3, P_FEW), (4, P_AGED)):
        res[slot] += codes.count(c)
    return out


# ---- the object form ----------------------------------------------------------------------------------------------------------------
class Map:
    def __init__(self):
        self.erased = []

    def erase_map_point(self, mp):
        self.erased.append(mp.row)


class MapPoint:
    def __init__(self, row, is_bad=False, point_map=None):
        self.row, self.is_bad, self.point_map = row, is_bad, point_map
        self.observations = {}                                     # KeyFrame -> feature index
        self.reference_kf, self.first_kf_id, self.num_visible, self.num_found = None, 0, 0, 0

    @classmethod
    def construct(cls, row, last_kf, cur_kf, match, point_map):    # MapPoint.cpp:16-30
        mp = cls(row, False, point_map)
        mp.reference_kf, mp.first_kf_id = cur_kf, cur_kf.id        # :18
        mp.observations[last_kf] = match[0]
        mp.observations[cur_kf] = match[1]
        mp.num_visible = 1                                         # :24
        mp.num_found = 1                                           # :25
        return mp

    def add_observation(self, kf, idx):                            # MapPoint.cpp:182-188
        if kf not in self.observations:
            self.observations[kf] = idx

    def get_num_obs(self):
        return len(self.observations)

    def get_found_ratio(self):                                     # MapPoint.cpp:276-279
        with np.errstate(all="ignore"):
            return np.float32(np.int32(self.num_found)) / np.float32(np.int32(self.num_visible))

    def set_bad(self):                                             # MapPoint.cpp:210-226
        self.is_bad = True
        obs, self.observations = self.observations, {}
        for kf in sorted(obs, key=lambda kf: kf.slot):
            kf.erase_map_point(obs[kf])
        self.point_map.erase_map_point(self)


class Frame:
    def __init__(self, map_points, R, t, kps, desc):
        self.map_points, self.R_cw, self.t_cw, self.key_points, self.descriptors, self.num_kps = map_points, R, t, kps, desc, len(map_points)


class KeyFrame:
    def __init__(self, slot, kf_id=None, is_bad=False, num_kps=0):
        self.slot, self.id, self.is_bad, self.num_kps = slot, slot if kf_id is None else kf_id, is_bad, num_kps
        self.map_points = [None] * num_kps

    @classmethod
    def from_frame(cls, slot, frame):                              # KeyFrame.cpp:15-25
        kf = cls(slot, num_kps=frame.num_kps)
        kf.key_points, kf.descriptors = frame.key_points, frame.descriptors
        kf.R_cw, kf.t_cw = frame.R_cw, frame.t_cw
        kf.map_points = list(frame.map_points)                     # a copy: the Frame's stay
        return kf

    def erase_map_point(self, idx):
        self.map_points[idx] = None


def process_new_key_frame(current_kf):
    """LocalMapping.cpp:93-105; -> the observations added"""
    added = 0
    map_points = list(current_kf.map_points)
    for i in range(current_kf.num_kps):
        mp = map_points[i]
        if mp:
            if mp.is_bad:
                current_kf.erase_map_point(i)
            else:
                before = mp.get_num_obs()
                mp.add_observation(current_kf, i)
                added += mp.get_num_obs() - before
    return added


def bookkeeping_of_new_points(kf, current_kf, matches, first_row, point_map, recent_map_points):
    """LocalMapping.cpp:243-248 for the accepted matches (i, matches12[i]) of one pair of key frames, in ascending i"""
    made = []
    for t, (i, m) in enumerate(matches):
        mp = MapPoint.construct(first_row + t, kf, current_kf, (i, m), point_map)
        kf.map_points[i] = mp
        current_kf.map_points[m] = mp
        recent_map_points.append(mp)
        made.append(mp)
    return made


def map_point_culling(recent_map_points, current_kf):
    """LocalMapping.cpp:117-144 as written; the ids are unsigned and their difference 64-bit.  -> (numFoundRatio, numBad)"""
    cur_kf_id = current_kf.id
    num_found_ratio = num_bad = 0
    at = 0
    while at < len(recent_map_points):
        mp = recent_map_points[at]
        if mp.is_bad:
            del recent_map_points[at]
            num_bad += 1
        elif mp.get_found_ratio() < QUARTER:
            mp.set_bad()
            del recent_map_points[at]
            num_found_ratio += 1
        elif (cur_kf_id - mp.first_kf_id) % (1 << 64) >= 2 and mp.get_num_obs() <= 2:
            mp.set_bad()
            del recent_map_points[at]
        elif (cur_kf_id - mp.first_kf_id) % (1 << 64) > 2:
            del recent_map_points[at]
        else:
            at += 1
    return num_found_ratio, num_bad


def world_objects(w, first_kf=None, found=None, visible=None):
    """the world's objects, the observations added from the slots in ascending (k, i) the way processNewKeyFrame adds them; a bad key
    frame observes nothing (KeyFrame::setBad erased that) and its slots stay"""
    point_map = Map()
    kfs = [KeyFrame(k, is_bad=bool(w["bad"][k]), num_kps=w["stride"]) for k in range(w["n_kf"])]
    mps = [MapPoint(p, not w["valid"][p], point_map) for p in range(w["cap_points"])]
    for p, mp in enumerate(mps):
        if first_kf is not None:
            mp.first_kf_id, mp.num_found, mp.num_visible = int(first_kf[p]), int(found[p]), int(visible[p])
    for k, kf in enumerate(kfs):
        for i in range(min(max(int(w["n"][k]), 0), w["stride"])):
            p = int(w["slots"][k, i])
            if 0 <= p < w["cap_points"]:
                kf.map_points[i] = mps[p]
                if not mps[p].is_bad and not kf.is_bad:
                    mps[p].add_observation(kf, i)
    return kfs, mps, point_map


def object_slots(kfs, w):
    """the key frames' map_points as a slot array; slots at and past d_n[k] as the world has them (no object holds them)"""
    out = np.array(w["slots"])
    for k, kf in enumerate(kfs):
        for i in range(min(max(int(w["n"][k]), 0), w["stride"])):
            out[k, i] = kf.map_points[i].row if kf.map_points[i] is not None else -1
    return out


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------
CUR = 10                                                           # current_kf->id of the culling scenes
BIG = (16777215, 67108861)   # found / visible: 4 * found < visible, so the exact ratio is below 1/4; (float) visible = 67108860 and the float ratio IS 1/4

# the designed entries of a culling scene: name -> (found, visible, CUR - first, live entries, valid, the code)
DESIGNED = {
    "quarter": (1, 4, 0, 3, 1, 0), "fifth": (1, 5, 0, 3, 1, 2), "zero_zero": (0, 0, 1, 3, 1, 0), "three_zero": (3, 0, 0, 3, 1, 0),
    "minus_quarter": (1, -4, 0, 3, 1, 2), "big": BIG + (0, 3, 1, 0), "both": (1, 9, 3, 1, 1, 2),
    "age0": (5, 5, 0, 0, 1, 0), "age1": (5, 5, 1, 1, 1, 0), "age2_live2": (5, 5, 2, 2, 1, 3), "age2_live3": (5, 5, 2, 3, 1, 0),
    "age3_live2": (5, 5, 3, 2, 1, 3), "age3_live3": (5, 5, 3, 3, 1, 4), "future_live3": (5, 5, -2, 3, 1, 4), "future_live0": (5, 5, -1, 0, 1, 3),
    "bad_row": (5, 5, 0, 0, 0, 1),
}
JUNK_ROWS = (-1, -7, 1 << 30)                                      # plus cap_points itself


def make_cull_scene(seed, n_list, n_kf=6, stride=64, cap_points=300, designed=True, n_junk=None, cap_recent=None, code_fill=-9):
    """-> dict(world, recent [cap_recent], n_recent, cur, first_kf, found, visible, code0, spec: name -> list position).  The world's CSR
    is the one observations_model.build left; behind it slots were cleared (stale entries), some of those entries forged out of range,
    and key frame n_kf - 2 went bad.  Every entry of the list names another row."""
    rng = np.random.RandomState(seed)
    n_junk = (4 if designed else min(4, n_list // 8)) if n_junk is None else n_junk
    n_rows = n_list - n_junk
    assert n_rows <= cap_points and (not designed or n_rows >= len(DESIGNED))
    bad_kf = n_kf - 2 if n_kf >= 3 else -1
    good_kfs = [k for k in range(n_kf) if k != bad_kf]
    n = np.full(n_kf, stride, np.int32)
    if n_kf > 1:
        n[1] = stride - 3
    valid = (rng.rand(cap_points) > 0.12).astype(np.uint8)
    rows = rng.permutation(cap_points)[:n_rows]
    names = list(DESIGNED) if designed else []
    first_kf = (CUR - rng.randint(0, 6, cap_points)).astype(np.int32)
    visible = rng.randint(1, 40, cap_points).astype(np.int32)
    found = np.minimum(visible, rng.randint(0, 16, cap_points)).astype(np.int32)
    want_live = rng.randint(0, 6, cap_points)
    first_kf[rng.rand(cap_points) < 0.05] = CUR + 2
    for name, p in zip(names, rows):
        f, v, d, live, ok, _ = DESIGNED[name]
        found[p], visible[p], first_kf[p], want_live[p], valid[p] = f, v, CUR - d, live, ok
    # ---- the slots before the CSR is built: live entries, entries to go stale, entries in the key frame to go bad
    free = {k: list(rng.permutation(int(n[k]))) for k in range(n_kf)}
    slots = np.full((n_kf, stride), -1, np.int32)
    stale = []
    listed_rows = set(rows.tolist())
    order = list(rows) + [p for p in rng.permutation(cap_points)[:4 * n_kf * stride] if p not in listed_rows]   # more than the slots can take
    for t, p in enumerate(order):
        designed_row = t < len(names)
        if t >= n_rows and not any(free[k] for k in good_kfs):
            break
        live = int(want_live[p]) if valid[p] else int(rng.rand() < 0.2)     # a slot may still name a bad row: no observation
        extra = int(rng.randint(0, 3)) if not designed_row or t % 2 else 1
        ks = [k for k in rng.permutation(good_kfs) if free[k]][:live + extra]
        if designed_row:
            assert len(ks) >= live, "the designed rows come first and find their slots"
        for c, k in enumerate(ks):
            i = free[k].pop()
            slots[k, i] = p
            if c >= live:
                stale.append((p, k, i))
        if bad_kf >= 0 and free[bad_kf] and rng.rand() < 0.3:
            slots[bad_kf, free[bad_kf].pop()] = p
    bad = np.zeros(n_kf, np.uint8)
    off, okf, okp, _ = om.build(n, bad, slots, stride, valid, cap_points, 1 << 30)
    okf, okp = okf.copy(), okp.copy()
    # ---- behind the build: the slots cleared, a third of their entries forged, the key frame bad
    for t, (p, k, i) in enumerate(stale):
        slots[k, i] = -1
        if valid[p] and t % 3 == 0:
            j = next(j for j in range(off[p], off[p + 1]) if okf[j] == k and okp[j] == i)
            which = (t // 3) % 4
            if which == 0:
                okf[j] = n_kf
            elif which == 1:
                okf[j] = -1
            elif which == 2:
                okp[j] = stride + 5
            else:
                okf[j], okp[j] = min(1, n_kf - 1), stride - 1      # past d_n[1] = stride - 3, inside the stride
    if bad_kf >= 0:
        bad[bad_kf] = 1
    w = dict(n_kf=n_kf, stride=stride, cap_points=cap_points, n=n, bad=bad, slots=slots, valid=valid, obs_off=off, obs_kf=okf, obs_kp=okp)
    junk = [(JUNK_ROWS + (cap_points,))[t % 4] for t in range(n_junk)]
    listed = np.array(list(rows) + junk, np.int64)
    place = rng.permutation(n_list)
    cap_recent = n_list + 5 if cap_recent is None else cap_recent
    recent = np.full(cap_recent, -3, np.int32)
    recent[place] = listed
    spec = {name: int(place[t]) for t, name in enumerate(names)}
    return dict(world=w, recent=recent, n_recent=n_list, cur=CUR, first_kf=first_kf, found=found, visible=visible, spec=spec,
                code0=np.full(cap_recent, code_fill, np.int32))


def run_cull(sc, **kw):
    return cull_map_points(sc["world"], sc["recent"], sc["n_recent"], sc["cur"], sc["first_kf"], sc["found"], sc["visible"], code=sc["code0"], **kw)


def check_cull_scene(sc, out):
    """every case the culling scenes are built for occurs"""
    w, code, res = sc["world"], out["code"], out["result"]
    n = sc["n_recent"]
    assert not res[P_REFUSED] and set(code[:n].tolist()) == {-1, 0, 1, 2, 3, 4}
    for name, j in sc["spec"].items():
        assert code[j] == DESIGNED[name][5], (name, int(code[j]))
        p = int(sc["recent"][j])
        f, v, d, live, ok, _ = DESIGNED[name]
        assert len(_live(w, w["slots"], p)) == (live if ok else 0) and age(sc["cur"], sc["first_kf"][p]) == d & 0xFFFFFFFF, name
    p = int(sc["recent"][sc["spec"]["both"]])                      # fails rules 2 and 3 at once: 2 wins
    assert found_ratio_low(sc["found"][p], sc["visible"][p]) and age(sc["cur"], sc["first_kf"][p]) >= 2 and len(_live(w, w["slots"], p)) <= 2
    assert BIG[0] / BIG[1] < 0.25 and not found_ratio_low(*BIG)    # the int -> float rounding decides
    states = [entry_state(w, w["slots"], j, int(p)) for p, c in zip(sc["recent"][:n], code[:n]) if c in (0, 3, 4) for j in _row_list(w, int(p))]
    assert states.count(0) >= 3 and states.count(-2) >= 3 and states.count(-1) >= 3 and states.count(1) >= 10
    assert res[P_CLEARED] >= 3 and res[P_DROPPED] > (code[:n] == -1).sum() and res[P_KEPT] == out["n_recent"] >= 3
    assert (out["recent"][out["n_recent"]:] == sc["recent"][out["n_recent"]:]).all()


def make_insert_calls(seed, cap_points, valid, stride, cap_kf, sizes):
    """a key-frame table full of an earlier use and one call per size n2: slots naming good rows, bad rows, -1, junk, and one row twice"""
    rng = np.random.RandomState(seed)
    table = dict(pose_R=rng.randn(cap_kf, 9), pose_t=rng.randn(cap_kf, 3), bad=rng.randint(0, 2, cap_kf).astype(np.uint8),
                 kps=rng.randint(1, 1 << 40, cap_kf).astype(np.int64) * 8, desc=rng.randint(1, 1 << 40, cap_kf).astype(np.int64) * 4,
                 n=rng.randint(0, stride + 1, cap_kf).astype(np.int32), slots=rng.randint(-1, cap_points, (cap_kf, stride)).astype(np.int32))
    good, gone = np.flatnonzero(valid), np.flatnonzero(valid == 0)
    calls = []
    for t, n2 in enumerate(sizes):
        fm = np.full(n2, -1, np.int32)
        pick = rng.rand(n2)
        if len(good):
            on = pick < 0.55
            fm[on] = rng.choice(good, on.sum(), replace=on.sum() > len(good))
        if len(gone):
            fm[(pick >= 0.55) & (pick < 0.65)] = rng.choice(gone, ((pick >= 0.55) & (pick < 0.65)).sum())
        junk = (pick >= 0.65) & (pick < 0.72)
        fm[junk] = rng.choice([cap_points, -2, 1 << 30, -(1 << 31)], junk.sum())
        if n2 >= 4 and len(good):
            fm[n2 - 1] = fm[0] = good[0]                           # one row twice, at both ends of the frame
        R, tt = rng.randn(9), rng.randn(3)
        R[4], tt[1] = -0.0, np.frombuffer(np.uint64(0x7FF80000DEADBEEF).tobytes(), np.float64)[0]   # bits a float move must keep
        calls.append(dict(K=int(rng.randint(0, cap_kf)) if t else cap_kf - 1, frame_mp=fm, frame_R=R, frame_t=tt,
                          frame_kps=int(rng.randint(1, 1 << 40)) * 8, frame_desc=int(rng.randint(1, 1 << 40)) * 4))
    return table, calls


def run_insert(table, call, valid, cap_points):
    return insert_keyframe(table, call["K"], valid, cap_points, call["frame_mp"], call["frame_R"], call["frame_t"], call["frame_kps"], call["frame_desc"])


def check_insert_calls(outs):
    """every class of slot occurs, a frame names one row twice, a frame is longer than the stride, and one is empty"""
    total = np.stack([o["result"] for o in outs]).sum(0)
    assert total[I_HELD] >= 20 and total[I_INVALID] >= 2 and total[I_RANGE] >= 2 and total[I_TWICE] >= 1 and total[I_CUT] >= 1, total.tolist()
    assert any(o["result"][I_HELD] == 0 for o in outs) and all(o["result"][[1, 6, 7]].sum() == 0 for o in outs)


def make_register_calls(seed, cap_points, cap_recent=40):
    """the state a triangulation leaves and the calls on it: ranges of several lengths, an empty one, the list exactly full and one short
    (refusal 1), *d_n_registered above *d_n_points (refusal 2), counters negative and above their capacity"""
    rng = np.random.RandomState(seed)
    state = dict(ref_kf=rng.randint(-1, 6, cap_points).astype(np.int32), first_kf=rng.randint(0, 9, cap_points).astype(np.int32),
                 found=rng.randint(0, 50, cap_points).astype(np.int32), visible=rng.randint(0, 50, cap_points).astype(np.int32),
                 recent=rng.randint(0, cap_points, cap_recent).astype(np.int32))
    h = cap_points // 2
    calls = [dict(n_points=h, n_registered=h - 17, n_recent=9), dict(n_points=h, n_registered=h, n_recent=9),
             dict(n_points=h, n_registered=h - 1, n_recent=0), dict(n_points=h, n_registered=h - 20, n_recent=cap_recent - 20),
             dict(n_points=h, n_registered=h - 20, n_recent=cap_recent - 19), dict(n_points=h - 3, n_registered=h, n_recent=4),
             dict(n_points=cap_points + 9, n_registered=cap_points - 5, n_recent=-6), dict(n_points=7, n_registered=-4, n_recent=cap_recent + 3),
             dict(n_points=-1, n_registered=-8, n_recent=cap_recent + 3), dict(n_points=3, n_registered=0, n_recent=cap_recent + 3)]
    for t, c in enumerate(calls):
        c.update(K=t % 6, kf_id=t % 6 + 3 * (t % 2), cap_points=cap_points)
    return state, calls


def run_register(state, call):
    return register_new_points(call["n_points"], call["n_registered"], call["n_recent"], call["K"], call["kf_id"], call["cap_points"], state["ref_kf"],
                               state["first_kf"], state["found"], state["visible"], state["recent"])


def check_register_calls(outs):
    refusals = [int(o["result"][G_REFUSED]) for o in outs]
    assert refusals.count(1) >= 2 and refusals.count(2) >= 1 and refusals.count(0) >= 5
    assert any(o["result"][G_ROWS] == 0 and not o["result"][G_REFUSED] for o in outs)
    assert any(o["result"][G_RECENT] == len(o["recent"]) and not o["result"][G_REFUSED] and o["result"][G_ROWS] for o in outs)   # exactly full


SCENES = {"small": dict(seed=3, n_list=60, cap_points=300), "mid": dict(seed=8, n_list=200, n_kf=9, stride=160, cap_points=900)}


def make_scene(name):
    """-> dict(cull: a culling scene with its two model runs, twice: the same list with one row twice; table / inserts / insert_outs;
    state / registers / register_outs)"""
    cfg = SCENES[name]
    cull = make_cull_scene(**cfg)
    w = cull["world"]
    dup = dict(cull, recent=cull["recent"].copy())
    dup["recent"][cull["n_recent"] - 1] = next(p for p in cull["recent"][:8] if 0 <= p < w["cap_points"])
    table, inserts = make_insert_calls(cfg["seed"] + 1, w["cap_points"], w["valid"], w["stride"], w["n_kf"],
                                       (0, 1, w["stride"] - 1, w["stride"], w["stride"] + 5, w["stride"] // 2))
    state, registers = make_register_calls(cfg["seed"] + 2, w["cap_points"])
    return dict(cull=cull, cull_out=run_cull(cull), twice=dup, twice_out=run_cull(dup), table=table, inserts=inserts,
                insert_outs=[run_insert(table, c, w["valid"], w["cap_points"]) for c in inserts], state=state, registers=registers,
                register_outs=[run_register(state, c) for c in registers])


def check_scene(sc):
    check_cull_scene(sc["cull"], sc["cull_out"])
    assert sc["twice_out"]["result"].tolist() == [0, 1, 0, 0, 0, 0, 0, 0]
    check_insert_calls(sc["insert_outs"])
    check_register_calls(sc["register_outs"])
