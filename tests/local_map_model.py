"""Two restatements of the tracker's local map on the device (include/orbm.h, "The tracker's local map on the device"), and the scenes.

The ARRAY form states the three calls on the header's arrays, exactly as the header does: it is the model the device is compared with.
The OBJECT form follows the reference line by line -- Tracking::updateLocalKeyFrames / updateLocalMapPoints (modules/Frontend/
Tracking.cpp:429-537), the counters of searchLocalPoints and trackLocalMap (:388-412, :362-364) and KeyFrame::getNumTrackedMapPoint
(modules/BasicObject/KeyFrame.cpp:146-152) -- on KeyFrame / MapPoint / Frame objects with track_frame_id stamps, observation dicts and
ordered lists; where the reference iterates an unordered_map or a set of pointers it iterates in ascending key-frame slot, the
header's canonicalisation.  A scene is a seeded world (slot arrays, the CSR observations_model.build leaves from them, a graph built
by graph_model.update from the key frames' real shared rows) and a list of calls on it.  No part of the library is used here."""
import numpy as np

import graph_model as gm
import observations_model as om

(R_KF, R_ROWS, R_REFUSED, R_MAX_KF, R_MAX_VOTES, R_CLEARED, R_CSR_DROPPED, R_CSR_STALE, R_VOTED, R_RECENT_BAD, R_LIST_DROPPED, R_END, R_INVALID,
 R_DUPLICATES) = range(14)
END_RAN_OUT, END_SIZE_LIMIT, END_PARENT = range(3)
C_VISIBLE_FRAME, C_VISIBLE_QUERIES, C_FOUND, C_CLEARED = range(4)
N_NEIGH, MAX_KF = 10, 80          # Tracking.cpp:495, :492


# ---- the array form ---------------------------------------------------------------------------------------------------------------
def _row_list(w, p):
    b, e = int(w["obs_off"][p]), int(w["obs_off"][p + 1])
    return range(b, e) if 0 <= b <= e <= len(w["obs_kf"]) else range(0)


def _entry_state(w, j, p):
    """CSR entry j of row p -> (1 live / 0 stale / -1 an index out of range, its key frame)"""
    k, i = int(w["obs_kf"][j]), int(w["obs_kp"][j])
    if not 0 <= k < w["n_kf"] or not 0 <= i < min(max(int(w["n"][k]), 0), w["stride"]):
        return -1, k
    return int(w["slots"][k, i] == p and w["bad"][k] == 0), k


def local_map(w, frame_mp, recent, n_neigh=N_NEIGH, max_kf=MAX_KF, cap_local_kf=1 << 30, cap_rows=1 << 30, ref=-7, tags=None):
    """-> dict(frame_mp: as the call leaves it, local_kf, rows: the FULL lists, mask u8 [cap_points], ref: *d_ref afterwards, result i32
    [16], lengths: the list's length at every position the walk entered).  tags: a set that receives the cases this call met."""
    tags = set() if tags is None else tags
    n_kf, cap, g = w["n_kf"], w["cap_points"], w["g"]
    res = np.zeros(16, np.int32)
    frame_mp = np.array(frame_mp, np.int32)
    votes = np.zeros(n_kf, np.int64)
    named = set()
    for i in range(len(frame_mp)):                                 # the votes (:431-460)
        p = int(frame_mp[i])
        if not 0 <= p < cap:
            continue
        if not w["valid"][p]:
            frame_mp[i] = -1
            res[R_CLEARED] += 1
            tags.add("frame_bad_row")
            continue
        if p in named:
            tags.add("frame_row_twice")
        named.add(p)
        for j in _row_list(w, p):
            state, k = _entry_state(w, j, p)
            if state > 0:
                votes[k] += 1
            elif state < 0:
                res[R_CSR_DROPPED] += 1
                tags.add("csr_out_of_range")
            else:
                res[R_CSR_STALE] += 1
                tags.add("csr_stale")
    marks, lst = set(), []
    for k in recent:                                               # :466-470
        k = int(k)
        assert 0 <= k < n_kf and k not in marks                    # an argument error
        lst.append(k)
        marks.add(k)
        if w["bad"][k]:
            res[R_RECENT_BAD] += 1
            tags.add("recent_bad")
    voted = np.flatnonzero(votes > 0)
    res[R_VOTED] = len(voted)
    for k in voted.tolist():                                       # :474-487 in ascending slot order
        if k in marks:
            tags.add("voted_in_recent")
            continue
        lst.append(k)
        marks.add(k)
    max_kf_slot = -1
    if len(voted):
        res[R_MAX_VOTES] = votes.max()
        top = np.flatnonzero(votes == votes.max())
        max_kf_slot = int(top[0])                                  # the least slot among the maxima
        if len(top) > 1:
            tags.add("vote_tie")
    else:
        tags.add("no_vote")
    end0, end, lengths = len(lst), END_RAN_OUT, []
    for pos in range(end0):                                        # the expansion (:490-519)
        if len(lst) > max_kf:
            end = END_SIZE_LIMIT
            tags.add("end0_over_limit" if pos == 0 else "size_limit")
            if pos and lengths[-1] == max_kf and len(lst) == max_kf + 1:
                tags.add("size_limit_exact")
            break
        lengths.append(len(lst))
        kf = lst[pos]
        nn = min(max(n_neigh, 0), min(max(int(g["ord_n"][kf]), 0), n_kf))
        for b in g["ord_kf"][kf, :nn].tolist():
            if not 0 <= b < n_kf:
                res[R_LIST_DROPPED] += 1
            elif w["bad"][b]:
                if b not in marks:
                    tags.add("bad_neighbour_skipped")
            elif b not in marks:
                lst.append(b)
                marks.add(b)
        children = np.flatnonzero(np.asarray(g["parent"][:n_kf]) == kf).tolist()
        for n_before, j in enumerate(children):
            if not w["bad"][j] and j not in marks:
                lst.append(j)
                marks.add(j)
                tags.add("child_taken")
                if n_before and w["bad"][children[0]] and children[0] not in marks:
                    tags.add("first_child_bad_second_taken")
                break
        P = int(g["parent"][kf])
        if 0 <= P < n_kf and P not in marks:                       # not tested for bad; the break leaves the whole walk
            lst.append(P)
            marks.add(P)
            end = END_PARENT
            tags.add("parent_break_at_0" if pos == 0 else "parent_break_later")
            if w["bad"][P]:
                tags.add("parent_bad_taken")
            break
    else:
        if end0:
            tags.add("ran_to_end0")
    seen, rows = set(), []
    for k in lst:                                                  # the points (:525-537)
        for i in range(min(max(int(w["n"][k]), 0), w["stride"])):
            p = int(w["slots"][k, i])
            if not 0 <= p < cap:
                continue
            if not w["valid"][p]:
                res[R_INVALID] += 1
            elif p in seen:
                res[R_DUPLICATES] += 1
            else:
                seen.add(p)
                rows.append(p)
    if res[R_INVALID] and res[R_DUPLICATES]:
        tags.add("point_duplicates_and_invalid")
    refused = (1 if len(lst) > cap_local_kf else 0) | (2 if len(rows) > cap_rows else 0)
    if refused:
        tags.add("refused_%d" % refused)
    mask = np.zeros(cap, np.uint8)
    if not refused:
        mask[rows] = 1
        if max_kf_slot >= 0:
            ref = max_kf_slot
    res[R_KF], res[R_ROWS], res[R_REFUSED], res[R_MAX_KF], res[R_END] = len(lst), len(rows), refused, max_kf_slot, end
    return dict(frame_mp=frame_mp, local_kf=np.array(lst, np.int32), rows=np.array(rows, np.int32), mask=mask, ref=ref, result=res, lengths=lengths)


def track_counters(frame_mp, valid, cap_points, q_ok, what, visible, found):
    """-> (frame_mp, visible, found as the call leaves them, result i32 [8])"""
    frame_mp, visible, found = np.array(frame_mp, np.int32), np.array(visible, np.int32), np.array(found, np.int32)
    res = np.zeros(8, np.int32)
    for i in range(len(frame_mp)):
        p = int(frame_mp[i])
        if not 0 <= p < cap_points:
            continue
        if what & 1:                                               # :388-398
            if not valid[p]:
                frame_mp[i] = -1
                res[C_CLEARED] += 1
                continue
            visible[p] += 1
            res[C_VISIBLE_FRAME] += 1
        if what & 4:                                               # :362-364
            found[p] += 1
            res[C_FOUND] += 1
    if what & 2:                                                   # :406-408
        on = np.flatnonzero(np.asarray(q_ok) != 0)
        visible[on] += 1
        res[C_VISIBLE_QUERIES] = len(on)
    return frame_mp, visible, found, res


def num_tracked(w, kf, min_obs):
    """-> d_count i32 [4]: [0] the count, [1] kf outside [0, n_kf), [2] CSR entries dropped for an index out of range, [3] 0"""
    out = np.zeros(4, np.int32)
    if not 0 <= kf < w["n_kf"]:
        out[1] = 1
        return out
    for i in range(min(max(int(w["n"][kf]), 0), w["stride"])):
        p = int(w["slots"][kf, i])
        if not 0 <= p < w["cap_points"]:
            continue
        states = [_entry_state(w, j, p)[0] for j in _row_list(w, p)]
        out[2] += states.count(-1)
        out[0] += states.count(1) >= min_obs
    return out


# ---- the object form ----------------------------------------------------------------------------------------------------------------
class MapPoint:
    def __init__(self, row, is_bad):
        self.row, self.is_bad = row, is_bad
        self.observations = {}                                     # KeyFrame -> feature index
        self.track_frame_id = self.last_frame_seen = None
        self.visible = self.found = 0

    def get_num_obs(self):
        return len(self.observations)


class KeyFrame:
    def __init__(self, slot):
        self.id = slot
        self.is_bad = False
        self.ordered_connected_kfs, self.parent, self.children = [], None, set()
        self.map_points = []
        self.track_frame_id = None

    def get_best_covisible_kfs(self, num):                         # KeyFrame.cpp:339-345
        return list(self.ordered_connected_kfs) if len(self.ordered_connected_kfs) < num else self.ordered_connected_kfs[:num]

    def get_num_tracked_map_point(self, min_obs):                  # KeyFrame.cpp:146-152
        num = 0
        for mp in self.map_points:
            if mp is not None and mp.get_num_obs() >= min_obs:
                num += 1
        return num


class Frame:
    def __init__(self, frame_id, map_points):
        self.id, self.map_points = frame_id, map_points


def world_objects(w):
    """the world as objects: a MapPoint per table row, its observations the LIVE CSR entries; key frames with their lists, parents,
    children and map points (None where a slot holds no row) -> (key frames, map points)"""
    n_kf, g = w["n_kf"], w["g"]
    mps = [MapPoint(p, not w["valid"][p]) for p in range(w["cap_points"])]
    kfs = [KeyFrame(k) for k in range(n_kf)]
    for k, kf in enumerate(kfs):
        kf.is_bad = bool(w["bad"][k])
        kf.ordered_connected_kfs = [kfs[j] for j in g["ord_kf"][k, :g["ord_n"][k]]]
        if g["parent"][k] >= 0:
            kf.parent = kfs[g["parent"][k]]
            kf.parent.children.add(kf)
        kf.map_points = [mps[p] if 0 <= p < w["cap_points"] else None for p in w["slots"][k, :min(max(int(w["n"][k]), 0), w["stride"])]]
    for p, mp in enumerate(mps):
        for j in _row_list(w, p):
            state, k = _entry_state(w, j, p)
            if state > 0:
                assert kfs[k] not in mp.observations               # the scenes name a row once per key frame
                mp.observations[kfs[k]] = int(w["obs_kp"][j])
    return kfs, mps


def frame_object(frame_id, frame_mp, mps):
    return Frame(frame_id, [mps[p] if 0 <= p < len(mps) else None for p in frame_mp])


def update_local_key_frames(frame, recent_kfs, reference_kf, n_neigh=N_NEIGH, max_kf=MAX_KF):
    """Tracking.cpp:429-523 -> (local_keyframes, reference_kf)"""
    kf_counter = {}
    for i in range(len(frame.map_points)):
        mp = frame.map_points[i]
        if mp is not None:
            if not mp.is_bad:
                for kf in mp.observations:
                    kf_counter[kf] = kf_counter.get(kf, 0) + 1
            else:
                frame.map_points[i] = None
    max_obs, max_kf_obj = 0, None
    local_keyframes = list(recent_kfs)
    for kf in local_keyframes:
        kf.track_frame_id = frame.id
    for kf in sorted(kf_counter, key=lambda k: k.id):              # canonical: ascending slot
        if kf.is_bad:
            continue
        if kf_counter[kf] > max_obs:
            max_obs, max_kf_obj = kf_counter[kf], kf
        if kf.track_frame_id != frame.id:
            local_keyframes.append(kf)
            kf.track_frame_id = frame.id
    it, it_end = 0, len(local_keyframes)
    while it < it_end:
        if len(local_keyframes) > max_kf:
            break
        kf = local_keyframes[it]
        for neigh in kf.get_best_covisible_kfs(n_neigh):
            if not neigh.is_bad and neigh.track_frame_id != frame.id:
                local_keyframes.append(neigh)
                neigh.track_frame_id = frame.id
        for child in sorted(kf.children, key=lambda k: k.id):      # canonical: ascending slot
            if not child.is_bad and child.track_frame_id != frame.id:
                local_keyframes.append(child)
                child.track_frame_id = frame.id
                break
        parent = kf.parent
        if parent is not None and parent.track_frame_id != frame.id:
            local_keyframes.append(parent)
            parent.track_frame_id = frame.id
            break
        it += 1
    if max_kf_obj is not None:
        reference_kf = max_kf_obj
    return local_keyframes, reference_kf


def update_local_map_points(frame, local_keyframes):
    """Tracking.cpp:525-537"""
    local_map_points = []
    for kf in local_keyframes:
        for mp in kf.map_points:
            if mp is not None and not mp.is_bad and mp.track_frame_id != frame.id:
                local_map_points.append(mp)
                mp.track_frame_id = frame.id
    return local_map_points


def search_local_points_counters(frame, local_map_points, in_frustum):
    """Tracking.cpp:388-412 without the search; in_frustum [row]: what Frame::isInFrustum returns"""
    for i, mp in enumerate(frame.map_points):
        if mp is not None:
            if mp.is_bad:
                frame.map_points[i] = None
            else:
                mp.visible += 1
                mp.last_frame_seen = frame.id
    for mp in local_map_points:
        if mp.last_frame_seen == frame.id or mp.is_bad:
            continue
        if in_frustum[mp.row]:
            mp.visible += 1


def increase_found(frame):
    """Tracking.cpp:362-364"""
    for mp in frame.map_points:
        if mp is not None:
            mp.found += 1


# ---- the worlds -----------------------------------------------------------------------------------------------------------------------
def make_world(seed, n_kf, stride, cap_points, span, step, th, bad=(), few=(), n_stale=0, n_junk=0, cap_kf=None):
    """A camera moving along the table: key frame k observes `stride` distinct rows of [k * step, k * step + span), so covisibility is
    local.  The graph is graph_model.update on the key frames' real shared-row counts, each key frame connected to the EARLIER ones when it
    is inserted (threshold th), so the parent is the best earlier key frame.  Then the key frames of `bad` go bad the way the culling leaves
    them (d_bad set, every slot -1) with the graph NOT yet erased; the CSR is observations_model.build's; afterwards n_stale slots
    change (their CSR entries are stale) and n_junk CSR entries get an index out of range.  few: key frames with three slots only."""
    rng = np.random.RandomState(seed)
    assert span <= cap_points and (n_kf - 1) * step + span <= cap_points + step * n_kf
    n = rng.randint(stride // 2, stride + 1, n_kf).astype(np.int32)
    n[rng.rand(n_kf) < 0.15] = stride + 5                          # more features than slots
    n[list(few)] = 3
    slots = np.full((n_kf, stride), -1, np.int32)
    for k in range(n_kf):
        lo = min(k * step, cap_points - span)
        slots[k] = lo + rng.choice(span, stride, replace=False)    # a row once per key frame
    slots[rng.rand(n_kf, stride) < 0.25] = -1
    slots[rng.rand(n_kf, stride) < 0.02] = cap_points + 5
    slots[rng.rand(n_kf, stride) < 0.02] = -7
    valid = (rng.rand(cap_points) < 0.9).astype(np.uint8)
    g = gm.new_graph(cap_kf or n_kf + 3)
    none_bad = np.zeros(n_kf, np.uint8)
    rows_of = []
    for k in range(n_kf):
        r = slots[k, :min(int(n[k]), stride)]
        r = r[(r >= 0) & (r < cap_points)]
        rows_of.append(set(r[valid[r] != 0].tolist()))
        covis = np.array([len(rows_of[k] & rows_of[j]) if j < k else 0 for j in range(n_kf)], np.int32)
        gm.update(g, n_kf, none_bad, covis, k, 0, th)
    is_bad = np.zeros(n_kf, np.uint8)
    is_bad[list(bad)] = 1
    slots[is_bad != 0] = -1
    off, okf, okp, _ = om.build(n, is_bad, slots, stride, valid, cap_points, 1 << 30)
    okf, okp = okf.copy(), okp.copy()
    for j in rng.choice(len(okf), n_stale, replace=False):
        slots[okf[j], okp[j]] = -1 if rng.rand() < 0.5 else rng.randint(cap_points)
    for t, j in enumerate(rng.choice(len(okf), n_junk, replace=False)):
        if t % 2:
            okf[j] = (n_kf, -1, 1 << 30)[t % 3]
        else:
            okp[j] = (stride, -2, 1 << 30)[t % 3]
    return dict(n_kf=n_kf, stride=stride, cap_points=cap_points, n=n, bad=is_bad, slots=slots, valid=valid, obs_off=off, obs_kf=okf, obs_kp=okp, g=g)


def frame_at(w, seed, at, n2, n_matched, step, span, n_bad_rows=2, n_twice=2):
    """the frame's slots: n_matched rows the camera sees at key-frame position `at`, some bad ones, some named twice, -1 and junk"""
    rng = np.random.RandomState(seed)
    fm = np.full(n2, -1, np.int32)
    if n_matched == 0:
        return fm
    cap = w["cap_points"]
    lo = min(at * step, cap - span)
    rows = lo + rng.choice(span, min(span, n_matched + n_bad_rows), replace=False)
    ok, bad_rows = rows[w["valid"][rows] != 0][:n_matched], rows[w["valid"][rows] == 0][:n_bad_rows]
    put = np.concatenate([ok, bad_rows, ok[:n_twice], [cap + 3, -9]]).astype(np.int32)[:n2]
    fm[rng.choice(n2, len(put), replace=False)] = put
    return fm


SCENES = dict(small=dict(world=dict(seed=5, n_kf=40, stride=32, cap_points=600, span=110, step=12, th=4, bad=(7, 14, 22, 31), few=(14, 26),
                                    n_stale=25, n_junk=12), n2=70, n_matched=22),
              mid=dict(world=dict(seed=6, n_kf=120, stride=96, cap_points=2400, span=300, step=18, th=8, bad=(9, 36, 40, 77, 101), few=(40, 63),
                                  n_stale=90, n_junk=30), n2=400, n_matched=120))
ALL_TAGS = {"frame_bad_row", "frame_row_twice", "csr_stale", "csr_out_of_range", "vote_tie", "no_vote", "recent_bad", "voted_in_recent",
            "bad_neighbour_skipped", "child_taken", "first_child_bad_second_taken", "parent_break_at_0", "parent_break_later", "ran_to_end0",
            "size_limit_exact", "end0_over_limit", "parent_bad_taken", "point_duplicates_and_invalid", "refused_1", "refused_2"}


def make_scene(name):
    """-> dict(world, calls: [dict(frame_mp, recent, n_neigh, max_kf, cap_local_kf, cap_rows)], outs: the array model's output per call,
    tags).  The calls: frames at several positions (one without a match, one with five), the recent key frames empty, one, ten as
    Map::getRecentKeyFrames(10) gives them (oldest first) and ten elsewhere, n_neigh 0, 1 and 10, max_kf 80, 0 and 1; then, found by
    search among them, calls whose size limit is met exactly, and both refusals of the first call with a vote."""
    cfg = SCENES[name]
    wc = cfg["world"]
    w = make_world(**wc)
    n_kf = w["n_kf"]
    frames = [frame_at(w, 50 + t, at, cfg["n2"], (0, cfg["n_matched"], cfg["n_matched"], cfg["n_matched"], 5)[t], wc["step"], wc["span"])
              for t, at in enumerate((0, n_kf // 5, n_kf // 2, n_kf - 8, n_kf // 3))]
    bad = sorted(wc["bad"])
    recents = [[], [5], list(range(n_kf - 10, n_kf)), list(range(bad[1] - 4, bad[1] + 6)), [bad[0] + 1], [bad[2] + 1, 3]]
    calls = []
    for fi, fm in enumerate(frames):
        for ri, rec in enumerate(recents):
            for n_neigh in (0, 1, N_NEIGH):
                if (fi + ri + n_neigh) % 2 == 0 or n_neigh == N_NEIGH:
                    calls.append(dict(frame_mp=fm, recent=np.array(rec, np.int32), n_neigh=n_neigh, max_kf=MAX_KF))
    calls.append(dict(calls[-1], max_kf=0))
    calls.append(dict(calls[-1], max_kf=1))
    tags, outs = set(), []
    for c in calls:
        outs.append(local_map(w, tags=tags, **c))
    exact = []
    for c, o in zip(list(calls), list(outs)):                      # a walk entered at length max_kf, the next one refused at max_kf + 1
        ln = o["lengths"]
        for a, b in zip(ln, ln[1:]):
            if b == a + 1 and len(exact) < 2:
                exact.append(dict(c, max_kf=a))
                break
    first = next(t for t, o in enumerate(outs) if o["result"][R_MAX_KF] >= 0 and o["result"][R_ROWS] > 1)
    short = [dict(calls[first], cap_local_kf=int(outs[first]["result"][R_KF]) - 1), dict(calls[first], cap_rows=int(outs[first]["result"][R_ROWS]) - 1)]
    for c in exact + short:
        calls.append(c)
        outs.append(local_map(w, tags=tags, **c))
    return dict(name=name, world=w, calls=calls, outs=outs, tags=tags)


def check_scene(sc):
    """the scene holds every case it was built for"""
    missing = ALL_TAGS - sc["tags"]
    assert not missing, missing
    w = sc["world"]
    assert (w["slots"] == -1).any() and (w["slots"] > w["cap_points"]).any() and (w["n"] > w["stride"]).any()
    ends = {int(o["result"][R_END]) for o in sc["outs"]}
    assert ends == {END_RAN_OUT, END_SIZE_LIMIT, END_PARENT}
    for o in sc["outs"]:
        r = o["result"]
        if r[R_REFUSED]:
            assert not o["mask"].any() and o["ref"] == -7 and r[R_KF] == len(o["local_kf"]) and r[R_ROWS] == len(o["rows"])


# ---- worlds at the sizes where the kernel changes path -----------------------------------------------------------------------------------
def make_direct_world(seed, n_kf, stride, cap_points, cap_kf=None, list_max=14, p_bad=0.05, p_stray=0.1, p_full=0.3):
    """A world whose graph is written directly (graph_model.update's Python loops are too slow for 4096 key frames): every key frame a
    random list of up to list_max distinct others; its parent is the head of that list (what updateConnections leaves) but for a share p_stray
    of them, which have any other key frame or none; some key frames bad; every key frame observes `stride` distinct random rows.  The CSR is observations_model.build's."""
    rng = np.random.RandomState(seed)
    cap_kf = cap_kf or n_kf + 3
    g = gm.new_graph(cap_kf)
    for k in range(n_kf):
        cnt = int(rng.randint(0, min(list_max, n_kf - 1) + 1))
        others = rng.choice(n_kf - 1, cnt, replace=False)
        g["ord_kf"][k, :cnt] = others + (others >= k)
        g["ord_n"][k] = cnt
        other = int(rng.randint(n_kf))
        g["parent"][k] = g["ord_kf"][k, 0] if cnt and rng.rand() >= p_stray else other if other != k and rng.rand() < 0.5 else -1
    bad = (rng.rand(n_kf) < p_bad).astype(np.uint8)
    n = rng.randint(stride // 2, stride + 1, n_kf).astype(np.int32)
    n[rng.rand(n_kf) < p_full] = stride
    n[rng.rand(n_kf) < 0.05] = stride + 7
    slots = np.stack([rng.choice(cap_points, stride, replace=False) for _ in range(n_kf)]).astype(np.int32)
    slots[rng.rand(n_kf, stride) < 0.2] = -1
    slots[rng.rand(n_kf, stride) < 0.01] = cap_points + 1
    slots[bad != 0] = -1
    valid = (rng.rand(cap_points) < 0.9).astype(np.uint8)
    off, okf, okp, _ = om.build(n, bad, slots, stride, valid, cap_points, 1 << 30)
    return dict(n_kf=n_kf, stride=stride, cap_points=cap_points, n=n, bad=bad, slots=slots, valid=valid, obs_off=off, obs_kf=okf, obs_kp=okp, g=g)


def direct_frame(w, seed, n2, n_matched):
    """n_matched observed rows (a few bad, a few twice) in a frame of n2 slots whose LAST slot holds one: the rest -1 and junk"""
    rng = np.random.RandomState(seed)
    fm = np.full(n2, -1, np.int32)
    observed = np.flatnonzero(np.diff(w["obs_off"]) > 0)
    if n2 == 0 or len(observed) == 0:
        return fm
    put = rng.choice(observed, min(n_matched, len(observed), n2), replace=False)
    spare = max(0, n2 - len(put))
    extra = np.concatenate([np.flatnonzero(w["valid"] == 0)[:2], put[:2], [w["cap_points"], -3]])[:spare]
    put = np.concatenate([put, extra]).astype(np.int32)
    at = rng.choice(n2, len(put), replace=False)
    if n2 - 1 not in at:
        at[0] = n2 - 1
    fm[at] = put
    return fm
