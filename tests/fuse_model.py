"""Plain numpy / Python restatement of include/orbm.h, "The fuse's hits applied on the device", twice:
  apply            the ARRAY form the header states: the sequential loop over the entries with obs() recomputed from the slot arrays at
                   every step, so it needs no CSR (the CSR enters only where the header says so: the lists over 1024 entries that leave a
                   replace undone, and the count of unusable CSR entries); the two refusals, found on the arrays as passed
  apply_objects    an independent OBJECT-style restatement of the reference: MapPoint / KeyFrame objects, MapPoint::addObservation and
                   MapPoint::replace (MapPoint.cpp:182-188, :233-264) and the loop of ORBMatcher.cpp:533-589, a point's observations
                   iterated in ascending key-frame slot (the idea of observations_model._MapPoint)
and the seeded scenes the test files use.  No part of the library is used here."""
import numpy as np

import observations_model as om

NONE, DROPPED, GATED, ADDED, BAD_OCCUPANT, LIST_REPLACED, OCCUPANT_REPLACED, UNDONE = range(8)
R_MATCHES, R_REFUSED, R_ADDED, R_LIST_REPLACED, R_OCCUPANT_REPLACED, R_CLEARED, R_GATED, R_DROPPED = range(8)
LONG = 1024


def _n_slots(sc, k):
    return min(max(int(sc["n"][k]), 0), sc["stride"])


def _rows(sc):
    nq = len(sc["best_idx"])
    return np.arange(nq, dtype=np.int64) if sc.get("rows") is None else np.asarray(sc["rows"], np.int64)


# ---- the array form -----------------------------------------------------------------------------------------------------------
def _list_lengths(sc, csr):
    """the CSR's list length per row, 0 where the offsets do not describe a list"""
    cap = sc["cap_points"]
    if csr is None:
        return np.zeros(cap, np.int64)
    off, n_obs = np.asarray(csr[0], np.int64), len(csr[1])
    b, e = off[:cap], off[1:cap + 1]
    return np.where((b < 0) | (e < b) | (e > n_obs), 0, e - b)


def _unusable(sc, csr):
    if csr is None:
        return 0
    n_kf = len(sc["n"])
    return sum(not (0 <= k < n_kf and 0 <= i < _n_slots(sc, k)) for k, i in zip(csr[1].tolist(), csr[2].tolist()))


def refusal(sc):
    """0, or the premise the arrays as passed violate: 1 a row in two live entries, 2 a hit slot's valid occupant in a second slot of K"""
    K, cap, slots, valid = sc["K"], sc["cap_points"], sc["slots"], sc["valid"]
    n_k = _n_slots(sc, K)
    named = [int(o) for o in slots[K, :n_k]]
    live = [(int(s), int(p)) for s, p in zip(sc["best_idx"], _rows(sc))
            if 0 <= s < n_k and 0 <= p < cap and valid[p] and p not in named]
    if len({p for _, p in live}) < len(live):
        return 1
    for s in {s for s, _ in live}:
        o = named[s]
        if 0 <= o < cap and valid[o] and named.count(o) > 1:
            return 2
    return 0


def apply(sc, csr=None):
    """sc: dict(best_idx, rows | None, n, bad, slots [n_kf, stride], stride, valid, cap_points, K, found | None, visible | None).
    -> dict(slots, valid, found, code, refresh_sel, result): the arrays after the call (code / refresh_sel None when refused)"""
    K, cap, stride, bad, n_kf = sc["K"], sc["cap_points"], sc["stride"], sc["bad"], len(sc["n"])
    slots, valid = sc["slots"].copy(), sc["valid"].copy()
    found = None if sc.get("found") is None else sc["found"].copy()
    nq = len(sc["best_idx"])
    result = np.zeros(8, np.int32)
    result[R_REFUSED] = refusal(sc)
    if result[R_REFUSED]:
        return dict(slots=slots, valid=valid, found=found, code=None, refresh_sel=None, result=result)
    counted = np.zeros((n_kf, stride), bool)                             # the slots that can be an observation at all
    for k in range(n_kf):
        counted[k, :_n_slots(sc, k)] = bad[k] == 0
    lengths = _list_lengths(sc, csr)
    n_k = _n_slots(sc, K)
    code, sel = np.zeros(nq, np.int32), np.full(nq, -1, np.int32)

    def obs(p):
        k, i = np.nonzero((slots == p) & counted)
        return list(zip(k.tolist(), i.tolist()))                         # ascending (k, i)

    for j, (s, p) in enumerate(zip(sc["best_idx"].tolist(), _rows(sc).tolist())):
        if s < 0:
            continue
        if s >= n_k or p < 0 or p >= cap:
            code[j] = DROPPED
            continue
        if not valid[p] or (slots[K, :n_k] == p).any():
            code[j] = GATED
            continue
        o = int(slots[K, s])
        if o < 0 or o >= cap:
            slots[K, s], code[j], sel[j] = p, ADDED, p
        elif not valid[o]:
            code[j] = BAD_OCCUPANT
        elif lengths[p] > LONG or lengths[o] > LONG:
            code[j] = UNDONE
        else:
            loser, winner = (p, o) if len(obs(o)) > len(obs(p)) else (o, p)
            for k, i in obs(loser):
                if any(k2 == k for k2, _ in obs(winner)):
                    slots[k, i] = -1
                    result[R_CLEARED] += 1
                else:
                    slots[k, i] = winner
            valid[loser] = 0
            if found is not None:
                found[winner] = np.int32(found[winner]) + np.int32(found[loser]) + np.int32(sc["visible"][loser])
            code[j], sel[j] = (LIST_REPLACED if loser == p else OCCUPANT_REPLACED), winner
    result[R_MATCHES] = (code >= ADDED).sum()
    for r, c in ((R_ADDED, ADDED), (R_LIST_REPLACED, LIST_REPLACED), (R_OCCUPANT_REPLACED, OCCUPANT_REPLACED), (R_GATED, GATED)):
        result[r] = (code == c).sum()
    result[R_DROPPED] = (code == DROPPED).sum() + (code == UNDONE).sum() + _unusable(sc, csr)
    return dict(slots=slots, valid=valid, found=found, code=code, refresh_sel=sel, result=result)


# ---- the object form ----------------------------------------------------------------------------------------------------------
class _MapPoint(om._MapPoint):
    def __init__(self, row, bad, found, visible):
        om._MapPoint.__init__(self, row, bad, -1)
        self.found, self.visible = int(found), int(visible)

    def observes(self, k):
        return k in self.observations

    def replace(self, other, world):
        """MapPoint.cpp:233-264 without computeDescriptor and Map::eraseMapPoint"""
        if other is self:
            return
        obs, self.observations, self.is_bad = self.observations, {}, True
        for k in sorted(obs):
            for i in obs[k]:
                if not other.observes(k):
                    world["kfs"][k].map_points[i] = other                # KeyFrame::addMapPoint
                    other.add_observation(k, i)
                else:
                    world["kfs"][k].map_points[i] = None                 # KeyFrame::eraseMapPoint
                    world["cleared"] += 1
        other.found += self.found                                        # increaseFound(numFound)
        other.found += self.visible                                      # increaseFound(numVisible): the reference's text


def apply_objects(sc):
    """the loop of ORBMatcher.cpp:533-589 from the hit on; for scenes whose K is not bad and whose lists are short.  -> what `apply`
    returns (result[7] without the CSR's part)"""
    K, cap, stride, n_kf = sc["K"], sc["cap_points"], sc["stride"], len(sc["n"])
    assert not sc["bad"][K]
    world = om._world(sc["n"], sc["bad"], sc["slots"], stride, sc["valid"], cap)
    zero = np.zeros(cap, np.int32)
    found_in, visible = (zero, zero) if sc.get("found") is None else (sc["found"], sc["visible"])
    mps = [_MapPoint(p, not sc["valid"][p], found_in[p], visible[p]) for p in range(cap)]
    for old, new in zip(world["mps"], mps):
        new.observations = old.observations
    kfs = world["kfs"]
    for kf in kfs:
        kf.map_points = [None if mp is None else mps[mp.row] for mp in kf.map_points]
    world["mps"] = mps
    key_frame = kfs[K]
    nq = len(sc["best_idx"])
    code, sel, result = np.zeros(nq, np.int32), np.full(nq, -1, np.int32), np.zeros(8, np.int32)
    for j, (s, p) in enumerate(zip(sc["best_idx"].tolist(), _rows(sc).tolist())):
        if s < 0:
            continue
        if s >= len(key_frame.map_points) or not 0 <= p < cap:
            code[j] = DROPPED
            continue
        mp = mps[p]
        if mp.is_bad or mp.observes(K):                                  # :534
            code[j] = GATED
            continue
        mp1 = key_frame.map_points[s]
        if mp1 is None:                                                  # :576-578
            mp.add_observation(K, s)
            key_frame.map_points[s] = mp
            code[j], sel[j] = ADDED, p
        elif not mp1.is_bad:
            if mp1.num_obs() > mp.num_obs():                             # :580
                mp.replace(mp1, world)
                code[j], sel[j] = LIST_REPLACED, mp1.row
            else:
                mp1.replace(mp, world)
                code[j], sel[j] = OCCUPANT_REPLACED, p
        else:
            code[j] = BAD_OCCUPANT
    slots = sc["slots"].copy()
    for k, kf in enumerate(kfs):
        for i, mp in enumerate(kf.map_points):
            if mp is not None:
                slots[k, i] = mp.row
            elif 0 <= slots[k, i] < cap:
                slots[k, i] = -1
    valid = sc["valid"].copy()
    valid[:cap][[mp.is_bad for mp in mps]] = 0
    found = None
    if sc.get("found") is not None:
        found = sc["found"].copy()
        found[:cap] = np.array([mp.found for mp in mps], np.int64).astype(np.int32)
    result[R_MATCHES], result[R_CLEARED] = (code >= ADDED).sum(), world["cleared"]
    for r, c in ((R_ADDED, ADDED), (R_LIST_REPLACED, LIST_REPLACED), (R_OCCUPANT_REPLACED, OCCUPANT_REPLACED), (R_GATED, GATED),
                 (R_DROPPED, DROPPED)):
        result[r] = (code == c).sum()
    return dict(slots=slots, valid=valid, found=found, code=code, refresh_sel=sel, result=result)


# ---- seeded scenes ------------------------------------------------------------------------------------------------------------
SCENES = {
    "small": dict(seed=31, n_kf=3, stride=64, cap_points=200, n_bad=1, noise=12),
    "mid": dict(seed=32, n_kf=12, stride=256, cap_points=1000, n_bad=2, noise=150),
}


def make_scene(seed, n_kf, stride, cap_points, n_bad, noise):
    """An engineered fuse into key frame K (seed permutes the key-frame numbering, the slot positions and the list order, and draws the
    noise).  G = the other key frames that are not bad, Z = the bad ones.  Every item below owns its rows and its slot of K; `expect`
    maps its name to (entries, codes).  obs(m) = m observers from G, cycling: with a single good key frame (the small scene) a row
    observed m times holds m slots of that key frame.  Items that need three key frames of G exist in the mid scene only."""
    rng = np.random.RandomState(seed)
    role = [int(x) for x in rng.permutation(n_kf)]
    K, Z, G = role[0], role[1:1 + n_bad], role[1 + n_bad:]
    free = [[int(x) for x in rng.permutation(stride - 4)] for _ in range(n_kf)]      # the last four slots stay out: behind d_n
    slots = np.full((n_kf, stride), -1, np.int32)
    rows = [0]
    entries, expect = [], {}                                             # (sort key, row, slot of K)

    def point(observers):
        p = rows[0]
        rows[0] += 1
        for k in observers:
            slots[k, free[k].pop()] = p
        return p

    def obs(m, first=0):
        return [G[(first + x) % len(G)] for x in range(m)]

    def slot_of_k(holder):
        """a slot of K holding `holder` (a row, -1 or junk)"""
        s = free[K].pop()
        slots[K, s] = holder
        return s

    def item(name, s, ps, codes):
        base = rng.uniform(0, 1)
        keys = sorted(rng.uniform(base, 1, len(ps)))
        expect[name] = ([len(entries) + x for x in range(len(ps))], list(codes))
        for key, p in zip(keys, ps):
            entries.append((key, p, s))

    item("add", slot_of_k(-1), [point(obs(1))], [ADDED])
    item("add_junk", slot_of_k(cap_points + 3), [point(obs(2))], [ADDED])
    lonely = [point([]), point([])]                                      # adjacent rows without an observation: their offsets get broken
    item("add_lonely0", slot_of_k(-1), lonely[:1], [ADDED])
    item("add_lonely1", slot_of_k(-7), lonely[1:], [ADDED])
    o = point([K] + obs(2))
    item("list_loses", int(np.flatnonzero(slots[K] == o)[0]), [point(obs(1))], [LIST_REPLACED])        # its one slot is cleared
    o = point([K])
    item("occupant_loses", int(np.flatnonzero(slots[K] == o)[0]), [point(obs(2))], [OCCUPANT_REPLACED])
    o = point([K] + obs(1))
    item("tie", int(np.flatnonzero(slots[K] == o)[0]), [point(obs(2, 1))], [OCCUPANT_REPLACED])         # 2 == 2
    o = point([K])
    # 1 < 2: the occupant goes and p1 holds 3; then 3 > 1; then 3 > 2 -- which holds only if the slot of K that moved to p1 counts
    item("chain3", int(np.flatnonzero(slots[K] == o)[0]), [point(obs(2)), point(obs(1)), point(obs(2))],
         [OCCUPANT_REPLACED, LIST_REPLACED, LIST_REPLACED])
    # added: 1 + 1 observations; then 2 == 2, a tie only if the added slot counts: the added row is replaced again
    item("chain_add", slot_of_k(-1), [point(obs(1)), point(obs(2))], [ADDED, OCCUPANT_REPLACED])
    o = point([K] + Z[:1])
    item("bad_kf_stays", int(np.flatnonzero(slots[K] == o)[0]), [point(obs(2))], [OCCUPANT_REPLACED])
    expect["bad_kf_stays_slot"] = (Z[0], o)
    o = point([K] + obs(1))
    item("bad_occupant", int(np.flatnonzero(slots[K] == o)[0]), [point(obs(1)), point(obs(2))], [BAD_OCCUPANT, BAD_OCCUPANT])
    invalid = [o, point(obs(2))]
    item("gated_invalid", slot_of_k(-1), invalid[1:], [GATED])
    in_k = point([K] + obs(1))
    item("gated_in_k", slot_of_k(-1), [in_k], [GATED])
    if len(G) >= 3:
        o = point([K, G[1], G[2]])
        p = point([G[0], G[0]])                                          # the loser twice in one key frame: one moves, one is cleared
        item("twice", int(np.flatnonzero(slots[K] == o)[0]), [p], [LIST_REPLACED])
        expect["twice_slots"] = (G[0], p, o)
        o = point([K, G[0], G[1]])
        item("partly_seen", int(np.flatnonzero(slots[K] == o)[0]), [point([G[1], G[2]])], [LIST_REPLACED])   # one cleared, one moves
    n_rows_engineered = rows[0]
    for _ in range(noise):                                               # the rest of the map: mostly without a hit
        ks = [int(k) for k in rng.permutation(role)[:rng.randint(1, min(n_kf, 6) + 1)]]
        p = point(ks)
        if K not in ks and rng.uniform() < 0.3:
            item("noise", slot_of_k(-1), [p], [ADDED])
        elif rng.uniform() < 0.5:
            entries.append((rng.uniform(), p, -1 - int(rng.randint(0, 5))))
    junk_rows = [-3, cap_points, cap_points + 5, -2 ** 31, 2 ** 31 - 1]
    for p in junk_rows:
        entries.append((rng.uniform(), p, free[K][0]))
    some = point(obs(1))
    entries += [(rng.uniform(), some, stride), (rng.uniform(), point(obs(1)), 2 ** 31 - 1)]          # s past the key frame's slots
    assert rows[0] <= cap_points and all(len(f) > 4 for f in free)
    n = np.full(n_kf, stride - 4, np.int32)
    n[K] = stride + 5                                                    # d_n[K] > stride: clamped; its last four slots are empty
    slots[:, stride - 4:] = rng.randint(0, rows[0], (n_kf, 4))           # behind d_n: ignored ...
    slots[K, stride - 4:] = -1                                           # ... but not in K
    order = np.argsort([e[0] for e in entries], kind="stable")
    where = np.empty(len(entries), np.int64)
    where[order] = np.arange(len(entries))
    expect = {k: (([int(where[x]) for x in v[0]], v[1]) if isinstance(v[0], list) else v) for k, v in expect.items()}
    best_idx = np.array([entries[x][2] for x in order], np.int64).astype(np.int32)
    rows_arr = np.array([entries[x][1] for x in order], np.int64).astype(np.int32)
    valid = np.zeros(cap_points + 4, np.uint8)
    valid[:rows[0]] = rng.randint(1, 200, rows[0])
    valid[invalid] = 0
    valid[cap_points:] = 1
    bad = np.zeros(n_kf, np.uint8)
    bad[Z] = rng.randint(1, 200, len(Z))
    found = rng.randint(0, 50, cap_points + 4).astype(np.int32)
    visible = rng.randint(50, 100, cap_points + 4).astype(np.int32)
    return dict(best_idx=best_idx, rows=rows_arr, n=n, bad=bad, slots=slots, stride=stride, valid=valid, cap_points=cap_points, K=K,
                found=found, visible=visible, expect=expect, n_rows=rows[0], n_rows_engineered=n_rows_engineered, lonely=lonely, G=G, Z=Z)


def by_row(sc):
    """the same scene with d_rows = NULL: entry p is row p.  Chains keep their order (their rows ascend); the out-of-range rows go"""
    cap = sc["cap_points"]
    best = np.full(cap, -1, np.int32)
    for s, p in zip(sc["best_idx"].tolist(), sc["rows"].tolist()):
        if 0 <= p < cap and s >= 0:
            assert best[p] == -1
            best[p] = s
    return dict(sc, best_idx=best, rows=None, expect={k: ((sc["rows"][v[0]].tolist(), v[1]) if isinstance(v[0], list) else v)
                                                     for k, v in sc["expect"].items()})


def fresh_csr(sc):
    return om.build(sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"], 1 << 30)[:3]


def spoil_csr(sc, csr, seed):
    """the CSR with unusable entries put INTO the lists of rows the call touches (each is dropped, so the answer stays) and the offsets
    between the two adjacent rows without an observation broken (both lists are empty either way).  -> (csr, unusable entries)"""
    rng = np.random.RandomState(seed)
    off, kf, kp = [np.asarray(a).copy() for a in csr]
    n_kf, cap = len(sc["n"]), sc["cap_points"]
    lists = om.lists_of(off, kf, kp)
    touched = [p for p in rng.permutation(sc["n_rows_engineered"])[:40] if p not in sc["lonely"]]
    junk = 0
    for p in touched:
        for _ in range(rng.randint(1, 4)):
            kind = rng.randint(4)
            k = [n_kf + rng.randint(0, 1000), -1 - rng.randint(0, 1000), rng.randint(0, n_kf), rng.randint(0, n_kf)][kind]
            i = [rng.randint(0, 9), rng.randint(0, 9), -1 - rng.randint(0, 9), 0][kind]
            if kind == 3:
                i = _n_slots(sc, k) + rng.randint(0, 2) * 100000
            lists[p].insert(rng.randint(0, len(lists[p]) + 1), (int(k), int(i)))
            junk += 1
    lengths = [len(v) for v in lists]
    off = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    flat = [e for v in lists for e in v]
    kf, kp = np.array([k for k, _ in flat], np.int32), np.array([i for _, i in flat], np.int32)
    a, b = sc["lonely"]
    assert b == a + 1 and off[a] == off[a + 1] == off[b + 1]
    off[b] = [-5, len(kf) + 7][seed % 2]                                 # row a ends below its start / past the end; row b starts there
    return (off, kf, kp), junk


def long_csr(csr, p, extra=LONG + 1):
    """the CSR with `extra` unusable entries appended to row p's list: every list keeps its entries, row p's is over the limit"""
    lists = om.lists_of(*[np.asarray(a) for a in csr])
    lists[p] = lists[p] + [(-1, -1)] * extra
    flat = [e for v in lists for e in v]
    return (np.concatenate([[0], np.cumsum([len(v) for v in lists])]).astype(np.int32), np.array([k for k, _ in flat], np.int32),
            np.array([i for _, i in flat], np.int32))


def lists_of_rows_kept(before, after, p):
    """every row's list but row p's is what it was"""
    a, b = om.lists_of(*before), om.lists_of(*after)
    return all(x == y for r, (x, y) in enumerate(zip(a, b)) if r != p) and b[p][:len(a[p])] == a[p]


def refusal_scenes(sc):
    """{1: a list row twice, 2: the occupant of a hit slot in a second slot of K}, each one edit away from sc"""
    ex = sc["expect"]
    one = dict(sc, best_idx=sc["best_idx"].copy(), rows=sc["rows"].copy())
    j_from, j_to = ex["add"][0][0], ex["noise"][0][0]
    one["rows"][j_to] = one["rows"][j_from]                             # the same row hits a second slot
    two = dict(sc, slots=sc["slots"].copy())
    j = ex["occupant_loses"][0][0]
    s = int(sc["best_idx"][j])
    hit = set(sc["best_idx"].tolist())
    spare = next(int(i) for i in np.flatnonzero(two["slots"][sc["K"], :sc["stride"] - 4] == -1) if int(i) not in hit)
    two["slots"][sc["K"], spare] = sc["slots"][sc["K"], s]
    return {1: one, 2: two}


def check_scene(sc, out):
    """the properties the scene was built for; `out` = apply(sc)"""
    code, K = out["code"], sc["K"]
    slots, before = out["slots"].copy(), sc["slots"].copy()
    for a in (slots, before):                                            # what lies behind d_n[k] names nothing
        a[np.arange(len(sc["n"])) != K, sc["stride"] - 4:] = -1
    sc = dict(sc, slots=before)
    for name, v in sc["expect"].items():
        if isinstance(v[0], list):
            assert code[v[0]].tolist() == v[1], (name, code[v[0]].tolist(), v[1])
    res = out["result"]
    assert res[R_REFUSED] == 0 and res[R_ADDED] >= 6 and res[R_LIST_REPLACED] >= 3 and res[R_OCCUPANT_REPLACED] >= 5
    assert res[R_CLEARED] >= 4 and res[R_GATED] >= 2 and res[R_DROPPED] >= (7 if sc.get("rows") is not None else 2) and res[R_MATCHES] == (code >= ADDED).sum()
    assert sc["n"][K] > sc["stride"] and (sc["best_idx"] == -1).any()
    entries = lambda name: sc["expect"][name][0]  # noqa: E731
    rows = _rows(sc)
    # the chain of three: the slot of K ends with the first list point, which holds three observations and both later rows are gone
    j1, j2, j3 = entries("chain3")
    s = int(sc["best_idx"][j1])
    assert slots[K, s] == rows[j1] and (slots == rows[j1]).sum() == 3 and not out["valid"][rows[j2]] and not out["valid"][rows[j3]]
    assert (slots == rows[j2]).sum() == 0 and (slots == rows[j3]).sum() == 0 and (sc["slots"] == rows[j3]).sum() == 2
    assert out["refresh_sel"][[j1, j2, j3]].tolist() == [rows[j1]] * 3
    # the chain behind an add: the added row lost the tie again
    ja, jb = entries("chain_add")
    assert slots[K, int(sc["best_idx"][ja])] == rows[jb] and not out["valid"][rows[ja]] and out["refresh_sel"][ja] == rows[ja]
    # the loser's slot in the bad key frame still names it
    z, o = sc["expect"]["bad_kf_stays_slot"]
    assert (slots[z] == o).sum() == 1 and not out["valid"][o] and (slots[[k for k in range(len(sc["n"])) if k != z]] == o).sum() == 0
    # the bad occupant keeps its slot and both hits count
    jo = entries("bad_occupant")[0]
    assert slots[K, int(sc["best_idx"][jo])] == sc["slots"][K, int(sc["best_idx"][jo])] and out["valid"][rows[jo]]
    if "twice" in sc["expect"]:
        g, p, o = sc["expect"]["twice_slots"]
        assert (sc["slots"][g] == p).sum() == 2 and (slots[g] == o).sum() == 1 and (slots == p).sum() == 0
        j = entries("partly_seen")[0]
        assert (slots == rows[j]).sum() == 0 and (sc["slots"] == rows[j]).sum() == 2
    if out["found"] is not None:
        j = entries("occupant_loses")[0]
        o = sc["slots"][K, int(sc["best_idx"][j])]
        assert out["found"][rows[j]] == sc["found"][rows[j]] + sc["found"][o] + sc["visible"][o]


def make_projected_scene(n_kp=2000, n_cand=4000, n_occ=1000, n_kf=8, seed=6, cap_points=None):
    """A fuse with geometry, for the chain builder -> search -> apply: key frame 0 = K at the identity pose with n_kp key points, n_cand
    candidate rows on a plane in front of it, the first half of which re-observe a key point each (position and descriptor), n_occ rows
    behind the camera that occupy every other slot of K, every row seen by one to three of the other key frames.  entry j = row j"""
    import projection_model as pm
    rng = np.random.RandomState(seed)
    w, h, fx, fy, cx, cy, Z = 752, 480, 460.0, 460.0, 376.0, 240.0, 10.0
    kps = np.zeros(n_kp, pm.KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(20, w - 20, n_kp), rng.uniform(20, h - 20, n_kp)
    kps["octave"], kps["class_id"], kps["angle"] = rng.randint(0, pm.N_LEVELS, n_kp), -1, rng.uniform(0, 360, n_kp)
    kps["size"] = 31.0 * pm.SCALE_FACTORS[kps["octave"]]
    desc = rng.randint(0, 256, (n_kp, 32)).astype(np.uint8)
    used_rows = n_cand + n_occ
    cap = cap_points or used_rows
    target = rng.permutation(n_kp)[:n_cand // 2]                           # candidate p < n_cand / 2 re-observes key point target[p]
    x = np.concatenate([kps["x"][target] + rng.normal(0, 0.5, len(target)), rng.uniform(20, w - 20, n_cand - len(target))])
    y = np.concatenate([kps["y"][target] + rng.normal(0, 0.5, len(target)), rng.uniform(20, h - 20, n_cand - len(target))])
    octave = np.concatenate([kps["octave"][target], rng.randint(0, pm.N_LEVELS, n_cand - len(target))])
    points = np.zeros((cap, 3), np.float32)
    points[:n_cand] = np.stack([(x - cx) * Z / fx, (y - cy) * Z / fy, np.full(n_cand, Z)], 1)
    points[n_cand:] = (0.0, 0.0, -5.0)                                     # the occupants are no candidates: behind the camera
    d0 = np.linalg.norm(points.astype(np.float64), axis=1)
    normals = (points / d0[:, None]).astype(np.float32)
    max_dist, min_dist = np.ones(cap, np.float32), (0.3 * d0).astype(np.float32)
    max_dist[:n_cand] = d0[:n_cand] * 1.2 ** (octave - 0.3)
    q_desc = rng.randint(0, 256, (cap, 32)).astype(np.uint8)
    flips = np.packbits(rng.uniform(size=(len(target), 256)) < 0.04, axis=1, bitorder="little")
    q_desc[:len(target)] = desc[target] ^ flips
    slots = np.full((n_kf, n_kp), -1, np.int32)
    slots[0, :2 * n_occ:2] = n_cand + np.arange(n_occ)                     # K = key frame 0: every other slot occupied
    used = np.zeros(n_kf, np.int64)
    for p in range(used_rows):                                             # one to three observers among the other key frames
        if p < n_cand or rng.uniform() < 0.6:
            ks = 1 + rng.permutation(n_kf - 1)[:rng.randint(1, 4)]
            slots[ks, used[ks]] = p
            used[ks] += 1
    assert used.max() <= n_kp
    return dict(w=w, h=h, cam=(fx, fy, cx, cy), kps=kps, desc=desc, q_desc=q_desc, points=points, normals=normals, min_dist=min_dist,
                max_dist=max_dist, n=np.full(n_kf, n_kp, np.int32), bad=np.zeros(n_kf, np.uint8), slots=slots, stride=n_kp,
                valid=(np.arange(cap) < used_rows).astype(np.uint8), cap_points=cap, K=0, found=rng.randint(0, 50, cap).astype(np.int32),
                visible=rng.randint(50, 100, cap).astype(np.int32), rows=None)
