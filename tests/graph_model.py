"""Two restatements of the covisibility graph on the device (include/orbm.h, "The covisibility graph on the device"), and the scenes.

The ARRAY form states the four calls on the header's arrays, exactly as the header does.  The OBJECT form follows the reference's
KeyFrame::updateConnections / addConnection / eraseConnection / updateBestCovisibles / setBad (modules/BasicObject/KeyFrame.cpp:225-337,
:402-467) and LocalMapping::searchInNeighbors (modules/Frontend/LocalMapping.cpp:263-300) line by line on KeyFrame objects with a dict
connected_kf_weights, a list ordered_connected_kfs, parent and children_set -- with the header's two canonical tie rules, and :428-460
restated literally (the loop, not its simplification).  A scene is a seeded sequence of operations run from an empty graph."""
import numpy as np

CONNECT_TH = 15
U_N, U_NOTHING, U_FALLBACK, U_REBUILT, U_PARENT, U_BAD, U_JUNK = range(7)
E_ERASED, E_CONNECTIONS, E_CHILDREN, E_NO_PARENT, E_LISTS = range(5)
T_TARGETS, T_ROWS, T_REFUSED, T_BAD, T_INVALID, T_DROPPED, T_DUPLICATES = range(7)
LIST_FILL = -99          # what the scenes' d_ord_kf holds where no call ever wrote


# ---- the array form ---------------------------------------------------------------------------------------------------------------
def new_graph(cap_kf):
    return dict(cap_kf=cap_kf, weight=np.zeros((cap_kf, cap_kf), np.int32), ord_kf=np.full((cap_kf, cap_kf), LIST_FILL, np.int32),
                ord_n=np.zeros(cap_kf, np.int32), parent=np.full(cap_kf, -1, np.int32))


def copy_graph(g):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items()}


def counts(covis, bad, K, n_kf):
    """c[j] of the header, and the two ignored kinds"""
    c = np.zeros(n_kf, np.int32)
    on_bad = junk = 0
    for j in range(n_kf):
        v = int(covis[j])
        if j == K:
            junk += v != 0
        elif v < 0:
            junk += 1
        elif v > 0 and bad[j]:
            on_bad += 1
        elif v > 0:
            c[j] = v
    return c, on_bad, junk


def list_of_row(row, n_kf):
    """the non-zero entries of a row in list order: descending weight, ascending slot"""
    js = np.flatnonzero(row[:n_kf])
    return js[np.lexsort((js, -row[js].astype(np.int64)))].astype(np.int32)


def _rebuild(g, j, n_kf):
    lst = list_of_row(g["weight"][j], n_kf)
    g["ord_kf"][j, :len(lst)] = lst
    g["ord_n"][j] = len(lst)


def update(g, n_kf, bad, covis, K, first_kf, th=CONNECT_TH):
    res = np.zeros(8, np.int32)
    c, res[U_BAD], res[U_JUNK] = counts(covis, bad, K, n_kf)
    if not (c > 0).any():
        res[U_NOTHING] = 1
        return res
    S = np.flatnonzero(c >= th)
    if len(S) == 0:
        S = np.array([int(np.flatnonzero(c == c.max())[0])])
        res[U_FALLBACK] = 1
    for j in S:
        if g["weight"][j, K] != c[j]:
            g["weight"][j, K] = c[j]
            _rebuild(g, j, n_kf)
            res[U_REBUILT] += 1
    g["weight"][K, :n_kf] = c
    S = S[np.lexsort((S, -c[S].astype(np.int64)))]
    g["ord_kf"][K, :len(S)] = S
    g["ord_n"][K] = len(S)
    if g["parent"][K] < 0 and K != first_kf:
        g["parent"][K] = S[0]
        res[U_PARENT] = 1
    res[U_N] = len(S)
    return res


def erase(g, n_kf, recent, code=None):
    res = np.zeros(8, np.int32)
    marked = set()
    for idx, c in enumerate(recent):
        if code is not None and code[idx] != 3:
            continue
        c = int(c)
        for j in range(n_kf):
            if j != c and g["weight"][c, j] > 0 and g["weight"][j, c] > 0:
                g["weight"][j, c] = 0
                marked.add(j)
                res[E_CONNECTIONS] += 1
        g["weight"][c, :n_kf] = 0
        g["ord_n"][c] = 0
        P = int(g["parent"][c])
        if P < 0:
            res[E_NO_PARENT] += 1
        else:
            kids = np.flatnonzero(g["parent"][:n_kf] == c)
            g["parent"][kids] = P
            res[E_CHILDREN] += len(kids)
        res[E_ERASED] += 1
    for j in sorted(marked):                  # a list's final bytes depend on its row's final values only
        _rebuild(g, j, n_kf)
    res[E_LISTS] = len(marked)
    return res


def _list(g, k, n_kf):
    return g["ord_kf"][k, :min(max(int(g["ord_n"][k]), 0), n_kf)]


def target_list(g, n_kf, cur, n_first=20, n_second=5):
    """-> (the target key frames in order, list entries dropped for an index out of range)"""
    marks, targets, dropped = set(), [], 0
    for a in _list(g, cur, n_kf)[:n_first]:
        a = int(a)
        if not 0 <= a < n_kf:
            dropped += 1
            continue
        if a in marks:
            continue
        marks.add(a)
        targets.append(a)
        for b in _list(g, a, n_kf)[:n_second]:
            b = int(b)
            if not 0 <= b < n_kf:
                dropped += 1
                continue
            if b in marks or b == cur:
                continue
            marks.add(b)
            targets.append(b)
    return targets, dropped


def fuse_targets(g, n_kf, n, bad, slots, stride, valid, cap_points, cur, n_first=20, n_second=5, cap_targets=1 << 30, cap_rows=1 << 30):
    """-> (targets, rows: the FULL lists, d_result)"""
    res = np.zeros(8, np.int32)
    targets, res[T_DROPPED] = target_list(g, n_kf, cur, n_first, n_second)
    seen, rows = set(), []
    for k in targets:
        res[T_BAD] += bad[k] != 0
        for i in range(min(max(int(n[k]), 0), stride)):
            p = int(slots[k, i])
            if not 0 <= p < cap_points:
                continue
            if not valid[p]:
                res[T_INVALID] += 1
            elif p in seen:
                res[T_DUPLICATES] += 1
            else:
                seen.add(p)
                rows.append(p)
    res[T_TARGETS], res[T_ROWS] = len(targets), len(rows)
    res[T_REFUSED] = (1 if len(targets) > cap_targets else 0) | (2 if len(rows) > cap_rows else 0)
    return np.array(targets, np.int32), np.array(rows, np.int32), res


def connected(g, n_kf, kf, include_self, max_n, n_out):
    """-> (d_out [n_out], *d_n_out)"""
    lst = ([kf] if include_self else []) + _list(g, kf, n_kf)[:max(max_n, 0)].tolist()
    lst = lst[:n_out]
    return np.array(lst + [-1] * (n_out - len(lst)), np.int32), len(lst)


# ---- the object form ----------------------------------------------------------------------------------------------------------------
class KeyFrame:
    def __init__(self, slot):
        self.id = slot
        self.connected_kf_weights = {}
        self.ordered_connected_kfs = []
        self.parent = None
        self.children_set = set()
        self.be_first_connection = True
        self.is_bad = False
        self.fuse_target_for_kf = None
        self.map_points = []

    # KeyFrame.cpp:225-291, from kfCounter on (the counting loop is the refresh's d_covis)
    def update_connections(self, kf_counter, first_id, th=CONNECT_TH):
        if not kf_counter:
            return
        max_obs, max_kf, vec_pairs = 0, None, []
        for kf in sorted(kf_counter, key=lambda k: k.id):         # canonical: "the first strictly greater" in ascending slot order
            n = kf_counter[kf]
            if n > max_obs:
                max_obs, max_kf = n, kf
            if n >= th:
                vec_pairs.append((n, kf))
                kf.add_connection(self, n)
        if not vec_pairs:
            vec_pairs.append((max_obs, max_kf))
            max_kf.add_connection(self, max_obs)
        vec_pairs.sort(key=lambda p: (p[0], -p[1].id))             # sort(pair): ties canonical, so that push_front leaves ascending slots
        list_kfs = []
        for n, kf in vec_pairs:
            list_kfs.insert(0, kf)                                 # push_front
        self.connected_kf_weights = dict(kf_counter)
        self.ordered_connected_kfs = list_kfs
        if self.be_first_connection and self.id != first_id:
            self.parent = self.ordered_connected_kfs[0]
            self.parent.add_child(self)
            self.be_first_connection = False

    def add_connection(self, kf, weight):                          # :293-304
        if kf not in self.connected_kf_weights:
            self.connected_kf_weights[kf] = weight
        elif self.connected_kf_weights[kf] != weight:
            self.connected_kf_weights[kf] = weight
        else:
            return
        self.update_best_covisibles()

    def erase_connection(self, kf):                                # :306-317
        if kf in self.connected_kf_weights:
            del self.connected_kf_weights[kf]
            self.update_best_covisibles()
            return True
        return False

    def update_best_covisibles(self):                              # :319-337
        vec_pairs = sorted(((w, kf) for kf, w in self.connected_kf_weights.items()), key=lambda p: (p[0], -p[1].id))
        list_kfs = []
        for w, kf in vec_pairs:
            list_kfs.insert(0, kf)
        self.ordered_connected_kfs = list_kfs

    def get_best_covisible_kfs(self, num):                         # :339-345
        return list(self.ordered_connected_kfs) if len(self.ordered_connected_kfs) < num else self.ordered_connected_kfs[:num]

    def get_weight(self, kf):
        return self.connected_kf_weights.get(kf, 0)

    def add_child(self, kf):
        self.children_set.add(kf)

    def erase_child(self, kf):
        self.children_set.discard(kf)

    def change_parent(self, kf):                                   # :390-395
        self.parent = kf
        kf.add_child(self)

    def set_bad(self):                                             # :402-467, the graph and the tree
        for kf in list(self.connected_kf_weights):
            kf.erase_connection(self)
        self.connected_kf_weights.clear()
        self.ordered_connected_kfs = []
        if self.parent is None:                                    # the reference would dereference null: the tree is left alone
            self.is_bad = True
            return
        parent_candidates = {self.parent}
        while self.children_set:                                   # :428-453, literally
            be_continue, max_weight, child_kf, parent_kf = False, 0, None, None
            for child in sorted(self.children_set, key=lambda k: k.id):
                if child.is_bad:
                    continue
                for cand in sorted(parent_candidates, key=lambda k: k.id):
                    weight = child.get_weight(cand)
                    if weight > max_weight:
                        child_kf, parent_kf, max_weight, be_continue = child, cand, weight, True
            if be_continue:
                child_kf.change_parent(parent_kf)
                parent_kf.add_child(child_kf)
                self.children_set.remove(child_kf)
            else:
                break
        if self.children_set:                                      # :456-460
            for child in self.children_set:
                child.change_parent(self.parent)
        self.parent.erase_child(self)
        self.is_bad = True


def search_in_neighbors(kfs, cur, stamp, n_first=20, n_second=5):
    """LocalMapping.cpp:263-300 on objects whose map_points are table rows (None = no point); -> (target ids, fuse rows)"""
    target_kfs = []
    for kf in cur.get_best_covisible_kfs(n_first):
        if kf.fuse_target_for_kf == stamp:
            continue
        target_kfs.append(kf)
        kf.fuse_target_for_kf = stamp
        for kf2 in kf.get_best_covisible_kfs(n_second):
            if kf2.fuse_target_for_kf == stamp or kf2.id == cur.id:
                continue
            kf2.fuse_target_for_kf = stamp
            target_kfs.append(kf2)
    candidate, fuse = set(), []
    for kf in target_kfs:
        for mp in kf.map_points:
            if mp is None or mp[1] == 0:                           # null, or "kf has bad map-point"
                continue
            if mp[0] in candidate:
                continue
            candidate.add(mp[0])
            fuse.append(mp[0])
    return [kf.id for kf in target_kfs], fuse


def objects_equal_arrays(kfs, g, n_kf, bad):
    """every key frame's map, list and parent; the children as the reference's consumers see them (not bad)"""
    for k, kf in enumerate(kfs):
        row = g["weight"][k, :n_kf]
        assert {o.id: w for o, w in kf.connected_kf_weights.items()} == {int(j): int(row[j]) for j in np.flatnonzero(row)}, k
        assert [o.id for o in kf.ordered_connected_kfs] == g["ord_kf"][k, :g["ord_n"][k]].tolist(), k
        assert bool(kf.is_bad) == bool(bad[k]), k
        if not kf.is_bad:                                          # a bad key frame is nobody's child any more in the reference (:462); here its
            assert (kf.parent.id if kf.parent is not None else -1) == g["parent"][k], k   # d_parent goes on following its parent's erasure
    for k, kf in enumerate(kfs):
        if not kf.is_bad:
            assert {c.id for c in kf.children_set if not c.is_bad} == {int(j) for j in np.flatnonzero(g["parent"][:n_kf] == k) if not bad[j]}, k


# ---- the scenes -----------------------------------------------------------------------------------------------------------------------
SCENES = dict(small=dict(seed=3, n_kf=24, cap_kf=40, n_ops=80, stride=32, cap_points=300),
              mid=dict(seed=4, n_kf=300, cap_kf=304, n_ops=400, stride=256, cap_points=3000))
FIRST_KF = 0
N_CHECKPOINTS = 8


def _covis(n_kf, entries):
    v = np.zeros(n_kf, np.int32)
    for j, c in entries.items():
        v[j] = c
    return v


def _script(n_kf):
    """the operations every scene starts with: the cases the header's quirks are about, by construction"""
    th = CONNECT_TH
    U = lambda K, e: ("update", K, _covis(n_kf, e))  # noqa: E731
    return [
        U(1, {0: 20}), U(0, {1: 20}),                              # the first connection of a non-first key frame, and of first_kf
        U(2, {3: 20, 4: 5}),                                       # list 2 = [3]: partial, row 2 holds the sub-threshold 4
        U(3, {2: 20}),                                             # weight[2][3] is 20 already: list 2 stays partial
        U(3, {2: 21}),                                             # ... and now differs: list 2 gains the sub-threshold entry
        U(3, {4: 17}),                                             # row 3 loses 2, the column entry weight[2][3] survives
        U(5, {0: 7, 1: 7, 2: 3}),                                  # the fallback with a tie for the maximum
        U(6, {}),                                                  # all zero
        U(6, {0: th, 1: th - 1, 2: th + 1}),                       # exactly at and one below the threshold
        U(7, {0: th, 1: th, 2: th, 3: th}),                        # four equal weights in one list
        U(8, {7: 30}), U(9, {8: 30}),                              # a chain 7 <- 8 <- 9 in the tree
        ("erase", np.array([8, 9, 5], np.int32), np.array([3, 3, 0], np.int32)),   # a culled child of a culled key frame; a code other than 3
        U(10, {8: 5, 0: 20, 1: -3, 10: 2}),                        # a count on a bad key frame, a negative one, one on itself
    ]


def make_ops(seed, n_kf, n_ops, **_):
    rng = np.random.RandomState(seed)
    th = CONNECT_TH
    ops = _script(n_kf)
    bad = np.zeros(n_kf, np.uint8)
    bad[[8, 9]] = 1
    values = [th - 1, th - 1, th, th, th + 1, th + 2, 3, 7, 7, 40]
    while len(ops) < n_ops:
        live = np.flatnonzero(bad == 0)
        r = rng.rand()
        if r < 0.08 and len(live) > n_kf // 2:
            rec = rng.choice(live, rng.randint(1, 4), replace=False).astype(np.int32)
            code = rng.choice([3, 3, 3, 0, 1, 2], len(rec)).astype(np.int32)
            ops.append(("erase", rec, code if rng.rand() < 0.8 else None))
            bad[rec[code == 3] if ops[-1][2] is not None else rec] = 1
            continue
        K = int(rng.choice(live))
        covis = np.zeros(n_kf, np.int32)
        others = rng.choice(n_kf, min(n_kf, rng.randint(1, 12)), replace=False)
        pool = [3, 7, 7] if r > 0.9 else values                   # one in ten: below the threshold only, ties likely
        covis[others] = rng.choice(pool, len(others))
        if rng.rand() < 0.1:
            covis[rng.randint(n_kf)] = -rng.randint(1, 9)
        if rng.rand() < 0.9:
            covis[K] = 0
        ops.append(("update", K, covis))
    return ops


def replay(name):
    """-> dict(ops, results [one per op], bad_before [per op], checkpoints {op index: graph after it}, final graph, tags, high water)"""
    cfg = SCENES[name]
    n_kf = cfg["n_kf"]
    ops = make_ops(**cfg)
    rng = np.random.RandomState(cfg["seed"] + 100)
    marks = set(rng.choice(len(ops) - 1, N_CHECKPOINTS, replace=False).tolist()) | {len(ops) - 1}
    g = new_graph(cfg["cap_kf"])
    bad = np.zeros(n_kf, np.uint8)
    kfs = [KeyFrame(k) for k in range(n_kf)]
    out = dict(cfg=cfg, ops=ops, results=[], bad_before=[], checkpoints={}, tags=set(), high=np.zeros(cfg["cap_kf"], np.int32), kfs=kfs)
    stayed_partial = set()
    th = CONNECT_TH
    for t, op in enumerate(ops):
        out["bad_before"].append(bad.copy())
        before = copy_graph(g)
        nnz = lambda gg, j: int((gg["weight"][j, :n_kf] != 0).sum())  # noqa: E731
        if op[0] == "update":
            _, K, covis = op
            c, _, _ = counts(covis, bad, K, n_kf)
            res = update(g, n_kf, bad, covis, K, FIRST_KF)
            kfs[K].update_connections({kfs[j]: int(c[j]) for j in np.flatnonzero(c)}, FIRST_KF)
            tg = out["tags"]
            if (c == th).any():
                tg.add("at_th")
            if (c == th - 1).any():
                tg.add("below_th")
            if res[U_FALLBACK] and (c == c.max()).sum() >= 2:
                tg.add("fallback_tie")
            if res[U_NOTHING] and not covis.any():
                tg.add("all_zero")
            if res[U_BAD]:
                tg.add("count_on_bad")
            if res[U_JUNK] and (covis < 0).any():
                tg.add("negative")
            if res[U_PARENT]:
                tg.add("first_connection")
            if K == FIRST_KF and before["parent"][K] < 0 and res[U_N] > 0 and g["parent"][K] < 0:
                tg.add("first_kf_connection")
            S = g["ord_kf"][K, :g["ord_n"][K]] if not res[U_NOTHING] else []
            for j in S:
                j = int(j)
                partial = before["ord_n"][j] < nnz(before, j)
                if partial and before["weight"][j, K] == c[j] and g["ord_n"][j] == before["ord_n"][j]:
                    tg.add("stays_partial")
                    stayed_partial.add(j)
                if partial and before["weight"][j, K] != c[j] and j in stayed_partial and g["ord_n"][j] == nnz(g, j):
                    w = g["weight"][j, g["ord_kf"][j, :g["ord_n"][j]]]
                    if (w < th).any():
                        tg.add("gains_sub_threshold")
            gone = (before["weight"][K, :n_kf] > 0) & (g["weight"][K, :n_kf] == 0) & (g["weight"][:n_kf, K] > 0)
            if not res[U_NOTHING] and gone.any():
                tg.add("row_gone_column_stays")
        else:
            _, rec, code = op
            res = erase(g, n_kf, rec, code)
            erased = []
            for idx, c in enumerate(rec):
                if code is not None and code[idx] != 3:
                    out["tags"].add("code_not_3")
                    continue
                if before["parent"][c] in erased:
                    out["tags"].add("culled_child_of_culled")
                erased.append(int(c))
                kfs[c].set_bad()
                bad[c] = 1
            if res[E_CHILDREN]:
                out["tags"].add("erase_with_children")
        for k in range(n_kf if "three_equal" not in out["tags"] else 0):
            w = g["weight"][k, g["ord_kf"][k, :g["ord_n"][k]]]
            if len(w) >= 3 and np.bincount(w).max() >= 3:
                out["tags"].add("three_equal")
                break
        out["results"].append(res)
        out["high"] = np.maximum(out["high"], g["ord_n"])
        objects_equal_arrays(kfs, g, n_kf, bad)
        if t in marks:
            out["checkpoints"][t] = copy_graph(g)
    out["graph"], out["bad"] = g, bad
    return out


ALL_TAGS = {"at_th", "below_th", "fallback_tie", "all_zero", "three_equal", "stays_partial", "gains_sub_threshold", "row_gone_column_stays",
            "count_on_bad", "negative", "first_connection", "first_kf_connection", "erase_with_children", "culled_child_of_culled", "code_not_3"}


def fuse_scene(rep):
    """the slot arrays and the current key frame of the fuse calls on a replayed scene's final graph: a bad target, duplicates across
    targets, invalid rows, -1 and junk slots, d_n[k] > stride"""
    cfg, g = rep["cfg"], rep["graph"]
    n_kf, stride, cap = cfg["n_kf"], cfg["stride"], cfg["cap_points"]
    rng = np.random.RandomState(cfg["seed"] + 200)
    live = [k for k in range(n_kf) if not rep["bad"][k]]
    # the current key frame: the live one whose target list is longest
    n = rng.randint(stride // 2, stride + 1, n_kf).astype(np.int32)
    slots = rng.randint(-1, cap, (n_kf, stride)).astype(np.int32)
    slots[rng.rand(n_kf, stride) < 0.3] = -1
    slots[rng.rand(n_kf, stride) < 0.02] = cap + 5
    slots[rng.rand(n_kf, stride) < 0.02] = -7
    valid = (rng.rand(cap) < 0.9).astype(np.uint8)
    bad = rep["bad"].copy()
    cur = max(live, key=lambda k: (len(target_list(g, n_kf, k)[0]), -k))
    targets = target_list(g, n_kf, cur)[0]
    n[targets[0]] = stride + 9                                    # more features than slots
    n[targets[-1]] = 0
    bad[targets[1]] = 1                                           # a bad key frame the graph still lists
    sc = dict(n_kf=n_kf, stride=stride, cap_points=cap, n=n, slots=slots, valid=valid, bad=bad, cur=int(cur))
    return sc


def run_fuse(rep, sc, g=None, **caps):
    return fuse_targets(g or rep["graph"], sc["n_kf"], sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"], sc["cur"], **caps)


def check_scene(rep):
    """the scene holds every case it was built for"""
    missing = ALL_TAGS - rep["tags"]
    assert not missing, missing
    cfg, g = rep["cfg"], rep["graph"]
    n_kf = cfg["n_kf"]
    sc = fuse_scene(rep)
    cur = sc["cur"]
    targets, rows, res = run_fuse(rep, sc)
    assert res[T_TARGETS] >= 4 and res[T_BAD] >= 1 and res[T_INVALID] >= 1 and res[T_DUPLICATES] >= 1 and res[T_REFUSED] == 0
    assert (sc["slots"] == -1).any() and (sc["slots"] > cfg["cap_points"]).any() and (sc["n"] > cfg["stride"]).any()
    second_is_cur = already_marked = False
    marks = set()
    for a in _list(g, cur, n_kf)[:20]:
        if a in marks:
            already_marked = True
            continue
        marks.add(int(a))
        for b in _list(g, a, n_kf)[:5]:
            second_is_cur |= b == cur
            already_marked |= b in marks
            if b != cur:
                marks.add(int(b))
    assert second_is_cur and already_marked
    for caps, bit in ((dict(cap_targets=len(targets) - 1), 1), (dict(cap_rows=len(rows) - 1), 2)):
        r = run_fuse(rep, sc, **caps)[2]
        assert r[T_REFUSED] == bit and r[T_TARGETS] == len(targets) and r[T_ROWS] == len(rows)
    return sc


# ---- :428-460 literally against its simplification ---------------------------------------------------------------------------------
def random_tree(seed):
    """a random tree with random (asymmetric) weights and bad key frames; -> (key frames, the one to set bad, which has a parent)"""
    rng = np.random.RandomState(seed)
    n = rng.randint(3, 14)
    kfs = [KeyFrame(k) for k in range(n)]
    for k in range(1, n):
        kfs[k].parent = kfs[rng.randint(k)]
        kfs[k].parent.add_child(kfs[k])
        kfs[k].be_first_connection = False
    for k in range(n):
        for j in rng.choice(n, rng.randint(0, n), replace=False):
            if j != k:
                kfs[k].connected_kf_weights[kfs[j]] = int(rng.randint(1, 40))
        kfs[k].update_best_covisibles()
        kfs[k].is_bad = k > 0 and rng.rand() < 0.2
    with_children = [k for k in range(1, n) if kfs[k].children_set]
    return kfs, kfs[with_children[rng.randint(len(with_children))] if with_children else rng.randint(1, n)]
