"""The covisibility graph on the MI355X (include/orbm.h, "The covisibility graph on the device") against the array model of
tests/graph_model.py, byte for byte: integers only, so no tolerance."""
import numpy as np
import pytest

import graph_model as gm
from test_observations_gpu import GUARD, _guards_intact, _padded  # noqa: F401 (GUARD: the padding _padded puts around every array)
from test_triangulation_gpu import _stream, _up

pytestmark = pytest.mark.gpu

_cache = {}
OUTSIDE = dict(weight=777, ord_n=55, parent=66)     # what rows and columns at and past n_kf hold: they must stay
FILLS = dict(weight=-11, ord_kf=-12, ord_n=-13, parent=-14)


def replayed(name):
    """a scene replayed by the models once, shared, never changed"""
    if name not in _cache:
        _cache[name] = gm.replay(name)
    return _cache[name]


def _device_graph(torch, dev, g, n_kf):
    """the model's graph in padded device arrays, rows and columns past n_kf filled with OUTSIDE -> (CovisGraph, pads)"""
    from monoorbslam3_amd.matcher import CovisGraph
    host = {k: g[k].copy() for k in ("weight", "ord_kf", "ord_n", "parent")}
    host["weight"][n_kf:, :], host["weight"][:, n_kf:] = OUTSIDE["weight"], OUTSIDE["weight"]
    host["ord_n"][n_kf:], host["parent"][n_kf:] = OUTSIDE["ord_n"], OUTSIDE["parent"]
    pads = {k: _padded(torch, dev, v, FILLS[k]) for k, v in host.items()}
    return CovisGraph.make(*(pads[k][1] for k in ("weight", "ord_kf", "ord_n", "parent"))), pads


def _download(pads, cap):
    d = {k: v[1].cpu().numpy() for k, v in pads.items()}
    return dict(weight=d["weight"].reshape(cap, cap), ord_kf=d["ord_kf"].reshape(cap, cap), ord_n=d["ord_n"], parent=d["parent"])


def _equals_model(got, want, n_kf):
    """the graph below n_kf equals the model's, and nothing else was written.  Both start from the same d_ord_kf and the model writes, per
    call, exactly the entries below the length that call leaves: so the WHOLE of d_ord_kf must equal the model's -- the stale entries of
    a list that shrank, the entries no call ever reached and the rows at and past n_kf included."""
    assert got["weight"][:n_kf, :n_kf].tobytes() == want["weight"][:n_kf, :n_kf].tobytes()
    assert got["ord_n"][:n_kf].tobytes() == want["ord_n"][:n_kf].tobytes() and got["parent"][:n_kf].tobytes() == want["parent"][:n_kf].tobytes()
    assert (got["weight"][n_kf:, :] == OUTSIDE["weight"]).all() and (got["weight"][:, n_kf:] == OUTSIDE["weight"]).all()
    assert (got["ord_n"][n_kf:] == OUTSIDE["ord_n"]).all() and (got["parent"][n_kf:] == OUTSIDE["parent"]).all()
    assert got["ord_kf"].tobytes() == want["ord_kf"].tobytes()


def _replay_on_device(torch, dev, rep, stream_kind, check):
    """the scene's operations one after another on one stream.  With check = True the model runs beside them and there is a wait after
    EVERY operation: d_ord_n and the whole of d_ord_kf equal the model's, so no call wrote a list entry at or past the length it left
    (a write there that a later call covered would not show at a checkpoint); at the checkpoints the whole graph and every d_result so
    far.  With check = False nothing waits before the end.  -> the final arrays"""
    from monoorbslam3_amd.matcher import ORBMatcher
    cfg, ops = rep["cfg"], rep["ops"]
    n_kf, cap = cfg["n_kf"], cfg["cap_kf"]
    start = gm.new_graph(cap)
    graph, pads = _device_graph(torch, dev, start, n_kf)
    results = _padded(torch, dev, np.full(8 * len(ops), 31, np.int32), -15)
    work = _padded(torch, dev, np.full(n_kf, 32, np.int32), -16)
    m = ORBMatcher()
    st = _stream(torch, dev, stream_kind)
    model = gm.new_graph(cap)
    for t, op in enumerate(ops):
        d = dict(work=work[1], result=results[1][8 * t:8 * t + 8])
        if op[0] == "update":
            d.update(bad=_up(torch, dev, rep["bad_before"][t]), covis=_up(torch, dev, op[2]))
            m.UpdateConnectionsDevice(graph, d, n_kf, op[1], first_kf=gm.FIRST_KF, stream=st)
        else:
            if op[2] is not None:
                d["code"] = _up(torch, dev, op[2])
            m.EraseConnectionsDevice(graph, d, n_kf, op[1], stream=st)
        if check:
            if op[0] == "update":
                gm.update(model, n_kf, rep["bad_before"][t], op[2], op[1], gm.FIRST_KF)
            else:
                gm.erase(model, n_kf, op[1], op[2])
            torch.cuda.synchronize()
            assert pads["ord_n"][1].cpu().numpy()[:n_kf].tobytes() == model["ord_n"][:n_kf].tobytes(), t
            assert pads["ord_kf"][1].cpu().numpy().tobytes() == model["ord_kf"].tobytes(), t
            if t in rep["checkpoints"]:
                _equals_model(_download(pads, cap), rep["checkpoints"][t], n_kf)
                res = results[1].cpu().numpy().reshape(-1, 8)[:t + 1]
                assert res.tobytes() == np.stack(rep["results"][:t + 1]).tobytes(), t
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k, fill in FILLS.items():
        assert _guards_intact(pads[k][0], fill), k
    assert _guards_intact(results[0], -15) and _guards_intact(work[0], -16)
    return {k: v[1].cpu().numpy() for k, v in pads.items()}, results[1].cpu().numpy()


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("name", sorted(gm.SCENES))
def test_a_replayed_scene_equals_the_model(name, stream_kind):
    """80 operations on 24 key frames in a pitch of 40, 400 on 300: updates and erases from an empty graph, with every case
    tests/graph_model.py's check_scene lists.  After the last operation and at 8 seeded checkpoints d_weight, d_ord_n, d_parent, every
    list and every d_result so far equal the model's; after EVERY operation the whole of d_ord_kf does, so each call left the entries at
    and past the length it set as they were; rows and columns at and past n_kf are as passed; guards intact; a second run, which waits
    only at its end, gives the same bytes."""
    import torch
    dev = torch.device("cuda", 0)
    rep = replayed(name)
    first, res1 = _replay_on_device(torch, dev, rep, stream_kind, True)
    print(name, "d_result sums", np.stack(rep["results"]).sum(0).tolist())
    second, res2 = _replay_on_device(torch, dev, rep, stream_kind, False)
    assert res1.tobytes() == res2.tobytes()
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("n_kf", [1, 2, 63, 64, 65, 1025, 4096])
def test_one_update_at_the_sizes_where_the_sort_changes(n_kf, stream_kind):
    """n_kf of 1, 2, around the wave, past one pass of the workgroup and the full 4096 (= cap_kf): a dense graph of weights from
    {0, 14, 15, 16} -- ties dominate --, every list empty, then ONE update with counts from the same set: list K and every rebuilt
    neighbour list (at the full size at least 64 of over 1000 entries each) equal the model's, nothing else is written, and a second
    run from the same start gives the same bytes"""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    key = ("size", n_kf)
    if key not in _cache:
        rng = np.random.RandomState(n_kf)
        cap = n_kf if n_kf == 4096 else n_kf + 3
        g = gm.new_graph(cap)
        g["weight"][:n_kf, :n_kf] = rng.choice([0, 14, 15, 16], (n_kf, n_kf)).astype(np.int32)
        g["weight"][np.arange(n_kf), np.arange(n_kf)] = 0
        K = n_kf // 2
        covis = np.zeros(n_kf, np.int32)
        some = rng.choice(n_kf, min(n_kf, 300), replace=False)
        covis[some] = rng.choice([0, 14, 15, 16], len(some))
        covis[K] = 0
        bad = np.zeros(n_kf, np.uint8)
        want = gm.copy_graph(g)
        res = gm.update(want, n_kf, bad, covis, K, -1)
        _cache[key] = (cap, g, K, covis, bad, want, res)
    cap, g, K, covis, bad, want, res = _cache[key]
    print("n_kf", n_kf, "model d_result", res.tolist())
    if n_kf == 4096:
        assert res[gm.U_REBUILT] >= 64 and (want["ord_n"] > 1000).sum() >= 64
    d = dict(bad=_up(torch, dev, bad), covis=_up(torch, dev, covis))
    runs = []
    for _ in range(2):                                                        # the second run: the same bytes, whatever the workgroups' order
        graph, pads = _device_graph(torch, dev, g, n_kf)
        result, work = _padded(torch, dev, np.full(8, 31, np.int32), -15), _padded(torch, dev, np.full(n_kf, 32, np.int32), -16)
        st = _stream(torch, dev, stream_kind)
        ORBMatcher().UpdateConnectionsDevice(graph, dict(d, work=work[1], result=result[1]), n_kf, K, stream=st)
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        for k, fill in FILLS.items():
            assert _guards_intact(pads[k][0], fill), k
        assert _guards_intact(result[0], -15) and _guards_intact(work[0], -16)
        runs.append(dict(_download(pads, cap), result=result[1].cpu().numpy()))
    assert runs[0]["result"].tobytes() == res.tobytes()
    _equals_model(runs[0], want, n_kf)
    for k in runs[0]:
        assert runs[1][k].tobytes() == runs[0][k].tobytes(), k


def _fuse(torch, dev, m, graph, sc, t, cap_targets, cap_rows, stream_kind):
    out = dict(targets=_padded(torch, dev, np.full(cap_targets, -21, np.int32), -22), rows=_padded(torch, dev, np.full(cap_rows, -23, np.int32), -24),
               result=_padded(torch, dev, np.full(8, 31, np.int32), -25), work=_padded(torch, dev, np.full(sc["cap_points"], 32, np.int32), -26))
    st = _stream(torch, dev, stream_kind)
    m.FuseTargetsDevice(graph, dict(t, **{k: v[1] for k, v in out.items()}), sc["n_kf"], sc["stride"], sc["cap_points"], sc["cur"], cap_targets,
                        cap_rows, stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k, fill in (("targets", -22), ("rows", -24), ("result", -25), ("work", -26)):
        assert _guards_intact(out[k][0], fill), k
    return {k: v[1].cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("name", sorted(gm.SCENES))
def test_the_fuse_targets_and_the_connected_key_frames_equal_the_model(name, stream_kind):
    """on a replayed scene's final graph: the targets (a second neighbour that is the current key frame, one already marked, a bad one)
    and the de-duplicated rows (duplicates across targets, invalid rows, -1 and junk slots, d_n > stride) in order, and d_result; the
    same bytes a second time; each capacity one too small: the refusal bit, the full counts, nothing at or past the capacity; a forged
    list (-5 and n_kf among the entries): dropped and counted; then getConnectedKFs / getBestCovisibleKFs with and without the key
    frame itself, cut and filled"""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    rep = replayed(name)
    sc = gm.fuse_scene(rep)
    n_kf, cap = sc["n_kf"], rep["cfg"]["cap_kf"]
    m = ORBMatcher()
    graph, pads = _device_graph(torch, dev, rep["graph"], n_kf)
    t = {k: _up(torch, dev, sc[k]) for k in ("n", "bad", "slots", "valid")}
    targets, rows, res = gm.run_fuse(rep, sc)
    runs = [_fuse(torch, dev, m, graph, sc, t, len(targets) + 3, len(rows) + 3, stream_kind) for _ in range(2)]
    got = runs[0]
    print(name, "device d_result", got["result"].tolist(), "model", res.tolist())
    assert got["result"].tobytes() == res.tobytes()
    assert got["targets"][:len(targets)].tobytes() == targets.tobytes() and (got["targets"][len(targets):] == -21).all()
    assert got["rows"][:len(rows)].tobytes() == rows.tobytes() and (got["rows"][len(rows):] == -23).all()
    for k in ("targets", "rows", "result"):
        assert runs[1][k].tobytes() == got[k].tobytes(), k
    for cut_t, cut_r, bit in ((1, 0, 1), (0, 1, 2)):
        r = _fuse(torch, dev, m, graph, sc, t, len(targets) - cut_t, len(rows) - cut_r, stream_kind)
        want = gm.run_fuse(rep, sc, cap_targets=len(targets) - cut_t, cap_rows=len(rows) - cut_r)[2]
        assert want[gm.T_REFUSED] == bit and r["result"].tobytes() == want.tobytes()
    forged = gm.copy_graph(rep["graph"])
    forged["ord_kf"][sc["cur"], 1], forged["ord_kf"][targets[0], 0] = -5, n_kf
    f_targets, f_rows, f_res = gm.run_fuse(rep, sc, g=forged)
    assert f_res[gm.T_DROPPED] == 2
    f_graph, f_pads = _device_graph(torch, dev, forged, n_kf)
    r = _fuse(torch, dev, m, f_graph, sc, t, len(f_targets), len(f_rows), stream_kind)
    assert r["result"].tobytes() == f_res.tobytes() and r["targets"].tobytes() == f_targets.tobytes() and r["rows"].tobytes() == f_rows.tobytes()
    # ---- getConnectedKFs / getBestCovisibleKFs
    for g_model, g_dev, kf, include_self, max_n, n_out in ((rep["graph"], graph, sc["cur"], True, None, n_kf + 1), (rep["graph"], graph, sc["cur"], False, 3, 7),
                                                         (rep["graph"], graph, int(targets[0]), True, 20, 4), (forged, f_graph, sc["cur"], True, None, 50),
                                                         (rep["graph"], graph, sc["cur"], True, 0, 0)):
        out = dict(out=_padded(torch, dev, np.full(n_out, -31, np.int32), -32), n_out=_padded(torch, dev, np.full(1, -33, np.int32), -34))
        st = _stream(torch, dev, stream_kind)
        m.ConnectedKeyFramesDevice(g_dev, {k: v[1] for k, v in out.items()}, n_kf, kf, include_self, max_n, stream=st)
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        want, n = gm.connected(g_model, n_kf, kf, include_self, n_kf if max_n is None else max_n, n_out)
        assert out["out"][1].cpu().numpy().tobytes() == want.tobytes() and int(out["n_out"][1].cpu()[0]) == n
        assert _guards_intact(out["out"][0], -32) and _guards_intact(out["n_out"][0], -34)
    for k, fill in FILLS.items():                                             # the graph was only read
        assert _guards_intact(pads[k][0], fill), k
    _equals_model(_download(pads, cap), rep["graph"], n_kf)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_the_erase_behind_a_real_cull(stream_kind):
    """orbm_cull_keyframes_device -> orbm_erase_connections_device on one stream with d_code passed straight through and ONE wait at the
    end, on the culling's own scene (12 key frames x 256 slots, two of them culled) and a graph in which every key frame is the child of
    the one before it: the graph, the tree and d_result equal the model fed the culling model's codes; a second run gives the same bytes"""
    import torch
    import observations_model as om
    from monoorbslam3_amd.matcher import KfTable, ORBMatcher
    from test_observations_gpu import _cull_scene
    dev = torch.device("cuda", 0)
    sc, off, kf, kp = _cull_scene(21)
    culled = om.cull(sc, off, kf, kp)
    n_kf, nr = len(sc["n"]), len(sc["recent"])
    assert (culled["code"] == 3).sum() >= 1 and set(culled["code"].tolist()) - {3} and n_kf >= 8
    g = gm.new_graph(n_kf + 2)
    for k in range(1, n_kf):
        covis = np.zeros(n_kf, np.int32)
        covis[(k * 5) % n_kf], covis[(k * 7) % n_kf] = 20, 9
        covis[k - 1], covis[k] = 30, 0
        gm.update(g, n_kf, np.zeros(n_kf, np.uint8), covis, k, 0)
    want = gm.copy_graph(g)
    res = gm.erase(want, n_kf, sc["recent"], culled["code"])
    print("model d_result", res.tolist(), "codes", culled["code"].tolist())
    assert res[gm.E_ERASED] == (culled["code"] == 3).sum() and res[gm.E_CONNECTIONS] >= 2 and res[gm.E_CHILDREN] >= 1 and res[gm.E_LISTS] >= 2
    zi = lambda n: torch.zeros(n, dtype=torch.int32, device=dev)  # noqa: E731
    z = torch.zeros(1, dtype=torch.float64, device=dev)
    m = ORBMatcher()
    runs = []
    for _ in range(2):                                                        # the second run: the same bytes
        graph, pads = _device_graph(torch, dev, g, n_kf)
        d = {k: _up(torch, dev, sc[k]) for k in ("bad", "slots", "valid", "ref_kf")}
        d.update(obs_off=_up(torch, dev, off), obs_kf=_up(torch, dev, kf), obs_kp=_up(torch, dev, kp), code=zi(nr), num_mp=zi(nr), num_redundant=zi(nr),
                 result=zi(8))
        table = KfTable.make(z, z, d["bad"], [_up(torch, dev, k) for k in sc["kps"]], torch.zeros(n_kf, dtype=torch.int64, device=dev),
                             _up(torch, dev, sc["n"]))
        result, work = _padded(torch, dev, np.full(8, 31, np.int32), -15), _padded(torch, dev, np.full(n_kf, 32, np.int32), -16)
        st = _stream(torch, dev, stream_kind)
        m.CullKeyFramesDevice(table, d, sc["stride"], sc["cap_points"], len(kf), sc["recent"], sc["timestamps"], first_kf=sc["first_kf"], stream=st)
        m.EraseConnectionsDevice(graph, dict(code=d["code"], work=work[1], result=result[1]), n_kf, sc["recent"], stream=st)
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        for k, fill in FILLS.items():
            assert _guards_intact(pads[k][0], fill), k
        assert _guards_intact(result[0], -15) and _guards_intact(work[0], -16)
        runs.append(dict(_download(pads, n_kf + 2), result=result[1].cpu().numpy(), code=d["code"].cpu().numpy(), bad=d["bad"].cpu().numpy()))
    got = runs[0]
    assert got["code"].tobytes() == culled["code"].tobytes() and got["bad"].tobytes() == np.ascontiguousarray(culled["bad"]).tobytes()
    assert got["result"].tobytes() == res.tobytes()
    _equals_model(got, want, n_kf)
    for k in got:
        assert runs[1][k].tobytes() == got[k].tobytes(), k


CHAIN_SLACK = 3                          # capacity beyond the model's counts


def _chain_scene(shared, connect_th):
    """the mid scene's final graph and its fuse scene's slot arrays (n, bad, slots, valid, cur), with what the other links read: poses,
    orbx_kp records and descriptors of every key frame, positions, reference key frames and a garbage table for the refresh to write.
    The models chained: observations_model.build -> refresh_model.refresh (d_sel = cur's slots, kf_self = cur) -> graph_model.update
    on the refresh's counts -> fuse_targets -> connected (include_self, all, n_out = n_kf + 1) -> local_ba_model.problem with that
    array as d_local.  With shared > 0 that many key frames first get 8 to 40 of their slots rewritten to rows the current key frame
    observes, so that the refresh's counts cross CONNECT_TH for many of them.  Computed once per case, shared, never changed."""
    key = ("chain", shared, connect_th)
    if key in _cache:
        return _cache[key]
    import local_ba_model as lm
    import observations_model as om
    import refresh_model as rm
    from projection_model import KP_DTYPE, N_LEVELS, SCALE_FACTORS
    rep = replayed("mid")
    sc = gm.fuse_scene(rep)
    n_kf, stride, cap, cur = sc["n_kf"], sc["stride"], sc["cap_points"], sc["cur"]
    if ("chain_map", shared) not in _cache:
        rng = np.random.RandomState(500)
        if shared:
            sc = dict(sc, slots=sc["slots"].copy())
            mine = sc["slots"][cur, :min(int(sc["n"][cur]), stride)]
            mine = np.unique(mine[(mine >= 0) & (mine < cap)])
            mine = mine[sc["valid"][mine] != 0]
            r2 = np.random.RandomState(501)
            others = r2.choice(np.delete(np.arange(n_kf), cur), shared, replace=False)
            for j in others[sc["n"][others] >= 64]:                           # on top of the five or six rows a key frame shares anyway
                c = int(r2.choice([8, 9, 9, 10, 10, 11, 12, 14, 25, 40]))
                sc["slots"][j, r2.choice(min(int(sc["n"][j]), stride), c, replace=False)] = r2.choice(mine, c, replace=False)
        pose_R = np.stack([rm._rodrigues(rng.uniform(-0.05, 0.05, 3) + 1e-3).reshape(9) for _ in range(n_kf)]).astype(np.float32).astype(np.float64)
        pose_t = rng.uniform(-0.4, 0.4, (n_kf, 3)).astype(np.float32).astype(np.float64)
        points = np.stack([rng.uniform(-3, 3, cap), rng.uniform(-2, 2, cap), rng.uniform(5, 10, cap)], 1).astype(np.float32)
        kps, kf_desc = [], []
        for k in range(n_kf):                                                 # records for every feature, where d_n > stride too
            kp = np.zeros(stride + 16, KP_DTYPE)
            kp["x"], kp["y"] = rng.uniform(0, 752, len(kp)), rng.uniform(0, 480, len(kp))
            kp["octave"], kp["class_id"] = rng.randint(0, N_LEVELS, len(kp)), -1
            kp["size"] = np.float32(31) * SCALE_FACTORS[kp["octave"]]
            kps.append(kp)
            kf_desc.append(rng.randint(0, 256, (len(kp), 32)).astype(np.uint8))
        table = dict(normals=rng.uniform(-1, 1, (cap, 3)).astype(np.float32), min_dist=rng.uniform(1, 2, cap).astype(np.float32),
                     max_dist=rng.uniform(20, 30, cap).astype(np.float32), desc=rng.randint(0, 256, (cap, 32)).astype(np.uint8))
        cap_obs = int(om.build(sc["n"], sc["bad"], sc["slots"], stride, sc["valid"], cap, 1 << 30)[3][om.NOBS]) + 40
        off, okf, okp, bres = om.build(sc["n"], sc["bad"], sc["slots"], stride, sc["valid"], cap, cap_obs)
        ref_kf = np.array([okf[off[p]] if off[p + 1] > off[p] else 0 for p in range(cap)], np.int32)
        n_sel = min(int(sc["n"][cur]), stride)
        rs = dict(n=sc["n"], bad=sc["bad"], pose_R=pose_R, pose_t=pose_t, kps=kps, kf_desc=kf_desc, points=points, valid=sc["valid"], obs_off=off,
                  obs_kf=okf, obs_kp=okp, ref_kf=ref_kf, **table)
        fresh = rm.refresh(rs, sc["slots"][cur, :n_sel], cap, kf_self=cur)
        _cache[("chain_map", shared)] = dict(sc, pose_R=pose_R, pose_t=pose_t, points=points, kps=kps, kf_desc=kf_desc, table=table, cap_obs=cap_obs,
                                   csr=(off, okf, okp), build=bres, ref_kf=ref_kf, n_sel=n_sel, fresh=fresh, first_kf=gm.FIRST_KF)
    cs = dict(_cache[("chain_map", shared)])
    g = gm.copy_graph(rep["graph"])
    cs["update"] = gm.update(g, n_kf, cs["bad"], cs["fresh"]["covis"], cur, gm.FIRST_KF, connect_th)
    cs["targets"], cs["rows"], cs["fuse"] = gm.fuse_targets(g, n_kf, cs["n"], cs["bad"], cs["slots"], stride, cs["valid"], cap, cur)
    cs["local"], cs["n_local"] = gm.connected(g, n_kf, cur, True, n_kf, n_kf + 1)
    cs["problem"] = lm.problem(dict(cs, local=cs["local"]), cs["csr"])
    cs.update(graph=g, start=rep["graph"], cap_kf=rep["cfg"]["cap_kf"], connect_th=connect_th)
    _cache[key] = cs
    return cs


def _chain_on_device(torch, dev, cs, stream_kind):
    """the six calls on one stream, every output in padded arrays, ONE wait at the end -> everything the calls wrote, as numpy arrays"""
    import local_ba_model as lm
    import refresh_model as rm
    from monoorbslam3_amd import matcher
    from test_local_ba_gpu import OUT_TYPES, PER, WIDTH
    n_kf, stride, cap, cur, cap_obs = cs["n_kf"], cs["stride"], cs["cap_points"], cs["cur"], cs["cap_obs"]
    pres = cs["problem"]["result"]
    caps = dict(poses=int(pres[lm.P_POSES]) + CHAIN_SLACK, points=int(pres[lm.P_POINTS]) + CHAIN_SLACK, edges=int(pres[lm.P_EDGES]) + CHAIN_SLACK)
    sizes = {"poses": caps["poses"], "points": caps["points"], "points+1": caps["points"] + 1, "edges": caps["edges"]}
    graph, gpads = _device_graph(torch, dev, cs["start"], n_kf)
    t = {k: _up(torch, dev, cs[k]) for k in ("n", "bad", "slots", "valid", "points", "ref_kf", "pose_R", "pose_t")}
    t["kps"], t["kf_desc"] = [_up(torch, dev, k) for k in cs["kps"]], [_up(torch, dev, x) for x in cs["kf_desc"]]
    kft = matcher.KfTable.make(t["pose_R"], t["pose_t"], t["bad"], t["kps"], t["kf_desc"], t["n"])
    pads = {k: _padded(torch, dev, v, 41) for k, v in cs["table"].items()}
    ints = dict(obs_off=cap + 1, obs_kf=cap_obs, obs_kp=cap_obs, covis=n_kf, work_kf=n_kf, work_rows=cap, work=cap + n_kf,
                targets=len(cs["targets"]) + CHAIN_SLACK, rows=len(cs["rows"]) + CHAIN_SLACK, local=n_kf + 1, n_local=1, r_build=8, r_refresh=8,
                r_update=8, r_fuse=8, result=16)
    pads.update({k: _padded(torch, dev, np.zeros(n, np.int32) if k in ("obs_kf", "obs_kp") else np.full(n, -51, np.int32), 41) for k, n in ints.items()})
    for k, dt in OUT_TYPES.items():
        pads[k] = _padded(torch, dev, np.full(sizes[PER.get(k, "edges")] * WIDTH.get(k, 1), 91 if dt == np.uint8 else -91, dt), 41)
    d = dict(t, **{k: v[1] for k, v in pads.items()})
    m = matcher.ORBMatcher()
    st = _stream(torch, dev, stream_kind)
    m.BuildObservationsDevice(dict(d, result=d["r_build"]), n_kf, stride, cap, cap_obs, stream=st)
    m.RefreshPointsDevice(kft, dict(d, sel=t["slots"][cur], result=d["r_refresh"]), cs["n_sel"], cap, cap_obs, float(rm.MAX_SCALE_FACTOR),
                          kf_self=cur, stream=st)
    m.UpdateConnectionsDevice(graph, dict(d, work=d["work_kf"], result=d["r_update"]), n_kf, cur, first_kf=cs["first_kf"],
                              connect_th=cs["connect_th"], stream=st)
    m.FuseTargetsDevice(graph, dict(d, work=d["work_rows"], result=d["r_fuse"]), n_kf, stride, cap, cur, ints["targets"], ints["rows"], stream=st)
    m.ConnectedKeyFramesDevice(graph, dict(out=d["local"], n_out=d["n_local"]), n_kf, cur, include_self=True, stream=st)
    m.LocalBaProblemDevice(kft, d, stride, cap, cap_obs, n_kf + 1, cs["first_kf"], caps["poses"], caps["points"], caps["edges"], stream=st)
    torch.cuda.synchronize()                                                  # the first and only wait of the chain
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k in pads:
        assert _guards_intact(pads[k][0], 41), k
    for k, fill in FILLS.items():
        assert _guards_intact(gpads[k][0], fill), k
    out = {k: v[1].cpu().numpy() for k, v in pads.items()}
    out["graph"] = _download(gpads, cs["cap_kf"])
    out["inputs"] = {k: t[k].cpu().numpy() for k in ("n", "bad", "slots", "valid", "points", "ref_kf")}
    return out


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("shared,connect_th", [(0, gm.CONNECT_TH), (0, 8), (60, gm.CONNECT_TH)])
def test_the_chain_from_the_observations_to_the_local_ba_with_one_wait(shared, connect_th, stream_kind):
    """orbm_build_observations_device -> orbm_refresh_points_device (d_sel = the current key frame's slots, d_covis, kf_self = cur) ->
    orbm_update_connections_device on that d_covis -> orbm_fuse_targets_device -> orbm_connected_keyframes_device (include_self, all,
    n_out = n_kf + 1) -> orbm_local_ba_problem_device with d_local = that d_out, its -1 fill included, and n_local = n_out: one stream,
    no read-back between the calls, ONE wait at the end, on the mid scene's graph and slot arrays (300 key frames x 256 slots, 3000
    rows, 30000 observations).  Everything the calls leave equals observations_model, refresh_model, graph_model and local_ba_model
    chained the same way, byte for byte (the refresh's normals by value); a second run gives the same bytes.
    The scene's counts reach CONNECT_TH = 15 once: with it the current key frame gets ONE connection, exactly at the threshold, and
    d_local is two key frames.  With connect_th = 8 -- the argument exists for this -- the same counts give 70 connections with long
    runs of equal weights, 82 targets, 2593 rows and a local BA of 71 key frames, 2582 points and 28736 edges.  The third case keeps
    CONNECT_TH and rewrites 8 to 40 slots of 60 key frames to rows the current key frame observes: its counts then straddle the shipped
    threshold, at least 20 key frames reach it, and counts exactly at it and one below it are among them."""
    import torch
    import local_ba_model as lm
    from test_local_ba_gpu import OUT_TYPES, PER, WIDTH
    dev = torch.device("cuda", 0)
    cs = _chain_scene(shared, connect_th)
    n_kf, fresh, prob = cs["n_kf"], cs["fresh"], cs["problem"]
    print("shared %d connect_th %d: build %s refresh %s update %s fuse %s n_local %d problem %s" % (
        shared, connect_th, cs["build"].tolist(), fresh["result"].tolist(), cs["update"].tolist(), cs["fuse"].tolist(), cs["n_local"], prob["result"].tolist()))
    assert cs["n"][0] >= 1                                                    # the CSR arrays' unused tail (0, 0) names a feature that exists
    assert cs["build"][1] == 0 and fresh["result"][0] >= 100 and fresh["covis"].max() >= gm.CONNECT_TH and cs["update"][gm.U_NOTHING] == 0
    assert (cs["update"][gm.U_N] >= 20 if shared else cs["update"][gm.U_N] == (1 if connect_th == gm.CONNECT_TH else 70))
    assert not shared or ((fresh["covis"] == gm.CONNECT_TH).any() and (fresh["covis"] == gm.CONNECT_TH - 1).any())
    assert cs["fuse"][gm.T_REFUSED] == 0 and cs["fuse"][gm.T_ROWS] >= 500
    assert cs["n_local"] == cs["update"][gm.U_N] + 1 and prob["result"][lm.P_REFUSED] == 0
    assert prob["result"][lm.P_LOCAL_DROPPED] == n_kf + 1 - cs["n_local"] and prob["result"][lm.P_LOCAL] + prob["result"][lm.P_LOCAL_BAD] == cs["n_local"]
    runs = [_chain_on_device(torch, dev, cs, stream_kind) for _ in range(2)]
    got = runs[0]
    off, okf, okp = cs["csr"]
    assert got["r_build"].tobytes() == cs["build"].tobytes() and got["obs_off"].tobytes() == off.tobytes()
    assert got["obs_kf"][:len(okf)].tobytes() == okf.tobytes() and got["obs_kp"][:len(okp)].tobytes() == okp.tobytes()
    assert np.array_equal(got["r_refresh"], fresh["result"]) and got["covis"].tobytes() == fresh["covis"].tobytes()
    assert np.array_equal(got["normals"].reshape(-1, 3), fresh["normals"])    # by value: -0 equals +0
    for key in ("min_dist", "max_dist"):
        assert got[key].view(np.uint32).tobytes() == fresh[key].view(np.uint32).tobytes(), key
    assert got["desc"].tobytes() == fresh["desc"].tobytes()
    assert got["r_update"].tobytes() == cs["update"].tobytes()
    _equals_model(got["graph"], cs["graph"], n_kf)
    assert got["r_fuse"].tobytes() == cs["fuse"].tobytes()
    assert got["targets"][:len(cs["targets"])].tobytes() == cs["targets"].tobytes() and (got["targets"][len(cs["targets"]):] == -51).all()
    assert got["rows"][:len(cs["rows"])].tobytes() == cs["rows"].tobytes() and (got["rows"][len(cs["rows"]):] == -51).all()
    assert got["local"].tobytes() == cs["local"].tobytes() and int(got["n_local"][0]) == cs["n_local"] and (got["local"][cs["n_local"]:] == -1).all()
    assert got["result"].tobytes() == prob["result"].tobytes()
    res = prob["result"]
    counts = {"poses": res[lm.P_POSES], "points": res[lm.P_POINTS], "points+1": res[lm.P_POINTS] + 1, "edges": res[lm.P_EDGES]}
    for k in OUT_TYPES:
        n = counts[PER.get(k, "edges")] * WIDTH.get(k, 1)
        assert got[k][:n].tobytes() == np.ascontiguousarray(prob[k]).reshape(-1).tobytes(), k
    for k, v in got["inputs"].items():                                        # the map itself was only read
        assert v.tobytes() == np.ascontiguousarray(cs[k]).tobytes(), k
    for k in got:
        if k == "graph":
            for kk in got[k]:
                assert runs[1][k][kk].tobytes() == got[k][kk].tobytes(), kk
        elif k != "inputs" and not k.startswith("work"):                      # a work array's contents after a call are unspecified
            assert runs[1][k].tobytes() == got[k].tobytes(), k
