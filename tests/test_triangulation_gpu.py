"""orbm_triangulate_matches_device / orbm_triangulate_matches on the MI355X (include/orbm.h, "New map points triangulated on the
device") against the numpy model of tests/triangulation_model.py, then chained behind orbm_search_for_triangulation_device and
ahead of orbm_project_fuse_device the way LocalMapping::createNewMapPoints / searchInNeighbors use them."""
import numpy as np
import pytest

import projection_model as pm
import triangulation_model as tm
from monoorbslam3_amd import synth
from test_triangulation_cpu import CLOUDS

pytestmark = pytest.mark.gpu

EXCLUDED_CAP = 0.005
# |cosParallax - 0.99998| below which the device may decide the parallax gate differently from float64: a dot product of unit
# vectors carries a few float ulps (6e-8 each) and a point 1e-4 of its distance off its ray turns the ray by 1e-4 rad, which at
# the limit's angle (6.3e-3 rad) moves the cosine by 6e-7.  The issue's +-1e-4 relative move of 0.99998 re-decides EVERY parallax
# rejection (the moved limit exceeds 1), so the comparison below uses this narrower band for that gate and the issue's for the cap.
NEAR_COS = 4e-6
TABLE_KEYS = ("points", "valid", "normals", "min_dist", "max_dist", "desc", "obs")
STATE_KEYS = TABLE_KEYS + ("n_points", "mp1", "mp2", "has_mp1", "has_mp2")


def _stream(torch, dev, kind):
    if kind == "null":
        return None
    chain = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    torch.cuda.set_stream(chain)
    assert chain.cuda_stream != 0
    return chain.cuda_stream


def _up(torch, dev, a):
    a = np.ascontiguousarray(a)
    if a.dtype.fields is not None:
        a = np.frombuffer(a.tobytes(), np.uint8).copy()
    return torch.from_numpy(a).to(dev)


def _host_state(cloud, cap, seed=1):
    """the table and the key frames' state as a caller holds them, every array GARBAGE where the call has to write"""
    rng = np.random.RandomState(seed)
    n1, n2 = cloud["n1"], cloud["n2"]
    return dict(n_points=np.array([cloud["n_points"]], np.int32), points=rng.uniform(-9, 9, (cap, 3)).astype(np.float32),
                valid=rng.randint(2, 200, cap).astype(np.uint8), normals=rng.uniform(-9, 9, (cap, 3)).astype(np.float32),
                min_dist=rng.uniform(50, 60, cap).astype(np.float32), max_dist=rng.uniform(70, 80, cap).astype(np.float32),
                desc=rng.randint(0, 256, (cap, 32)).astype(np.uint8), obs=rng.randint(-99, -9, (cap, 2)).astype(np.int32),
                mp1=np.where(rng.uniform(size=n1) < 0.1, rng.randint(0, 30, n1), -1).astype(np.int32),
                mp2=np.where(rng.uniform(size=n2) < 0.1, rng.randint(0, 30, n2), -1).astype(np.int32),
                has_mp1=(rng.uniform(size=n1) < 0.1).astype(np.uint8), has_mp2=(rng.uniform(size=n2) < 0.1).astype(np.uint8))


def _device_dict(torch, dev, cloud, state):
    d = {k: _up(torch, dev, v) for k, v in state.items()}
    d.update(pose_R1=_up(torch, dev, np.asarray(cloud["R1"], np.float64).reshape(9)), pose_t1=_up(torch, dev, np.asarray(cloud["t1"], np.float64)),
             pose_R2=_up(torch, dev, np.asarray(cloud["R2"], np.float64).reshape(9)), pose_t2=_up(torch, dev, np.asarray(cloud["t2"], np.float64)),
             kps1=_up(torch, dev, cloud["kps1"]), kps2=_up(torch, dev, cloud["kps2"]), desc2=_up(torch, dev, cloud["desc2"]),
             matches12=_up(torch, dev, cloud["matches12"]), code=torch.full((cloud["n1"],), 77, dtype=torch.int32, device=dev),
             result=torch.full((8,), 77, dtype=torch.int32, device=dev))
    if cloud["fisheye"]:
        d["fisheye_scale"] = _up(torch, dev, cloud["scale_table"])
    return d


def _call_device(m, cam, d, cloud, cap, stream=None):
    m.TriangulateMatchesDevice(cam, d, cloud["n1"], cloud["n2"], cap, tm.SIGMA2, float(tm.MAX_SCALE_FACTOR), float(tm.RATIO_FACTOR),
                               stream=stream)


def _exclusions(cloud, e32, e64):
    """(the issue's exclusion set, the narrower one the comparison uses): masks over the features of key frame 1"""
    flips = e32["code"] != e64["code"]
    band_cos, band_chi2, band_ratio = (tm.threshold_band(cloud, e64, w) for w in range(3))
    near_cos = np.zeros(len(flips), bool)
    with np.errstate(invalid="ignore"):
        near_cos[e64["all_feat1"]] = np.abs(e64["cosp"] - tm.COS_PARALLAX) < NEAR_COS
    return flips | band_cos | band_chi2 | band_ratio, flips | near_cos | band_chi2 | band_ratio


def _compare(cloud, got, state0, e32, e64, cap):
    """device (or host-twin) outputs `got` against the float64 model; returns the two maxima of the position yardstick"""
    n0 = cloud["n_points"]
    n_matches = int((e64["code"] >= 0).sum())
    issue_set, excluded = _exclusions(cloud, e32, e64)
    assert not (excluded & ~issue_set).any()
    print("excluded %d of %d matches (the issue's set %d)" % (excluded.sum(), n_matches, issue_set.sum()))
    assert issue_set.sum() <= EXCLUDED_CAP * n_matches
    keep = ~excluded
    code = got["code"]
    assert np.array_equal(code[keep], e64["code"][keep])
    assert np.array_equal(code < 0, e64["code"] < 0)
    res = got["result"]
    want = np.bincount(code[code >= 0], minlength=8)[:8]
    assert res[1] == 0 and np.array_equal(np.delete(res, 1), np.delete(want, 1))           # the counters are the codes'
    assert np.abs(res.astype(np.int64) - e64["result"]).max() <= excluded.sum()
    if not (code != e64["code"]).any():
        assert np.array_equal(res, e64["result"])
    # rows in ascending feature order behind the old counter; the counter advanced
    acc = np.flatnonzero(code == 0)
    k = len(acc)
    assert int(got["n_points"][0]) == n0 + k and k == res[0] and n0 + k <= cap
    rows = n0 + np.arange(k)
    assert np.array_equal(got["obs"][rows, 0], acc) and np.array_equal(got["obs"][rows, 1], cloud["matches12"][acc])
    assert (got["valid"][rows] == 1).all()
    assert np.array_equal(got["desc"][rows], cloud["desc2"][cloud["matches12"][acc]])
    # slots and flags: exactly the accepted features', everything else as passed
    m_acc = cloud["matches12"][acc]
    mp1, mp2, h1, h2 = state0["mp1"].copy(), state0["mp2"].copy(), state0["has_mp1"].copy(), state0["has_mp2"].copy()
    mp1[acc], mp2[m_acc], h1[acc], h2[m_acc] = rows, rows, 1, 1
    for key, w in (("mp1", mp1), ("mp2", mp2), ("has_mp1", h1), ("has_mp2", h2)):
        assert np.array_equal(got[key], w), key
    # rows below the old counter and past the new one are untouched
    rest = np.r_[0:n0, n0 + k:cap]
    for key in TABLE_KEYS:
        assert np.array_equal(got[key][rest], state0[key][rest]), key
    # positions, normals, distance ranges of the points both the device and float64 accept: the yardstick is the float64 run
    both = np.flatnonzero((code == 0) & (e64["code"] == 0))
    r_dev, r64 = n0 + np.searchsorted(acc, both), e64["index"][both] - n0
    dist2 = e64["dist2"][r64]
    dev_err = np.linalg.norm(got["points"][r_dev].astype(np.float64) - e64["points"][r64], axis=1) / dist2
    b32 = np.flatnonzero((e32["code"] == 0) & (e64["code"] == 0))
    q32, q64 = e32["index"][b32] - n0, e64["index"][b32] - n0
    mod_err = np.linalg.norm(e32["points"][q32].astype(np.float64) - e64["points"][q64], axis=1) / e64["dist2"][q64]
    print("largest |Pw - Pw64| / dist2: device %.3e, numpy float32 model %.3e (ratio %.2f)" % (dev_err.max(), mod_err.max(), dev_err.max() / mod_err.max()))
    # the remaining outputs are short float expressions of Pw: a deviation of Pw moves a unit normal by that much relative to the
    # distance and a range by that much relative to itself; 4 float ulps (2.4e-7) for their own roundings
    slack = 2 * dev_err.max() + 2.4e-7
    assert np.abs(got["normals"][r_dev].astype(np.float64) - e64["normals"][r64]).max() <= slack
    assert np.abs(got["max_dist"][r_dev] / e64["max_dist"][r64] - 1).max() <= slack
    assert np.abs(got["min_dist"][r_dev] / e64["min_dist"][r64] - 1).max() <= slack
    assert dev_err.max() <= 4 * mod_err.max()
    return dev_err.max(), mod_err.max()


def _read(d):
    return {k: d[k].cpu().numpy() for k in STATE_KEYS + ("code", "result")}


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("fisheye,n,seed,baseline,mismatched,margin", CLOUDS)
def test_device_against_the_model(fisheye, n, seed, baseline, mismatched, margin, stream_kind):
    """Gate code per match, every counter, order and number of the appended rows, slots, flags, observation pairs and descriptors
    equal the float64 model's outside the excluded matches (at most 0.5 %); positions deviate from float64, relative to the
    distance to the current key frame, by at most 4 x what numpy's float32 model (LAPACK's SVD) does; every output starts as
    garbage and rows outside [old counter, new counter) keep it."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    cloud = tm.make_cloud(fisheye, n, seed, baseline, mismatched, margin)
    e32, e64 = tm.run_model(cloud), tm.run_model(cloud, np.float64)
    cap = cloud["n_points"] + n + 50
    state0 = _host_state(cloud, cap)
    d = _device_dict(torch, dev, cloud, state0)
    st = _stream(torch, dev, stream_kind)
    _call_device(ORBMatcher(), ProjCamera.make(cloud["cam"], cloud["bounds"]), d, cloud, cap, st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    got = _read(d)
    print("%s baseline %.1f mismatched %d: device result %s, float64 %s" % ("fisheye" if fisheye else "pinhole", baseline, mismatched,
                                                                          got["result"].tolist(), e64["result"].tolist()))
    _compare(cloud, got, state0, e32, e64, cap)


@pytest.mark.parametrize("fisheye", [False, True])
def test_a_full_table_is_reported_and_nothing_changes(fisheye):
    """cap_points one row short of what the call would append: d_result[1] = 1, d_result[0] = 0, and the table, the slots, the flags
    and the counter are byte-identical to what was passed; with exactly enough rows the same call succeeds."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    cloud = tm.make_cloud(fisheye, 3000, 91, 4.0, False, 150 if fisheye else 40)
    e64 = tm.run_model(cloud, np.float64)
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    m = ORBMatcher()
    # the device's own count decides what "one row short" is
    big = cloud["n_points"] + 3000
    state0 = _host_state(cloud, big, seed=2)
    d = _device_dict(torch, dev, cloud, state0)
    _call_device(m, cam, d, cloud, big)
    torch.cuda.synchronize()
    k = int(d["result"][0])
    assert abs(k - e64["result"][0]) <= 15 and int(d["result"][1]) == 0 and int(d["n_points"][0]) == cloud["n_points"] + k
    for cap, fits in ((cloud["n_points"] + k - 1, False), (cloud["n_points"] + k, True)):
        state = {key: (v[:cap].copy() if key in TABLE_KEYS else v.copy()) for key, v in state0.items()}
        d = _device_dict(torch, dev, cloud, state)
        _call_device(m, cam, d, cloud, cap)
        torch.cuda.synchronize()
        got = _read(d)
        if fits:
            assert got["result"][1] == 0 and got["result"][0] == k and got["n_points"][0] == cap
        else:
            assert got["result"][1] == 1 and got["result"][0] == 0
            assert np.array_equal(got["result"][2:], np.bincount(got["code"][got["code"] >= 0], minlength=8)[2:8])
            for key in STATE_KEYS:
                assert got[key].tobytes() == state[key].tobytes(), key


def test_no_match_and_no_feature():
    """n1 = 0 and a call without any match are allowed: zero counters, nothing touched."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    cloud = tm.make_cloud(False, 500, 5)
    cloud["matches12"][:] = -1
    cloud["matches12"][::7] = cloud["n2"] + 3           # out of range counts as no match
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    cap = 100
    state0 = _host_state(cloud, cap, seed=3)
    for n1 in (cloud["n1"], 0):
        d = _device_dict(torch, dev, cloud, state0)
        ORBMatcher().TriangulateMatchesDevice(cam, d, n1, cloud["n2"], cap, tm.SIGMA2, float(tm.MAX_SCALE_FACTOR), float(tm.RATIO_FACTOR))
        torch.cuda.synchronize()
        got = _read(d)
        assert not got["result"].any()
        assert (got["code"][:n1] == -1).all() and (got["code"][n1:] == 77).all()
        for key in STATE_KEYS:
            assert got[key].tobytes() == state0[key].tobytes(), key


@pytest.mark.parametrize("which", [0, 4])
def test_host_twin_gives_the_same_bytes(which):
    """orbm_triangulate_matches on numpy arrays against orbm_triangulate_matches_device on the same inputs, Pinhole and Fisheye
    (whose scale entries the host entry point gathers per key point); and with a table that is too small."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    cloud = tm.make_cloud(*CLOUDS[which])
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    m = ORBMatcher()
    for cap in (cloud["n_points"] + CLOUDS[which][1], cloud["n_points"] + 100):
        state0 = _host_state(cloud, cap, seed=4)
        d = _device_dict(torch, dev, cloud, state0)
        _call_device(m, cam, d, cloud, cap)
        torch.cuda.synchronize()
        want = _read(d)
        t = {k: v.copy() for k, v in state0.items()}
        code, result = m.TriangulateMatches(cam, t, cloud["kps1"], cloud["kps2"], cloud["desc2"], cloud["matches12"], (cloud["R1"], cloud["t1"]),
                                            (cloud["R2"], cloud["t2"]), tm.SIGMA2, float(tm.MAX_SCALE_FACTOR), float(tm.RATIO_FACTOR),
                                            fisheye_scale=cloud["scale_table"])
        assert np.array_equal(code, want["code"]) and np.array_equal(result, want["result"])
        assert result[1] == (0 if cap > cloud["n_points"] + 100 else 1) and (result[0] > 1000 or result[1] == 1)
        for key in STATE_KEYS:
            assert t[key].tobytes() == want[key].tobytes(), key


# ---- the mapper's chain with one wait --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_mapper_chain_with_one_wait(stream_kind):
    """LocalMapping::createNewMapPoints then the first step of searchInNeighbors on ONE stream, the only wait at the end: four views
    of a textured plane at Z = 10 m (three older key frames and the current one, a camera that translates) -> extract (one batch)
    -> frame post -> orbv_transform_device -> three times [orbm_search_for_triangulation_device -> orbm_triangulate_matches_device]
    against the current key frame, each search reading the flags the triangulation before it set -> orbm_project_fuse_device on the
    grown table.  Against a host loop of orbm_search_for_triangulation and the float64 model on the records read back."""
    import torch
    from monoorbslam3_amd.extractor import ORBExtractor, KP_DTYPE
    from monoorbslam3_amd.frame import FramePost
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    from monoorbslam3_amd.vocabulary import ORBVocabulary
    dev = torch.device("cuda", 0)
    w, h, Z = 752, 480, 10.0
    fx = fy = 460.0
    cx, cy = 376.0, 240.0
    camt, bounds = (fx, fy, cx, cy), (0.0, float(w), 0.0, float(h))
    canvas = synth.make_canvas(w + 80, h + 60, seed=606)
    shifts = [(26, 12), (-30, 16), (14, -24), (0, 0)]                      # the crops of key frames 0, 1, 2 and of the current one
    f = np.stack([canvas[30 + dy:30 + dy + h, 40 + dx:40 + dx + w] for dx, dy in shifts])
    poses = [(np.eye(3), np.array([-dx * Z / fx, -dy * Z / fy, 0.0])) for dx, dy in shifts]   # P_c = P_w + t, world = the current camera
    K = 3
    ex = ORBExtractor(1500, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=4)
    post = FramePost(w, h, fx, fy, cx, cy)
    voc = ORBVocabulary.from_arrays(synth.make_vocabulary(10, 5, seed=3), device=0)
    cap = ex.max_keypoints(w, h)
    cap_points = 4000
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    img = torch.from_numpy(np.ascontiguousarray(f)).to(dev)
    d_kp, d_un, d_desc, d_n = z((4, cap, 28), torch.uint8), z((4, cap, 28), torch.uint8), z((4, cap, 32), torch.uint8), z((4,), torch.int32)
    d_start, d_items = z((4, post.n_cells + 1), torch.int32), z((4, cap), torch.int32)
    bow_ids, bow_vals, n_words = z((4, cap), torch.int32), z((4, cap), torch.float64), z((4,), torch.int32)
    fv_nodes, fv_off, fv_idx, n_fv = z((4, cap), torch.int32), z((4, cap + 1), torch.int32), z((4, cap), torch.int32), z((4,), torch.int32)
    has_mp, slots = z((4, cap), torch.uint8), torch.full((4, cap), -1, dtype=torch.int32, device=dev)
    m12, codes = torch.full((K, cap), -7, dtype=torch.int32, device=dev), torch.full((K, cap), -7, dtype=torch.int32, device=dev)
    s_res, t_res = z((K, 8), torch.int32), z((K, 8), torch.int32)
    table = dict(n_points=z((1,), torch.int32), points=z((cap_points, 3), torch.float32), valid=z((cap_points,), torch.uint8),
                 normals=z((cap_points, 3), torch.float32), min_dist=z((cap_points,), torch.float32), max_dist=z((cap_points,), torch.float32),
                 desc=z((cap_points, 32), torch.uint8), obs=z((cap_points, 2), torch.int32))
    d_pose = [(_up(torch, dev, R.reshape(9)), _up(torch, dev, t)) for R, t in poses]
    fuse = dict(table, pose_R=d_pose[0][0], pose_t=d_pose[0][1], q_xy=z((cap_points, 2), torch.float32), q_radius=z((cap_points,), torch.float32),
                q_level=z((cap_points,), torch.int32), q_ok=z((cap_points,), torch.uint8), result=z((8,), torch.int32))
    cam = ProjCamera.make(camt, bounds)
    m = ORBMatcher(0.6, False)                                              # LocalMapping.cpp:151
    st = _stream(torch, dev, stream_kind)
    ex.extract_batch_device(img.data_ptr(), 4, w, h, w, w * h, d_kp.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    post.post_device(4, d_kp.data_ptr(), d_n.data_ptr(), cap, d_un.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), st)
    voc.transform_device(4, d_desc.data_ptr(), d_n.data_ptr(), cap, 4, bow_ids.data_ptr(), bow_vals.data_ptr(), n_words.data_ptr(),
                         fv_nodes.data_ptr(), fv_off.data_ptr(), fv_idx.data_ptr(), n_fv.data_ptr(), st)
    for k in range(K):
        d = dict(table, desc1=d_desc[k], kps1=d_un[k], has_mp1=has_mp[k], fv1=(fv_nodes[k], fv_off[k], fv_idx[k], n_fv[k:k + 1]), desc2=d_desc[3],
                 kps2=d_un[3], has_mp2=has_mp[3], fv2=(fv_nodes[3], fv_off[3], fv_idx[3], n_fv[3:4]), matches12=m12[k], result=s_res[k])
        m.SearchForTriangulationDevice(d, cap, cap, stream=st)
        d.update(pose_R1=d_pose[k][0], pose_t1=d_pose[k][1], pose_R2=d_pose[3][0], pose_t2=d_pose[3][1], mp1=slots[k], mp2=slots[3], code=codes[k],
                 result=t_res[k])
        m.TriangulateMatchesDevice(cam, d, cap, cap, cap_points, tm.SIGMA2, float(tm.MAX_SCALE_FACTOR), float(tm.RATIO_FACTOR), stream=st)
    m.ProjectFuseDevice(cam, fuse, cap_points, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), 3.0, stream=st)
    torch.cuda.synchronize()   # the first and only wait of the chain
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    # ---- the host loop on the records read back
    g = lambda tns: tns.cpu().numpy()  # noqa: E731
    n = g(d_n)
    kps = [np.frombuffer(g(d_un[i, :n[i]]).tobytes(), KP_DTYPE) for i in range(4)]
    desc = [g(d_desc[i, :n[i]]) for i in range(4)]
    nf = g(n_fv)
    fvs = [(g(fv_nodes[i, :nf[i]]).view(np.uint32), g(fv_off[i, :nf[i] + 1]), g(fv_idx[i, :int(fv_off[i, nf[i]])]).view(np.uint32)) for i in range(4)]
    has2 = np.zeros(n[3], np.uint8)
    slot2 = np.full(n[3], -1, np.int32)
    n_pts, total_excluded = 0, 0
    got_table = {key: g(table[key]) for key in table}
    for k in range(K):
        n_host, m_host = m.SearchForTriangulation(desc[k], kps[k]["angle"], np.zeros(n[k], np.uint8), fvs[k], desc[3], kps[3]["angle"], has2, fvs[3])
        got_m = g(m12[k])
        assert int(s_res[k, 1]) == 0 and int(s_res[k, 0]) == n_host and n_host > 50
        assert np.array_equal(got_m[:n[k]], m_host) and (got_m[n[k]:] == -1).all()
        cloud = dict(cam=camt, scale_table=None, R1=poses[k][0], t1=poses[k][1], R2=poses[3][0], t2=poses[3][1], kps1=kps[k], kps2=kps[3],
                     desc2=desc[3], matches12=m_host, n_points=n_pts)
        e32, e64 = tm.run_model(cloud), tm.run_model(cloud, np.float64)
        _, excluded = _exclusions(cloud, e32, e64)
        code = g(codes[k])
        assert (code[n[k]:] == -1).all()
        code = code[:n[k]]
        assert np.array_equal(code[~excluded], e64["code"][~excluded])
        total_excluded += int(excluded.sum())
        res = g(t_res[k])
        acc = np.flatnonzero(code == 0)
        assert res[1] == 0 and res[0] == len(acc) and np.array_equal(res[2:], np.bincount(code[code >= 0], minlength=8)[2:8])
        rows = n_pts + np.arange(len(acc))
        assert np.array_equal(got_table["obs"][rows], np.stack([acc, m_host[acc]], 1))
        assert np.array_equal(got_table["desc"][rows], desc[3][m_host[acc]])
        both = np.flatnonzero((code == 0) & (e64["code"] == 0))
        if len(both):
            dev_rows, r64 = n_pts + np.searchsorted(acc, both), e64["index"][both] - n_pts
            err = np.linalg.norm(got_table["points"][dev_rows].astype(np.float64) - e64["points"][r64], axis=1) / e64["dist2"][r64]
            assert err.max() < 1e-4
        want_slots = np.full(cap, -1, np.int32)
        want_slots[acc] = rows
        assert np.array_equal(g(slots[k]), want_slots) and np.array_equal(g(has_mp[k]), (want_slots >= 0).astype(np.uint8))
        # the coupling: the next search sees the points this key frame gave the current one (the device's decisions carry on)
        assert not has2[m_host[acc]].any()
        has2[m_host[acc]] = 1
        slot2[m_host[acc]] = rows
        print("key frame %d: %d matches, device result %s, float64 %s, excluded %d" % (k, n_host, res.tolist(), e64["result"].tolist(), excluded.sum()))
        n_pts += len(acc)
    assert int(got_table["n_points"][0]) == n_pts and n_pts > 100
    assert np.array_equal(g(has_mp[3])[:n[3]], has2) and np.array_equal(g(slots[3])[:n[3]], slot2) and not g(has_mp[3])[n[3]:].any()
    # a feature of the current key frame holds at most one point
    assert len(np.unique(got_table["obs"][:n_pts, 1])) == n_pts
    assert (got_table["valid"][:n_pts] == 1).all() and not got_table["valid"][n_pts:].any()
    P = got_table["points"][:n_pts]
    print("%d new points, median |z - %g| = %.3f m, excluded matches %d" % (n_pts, Z, np.median(np.abs(P[:, 2] - Z)), total_excluded))
    assert np.median(np.abs(P[:, 2] - Z)) < 0.5
    # the fuse queries on the grown table equal the float32 model of the builders on the table read back
    fc = dict(form=pm.FUSE, cam=camt, bounds=bounds, R=poses[0][0], t=poses[0][1], points=got_table["points"], valid=got_table["valid"],
              normals=got_table["normals"], min_dist=got_table["min_dist"], max_dist=got_table["max_dist"], th=3.0, view_cos_limit=0.5, n=cap_points)
    f32, f64 = pm.run_model(fc), pm.run_model(fc, np.float64)
    near = pm.near_threshold(pm.FUSE, fc, f64)
    q_ok = g(fuse["q_ok"])
    assert np.array_equal(q_ok, f32["q_ok"]) and np.array_equal(g(fuse["q_xy"]).view(np.uint32), f32["q_xy"].view(np.uint32))
    free = near["level"]
    assert np.array_equal(g(fuse["q_level"])[~free], f32["q_level"][~free])
    assert np.array_equal(g(fuse["result"]), f32["result"]) and q_ok.sum() > 50 and not q_ok[n_pts:].any()
