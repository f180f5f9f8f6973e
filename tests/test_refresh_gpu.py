"""orbm_refresh_points_device / orbm_scene_median_depth_device on the MI355X (include/orbm.h, "Map points refreshed on the device")
against the float32 numpy model of tests/refresh_model.py, bit for bit and without exclusions, then chained behind
orbm_triangulate_matches_device and ahead of orbm_project_fuse_device with one host wait."""
import numpy as np
import pytest

import projection_model as pm
import refresh_model as rm
import triangulation_model as tm
from monoorbslam3_amd import synth
from test_triangulation_gpu import _stream, _up

pytestmark = pytest.mark.gpu

SCENES = {41: dict(n_kf=12), 42: dict(n_kf=3, feats=(50, 120), n_rows=200), 43: dict(n_kf=40, n_rows=600)}
KF_SELF = 1
_cache = {}


def _scene(seed):
    """(scene, selection, float32 model): computed once, shared, never changed"""
    if seed not in _cache:
        sc = rm.make_scene(seed, **SCENES[seed])
        sel = rm.make_selection(sc, seed)
        _cache[seed] = (sc, sel, rm.refresh(sc, sel, sc["n_rows"], kf_self=KF_SELF))
    return _cache[seed]


def _kf_table(torch, dev, sc):
    from monoorbslam3_amd.matcher import KfTable
    return KfTable.make(_up(torch, dev, sc["pose_R"]), _up(torch, dev, sc["pose_t"]), _up(torch, dev, sc["bad"]),
                        [_up(torch, dev, k) for k in sc["kps"]], [_up(torch, dev, d) for d in sc["kf_desc"]], _up(torch, dev, sc["n"]))


def _device(torch, dev, sc, sel, covis=True):
    d = {k: _up(torch, dev, sc[k]) for k in ("points", "valid", "normals", "min_dist", "max_dist", "desc", "obs_off", "obs_kf", "obs_kp", "ref_kf")}
    d.update(sel=_up(torch, dev, sel), result=torch.full((8,), 77, dtype=torch.int32, device=dev))
    if covis:
        d["covis"] = torch.full((len(sc["n"]),), -99, dtype=torch.int32, device=dev)
    return d


def _check_table(d, want, sc):
    """every row of every output array, the spare rows past cap_points included: the selected rows equal the model's, the others
    are the bytes that were passed (the model copies them)"""
    g = lambda k: d[k].cpu().numpy()  # noqa: E731
    normals = g("normals")
    assert np.array_equal(normals, want["normals"])                       # by value: -0 equals +0
    assert not np.isnan(normals).any()
    for key in ("min_dist", "max_dist"):
        assert np.array_equal(g(key).view(np.uint32), want[key].view(np.uint32)), key
    assert np.array_equal(g("desc"), want["desc"])
    rest = ~want["touched"]
    assert rest[sc["n_rows"]:].all() and rest.sum() > 20
    for key in ("normals", "min_dist", "max_dist", "desc"):
        assert g(key)[rest].tobytes() == sc[key][rest].tobytes(), key
    for key in ("points", "valid"):
        assert g(key).tobytes() == sc[key].tobytes(), key


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("seed", sorted(SCENES))
def test_refresh_equals_the_float32_model(seed, stream_kind):
    """normals, distance ranges and descriptors bit for bit (normals by value), every counter and the covisibility counts exact, on
    lists of 0, 1, 2, 3, 31 .. 33, 63 .. 65, 127 .. 129, 200, 1024 and 1025 remaining observations (2 | 3 and 64 | 65 raw are the
    kernel's path switches), bad key frames, an all-bad row, an unobserved and a missing reference key frame, invalid rows, -1,
    out-of-range and duplicate entries of d_sel, dropped observations; the table starts as garbage and only selected rows change."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    sc, sel, want = _scene(seed)
    kf = _kf_table(torch, dev, sc)
    d = _device(torch, dev, sc, sel)
    st = _stream(torch, dev, stream_kind)
    ORBMatcher().RefreshPointsDevice(kf, d, len(sel), sc["n_rows"], len(sc["obs_kf"]), float(rm.MAX_SCALE_FACTOR), kf_self=KF_SELF, stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    result, covis = d["result"].cpu().numpy(), d["covis"].cpu().numpy()
    print("seed %d: device result %s, model %s" % (seed, result.tolist(), want["result"].tolist()))
    assert np.array_equal(result, want["result"])
    assert np.array_equal(covis, want["covis"]) and covis[KF_SELF] == 0 and covis.sum() > 1000
    _check_table(d, want, sc)


def test_refresh_without_covisibility_and_with_an_empty_selection():
    """d_covis = NULL runs and gives the same table; n_sel = 0 zeroes d_result and d_covis and touches nothing."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    sc, sel, want = _scene(42)
    kf = _kf_table(torch, dev, sc)
    m = ORBMatcher()
    d = _device(torch, dev, sc, sel, covis=False)
    m.RefreshPointsDevice(kf, d, len(sel), sc["n_rows"], len(sc["obs_kf"]), float(rm.MAX_SCALE_FACTOR), kf_self=KF_SELF)
    torch.cuda.synchronize()
    assert np.array_equal(d["result"].cpu().numpy(), want["result"])
    _check_table(d, want, sc)
    d = _device(torch, dev, sc, sel)
    m.RefreshPointsDevice(kf, d, 0, sc["n_rows"], len(sc["obs_kf"]), float(rm.MAX_SCALE_FACTOR), kf_self=KF_SELF)
    torch.cuda.synchronize()
    assert not d["result"].cpu().numpy().any() and not d["covis"].cpu().numpy().any()
    for key in ("normals", "min_dist", "max_dist", "desc"):
        assert d[key].cpu().numpy().tobytes() == sc[key].tobytes(), key


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_scene_median_depth_equals_the_model(stream_kind):
    """Counts 0 (NaN), 1, 2, odd, even, all-equal depths, negative depths, d_n > stride (clamped), a negative d_n, a full row at the
    stride limit with -1 and out-of-range slots: median, count and baseline bit-identical to the model."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(77)
    stride, cap_points, rows = 8192, 3000, 3040
    points = (rng.uniform(-4, 4, (rows, 3)) + [0, 0, 6]).astype(np.float32)
    counts = [0, 1, 2, 7, 8, 33, 500, 8192, 9000, -3, 2001, 64]
    n_kf = len(counts)
    slots = rng.randint(-400, rows + 200, (n_kf, stride)).astype(np.int32)      # -1s, rows past cap_points, rows past the arrays
    slots[:7] = rng.randint(0, cap_points, (7, stride))                           # exact counts for the small ones
    slots[0, :] = -1
    slots[5, :] = 17                                                              # all-equal depths
    pose_R = np.stack([rm._rodrigues(rng.uniform(-0.4, 0.4, 3) + 1e-3) for _ in range(n_kf)]).reshape(n_kf, 9)
    pose_t = rng.uniform(-2, 2, (n_kf, 3))
    pose_t[6, 2] = -40.0                                                          # negative depths
    n = np.array(counts, np.int32)
    n[0] = 50                                                                     # fifty empty slots: count 0
    cur = 3
    med, cnt, base = rm.median_depth(pose_R, pose_t, slots, n, stride, points, cap_points, cur=cur)
    assert cnt.tolist()[:7] == [0, 1, 2, 7, 8, 33, 500] and np.isnan(med[0]) and np.isnan(med[9]) and med[6] < -20 and 4000 < cnt[7] < 8192
    assert cnt[8] > 4000 and cnt[9] == 0
    d = dict(pose_R=_up(torch, dev, pose_R), pose_t=_up(torch, dev, pose_t), slots=_up(torch, dev, slots), n=_up(torch, dev, n),
             points=_up(torch, dev, points), median=torch.full((n_kf,), 5.0, dtype=torch.float32, device=dev),
             count=torch.full((n_kf,), -5, dtype=torch.int32, device=dev), baseline=torch.full((n_kf,), 5.0, dtype=torch.float32, device=dev))
    st = _stream(torch, dev, stream_kind)
    m = ORBMatcher()
    m.SceneMedianDepthDevice(d, n_kf, stride, cap_points, cur=cur, stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    g = lambda k: d[k].cpu().numpy()  # noqa: E731
    print("counts %s\nmedians %s" % (g("count").tolist(), g("median").tolist()))
    assert np.array_equal(g("count"), cnt)
    assert np.array_equal(g("median").view(np.uint32), med.view(np.uint32))
    assert np.array_equal(g("baseline").view(np.uint32), base.astype(np.float32).view(np.uint32)) and g("baseline")[cur] == 0
    # without the baseline: d_baseline stays as it was
    d["baseline"].fill_(5.0)
    d2 = dict(d, baseline=None)
    m.SceneMedianDepthDevice(d2, n_kf, stride, cap_points)
    torch.cuda.synchronize()
    assert np.array_equal(g("median").view(np.uint32), med.view(np.uint32)) and (g("baseline") == 5.0).all()


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_mapper_chain_with_one_wait(stream_kind):
    """Two views of a textured plane -> extract -> frame post -> orbv_transform_device -> orbm_search_for_triangulation_device ->
    orbm_triangulate_matches_device -> the CSR of the new rows built with tensor operations -> orbm_refresh_points_device on the
    current key frame's slots, ONE wait at the end.  A new point has its two observations in the order (older key frame, current key
    frame) and the current one as its reference, so the refresh evaluates the expressions the triangulation evaluated on the same
    poses: normals and distance ranges must come out bit for bit as the triangulation wrote them; both medians are 0, so the
    descriptor becomes the OLDER key frame's row (first in CSR order); d_covis[older] is the number of new points; and the fuse
    queries built from the refreshed table give the d_result they gave before."""
    import torch
    from monoorbslam3_amd.extractor import ORBExtractor
    from monoorbslam3_amd.frame import FramePost
    from monoorbslam3_amd.matcher import KfTable, ORBMatcher, ProjCamera
    from monoorbslam3_amd.vocabulary import ORBVocabulary
    dev = torch.device("cuda", 0)
    w, h, Z = 752, 480, 10.0
    fx = fy = 460.0
    cx, cy = 376.0, 240.0
    camt, bounds = (fx, fy, cx, cy), (0.0, float(w), 0.0, float(h))
    canvas = synth.make_canvas(w + 80, h + 60, seed=606)
    shifts = [(26, 12), (0, 0)]                                            # the older key frame, the current one
    f = np.stack([canvas[30 + dy:30 + dy + h, 40 + dx:40 + dx + w] for dx, dy in shifts])
    poses = [(np.eye(3), np.array([-dx * Z / fx, -dy * Z / fy, 0.0])) for dx, dy in shifts]
    ex = ORBExtractor(1500, 1.2, 8, 20, 7, max_width=w, max_height=h, max_batch=2)
    post = FramePost(w, h, fx, fy, cx, cy)
    voc = ORBVocabulary.from_arrays(synth.make_vocabulary(10, 5, seed=3), device=0)
    cap = ex.max_keypoints(w, h)
    cap_points = 3000
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    img = torch.from_numpy(np.ascontiguousarray(f)).to(dev)
    d_kp, d_un, d_desc, d_n = z((2, cap, 28), torch.uint8), z((2, cap, 28), torch.uint8), z((2, cap, 32), torch.uint8), z((2,), torch.int32)
    d_start, d_items = z((2, post.n_cells + 1), torch.int32), z((2, cap), torch.int32)
    bow_ids, bow_vals, n_words = z((2, cap), torch.int32), z((2, cap), torch.float64), z((2,), torch.int32)
    fv_nodes, fv_off, fv_idx, n_fv = z((2, cap), torch.int32), z((2, cap + 1), torch.int32), z((2, cap), torch.int32), z((2,), torch.int32)
    has_mp, slots = z((2, cap), torch.uint8), torch.full((2, cap), -1, dtype=torch.int32, device=dev)
    table = dict(n_points=z((1,), torch.int32), points=z((cap_points, 3), torch.float32), valid=z((cap_points,), torch.uint8),
                 normals=z((cap_points, 3), torch.float32), min_dist=z((cap_points,), torch.float32), max_dist=z((cap_points,), torch.float32),
                 desc=z((cap_points, 32), torch.uint8), obs=z((cap_points, 2), torch.int32))
    pose_R = _up(torch, dev, np.stack([R.reshape(9) for R, _ in poses]))
    pose_t = _up(torch, dev, np.stack([t for _, t in poses]))
    results = {k: torch.full((8,), 77, dtype=torch.int32, device=dev) for k in ("search", "tri", "refresh", "fuse_before", "fuse_after")}
    cam = ProjCamera.make(camt, bounds)
    m = ORBMatcher(0.6, False)
    kf = KfTable.make(pose_R, pose_t, z((2,), torch.uint8), [d_un[0], d_un[1]], [d_desc[0], d_desc[1]], d_n)
    st = _stream(torch, dev, stream_kind)
    ex.extract_batch_device(img.data_ptr(), 2, w, h, w, w * h, d_kp.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr(), st)
    post.post_device(2, d_kp.data_ptr(), d_n.data_ptr(), cap, d_un.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), st)
    voc.transform_device(2, d_desc.data_ptr(), d_n.data_ptr(), cap, 4, bow_ids.data_ptr(), bow_vals.data_ptr(), n_words.data_ptr(),
                         fv_nodes.data_ptr(), fv_off.data_ptr(), fv_idx.data_ptr(), n_fv.data_ptr(), st)
    d = dict(table, desc1=d_desc[0], kps1=d_un[0], has_mp1=has_mp[0], fv1=(fv_nodes[0], fv_off[0], fv_idx[0], n_fv[0:1]), desc2=d_desc[1],
             kps2=d_un[1], has_mp2=has_mp[1], fv2=(fv_nodes[1], fv_off[1], fv_idx[1], n_fv[1:2]),
             matches12=torch.full((cap,), -7, dtype=torch.int32, device=dev), result=results["search"])
    m.SearchForTriangulationDevice(d, cap, cap, stream=st)
    d.update(pose_R1=pose_R[0], pose_t1=pose_t[0], pose_R2=pose_R[1], pose_t2=pose_t[1], mp1=slots[0], mp2=slots[1], result=results["tri"])
    m.TriangulateMatchesDevice(cam, d, cap, cap, cap_points, tm.SIGMA2, float(tm.MAX_SCALE_FACTOR), float(tm.RATIO_FACTOR), stream=st)
    fuse = dict(table, pose_R=pose_R[0], pose_t=pose_t[0], q_xy=z((cap_points, 2), torch.float32), q_radius=z((cap_points,), torch.float32),
                q_level=z((cap_points,), torch.int32), q_ok=z((cap_points,), torch.uint8), result=results["fuse_before"])
    m.ProjectFuseDevice(cam, fuse, cap_points, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), 3.0, stream=st)
    before = {k: table[k].clone() for k in ("normals", "min_dist", "max_dist", "desc")}     # device copies on the chain's stream
    q_before = {k: fuse[k].clone() for k in ("q_xy", "q_radius", "q_level", "q_ok")}
    # the CSR of the new rows, on the device: row p's observations are (key frame 0, obs[p][0]) and (key frame 1, obs[p][1])
    ref = dict(table, sel=slots[1], obs_off=2 * torch.arange(cap_points + 1, dtype=torch.int32, device=dev),
               obs_kf=torch.arange(2 * cap_points, dtype=torch.int32, device=dev) % 2, obs_kp=table["obs"].view(-1),
               ref_kf=torch.ones(cap_points, dtype=torch.int32, device=dev), covis=torch.full((2,), -99, dtype=torch.int32, device=dev),
               result=results["refresh"])
    m.RefreshPointsDevice(kf, ref, cap, cap_points, 2 * cap_points, float(tm.MAX_SCALE_FACTOR), kf_self=1, stream=st)
    fuse["result"] = results["fuse_after"]
    m.ProjectFuseDevice(cam, fuse, cap_points, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), 3.0, stream=st)
    torch.cuda.synchronize()   # the first and only wait of the chain
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    g = lambda t: t.cpu().numpy()  # noqa: E731
    n_new = int(results["tri"][0])
    res = g(results["refresh"])
    print("new points %d; refresh d_result %s, d_covis %s" % (n_new, res.tolist(), g(ref["covis"]).tolist()))
    assert n_new > 100 and int(table["n_points"][0]) == n_new and int(results["tri"][1]) == 0
    assert res.tolist() == [n_new, 0, 0, 0, 0, 0, 0, 0]
    assert g(ref["covis"]).tolist() == [n_new, 0]
    assert np.array_equal(g(table["normals"]), g(before["normals"]))                   # by value
    for key in ("min_dist", "max_dist"):
        assert g(table[key]).tobytes() == g(before[key]).tobytes(), key
    obs, desc_after = g(table["obs"])[:n_new], g(table["desc"])
    assert np.array_equal(desc_after[:n_new], g(d_desc[0])[obs[:, 0]])
    assert np.array_equal(g(before["desc"])[:n_new], g(d_desc[1])[obs[:, 1]]) and (desc_after[:n_new] != g(before["desc"])[:n_new]).any()
    assert not desc_after[n_new:].any()
    assert np.array_equal(g(results["fuse_after"]), g(results["fuse_before"])) and int(results["fuse_before"][0]) > 50
    for key in q_before:
        assert g(fuse[key]).tobytes() == g(q_before[key]).tobytes(), key
