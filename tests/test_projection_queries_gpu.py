"""The projection-search query builders on the MI355X (include/orbm.h: orbm_project_{frame,frustum,fuse}_device; include/orbba.h:
orbba_pose_drop_outliers_device) against the numpy float32 model of tests/projection_model.py, then chained with the searches
and poseOptimize the way Tracking.cpp:284-314, :386-427 uses them."""
import numpy as np
import pytest

import projection_model as pm
from monoorbslam3_amd import synth

pytestmark = pytest.mark.gpu

FORMS = [pm.FRAME, pm.FRUSTUM, pm.FUSE]
IMG_CODE = {pm.FRAME: 3, pm.FRUSTUM: 4, pm.FUSE: 3}


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


def _device_inputs(torch, dev, cloud):
    n = cloud["n"]
    d = dict(pose_R=_up(torch, dev, np.asarray(cloud["R"], np.float64).reshape(9)), pose_t=_up(torch, dev, np.asarray(cloud["t"], np.float64)),
             points=_up(torch, dev, cloud["points"]), valid=_up(torch, dev, cloud["valid"]))
    for k in ("kps1", "normals", "min_dist", "max_dist", "frame_mp"):
        if k in cloud:
            d[k] = _up(torch, dev, cloud[k])
    # outputs start as garbage: the call must write every entry
    d.update(q_xy=torch.full((n, 2), 7.5, dtype=torch.float32, device=dev), q_radius=torch.full((n,), 7.5, dtype=torch.float32, device=dev),
             q_level=torch.full((n,), 77, dtype=torch.int32, device=dev), q_angle=torch.full((n,), 7.5, dtype=torch.float32, device=dev),
             q_ok=torch.full((n,), 7, dtype=torch.uint8, device=dev), view_cos=torch.full((n,), 7.5, dtype=torch.float32, device=dev),
             result=torch.full((8,), 77, dtype=torch.int32, device=dev))
    return d


def _build(m, cam, form, d, cloud, stream=None):
    n = cloud["n"]
    if form == pm.FRAME:
        m.ProjectFrameDevice(cam, d, n, cloud["th"], stream=stream)
    elif form == pm.FRUSTUM:
        m.ProjectFrustumDevice(cam, d, n, cloud["n2"], pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), cloud["th"], cloud["view_cos_limit"],
                               stream=stream)
    else:
        m.ProjectFuseDevice(cam, d, n, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), cloud["th"], stream=stream)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


CLOUDS = [(pm.FRAME, False, 5000, 11), (pm.FRAME, True, 4000, 12), (pm.FRUSTUM, False, 8000, 13), (pm.FRUSTUM, True, 6000, 14),
          (pm.FUSE, False, 6000, 15), (pm.FUSE, True, 3000, 16)]


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("form,fisheye,n,seed", CLOUDS)
def test_builder_against_the_model(form, fisheye, n, seed, stream_kind):
    """Pinhole: q_ok, q_xy, q_radius, q_octave, q_angle, view_cos and every counter equal the float32 model bit for bit; q_level (and
    the radius that goes with it) outside the points whose x = log(max_dist / dist) / log_scale_factor lies within 1e-4 of an
    integer in float64 -- there the level may differ by one and the radius is the returned level's.  Fisheye: q_xy passes through
    atanf, so the yardstick is float64 and the device's largest deviation may be at most twice the model's own; points whose
    in-image decision flips between the model and float64 are excluded (at most 0.5 % with the level exclusion)."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    cloud = pm.make_cloud(form, fisheye, n, seed)
    e32, e64 = pm.run_model(cloud), pm.run_model(cloud, np.float64)
    near = pm.near_threshold(form, cloud, e64)
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    d = _device_inputs(torch, dev, cloud)
    m = ORBMatcher()
    st = _stream(torch, dev, stream_kind)
    _build(m, cam, form, d, cloud, st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    got = {k: d[k].cpu().numpy() for k in ("q_ok", "q_xy", "q_radius", "q_level", "q_angle", "view_cos", "result")}
    res = got["result"]
    print("%s %s n=%d device result %s model %s" % (form, "fisheye" if fisheye else "pinhole", n, res.tolist(), e32["result"].tolist()))
    n_gates = {pm.FRAME: 3, pm.FRUSTUM: 6, pm.FUSE: 5}[form]
    assert e32["result"][0] >= 0.30 * n and (e32["result"][1:1 + n_gates] >= 0.02 * n).all()
    assert cloud["on_bound"].sum() >= 2
    excluded = np.zeros(n, bool)
    if fisheye:
        excluded = (e32["code"] == IMG_CODE[form]) != (e64["code"] == IMG_CODE[form])
    level_free = near["level"] if form != pm.FRAME else np.zeros(n, bool)
    assert (excluded | level_free).mean() <= 0.005
    keep = ~excluded
    assert np.array_equal(got["q_ok"][keep], e32["q_ok"][keep])
    if not excluded.any():
        assert np.array_equal(res, e32["result"])
    else:
        assert np.abs(res.astype(np.int64) - e32["result"]).max() <= excluded.sum() and res[:1 + n_gates].sum() == n
    if form == pm.FRUSTUM:
        assert res[7] == res[3:7].sum()
    on = keep & (e32["q_ok"] == 1)
    off = got["q_ok"] == 0
    for k in ("q_xy", "q_radius", "q_level", "q_angle", "view_cos"):      # a query that is off holds zeros
        if not (form != pm.FRAME and k == "q_angle") and not (form != pm.FRUSTUM and k == "view_cos"):
            assert not got[k][off].any(), k
    if fisheye:
        dev_err = np.abs(got["q_xy"][on].astype(np.float64) - e64["q_xy"][on]).max()
        mod_err = np.abs(e32["q_xy"][on].astype(np.float64) - e64["q_xy"][on]).max()
        print("fisheye q_xy: largest deviation from float64: device %.3e px, numpy float32 model %.3e px" % (dev_err, mod_err))
        assert dev_err <= 2 * mod_err
    else:
        assert np.array_equal(_bits(got["q_xy"][on]), _bits(e32["q_xy"][on]))
    if form == pm.FRAME:
        assert np.array_equal(got["q_level"][on], e32["q_level"][on])
        assert np.array_equal(_bits(got["q_angle"][on]), _bits(e32["q_angle"][on]))
        assert np.array_equal(_bits(got["q_radius"][on]), _bits(e32["q_radius"][on]))
    else:
        strict = on & ~level_free
        assert np.array_equal(got["q_level"][strict], e32["q_level"][strict])
        assert np.array_equal(_bits(got["q_radius"][strict]), _bits(e32["q_radius"][strict]))
        loose = on & level_free
        assert (np.abs(got["q_level"][loose] - e32["q_level"][loose]) <= 1).all()
        want = (e32["th_c"][loose] * pm.SCALE_FACTORS[got["q_level"][loose]]).astype(np.float32)
        assert np.array_equal(_bits(got["q_radius"][loose]), _bits(want))
        if form == pm.FRUSTUM:
            assert np.array_equal(_bits(got["view_cos"][on]), _bits(e32["view_cos"][on]))
            assert (e32["view_cos"][on] > 0.998).any() and (e32["view_cos"][on] <= 0.998).any()   # both radius classes


def test_division_and_square_root_are_correctly_rounded():
    """Operands whose float quotient / root differ in the last bit between the correctly rounded evaluation and a reciprocal-based
    one (x * (1 / z); s * (1 / sqrt(s))): the device returns the correctly rounded bits.  The quotient is read from q_xy of a
    Pinhole camera with fx = 1, cx = 0 under the identity pose (u = 1 * (X / Z) + 0); the root from view_cos = z / sqrt(x^2 + z^2)
    with a normal along z and integer coordinates (the sum of squares is exact)."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(5)
    f32 = np.float32
    x = rng.uniform(0.1, 0.9, 4000).astype(f32)
    z = rng.uniform(1.0, 2.0, 4000).astype(f32)
    pick = np.flatnonzero((x / z) != x * (f32(1) / z))[:200]
    assert len(pick) == 200
    xi = rng.randint(1, 400, 4000).astype(f32)
    zi = rng.randint(400, 2000, 4000).astype(f32)
    s = xi * xi + zi * zi                       # exact: below 2^24
    root = np.sqrt(s)
    fast = s * (f32(1) / root)                  # a reciprocal-square-root style evaluation
    pick2 = np.flatnonzero((fast != root) & ((zi / root) != (zi / fast)))[:200]
    assert len(pick2) == 200
    P = np.concatenate([np.stack([x[pick], np.zeros(200, f32), z[pick]], 1), np.stack([xi[pick2], np.zeros(200, f32), zi[pick2]], 1)])
    n = len(P)
    cloud = dict(form=pm.FRUSTUM, cam=(1.0, 1.0, 0.0, 0.0), bounds=(-10.0, 10.0, -10.0, 10.0), R=np.eye(3), t=np.zeros(3), points=P,
                 valid=np.ones(n, np.uint8), normals=np.tile(np.array([0, 0, 1], f32), (n, 1)), min_dist=np.zeros(n, f32),
                 max_dist=np.full(n, 1e6, f32), frame_mp=np.full(4, -1, np.int32), n2=4, th=1.0, view_cos_limit=-1.0, n=n)
    e32 = pm.run_model(cloud)
    assert (e32["q_ok"] == 1).all()
    assert np.array_equal(_bits(e32["q_xy"][:200, 0]), _bits(x[pick] / z[pick]))
    assert np.array_equal(_bits(e32["view_cos"][200:]), _bits(zi[pick2] / root[pick2]))
    d = _device_inputs(torch, dev, cloud)
    _build(ORBMatcher(), ProjCamera.make(cloud["cam"], cloud["bounds"]), pm.FRUSTUM, d, cloud)
    torch.cuda.synchronize()
    assert d["q_ok"].cpu().numpy().all()
    assert np.array_equal(_bits(d["q_xy"].cpu().numpy()), _bits(e32["q_xy"]))
    assert np.array_equal(_bits(d["view_cos"].cpu().numpy()), _bits(e32["view_cos"]))


def test_drop_outliers_alone():
    """Exactly the outliers' slots become -1, nothing else changes, edges past edge_off[1] are ignored (Optimize.cpp:531-537)."""
    import torch
    from monoorbslam3_amd import ba
    dev = torch.device("cuda", 0)
    rng = np.random.RandomState(3)
    n2, ne, ne_cap = 3000, 1100, 1500
    frame_mp = rng.randint(-1, 900, n2).astype(np.int32)
    edge_kp = rng.choice(n2, ne_cap, replace=False).astype(np.int32)
    inlier = (rng.uniform(size=ne_cap) > 0.3).astype(np.uint8)
    inlier[ne:] = 0                                            # past the edge count: must be ignored
    want = frame_mp.copy()
    want[edge_kp[:ne][inlier[:ne] == 0]] = -1
    t = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    d_mp, d_kp, d_in = t(frame_mp), t(edge_kp), t(inlier)
    for st_kind in ("null", "explicit"):
        d_mp.copy_(t(frame_mp))
        st = _stream(torch, dev, st_kind)
        ba.pose_drop_outliers_device(n2, t(np.array([0, ne], np.int32)), d_kp, d_in, d_mp, stream=st)
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        assert np.array_equal(d_mp.cpu().numpy(), want)
        assert np.array_equal(d_kp.cpu().numpy(), edge_kp) and np.array_equal(d_in.cpu().numpy(), inlier)
    assert (want != frame_mp).sum() > 100


def test_the_new_kernels_use_no_scratch_memory():
    """read from the gfx950 ISA under build/isa, by the method of tests/test_kernel_resources.py"""
    from resource_checks import _isa, _kernels
    k = _kernels(_isa("orbm_project"))
    proj = {name: v for name, v in k.items() if "k_project" in name}
    assert len(proj) == 3, sorted(k)
    for name, (vgpr, scratch, lds) in proj.items():
        print(name, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0 and vgpr <= 128, name         # 1024 threads: 128 VGPRs is all a thread can have
    drop = [v for name, v in _kernels(_isa("orbba")).items() if "k_pose_drop_outliers" in name]
    assert len(drop) == 1 and drop[0][1] == 0


# ---- builder -> search against host-built queries -> host search --------------------------------------------------------------
def _scene(seed, dx, dy, nf=1500):
    """two crops of one canvas: a fronto-parallel plane at Z = 10 m seen by a camera that translates (tests/test_tracking_flow_gpu.py)"""
    from monoorbslam3_amd.extractor import ORBExtractor
    from monoorbslam3_amd.frame import FramePost
    w, h, Z = 752, 480, 10.0
    fx = fy = 460.0
    cx, cy = 376.0, 240.0
    canvas = synth.make_canvas(w + 80, h + 60, seed=seed)
    f1 = np.ascontiguousarray(canvas[30:30 + h, 40:40 + w])
    f2 = np.ascontiguousarray(canvas[30 + dy:30 + dy + h, 40 + dx:40 + dx + w])
    ex = ORBExtractor(nf, 1.2, 8, 20, 7, max_width=w, max_height=h)
    post = FramePost(w, h, fx, fy, cx, cy)
    k1, d1 = ex(f1)
    _, k1u, _, _ = post(k1)
    nq = len(k1u)
    Pw = np.stack([(k1u["x"] - cx) * Z / fx, (k1u["y"] - cy) * Z / fy, np.full(nq, Z)], 1).astype(np.float32)
    d0 = np.linalg.norm(Pw.astype(np.float64), axis=1)
    normals = (Pw.astype(np.float64) / d0[:, None]).astype(np.float32)     # mean viewing direction = the ray of view 1 (camera 1 = world)
    max_dist = (d0 * 1.2 ** (k1u["octave"] - 0.3)).astype(np.float32)      # predictScaleLevel gives the octave back
    min_dist = (0.3 * d0).astype(np.float32)
    t_true = np.array([-dx * Z / fx, -dy * Z / fy, 0.0])
    return dict(w=w, h=h, cam=(fx, fy, cx, cy), bounds=(0.0, float(w), 0.0, float(h)), f2=f2, ex=ex, post=post, k1u=k1u, d1=d1, nq=nq,
                points=Pw, normals=normals, max_dist=max_dist, min_dist=min_dist, t_true=t_true, valid=np.ones(nq, np.uint8))


def _frame_record(torch, dev, sc, stream=None):
    """view 2 extracted and post-processed on the device: (kps undistorted, desc, count, cell_start, cell_items, capacity)"""
    ex, post, w, h = sc["ex"], sc["post"], sc["w"], sc["h"]
    capk = ex.max_keypoints(w, h)
    img = torch.from_numpy(np.ascontiguousarray(sc["f2"][None])).to(dev)
    d_kp = torch.zeros((1, capk, 28), dtype=torch.uint8, device=dev)
    d_un = torch.zeros((1, capk, 28), dtype=torch.uint8, device=dev)
    d_desc = torch.zeros((1, capk, 32), dtype=torch.uint8, device=dev)
    d_n = torch.zeros((1,), dtype=torch.int32, device=dev)
    d_start = torch.zeros((1, post.n_cells + 1), dtype=torch.int32, device=dev)
    d_items = torch.zeros((1, capk), dtype=torch.int32, device=dev)
    ex.extract_batch_device(img.data_ptr(), 1, w, h, w, w * h, d_kp.data_ptr(), d_desc.data_ptr(), capk, d_n.data_ptr(), stream)
    post.post_device(1, d_kp.data_ptr(), d_n.data_ptr(), capk, d_un.data_ptr(), d_start.data_ptr(), d_items.data_ptr(), stream)
    return dict(kps2=d_un, desc2=d_desc, n=d_n, cell_start=d_start, cell_items=d_items, capk=capk, img=img, kp_raw=d_kp)


def _scene_cloud(sc, form, R, t, th, frame_mp=None):
    c = dict(form=form, cam=sc["cam"], bounds=sc["bounds"], R=R, t=t, points=sc["points"], valid=sc["valid"], th=th, view_cos_limit=0.5,
             n=sc["nq"])
    if form == pm.FRAME:
        c["kps1"] = sc["k1u"]
    else:
        c.update(normals=sc["normals"], min_dist=sc["min_dist"], max_dist=sc["max_dist"])
    if form == pm.FRUSTUM:
        c.update(frame_mp=frame_mp, n2=len(frame_mp))
    return c


@pytest.mark.parametrize("form", FORMS)
def test_builder_then_search_equals_host_built_queries_then_host_search(form):
    import torch
    from monoorbslam3_amd.extractor import KP_DTYPE
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    sc = _scene(4242, 8, 5)
    rec = _frame_record(torch, dev, sc)
    capk, nq, post = rec["capk"], sc["nq"], sc["post"]
    R = pm._rodrigues(np.array([0.002, -0.003, 0.001]))
    t = sc["t_true"] + np.array([0.004, -0.003, 0.01])
    rng = np.random.RandomState(9)
    mp0 = np.full(capk, -1, np.int32)
    if form == pm.FRUSTUM:
        mp0[rng.choice(capk, 150, replace=False)] = rng.choice(nq, 150, replace=False)     # already matched map points
    th = {pm.FRAME: 7.0, pm.FRUSTUM: 3.0, pm.FUSE: 3.0}[form]
    cloud = _scene_cloud(sc, form, R, t, th, mp0)
    e32 = pm.run_model(cloud)
    cam = ProjCamera.make(sc["cam"], sc["bounds"])
    d = _device_inputs(torch, dev, cloud)
    sigma2 = (pm.SCALE_FACTORS * pm.SCALE_FACTORS).astype(np.float32)
    d.update(q_desc=_up(torch, dev, sc["d1"]), kps2=rec["kps2"], desc2=rec["desc2"], kps=rec["kps2"], desc=rec["desc2"],
             cell_start=rec["cell_start"], cell_items=rec["cell_items"], sigma2=_up(torch, dev, sigma2),
             best_idx=torch.full((nq,), 9, dtype=torch.int32, device=dev), best_dist=torch.full((nq,), 9, dtype=torch.int32, device=dev))
    if form != pm.FRUSTUM:
        d["frame_mp"] = _up(torch, dev, mp0)
    m = ORBMatcher(0.8, True)
    _build(m, cam, form, d, cloud)
    search = dict(d, result=torch.zeros(8, dtype=torch.int32, device=dev))
    if form == pm.FUSE:
        m.SearchFuseDevice(search, nq, post.cols, post.rows, list_cap=64)
    else:
        m.SearchByProjectionDevice("frame" if form == pm.FRAME else "points", search, nq, capk, post.cols, post.rows, list_cap=64)
    torch.cuda.synchronize()
    for k in ("q_ok", "q_xy", "q_radius", "q_level"):
        assert np.array_equal(_bits(d[k].cpu().numpy()), _bits(e32[k])), k
    n2 = int(rec["n"][0])
    k2u = np.frombuffer(rec["kps2"][0, :n2].cpu().numpy().tobytes(), KP_DTYPE)
    d2 = rec["desc2"][0, :n2].cpu().numpy()
    res = search["result"].cpu().numpy()
    w, h = sc["w"], sc["h"]
    if form == pm.FRAME:
        n_host, mp = m.SearchByProjectionFrame(sc["d1"], e32["q_xy"], e32["q_radius"], e32["q_level"], e32["q_angle"], e32["q_ok"], k2u, d2,
                                               w, h, mp0[:n2])
    elif form == pm.FRUSTUM:
        n_host, mp, cnt = m.SearchByProjectionPoints(sc["d1"], e32["q_xy"], e32["q_radius"], e32["q_level"], e32["q_ok"], k2u, d2, w, h,
                                                     mp0[:n2])
        assert res[4:7].tolist() == list(cnt)
    else:
        bi, bd, n_host = m.SearchFuse(sc["d1"], e32["q_xy"], e32["q_radius"], e32["q_level"], e32["q_ok"], k2u, d2, w, h, sigma2)
        assert np.array_equal(search["best_idx"].cpu().numpy(), bi) and np.array_equal(search["best_dist"].cpu().numpy(), bd)
    print("%s: builder result %s, search result %s, host matches %d" % (form, d["result"].cpu().numpy().tolist(), res.tolist(), n_host))
    assert res[1] == 0 and res[0] == n_host and n_host > 200
    if form != pm.FUSE:
        got = search["frame_mp"].cpu().numpy()
        assert np.array_equal(got[:n2], mp) and np.array_equal(got[n2:], mp0[n2:])


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_two_stage_track_with_one_wait(stream_kind):
    """Tracking.cpp:284-314 then :386-427 on ONE stream with the first and only wait at the end: extract -> frame post ->
    ProjectFrameDevice (identity prediction, th 15) -> frame search -> pose edges -> poseOptimize -> drop outliers ->
    ProjectFrustumDevice reading the pose the optimiser just wrote (th 1, limit 0.5) -> points search in the shared index space ->
    pose edges -> poseOptimize.  Everything equals the same sequence stage by stage through the host entry points with the
    model's queries; the final translation meets the ground-truth bound of test_tracking_chain_stays_on_the_device."""
    import torch
    from monoorbslam3_amd import ba
    from monoorbslam3_amd.extractor import KP_DTYPE
    from monoorbslam3_amd.matcher import ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    sc = _scene(2024, 9, 6)
    nq, post, w, h, camt = sc["nq"], sc["post"], sc["w"], sc["h"], sc["cam"]
    cam = ProjCamera.make(camt, sc["bounds"])
    t_ = lambda a: _up(torch, dev, a)  # noqa: E731
    capk = sc["ex"].max_keypoints(w, h)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table = dict(points=t_(sc["points"]), valid=t_(sc["valid"]), kps1=t_(sc["k1u"]), normals=t_(sc["normals"]), min_dist=t_(sc["min_dist"]),
                 max_dist=t_(sc["max_dist"]), q_desc=t_(sc["d1"]))
    frame_mp = torch.full((capk,), -1, dtype=torch.int32, device=dev)
    R0, t0 = t_(np.eye(3).reshape(1, 9)), t_(np.zeros((1, 3)))
    outs = [dict(q_xy=z((nq, 2), torch.float32), q_radius=z((nq,), torch.float32), q_level=z((nq,), torch.int32), q_angle=z((nq,), torch.float32),
                 q_ok=z((nq,), torch.uint8), view_cos=z((nq,), torch.float32), result=z((8,), torch.int32), s_result=z((8,), torch.int32),
                 e_off=z((2,), torch.int32), e_P=z((capk, 3), torch.float64), e_z=z((capk, 2), torch.float64), e_w=z((capk,), torch.float64),
                 e_kp=z((capk,), torch.int32), R=z((1, 9), torch.float64), t=z((1, 3), torch.float64), inl=z((capk,), torch.uint8),
                 n_inl=z((1,), torch.int32), chi2=z((capk,), torch.float64), mp=None) for _ in range(2)]
    m = ORBMatcher(0.8, True)
    st = _stream(torch, dev, stream_kind)
    rec = _frame_record(torch, dev, sc, st)
    rec_d = dict(kps2=rec["kps2"], desc2=rec["desc2"], cell_start=rec["cell_start"], cell_items=rec["cell_items"], frame_mp=frame_mp)
    # stage 1
    o = outs[0]
    d1 = dict(table, **rec_d, pose_R=R0, pose_t=t0, **{k: o[k] for k in ("q_xy", "q_radius", "q_level", "q_angle", "q_ok", "result")})
    m.ProjectFrameDevice(cam, d1, nq, 15.0, stream=st)
    m.SearchByProjectionDevice("frame", dict(d1, result=o["s_result"]), nq, capk, post.cols, post.rows, list_cap=192, stream=st)
    ba.pose_edges_device(capk, nq, frame_mp, rec["kps2"], table["points"], o["e_off"], o["e_P"], o["e_z"], o["e_w"], o["e_kp"], stream=st)
    ba.pose_optimize_batch_device(camt, R0, t0, o["e_off"], o["e_P"], o["e_z"], o["e_w"], o["R"], o["t"], o["inl"], o["n_inl"], o["chi2"], stream=st)
    ba.pose_drop_outliers_device(capk, o["e_off"], o["e_kp"], o["inl"], frame_mp, stream=st)
    # stage 2: the queries depend on the pose stage 1 left in device memory
    p = outs[1]
    d2 = dict(table, **rec_d, pose_R=o["R"], pose_t=o["t"], **{k: p[k] for k in ("q_xy", "q_radius", "q_level", "q_ok", "view_cos", "result")})
    m.ProjectFrustumDevice(cam, d2, nq, capk, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), 1.0, 0.5, stream=st)
    m.SearchByProjectionDevice("points", dict(d2, result=p["s_result"]), nq, capk, post.cols, post.rows, list_cap=64, stream=st)
    ba.pose_edges_device(capk, nq, frame_mp, rec["kps2"], table["points"], p["e_off"], p["e_P"], p["e_z"], p["e_w"], p["e_kp"], stream=st)
    ba.pose_optimize_batch_device(camt, o["R"], o["t"], p["e_off"], p["e_P"], p["e_z"], p["e_w"], p["R"], p["t"], p["inl"], p["n_inl"], p["chi2"],
                                  stream=st)
    torch.cuda.synchronize()   # the first and only wait of the chain
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    # ---- the same, stage by stage through the host entry points
    n2 = int(rec["n"][0])
    k2u = np.frombuffer(rec["kps2"][0, :n2].cpu().numpy().tobytes(), KP_DTYPE)
    desc2 = rec["desc2"][0, :n2].cpu().numpy()
    g = lambda tns: tns.cpu().numpy()  # noqa: E731

    def edges(mp):
        idx2 = np.flatnonzero((mp >= 0) & (mp < nq))
        zz = np.stack([k2u["x"][idx2], k2u["y"][idx2]], 1).astype(np.float64)
        ww = (np.float32(1.0) / k2u["size"][idx2] / k2u["size"][idx2]).astype(np.float64)
        return idx2, sc["points"][mp[idx2]].astype(np.float64), zz, ww

    e1 = pm.run_model(_scene_cloud(sc, pm.FRAME, np.eye(3), np.zeros(3), 15.0))
    for k in ("q_ok", "q_xy", "q_radius", "q_level", "q_angle", "result"):
        assert np.array_equal(_bits(g(o[k])), _bits(e1[k])), k
    n1m, mp = m.SearchByProjectionFrame(sc["d1"], e1["q_xy"], e1["q_radius"], e1["q_level"], e1["q_angle"], e1["q_ok"], k2u, desc2, w, h,
                                        np.full(n2, -1, np.int32))
    assert int(o["s_result"][1]) == 0 and int(o["s_result"][0]) == n1m and n1m > 300
    idx2, PP, zz, ww = edges(mp)
    ne = len(idx2)
    assert int(o["e_off"][1]) == ne and np.array_equal(g(o["e_kp"])[:ne], idx2)
    ref1 = ba.pose_optimize_batch(camt, np.eye(3)[None], np.zeros((1, 3)), np.array([0, ne], np.int32), PP, zz, ww)
    assert np.array_equal(g(o["R"]).reshape(1, 3, 3), ref1["pose_R"]) and np.array_equal(g(o["t"]), ref1["pose_t"])
    assert np.array_equal(g(o["inl"])[:ne].astype(bool), ref1["inlier"]) and int(o["n_inl"][0]) == ref1["n_inliers"][0]
    mp = mp.copy()
    mp[idx2[~ref1["inlier"]]] = -1                                           # Optimize.cpp:531-537
    assert (~ref1["inlier"]).sum() > 0
    mp_full = np.concatenate([mp, np.full(capk - n2, -1, np.int32)])
    e2 = pm.run_model(_scene_cloud(sc, pm.FRUSTUM, ref1["pose_R"][0], ref1["pose_t"][0], 1.0, mp_full))
    near = pm.near_threshold(pm.FRUSTUM, _scene_cloud(sc, pm.FRUSTUM, ref1["pose_R"][0], ref1["pose_t"][0], 1.0, mp_full),
                             pm.run_model(_scene_cloud(sc, pm.FRUSTUM, ref1["pose_R"][0], ref1["pose_t"][0], 1.0, mp_full), np.float64))
    assert not near["level"][e2["q_ok"] == 1].any()      # (max_dist puts x 0.3 below an integer: no level is in doubt here)
    for k in ("q_ok", "q_xy", "q_radius", "q_level", "view_cos", "result"):
        assert np.array_equal(_bits(g(p[k])), _bits(e2[k])), k
    assert e2["result"][2] == ref1["n_inliers"][0] and e2["result"][0] > 100
    n2m, mp2, cnt = m.SearchByProjectionPoints(sc["d1"], e2["q_xy"], e2["q_radius"], e2["q_level"], e2["q_ok"], k2u, desc2, w, h, mp)
    assert int(p["s_result"][1]) == 0 and int(p["s_result"][0]) == n2m and n2m > 20
    got_mp = g(frame_mp)
    assert np.array_equal(got_mp[:n2], mp2) and np.all(got_mp[n2:] == -1)
    idx2, PP, zz, ww = edges(mp2)
    ne2 = len(idx2)
    assert int(p["e_off"][1]) == ne2 and np.array_equal(g(p["e_kp"])[:ne2], idx2)
    ref2 = ba.pose_optimize_batch(camt, ref1["pose_R"], ref1["pose_t"], np.array([0, ne2], np.int32), PP, zz, ww)
    assert np.array_equal(g(p["R"]).reshape(1, 3, 3), ref2["pose_R"]) and np.array_equal(g(p["t"]), ref2["pose_t"])
    assert np.array_equal(g(p["inl"])[:ne2].astype(bool), ref2["inlier"]) and int(p["n_inl"][0]) == ref2["n_inliers"][0]
    print("stage 1: %d matches, %d inliers; stage 2: %d queries on, %d new matches, %d edges, %d inliers; t = %s (true %s)" % (
        n1m, ref1["n_inliers"][0], e2["result"][0], n2m, ne2, ref2["n_inliers"][0], g(p["t"])[0], sc["t_true"]))
    assert np.abs(g(p["t"])[0] - sc["t_true"]).max() < 0.02
