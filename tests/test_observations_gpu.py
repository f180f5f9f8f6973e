"""orbm_build_observations_device / orbm_cull_keyframes_device on the MI355X (include/orbm.h, "Observations built and key frames
culled on the device") against the array model of tests/observations_model.py, byte for byte: integers only, so no tolerance."""
import numpy as np
import pytest

import observations_model as om
import refresh_model as rm
import triangulation_model as tm
from test_triangulation_gpu import _stream, _up

pytestmark = pytest.mark.gpu

GUARD = 16            # rows of padding around every output, compared afterwards
_build_cache, _cull_cache = {}, {}     # separate: both have a scene called "small"


def _build_scene(name):
    """(scene, model outputs): computed once, shared, never changed"""
    if name not in _build_cache:
        sc = om.make_build_scene(**om.BUILD_SCENES[name])
        _build_cache[name] = (sc, om.build(sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"], 1 << 30))
    return _build_cache[name]


def _cull_scene(key):
    if key not in _cull_cache:
        sc = om.make_small_cull_scene(5) if key == "small" else om.make_cull_scene(key)
        off, kf, kp, res = om.build(sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"], 1 << 30)
        _cull_cache[key] = (sc, off, kf, kp)
    return _cull_cache[key]


def _padded(torch, dev, a, fill):
    """a device tensor with GUARD elements of `fill` on either side of a; returns (whole, view of the middle)"""
    a = np.ascontiguousarray(a)
    whole = np.full(len(a.reshape(-1)) + 2 * GUARD, fill, a.dtype)
    whole[GUARD:-GUARD] = a.reshape(-1)
    t = torch.from_numpy(whole).to(dev)
    return t, t[GUARD:-GUARD]


def _guards_intact(t, fill):
    h = t.cpu().numpy()
    return (h[:GUARD] == fill).all() and (h[-GUARD:] == fill).all()


def _build_inputs(torch, dev, sc):
    return dict(n=_up(torch, dev, sc["n"]), bad=_up(torch, dev, sc["bad"]), slots=_up(torch, dev, sc["slots"]), valid=_up(torch, dev, sc["valid"]))


def _run_build(torch, dev, sc, cap_obs, stream_kind, d=None):
    from monoorbslam3_amd.matcher import ORBMatcher
    d = d or _build_inputs(torch, dev, sc)
    cap = sc["cap_points"]
    pads = dict(obs_off=_padded(torch, dev, np.full(cap + 1, -77, np.int32), -3), obs_kf=_padded(torch, dev, np.full(cap_obs, -78, np.int32), -4),
                obs_kp=_padded(torch, dev, np.full(cap_obs, -79, np.int32), -5), result=_padded(torch, dev, np.full(8, 77, np.int32), -6))
    d.update({k: v[1] for k, v in pads.items()})
    st = _stream(torch, dev, stream_kind)
    ORBMatcher().BuildObservationsDevice(d, len(sc["n"]), sc["stride"], cap, cap_obs, stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k, fill in (("obs_off", -3), ("obs_kf", -4), ("obs_kp", -5), ("result", -6)):
        assert _guards_intact(pads[k][0], fill), k
    return d


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("name", sorted(om.BUILD_SCENES))
def test_build_equals_the_model(name, stream_kind):
    """Offsets, the first n_obs entries of both lists and d_result byte for byte the model's -- lists of 0, 1, 2, 3, 4, 63, 64, 65,
    1024 and 1025 entries (64 | 65: one tile | tiles of the rank sort) over 1100 key frames of at most 8 slots, 3 x 64 and 12 x 256;
    bad key frames, invalid rows, -1 and out-of-range slots, rows named behind d_n[k], d_n[k] > stride and <= 0, a row twice in one
    key frame --, entries past n_obs and every input as passed, and a second run gives the same bytes."""
    import torch
    dev = torch.device("cuda", 0)
    sc, (off, kf, kp, res) = _build_scene(name)
    n_obs, cap_obs = len(kf), len(kf) + 37
    runs = [_run_build(torch, dev, sc, cap_obs, stream_kind) for _ in range(2)]
    g = lambda t: t.cpu().numpy()  # noqa: E731
    d = runs[0]
    print("%s: device d_result %s, model %s" % (name, g(d["result"]).tolist(), res.tolist()))
    assert np.array_equal(g(d["result"]), res)
    assert g(d["obs_off"]).tobytes() == off.tobytes()
    assert g(d["obs_kf"])[:n_obs].tobytes() == kf.tobytes() and g(d["obs_kp"])[:n_obs].tobytes() == kp.tobytes()
    assert (g(d["obs_kf"])[n_obs:] == -78).all() and (g(d["obs_kp"])[n_obs:] == -79).all()
    for key in ("n", "bad", "slots", "valid"):
        assert g(d[key]).tobytes() == np.ascontiguousarray(sc[key]).tobytes(), key
    for key in ("obs_off", "obs_kf", "obs_kp", "result"):
        assert g(runs[1][key]).tobytes() == g(d[key]).tobytes(), key
    lengths = (off[1:] - off[:-1])[:len(om.BUILD_SCENES[name]["lengths"])]
    assert lengths.tolist() == list(om.BUILD_SCENES[name]["lengths"]) and res[om.TWICE] == 1


def test_build_exact_fit_no_key_frames_and_the_largest_table():
    """cap_obs == n_obs is no overflow; n_kf = 0 gives all-zero offsets; cap_points at the limit of 524288 rows (the scan's longest
    chunks) with observations in its first and last rows."""
    import torch
    dev = torch.device("cuda", 0)
    g = lambda t: t.cpu().numpy()  # noqa: E731
    sc, (off, kf, kp, res) = _build_scene("small")
    d = _run_build(torch, dev, sc, len(kf), "null")
    assert np.array_equal(g(d["result"]), res) and g(d["obs_kf"]).tobytes() == kf.tobytes() and g(d["obs_kp"]).tobytes() == kp.tobytes()
    empty = dict(sc, n=np.zeros(0, np.int32), bad=np.zeros(0, np.uint8), slots=np.zeros((0, sc["stride"]), np.int32))
    d = _run_build(torch, dev, empty, 5, "null", d=dict(n=_up(torch, dev, np.zeros(1, np.int32)), bad=_up(torch, dev, np.zeros(1, np.uint8)),
                                                          slots=_up(torch, dev, np.zeros(1, np.int32)), valid=_up(torch, dev, sc["valid"])))
    assert not g(d["obs_off"]).any() and not g(d["result"]).any() and (g(d["obs_kf"]) == -78).all()
    cap = om.MAX_POINTS
    rng = np.random.RandomState(3)
    slots = rng.randint(0, cap, (4, 512)).astype(np.int32)
    slots[:, 0], slots[:, 1], slots[2, 2] = 0, cap - 1, cap
    big = dict(n=np.full(4, 512, np.int32), bad=np.zeros(4, np.uint8), slots=slots, stride=512, valid=np.ones(cap, np.uint8), cap_points=cap)
    want = om.build(big["n"], big["bad"], slots, 512, big["valid"], cap, 4096)
    d = _run_build(torch, dev, big, 4096, "null")
    assert np.array_equal(g(d["result"]), want[3]) and want[3][om.NOBS] == 4 * 512 - 1
    assert g(d["obs_off"]).tobytes() == want[0].tobytes() and want[0][1] == 4 and want[0][-1] - want[0][-2] == 4
    assert g(d["obs_kf"])[:len(want[1])].tobytes() == want[1].tobytes() and g(d["obs_kp"])[:len(want[2])].tobytes() == want[2].tobytes()


def test_build_overflow_leaves_empty_lists_and_a_refresh_behind_it_changes_nothing():
    """cap_obs = n_obs - 1: d_result[1] = 1 with the full count in [0], every offset zero, both lists untouched; an
    orbm_refresh_points_device enqueued behind it on the same stream leaves the table's bytes as they were."""
    import torch
    from monoorbslam3_amd.matcher import KfTable, ORBMatcher
    dev = torch.device("cuda", 0)
    sc, (off, kf, kp, res) = _build_scene("mid")
    n_obs = len(kf)
    want = om.build(sc["n"], sc["bad"], sc["slots"], sc["stride"], sc["valid"], sc["cap_points"], n_obs - 1)
    assert want[3][om.OVERFLOW] == 1 and want[3][om.NOBS] == n_obs and not want[0].any()
    rs = rm.make_scene(41, n_kf=len(sc["n"]), n_rows=sc["cap_points"], lengths=(), spare_rows=0)      # a table and key frames to refresh
    d = _build_inputs(torch, dev, sc)
    cap = sc["cap_points"]
    d.update(obs_off=torch.full((cap + 1,), -77, dtype=torch.int32, device=dev), obs_kf=torch.full((n_obs - 1,), -78, dtype=torch.int32, device=dev),
             obs_kp=torch.full((n_obs - 1,), -79, dtype=torch.int32, device=dev), result=torch.full((8,), 77, dtype=torch.int32, device=dev))
    table = {k: _up(torch, dev, rs[k]) for k in ("points", "normals", "min_dist", "max_dist", "desc", "ref_kf")}
    kft = KfTable.make(_up(torch, dev, rs["pose_R"]), _up(torch, dev, rs["pose_t"]), d["bad"], [_up(torch, dev, k) for k in rs["kps"]],
                       [_up(torch, dev, x) for x in rs["kf_desc"]], _up(torch, dev, rs["n"]))
    ref = dict(table, valid=d["valid"], sel=torch.arange(cap, dtype=torch.int32, device=dev), obs_off=d["obs_off"], obs_kf=d["obs_kf"],
               obs_kp=d["obs_kp"], result=torch.full((8,), 77, dtype=torch.int32, device=dev))
    m = ORBMatcher()
    m.BuildObservationsDevice(d, len(sc["n"]), sc["stride"], cap, n_obs - 1)
    m.RefreshPointsDevice(kft, ref, cap, cap, n_obs - 1, float(rm.MAX_SCALE_FACTOR))
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy()  # noqa: E731
    assert np.array_equal(g(d["result"]), want[3])
    assert not g(d["obs_off"]).any() and (g(d["obs_kf"]) == -78).all() and (g(d["obs_kp"]) == -79).all()
    n_valid = int((sc["valid"][:cap] != 0).sum())
    assert g(ref["result"]).tolist() == [0, cap - n_valid, n_valid, 0, 0, 0, 0, 0]      # every valid row: no usable observation
    for key in ("points", "normals", "min_dist", "max_dist", "desc"):
        assert g(table[key]).tobytes() == np.ascontiguousarray(rs[key]).tobytes(), key


def _run_cull(torch, dev, sc, off, kf, kp, stream_kind, th_obs=om.TH_OBS):
    from monoorbslam3_amd.matcher import KfTable, ORBMatcher
    n_kf, nr = len(sc["n"]), len(sc["recent"])
    z = torch.zeros(1, dtype=torch.float64, device=dev)
    fills = dict(bad=201, slots=-31, valid=202, ref_kf=-32, code=-33, num_mp=-34, num_redundant=-35, result=-36, obs_off=-37, obs_kf=-38, obs_kp=-39)
    start = dict(bad=sc["bad"], slots=sc["slots"], valid=sc["valid"], ref_kf=sc["ref_kf"], code=np.full(nr, 55, np.int32),
                 num_mp=np.full(nr, 56, np.int32), num_redundant=np.full(nr, 57, np.int32), result=np.full(8, 58, np.int32), obs_off=off,
                 obs_kf=kf, obs_kp=kp)
    pads = {k: _padded(torch, dev, start[k], fills[k]) for k in fills}
    d = {k: v[1] for k, v in pads.items()}
    table = KfTable.make(z, z, d["bad"], [_up(torch, dev, k) for k in sc["kps"]], torch.zeros(n_kf, dtype=torch.int64, device=dev),
                         _up(torch, dev, sc["n"]))
    st = _stream(torch, dev, stream_kind)
    ORBMatcher().CullKeyFramesDevice(table, d, sc["stride"], sc["cap_points"], len(kf), sc["recent"], sc["timestamps"], first_kf=sc["first_kf"],
                                     th_obs=th_obs, stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k in fills:
        assert _guards_intact(pads[k][0], fills[k]), k
    return {k: v.cpu().numpy() for k, v in d.items()}


def _check_cull(got, want, sc, off, kf, kp):
    print("device d_result %s, model %s; d_code %s" % (got["result"].tolist(), want["result"].tolist(), got["code"].tolist()))
    for key in ("result", "code", "num_mp", "num_redundant", "bad", "valid", "ref_kf"):
        assert got[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), key
    assert got["slots"].tobytes() == np.ascontiguousarray(want["slots"]).tobytes()
    assert got["obs_off"].tobytes() == off.tobytes() and got["obs_kf"].tobytes() == kf.tobytes() and got["obs_kp"].tobytes() == kp.tobytes()


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("seed", [21, 22])
def test_cull_equals_the_model(seed, stream_kind):
    """12 key frames x 256 slots: codes 1, 3, 3, 0, 0, 0, 2, 2 in one call; the first cull sets two points bad and clears their slots
    in the next candidate, which is culled only because of that (18 of 18 instead of 18 of 20); d_ref_kf reassigned to the first
    live entry in CSR order; numMP == 0; the boundary 9 == 0.9 * 10 kept; a row named by two slots of the culled key frame; a key
    frame that was bad before.  Every in / out array and every output byte for byte, the CSR unchanged, guard rows intact."""
    import torch
    dev = torch.device("cuda", 0)
    sc, off, kf, kp = _cull_scene(seed)
    trace = []
    want = om.cull(sc, off, kf, kp, trace=trace)
    om.check_cull_scene(sc, want, trace)
    _check_cull(_run_cull(torch, dev, sc, off, kf, kp, stream_kind), want, sc, off, kf, kp)


@pytest.mark.parametrize("th_obs", [3, 2])
def test_cull_smallest_shape(th_obs):
    """3 key frames x 64 slots, 200 rows, one candidate: kept with th_obs = 3, culled with th_obs = 2, which sets all 40 points bad
    and clears 80 slots in the two other key frames."""
    import torch
    dev = torch.device("cuda", 0)
    sc, off, kf, kp = _cull_scene("small")
    want = om.cull(sc, off, kf, kp, th_obs=th_obs)
    assert want["code"].tolist() == [-1, 0 if th_obs == 3 else 3, -1] and want["result"][om.POINTS_BAD] == (0 if th_obs == 3 else 40)
    _check_cull(_run_cull(torch, dev, sc, off, kf, kp, "null", th_obs=th_obs), want, sc, off, kf, kp)


def test_cull_at_the_largest_table():
    """cap_points = 524288: the claim mask takes the whole 64 KB of dynamic LDS; rows at both ends of the table are cascaded."""
    import torch
    dev = torch.device("cuda", 0)
    small = _cull_scene("small")[0]
    cap = om.MAX_POINTS
    slots = small["slots"].copy()
    slots[slots == 5], slots[slots == 6] = 0, cap - 1
    sc = dict(small, cap_points=cap, slots=slots, valid=np.ones(cap + 4, np.uint8), ref_kf=np.zeros(cap + 4, np.int32))
    off, kf, kp, _ = om.build(sc["n"], sc["bad"], slots, sc["stride"], sc["valid"], cap, 1 << 30)
    want = om.cull(sc, off, kf, kp, th_obs=2)
    assert want["result"][om.POINTS_BAD] == 40 and not want["valid"][0] and not want["valid"][cap - 1] and want["result"][om.REASSIGNED] == 40
    _check_cull(_run_cull(torch, dev, sc, off, kf, kp, "null", th_obs=2), want, sc, off, kf, kp)


def test_rebuild_after_a_cull_gives_the_observation_sets_of_the_objects():
    """The doctrine's consistency check: build -> cull -> build on the device; the second CSR is exactly the observation lists the
    object restatement is left with after its KeyFrameCulling."""
    import torch
    from monoorbslam3_amd.matcher import ORBMatcher
    dev = torch.device("cuda", 0)
    sc, off, kf, kp = _cull_scene(23)
    got = _run_cull(torch, dev, sc, off, kf, kp, "null")
    obj = om.cull_objects(sc)
    cap = sc["cap_points"]
    d = dict(n=_up(torch, dev, sc["n"]), bad=_up(torch, dev, got["bad"]), slots=_up(torch, dev, got["slots"]), valid=_up(torch, dev, got["valid"]),
             obs_off=torch.zeros(cap + 1, dtype=torch.int32, device=dev), obs_kf=torch.zeros(len(kf), dtype=torch.int32, device=dev),
             obs_kp=torch.zeros(len(kf), dtype=torch.int32, device=dev), result=torch.zeros(8, dtype=torch.int32, device=dev))
    ORBMatcher().BuildObservationsDevice(d, len(sc["n"]), sc["stride"], cap, len(kf))
    torch.cuda.synchronize()
    g = lambda t: t.cpu().numpy()  # noqa: E731
    n_obs = int(g(d["result"])[0])
    assert 0 < n_obs < len(kf) and g(d["result"])[1] == 0
    assert om.lists_of(g(d["obs_off"]), g(d["obs_kf"])[:n_obs], g(d["obs_kp"])[:n_obs]) == obj["lists"]


def test_cull_distrusts_the_csr():
    """Negative, descending and past-the-end offsets give empty lists; entries with a key frame or a feature out of range are dropped
    and counted once each in d_result[6], never dereferenced; nothing outside the documented arrays is written."""
    import torch
    dev = torch.device("cuda", 0)
    sc, off, kf, kp = _cull_scene(21)
    rng = np.random.RandomState(9)
    off, kf, kp = off.copy(), kf.copy(), kp.copy()
    n_kf = len(sc["n"])
    first = 72                                                            # the engineered rows stay whole: both culls still happen
    hit = off[first] + rng.permutation(len(kf) - off[first])[:200]
    kf[hit[:50]], kf[hit[50:100]] = n_kf + rng.randint(0, 1000, 50), -1 - rng.randint(0, 1000, 50)
    kp[hit[100:150]] = -1 - rng.randint(0, 9, 50)
    kp[hit[150:]] = np.minimum(sc["n"][kf[hit[150:]]], sc["stride"]) + rng.randint(0, 2, 50) * 100000
    rows = first + 1 + rng.permutation(sc["n_rows"] - first - 1)[:30]
    off[rows[:10]] = -5                                                   # row p - 1 ends below its start, row p starts below 0
    off[rows[10:20]] += 40                                                # descending further on
    off[rows[20:]] = len(kf) + 7                                          # past the end
    want = om.cull(sc, off, kf, kp)
    assert want["result"][om.DROPPED] == 200 and want["result"][om.CULLED] == 2 and want["result"][om.KEPT] == 3
    assert (want["num_mp"] != om.cull(sc, *_cull_scene(21)[1:])["num_mp"]).sum() == 0 and want["result"][om.REASSIGNED] > 0
    _check_cull(_run_cull(torch, dev, sc, off, kf, kp, "explicit"), want, sc, off, kf, kp)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_mapper_chain_with_one_wait(stream_kind):
    """orbm_triangulate_matches_device on two key-frame pairs (0, 2) and (1, 2) -- two older key frames that share the matches of
    the current one between them -> orbm_build_observations_device -> orbm_refresh_points_device on the current key frame's slots ->
    orbm_cull_keyframes_device, on one stream with ONE wait at the end.  Then the same sequence with the MODEL's CSR (built on the
    host from the slots the triangulations leave) uploaded in place of the built one: the CSR, the refreshed table and everything
    the cull writes are byte for byte the same."""
    import torch
    from monoorbslam3_amd.matcher import KfTable, ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    cloud = tm.make_cloud(False, 400, 7)
    n_kf, cap_points, cap_obs = 3, 1000, 2500
    n1, n2 = cloud["n1"], cloud["n2"]
    stride = max(n1, n2)
    cam = ProjCamera.make(cloud["cam"], cloud["bounds"])
    m = ORBMatcher()
    rng = np.random.RandomState(70)
    desc1 = rng.randint(0, 256, (n1, 32)).astype(np.uint8)
    share = [np.where(np.arange(n1) % 2 == 0, cloud["matches12"], -1).astype(np.int32),
             np.where(np.arange(n1) % 2 == 1, cloud["matches12"], -1).astype(np.int32)]
    n_host = np.array([n1, n1, n2], np.int32)

    def run(model_csr):
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
        table = dict(n_points=z((1,), torch.int32), points=z((cap_points, 3), torch.float32), valid=z((cap_points,), torch.uint8),
                     normals=z((cap_points, 3), torch.float32), min_dist=z((cap_points,), torch.float32), max_dist=z((cap_points,), torch.float32),
                     desc=z((cap_points, 32), torch.uint8), obs=z((cap_points, 2), torch.int32))
        slots = torch.full((n_kf, stride), -1, dtype=torch.int32, device=dev)
        has_mp = z((n_kf, stride), torch.uint8)
        kps = [_up(torch, dev, cloud["kps1"]), _up(torch, dev, cloud["kps1"]), _up(torch, dev, cloud["kps2"])]
        descs = [_up(torch, dev, desc1), _up(torch, dev, desc1), _up(torch, dev, cloud["desc2"])]
        pose_R = _up(torch, dev, np.stack([np.asarray(cloud[k], np.float64).reshape(9) for k in ("R1", "R1", "R2")]))
        pose_t = _up(torch, dev, np.stack([np.asarray(cloud[k], np.float64) for k in ("t1", "t1", "t2")]))
        n, bad = _up(torch, dev, n_host), z((n_kf,), torch.uint8)
        kft = KfTable.make(pose_R, pose_t, bad, kps, descs, n)
        res = {k: torch.full((8,), 77, dtype=torch.int32, device=dev) for k in ("tri0", "tri1", "build", "refresh", "cull")}
        matches = [_up(torch, dev, a) for a in share]
        csr = dict(obs_off=z((cap_points + 1,), torch.int32), obs_kf=z((cap_obs,), torch.int32), obs_kp=z((cap_obs,), torch.int32))
        up_csr = None if model_csr is None else [torch.from_numpy(a).to(dev) for a in model_csr]
        ref_kf = torch.full((cap_points,), 2, dtype=torch.int32, device=dev)
        covis, code, num_mp, num_red = z((n_kf,), torch.int32), z((3,), torch.int32), z((3,), torch.int32), z((3,), torch.int32)
        st = _stream(torch, dev, stream_kind)
        for pair in (0, 1):
            d = dict(table, pose_R1=pose_R[pair], pose_t1=pose_t[pair], pose_R2=pose_R[2], pose_t2=pose_t[2], kps1=kps[pair], kps2=kps[2],
                     desc2=descs[2], matches12=matches[pair], mp1=slots[pair], mp2=slots[2], has_mp1=has_mp[pair], has_mp2=has_mp[2],
                     result=res["tri%d" % pair])
            m.TriangulateMatchesDevice(cam, d, n1, n2, cap_points, tm.SIGMA2, float(tm.MAX_SCALE_FACTOR), float(tm.RATIO_FACTOR), stream=st)
        m.BuildObservationsDevice(dict(csr, n=n, bad=bad, slots=slots, valid=table["valid"], result=res["build"]), n_kf, stride, cap_points,
                                  cap_obs, stream=st)
        if up_csr is not None:                                           # the model's CSR in place of the built one, device to device
            for key, a in zip(("obs_off", "obs_kf", "obs_kp"), up_csr):
                csr[key].zero_()
                csr[key][:len(a)].copy_(a)
        m.RefreshPointsDevice(kft, dict(table, **csr, sel=slots[2], ref_kf=ref_kf, covis=covis, result=res["refresh"]), stride, cap_points,
                              cap_obs, float(tm.MAX_SCALE_FACTOR), kf_self=2, stream=st)
        m.CullKeyFramesDevice(kft, dict(csr, bad=bad, slots=slots, valid=table["valid"], ref_kf=ref_kf, code=code, num_mp=num_mp,
                                        num_redundant=num_red, result=res["cull"]), stride, cap_points, cap_obs, [0, 1, 2], [0.0, 0.1, 0.2],
                              th_obs=1, stream=st)
        torch.cuda.synchronize()                                         # the first and only wait of the chain
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        out = {k: v.cpu().numpy() for k, v in dict(table, **csr, slots=slots, bad=bad, ref_kf=ref_kf, covis=covis, code=code, num_mp=num_mp,
                                                    num_redundant=num_red).items()}
        out.update({"result_" + k: v.cpu().numpy() for k, v in res.items()})
        return out

    first = run(None)
    n_a, n_new = int(first["result_tri0"][0]), int(first["n_points"][0])
    print("new points %d + %d; build %s; refresh %s; cull %s, d_code %s" % (n_a, n_new - n_a, first["result_build"].tolist(),
                                                                          first["result_refresh"].tolist(), first["result_cull"].tolist(),
                                                                          first["code"].tolist()))
    assert n_a > 50 and n_new - n_a > 50 and first["result_build"][om.OVERFLOW] == 0 and first["result_refresh"][0] == n_new
    # the slots as the triangulations left them (the cull has edited the device's since): d_obs[row] = (i, m)
    slots0 = np.full((n_kf, stride), -1, np.int32)
    obs = first["obs"][:n_new]
    slots0[0, obs[:n_a, 0]], slots0[1, obs[n_a:, 0]], slots0[2, obs[:, 1]] = np.arange(n_a), np.arange(n_a, n_new), np.arange(n_new)
    valid0 = np.zeros(cap_points, np.uint8)
    valid0[:n_new] = 1
    model = om.build(n_host, np.zeros(n_kf, np.uint8), slots0, stride, valid0, cap_points, cap_obs)
    assert np.array_equal(first["result_build"], model[3]) and model[3][om.NOBS] == 2 * n_new
    assert first["obs_off"].tobytes() == model[0].tobytes()
    assert first["obs_kf"][:2 * n_new].tobytes() == model[1].tobytes() and first["obs_kp"][:2 * n_new].tobytes() == model[2].tobytes()
    assert first["result_cull"][om.CULLED] + first["result_cull"][om.KEPT] == 1
    second = run(model[:3])
    for key in first:
        assert first[key].tobytes() == second[key].tobytes(), key
