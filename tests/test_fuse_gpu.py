"""orbm_fuse_apply_device on the MI355X (include/orbm.h, "The fuse's hits applied on the device") against the array model of
tests/fuse_model.py, byte for byte: integers only, so no tolerance."""
import numpy as np
import pytest

import fuse_model as fm
from test_observations_gpu import GUARD, _guards_intact, _padded
from test_triangulation_gpu import _stream, _up

pytestmark = pytest.mark.gpu

_cache = {}
IN_OUT = ("slots", "valid", "found")
OUTPUTS = ("code", "refresh_sel", "result")
FILLS = dict(best_idx=-41, rows=-42, n=-43, bad=203, slots=-44, valid=204, obs_off=-45, obs_kf=-46, obs_kp=-47, found=-48, visible=-49,
             work=-50, code=-51, refresh_sel=-52, result=-53)


def _scene(name):
    """(scene, fresh CSR, model outputs): computed once, shared, never changed"""
    if name not in _cache:
        sc = fm.make_scene(**fm.SCENES[name])
        csr = fm.fresh_csr(sc)
        _cache[name] = (sc, csr, fm.apply(sc, csr))
    return _cache[name]


def _run(torch, dev, sc, csr, stream_kind, counters=True):
    """one call on padded copies of everything -> (arrays after the call, arrays as passed)"""
    from monoorbslam3_amd.matcher import ORBMatcher
    nq = len(sc["best_idx"])
    start = dict(best_idx=sc["best_idx"], n=sc["n"], bad=sc["bad"], slots=sc["slots"], valid=sc["valid"], obs_off=csr[0], obs_kf=csr[1],
                 obs_kp=csr[2], work=np.full(nq, 61, np.int32), code=np.full(nq, 62, np.int32), refresh_sel=np.full(nq, 63, np.int32),
                 result=np.full(8, 64, np.int32))
    if sc.get("rows") is not None:
        start["rows"] = sc["rows"]
    if counters:
        start.update(found=sc["found"], visible=sc["visible"])
    pads = {k: _padded(torch, dev, v, FILLS[k]) for k, v in start.items()}
    d = {k: v[1] for k, v in pads.items()}
    st = _stream(torch, dev, stream_kind)
    ORBMatcher().FuseApplyDevice(d, nq, len(sc["n"]), sc["K"], sc["stride"], sc["cap_points"], len(csr[1]), stream=st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k in pads:
        assert _guards_intact(pads[k][0], FILLS[k]), k
    return {k: v.cpu().numpy() for k, v in d.items()}, start


def _check(got, start, want, counters=True):
    print("device d_result %s, model %s; codes %s" % (got["result"].tolist(), want["result"].tolist(),
                                                      np.bincount(np.clip(got["code"], 0, 8), minlength=9).tolist()))
    assert got["result"].tobytes() == want["result"].tobytes()
    for key in ("code", "refresh_sel", "valid") + (("found",) if counters else ()):
        assert got[key].tobytes() == np.ascontiguousarray(want[key]).tobytes(), key
    assert got["slots"].tobytes() == np.ascontiguousarray(want["slots"]).tobytes()
    for key in start:                                                     # inputs as passed
        if key not in IN_OUT + OUTPUTS + ("work",):
            assert got[key].tobytes() == np.ascontiguousarray(start[key]).tobytes(), key


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
@pytest.mark.parametrize("name", sorted(fm.SCENES))
def test_apply_equals_the_model(name, stream_kind):
    """3 x 64 slots with 200 rows and 12 x 256 with 1000: an added observation (into -1 and into junk), a replace in each direction,
    the exact tie, a chain of three entries on one slot whose counts need the moved observations, a chain behind an add, a winner that
    already observes the loser's key frames, a loser twice in one key frame (mid), a loser seen from a bad key frame, a bad occupant
    hit twice, gated entries (invalid, already in K), -1 and out-of-range d_best_idx and d_rows, d_n[K] > stride.  Slots, validity,
    found counters, codes, d_refresh_sel and d_result byte for byte; inputs as passed; guards intact; a second run the same bytes."""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, want = _scene(name)
    fm.check_scene(sc, want)
    got, start = _run(torch, dev, sc, csr, stream_kind)
    _check(got, start, want)
    again, _ = _run(torch, dev, sc, csr, stream_kind)
    for key in IN_OUT + OUTPUTS:
        assert again[key].tobytes() == got[key].tobytes(), key


@pytest.mark.parametrize("name", sorted(fm.SCENES))
def test_apply_distrusts_the_csr_and_runs_without_the_counters(name):
    """Unusable entries inside the lists of rows the call touches are dropped and counted in d_result[7], never dereferenced; broken
    offsets (below zero, past the end) between two rows without an observation give empty lists; d_found / d_visible NULL."""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, _ = _scene(name)
    for seed in (4, 5):
        spoilt, junk = fm.spoil_csr(sc, csr, seed)
        want = fm.apply(sc, spoilt)
        assert want["result"][fm.R_DROPPED] == _scene(name)[2]["result"][fm.R_DROPPED] + junk
        got, start = _run(torch, dev, sc, spoilt, "explicit")
        _check(got, start, want)
    bare = dict(sc, found=None, visible=None)
    got, start = _run(torch, dev, bare, csr, "null", counters=False)
    _check(got, start, fm.apply(bare, csr), counters=False)


def test_apply_with_entry_j_as_row_j_and_an_empty_list():
    """d_rows = NULL: the builders' indexing, nq = cap_points; nq = 0 writes d_result only"""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, _ = _scene("mid")
    flat = fm.by_row(sc)
    want = fm.apply(flat, csr)
    fm.check_scene(flat, want)
    got, start = _run(torch, dev, flat, csr, "explicit")
    _check(got, start, want)
    none = dict(sc, best_idx=np.zeros(0, np.int32), rows=np.zeros(0, np.int32))
    got, start = _run(torch, dev, none, csr, "null")
    assert got["result"].tolist() == [0] * 8 and got["slots"].tobytes() == sc["slots"].tobytes() and got["valid"].tobytes() == sc["valid"].tobytes()


def test_apply_into_a_bad_key_frame_and_over_a_long_list():
    """K bad: its slots are no observations, so a losing occupant keeps its slot; a CSR list of more than 1024 entries leaves the
    replace undone (code 7)"""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, _ = _scene("small")
    bad = sc["bad"].copy()
    bad[sc["K"]] = 1
    into_bad = dict(sc, bad=bad)
    csr_bad = fm.fresh_csr(into_bad)
    want = fm.apply(into_bad, csr_bad)
    assert want["result"][fm.R_OCCUPANT_REPLACED] >= 3
    got, start = _run(torch, dev, into_bad, csr_bad, "null")
    _check(got, start, want)
    j = sc["expect"]["occupant_loses"][0][0]
    long_csr = fm.long_csr(csr, int(sc["rows"][j]))
    want = fm.apply(sc, long_csr)
    assert want["code"][j] == fm.UNDONE
    got, start = _run(torch, dev, sc, long_csr, "explicit")
    _check(got, start, want)


@pytest.mark.parametrize("name", sorted(fm.SCENES))
def test_both_refusals_leave_every_array_as_passed(name):
    """a row in two live entries: d_result[1] = 1; the occupant of a hit slot in a second slot of K: 2; d_slots, d_valid, d_found,
    d_code and d_refresh_sel are byte for byte as passed"""
    import torch
    dev = torch.device("cuda", 0)
    sc, csr, _ = _scene(name)
    for want, bad_scene in fm.refusal_scenes(sc).items():
        assert fm.refusal(bad_scene) == want
        got, start = _run(torch, dev, bad_scene, fm.fresh_csr(bad_scene), "explicit")
        assert got["result"].tolist() == [0, want, 0, 0, 0, 0, 0, 0]
        for key in start:
            if key != "work" and key != "result":
                assert got[key].tobytes() == np.ascontiguousarray(start[key]).tobytes(), key


def test_apply_at_the_largest_table():
    """cap_points = 524288 and stride = 8192: the mask and the slot heads take 96 KB of dynamic LDS; rows at both ends of the table
    and the last slot of K take part"""
    import torch
    dev = torch.device("cuda", 0)
    cap, stride = 524288, 8192
    slots = np.full((2, stride), -1, np.int32)
    slots[0, stride - 1], slots[1, 0], slots[1, 5] = cap - 1, 0, 7       # K = 0: its last slot holds the last row
    sc = dict(best_idx=np.array([stride - 1, 3, -1], np.int32), rows=np.array([0, 7, 9], np.int32), n=np.full(2, stride, np.int32),
              bad=np.zeros(2, np.uint8), slots=slots, stride=stride, valid=np.ones(cap, np.uint8), cap_points=cap, K=0,
              found=np.arange(cap, dtype=np.int32), visible=np.ones(cap, np.int32))
    csr = fm.fresh_csr(sc)
    want = fm.apply(sc, csr)
    assert want["code"].tolist() == [fm.OCCUPANT_REPLACED, fm.ADDED, fm.NONE] and want["slots"][0, stride - 1] == 0 and not want["valid"][cap - 1]
    got, start = _run(torch, dev, sc, csr, "null")
    _check(got, start, want)


@pytest.mark.parametrize("stream_kind", ["explicit", "null"])
def test_fuse_chain_with_one_wait(stream_kind):
    """orbm_project_fuse_device -> orbm_search_fuse_device -> orbm_fuse_apply_device -> orbm_build_observations_device ->
    orbm_refresh_points_device (d_sel = d_refresh_sel) on one stream with ONE wait at the end, 3 key frames x 64 slots, 200 rows: the
    slots, d_valid and d_found equal the model's on the d_best_idx the search left, the rebuilt CSR is the model's of those slots, and
    the refreshed rows equal refresh_model's on them."""
    import torch
    import observations_model as om
    import projection_model as pm
    import refresh_model as rm
    from monoorbslam3_amd.frame import FramePost
    from monoorbslam3_amd.matcher import KfTable, ORBMatcher, ProjCamera
    dev = torch.device("cuda", 0)
    sc = fm.make_projected_scene(n_kp=64, n_cand=50, n_occ=16, n_kf=3, seed=8, cap_points=200)
    cap, stride, n_kf = sc["cap_points"], sc["stride"], 3
    rng = np.random.RandomState(80)
    csr = fm.fresh_csr(sc)
    n_obs, cap_obs = len(csr[1]), len(csr[1]) + 40
    post = FramePost(sc["w"], sc["h"], *sc["cam"])
    _, kpu, start, items = post(sc["kps"])
    assert kpu.tobytes() == np.ascontiguousarray(sc["kps"]).tobytes()
    kps = [sc["kps"]]
    for k in (1, 2):                                                      # the other key frames: records and descriptors for the refresh
        kp = np.zeros(stride, pm.KP_DTYPE)
        kp["octave"], kp["class_id"] = rng.randint(0, pm.N_LEVELS, stride), -1
        kp["size"] = 31.0 * pm.SCALE_FACTORS[kp["octave"]]
        kps.append(kp)
    kf_desc = [sc["desc"]] + [rng.randint(0, 256, (stride, 32)).astype(np.uint8) for _ in (1, 2)]
    pose_R = np.stack([np.eye(3).reshape(9)] * 3)
    pose_t = np.array([[0.0, 0.0, 0.0], [0.3, -0.1, 0.05], [-0.2, 0.15, -0.04]])
    ref_kf = np.zeros(cap, np.int32)
    for p in range(cap):
        seen = [k for k in (1, 2) if (sc["slots"][k] == p).any()]
        ref_kf[p] = seen[0] if seen else 1
    sigma2 = (pm.SCALE_FACTORS * pm.SCALE_FACTORS).astype(np.float32)
    z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)  # noqa: E731
    table = dict(points=_up(torch, dev, sc["points"]), valid=_up(torch, dev, sc["valid"]), normals=_up(torch, dev, sc["normals"]),
                 min_dist=_up(torch, dev, sc["min_dist"]), max_dist=_up(torch, dev, sc["max_dist"]), desc=_up(torch, dev, sc["q_desc"]))
    n, bad = _up(torch, dev, sc["n"]), _up(torch, dev, sc["bad"])
    slots, found = _up(torch, dev, sc["slots"]), _up(torch, dev, sc["found"])
    res = {k: torch.full((8,), 77, dtype=torch.int32, device=dev) for k in ("project", "search", "apply", "build", "refresh")}
    d = dict(table, pose_R=_up(torch, dev, pose_R[0]), pose_t=_up(torch, dev, pose_t[0]), q_xy=z((cap, 2), torch.float32), q_radius=z((cap,), torch.float32),
             q_level=z((cap,), torch.int32), q_ok=z((cap,), torch.uint8), q_desc=table["desc"], kps=_up(torch, dev, kpu), desc=_up(torch, dev, sc["desc"]),
             cell_start=_up(torch, dev, start.astype(np.int32)), cell_items=_up(torch, dev, np.concatenate([items, np.zeros(1, items.dtype)]).astype(np.int32)),
             sigma2=_up(torch, dev, sigma2), best_idx=z((cap,), torch.int32), best_dist=z((cap,), torch.int32), n=n, bad=bad, slots=slots,
             found=found, visible=_up(torch, dev, sc["visible"]), obs_off=_up(torch, dev, csr[0]), obs_kf=_up(torch, dev, csr[1]),
             obs_kp=_up(torch, dev, csr[2]), work=z((cap,), torch.int32), code=z((cap,), torch.int32), refresh_sel=z((cap,), torch.int32))
    csr2 = dict(obs_off=z((cap + 1,), torch.int32), obs_kf=z((cap_obs,), torch.int32), obs_kp=z((cap_obs,), torch.int32))
    kft = KfTable.make(_up(torch, dev, pose_R), _up(torch, dev, pose_t), bad, [_up(torch, dev, k) for k in kps], [_up(torch, dev, x) for x in kf_desc], n)
    cam = ProjCamera.make(sc["cam"], (0.0, float(sc["w"]), 0.0, float(sc["h"])))
    m = ORBMatcher()
    st = _stream(torch, dev, stream_kind)
    m.ProjectFuseDevice(cam, dict(d, result=res["project"]), cap, pm.SCALE_FACTORS, float(pm.LOG_SCALE_FACTOR), 3.0, stream=st)
    m.SearchFuseDevice(dict(d, result=res["search"]), cap, post.cols, post.rows, list_cap=48, stream=st)
    m.FuseApplyDevice(dict(d, result=res["apply"]), cap, n_kf, sc["K"], stride, cap, n_obs, stream=st)
    m.BuildObservationsDevice(dict(csr2, n=n, bad=bad, slots=slots, valid=table["valid"], result=res["build"]), n_kf, stride, cap, cap_obs, stream=st)
    m.RefreshPointsDevice(kft, dict(table, **csr2, sel=d["refresh_sel"], ref_kf=_up(torch, dev, ref_kf), result=res["refresh"]), cap, cap, cap_obs,
                          float(rm.MAX_SCALE_FACTOR), stream=st)
    torch.cuda.synchronize()                                              # the first and only wait of the chain
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    g = lambda t: t.cpu().numpy()  # noqa: E731
    best = g(d["best_idx"])
    want = fm.apply(dict(sc, best_idx=best), csr)
    print("search %s, apply device %s, model %s, build %s, refresh %s" % (g(res["search"])[:2].tolist(), g(res["apply"]).tolist(),
                                                                          want["result"].tolist(), g(res["build"]).tolist(), g(res["refresh"]).tolist()))
    assert (best >= 0).sum() >= 20 and want["result"][fm.R_ADDED] >= 5 and want["result"][fm.R_LIST_REPLACED] + want["result"][fm.R_OCCUPANT_REPLACED] >= 3
    assert g(res["apply"]).tobytes() == want["result"].tobytes()
    for key, t in (("slots", slots), ("valid", table["valid"]), ("found", found), ("code", d["code"]), ("refresh_sel", d["refresh_sel"])):
        assert g(t).tobytes() == np.ascontiguousarray(want[key]).tobytes(), key
    off, okf, okp, bres = om.build(sc["n"], sc["bad"], want["slots"], stride, want["valid"], cap, cap_obs)
    assert np.array_equal(g(res["build"]), bres) and g(csr2["obs_off"]).tobytes() == off.tobytes()
    assert g(csr2["obs_kf"])[:len(okf)].tobytes() == okf.tobytes() and g(csr2["obs_kp"])[:len(okp)].tobytes() == okp.tobytes()
    rs = dict(n=sc["n"], bad=sc["bad"], pose_R=pose_R, pose_t=pose_t, kps=kps, kf_desc=kf_desc, points=sc["points"], valid=want["valid"],
              normals=sc["normals"], min_dist=sc["min_dist"], max_dist=sc["max_dist"], desc=sc["q_desc"], obs_off=off, obs_kf=okf, obs_kp=okp,
              ref_kf=ref_kf)
    fresh = rm.refresh(rs, want["refresh_sel"], cap)
    assert np.array_equal(g(res["refresh"]), fresh["result"]) and fresh["result"][0] >= 8
    assert np.array_equal(g(table["normals"]), fresh["normals"])          # by value: -0 equals +0
    for key in ("min_dist", "max_dist"):
        assert g(table[key]).view(np.uint32).tobytes() == fresh[key].view(np.uint32).tobytes(), key
    assert np.array_equal(g(table["desc"]), fresh["desc"]) and (fresh["desc"] != sc["q_desc"]).any()
