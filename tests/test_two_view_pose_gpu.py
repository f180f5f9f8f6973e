"""orbm_two_view_pose{,_device} on the GPU against tests/two_view_pose_model.py, each check against a yardstick of its own so that one
cannot hide another: (a) the hypotheses against the float64 model, matched by nearest (R, t); (b) the gates against the float64 CheckRT on
the device's own hypotheses; (c) the parallax against the float64 angles around its rank; (d) the decision and what follows from it,
exactly; (e) the status and the winner against the float64 model's; (f) plumbing; (g) the chain behind the search and the RANSAC.

Every test prints its measured figures before it asserts."""
import numpy as np
import pytest

import two_view_model as tm
import two_view_pose_model as pm

pytestmark = pytest.mark.gpu

SIGMA, MIN_PARALLAX = 1.0, 1.0
OUT = dict(R21=("float32", lambda n1: (9,)), t21=("float32", lambda n1: (3,)), points3D=("float32", lambda n1: (n1, 3)),
           triangulated=("uint8", lambda n1: (n1,)), matches12_out=("int32", lambda n1: (n1,)), hyp_R=("float32", lambda n1: (8, 9)),
           hyp_t=("float32", lambda n1: (8, 3)), hyp_good=("int32", lambda n1: (8,)), hyp_parallax=("float32", lambda n1: (8,)),
           hyp_code=("uint8", lambda n1: (8, n1)), result=("int32", lambda n1: (16,)))
RANSAC_KEYS = ("pairs", "H", "F", "inl_H", "inl_F")
NAMES = list(pm.SCENES)


def _kps(xy):
    from monoorbslam3_amd.extractor import KP_DTYPE
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"], k["octave"], k["class_id"] = 31.0, 77.0, 0, -1
    return k


def _garbage(shape, dtype, dev, salt):
    """an output filled with garbage first: a call must write every byte it owns and nothing else"""
    import torch
    r = np.random.RandomState(2000 + salt)
    raw = r.randint(1, 255, int(np.prod(shape)) * np.dtype(dtype).itemsize).astype(np.uint8)
    return torch.from_numpy(raw.view(dtype).reshape(shape).copy()).to(dev)


def _inputs(sc, dev, ransac_result=None):
    import torch
    rec = lambda k: torch.from_numpy(np.frombuffer(np.ascontiguousarray(k).tobytes(), np.uint8).copy()).to(dev)  # noqa: E731
    d = dict(kps1=rec(_kps(sc["xy1"])), kps2=rec(_kps(sc["xy2"])), matches12=torch.from_numpy(sc["matches12"]).to(dev))
    for k in RANSAC_KEYS:
        d[k] = torch.from_numpy(np.ascontiguousarray(sc[k])).to(dev)
    d["ransac_result"] = torch.from_numpy(np.ascontiguousarray(sc["ransac_result"] if ransac_result is None else ransac_result, np.int32)).to(dev)
    return d


def _device_call(m, sc, family, stream=None, with_code=True, ransac_result=None, d=None):
    """one orbm_two_view_pose_device call on garbage-filled outputs; returns (numpy outputs, the garbage they held)"""
    import torch
    dev = torch.device("cuda", 0)
    n1, n2 = len(sc["xy1"]), len(sc["xy2"])
    d = _inputs(sc, dev, ransac_result) if d is None else d
    before = {}
    for salt, (k, (dt, shape)) in enumerate(OUT.items()):
        if not with_code and k == "hyp_code":
            d.pop(k, None)
            continue
        d[k] = _garbage(shape(n1), dt, dev, salt)
        before[k] = d[k].cpu().numpy().copy()
    torch.cuda.synchronize()
    if stream is None:
        m.TwoViewPoseDevice(d, n1, n2, pm.K4, family, SIGMA, MIN_PARALLAX)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            m.TwoViewPoseDevice(d, n1, n2, pm.K4, family, SIGMA, MIN_PARALLAX)
        stream.synchronize()
    return {k: d[k].cpu().numpy() for k in before}, before


@pytest.fixture(scope="module")
def matcher():
    from monoorbslam3_amd.matcher import MatcherHandle, ORBMatcher
    return ORBMatcher(handle=MatcherHandle(device=0))


def _nonblocking_stream():
    """a stream of the test's own: torch creates its streams non-blocking, so nothing orders it with stream 0"""
    import torch
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    assert s.cuda_stream != 0
    return s


_runs = {}


def _run(matcher, name):
    """the device's outputs on one entry of pm.SCENES, computed once: the even scenes on the null stream with the family forced, the odd
    ones on a non-blocking stream of their own with family = -1, read from d_ransac_result on the device"""
    if name not in _runs:
        sc, m64, m32 = pm.scene_models(name)
        odd = NAMES.index(name) % 2
        _runs[name] = _device_call(matcher, sc, -1 if odd else sc["family"], stream=_nonblocking_stream() if odd else None)[0]
    return _runs[name]


def _hyps(out):
    n = int(out["result"][2])
    return [(out["hyp_R"][k].reshape(3, 3), out["hyp_t"][k]) for k in range(n)]


def _inlier_points(sc, m64):
    rows = m64["rows"]
    return sc["xy1"][sc["pairs"][rows, 0]], sc["xy2"][sc["pairs"][rows, 1]], sc["pairs"][rows, 0]


@pytest.mark.parametrize("name", NAMES)
def test_a_hypotheses_against_the_float64_model(matcher, name):
    """Each device (R, t) is matched to the nearest float64 hypothesis and the matching is one to one.  Its rotation angle error and its
    translation angle error are at most 4 x the float32 model's largest on the same scene (pm.FLOOR, its largest over all scenes, where
    it is zero on this one).  R is orthonormal with det +1 and |t| = 1 to float precision."""
    sc, m64, m32 = pm.scene_models(name)
    out = _run(matcher, name)
    hyps = _hyps(out)
    assert len(hyps) == len(m64["hyps"]) and out["result"][1] == sc["family"]
    assert not out["hyp_R"][len(hyps):].any() and not out["hyp_t"][len(hyps):].any()
    if not hyps:
        return
    e32 = [pm.nearest(R, t, m64["hyps"])[1:] for R, t in m32["hyps"]]
    bar_r, bar_t = 4 * (max(e[0] for e in e32) or pm.FLOOR[0]), 4 * (max(e[1] for e in e32) or pm.FLOOR[1])
    got = [pm.nearest(R, t, m64["hyps"]) for R, t in hyps]
    print("%s: device rotation error %.3e translation %.3e; float32 model %.3e / %.3e; bars %.3e / %.3e; order %s" % (
        name, max(g[1] for g in got), max(g[2] for g in got), max(e[0] for e in e32), max(e[1] for e in e32), bar_r, bar_t, [g[0] for g in got]))
    assert sorted(g[0] for g in got) == list(range(len(hyps)))
    for (k, er, et), (R, t) in zip(got, hyps):
        assert er <= bar_r and et <= bar_t, (name, k, er, et)
        R = R.astype(np.float64)
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-6 and abs(np.linalg.det(R) - 1) < 1e-6 and abs(np.linalg.norm(t.astype(np.float64)) - 1) < 1e-6


@pytest.mark.parametrize("name", NAMES)
def test_b_gates_and_c_parallax_on_the_devices_own_hypotheses(matcher, name):
    """The float64 check_rt on each device (R, t).  (b) d_hyp_code equals its code except for banded matches (a gate quantity within
    pm.BAND of its threshold), key points without a match are 0 and matched non-inliers 1; d_hyp_good lies between the model's counts
    without and with the banded matches.  (c) d_hyp_parallax lies within the float64 angles at ranks idx - b .. idx + b, widened by
    pm.ACOS."""
    sc, m64, m32 = pm.scene_models(name)
    out = _run(matcher, name)
    x1, x2, at = _inlier_points(sc, m64)
    n1 = len(sc["xy1"])
    base = np.zeros(n1, np.uint8)
    base[sc["pairs"][:sc["n_matches"], 0]] = pm.NOT_INLIER
    hyps = _hyps(out)
    for h in range(8):
        code = out["hyp_code"][h]
        if h >= len(hyps):
            assert not code.any() and out["hyp_good"][h] == 0 and out["hyp_parallax"][h] == 0
            continue
        c = pm.check_rt(hyps[h][0].astype(np.float64), hyps[h][1].astype(np.float64), x1, x2, m64["th2"], np.float64)
        band = pm.banded(c, m64["th2"])
        want = base.copy()
        want[at] = c["code"]
        differ = code != want
        excused = np.zeros(n1, bool)
        excused[at] = band
        lo, hi = pm.good_range(c, m64["th2"])
        plo, phi = pm.parallax_range(c, m64["th2"])
        print("%s hypothesis %d: nGood %d in [%d, %d], parallax %.4f in [%.4f, %.4f], codes differ at %d, banded %d" % (
            name, h, out["hyp_good"][h], lo, hi, out["hyp_parallax"][h], plo, phi, differ.sum(), band.sum()))
        assert not (differ & ~excused).any(), (name, h, np.flatnonzero(differ & ~excused)[:8], code[differ][:8], want[differ][:8])
        assert out["hyp_good"][h] == (code >= pm.GOOD).sum() and lo <= out["hyp_good"][h] <= hi
        assert plo <= out["hyp_parallax"][h] <= phi, (name, h)


@pytest.mark.parametrize("name", NAMES)
def test_d_decision_exact(matcher, name):
    """two_view_decide on the device's own d_hyp_good, d_hyp_parallax and d_result[4] reproduces d_result[0], [3], [5]; d_R21 / d_t21 are
    the bytes of the winning rows; d_points3D and d_triangulated follow from the winner's d_hyp_code; d_matches12_out and d_result[6],
    [7] follow from them; [8..15] copy d_hyp_good."""
    from monoorbslam3_amd.matcher import two_view_decide
    sc, m64, m32 = pm.scene_models(name)
    out = _run(matcher, name)
    res = out["result"]
    fam, n2 = sc["family"], len(sc["xy2"])
    mask = (sc["inl_H"] if fam else sc["inl_F"])
    assert res[1] == fam and res[4] == mask.sum() and np.array_equal(res[8:], out["hyp_good"])
    w, mg, why = two_view_decide(fam, out["hyp_good"], out["hyp_parallax"], int(res[4]), MIN_PARALLAX)
    print("%s: result %s, parallax %s" % (name, res.tolist(), out["hyp_parallax"].round(4).tolist()))
    if res[2] == 0:
        assert res[0] == 2 and res[3] == -1 and res[5] == mg
    else:
        assert (res[0], res[3], res[5]) == (why, w, mg) and res[2] == (8 if fam else 4)
    m12 = sc["matches12"]
    if res[0] == 0:
        code = out["hyp_code"][res[3]]
        assert out["R21"].tobytes() == out["hyp_R"][res[3]].tobytes() and out["t21"].tobytes() == out["hyp_t"][res[3]].tobytes()
        assert np.array_equal(out["triangulated"], (code == pm.GOOD).astype(np.uint8))
        stored = code >= pm.GOOD
        assert not out["points3D"][~stored].any() and np.isfinite(out["points3D"]).all()
        assert (out["points3D"][code == pm.GOOD][:, 2] > 0).all() and (np.abs(out["points3D"][stored]).sum(axis=1) > 0).all()
        want = np.where((m12 >= 0) & (out["triangulated"] == 0), -1, m12)
    else:
        assert res[3] == -1
        for k in ("R21", "t21", "points3D", "triangulated"):
            assert not out[k].any(), k
        want = m12
    assert np.array_equal(out["matches12_out"], want)
    assert res[6] == out["triangulated"].sum() and res[7] == ((want >= 0) & (want < n2)).sum()


@pytest.mark.parametrize("name", NAMES)
def test_e_status_and_winner_are_the_float64_models(matcher, name):
    sc, m64, m32 = pm.scene_models(name)
    out = _run(matcher, name)
    res = out["result"]
    print("%s: device status %d winner %d; float64 model status %d winner %d good %s" % (name, res[0], res[3], m64["status"], m64["winner"], m64["good"]))
    assert res[0] == m64["status"]
    if m64["winner"] >= 0:
        assert pm.nearest(out["R21"].reshape(3, 3), out["t21"], m64["hyps"])[0] == m64["winner"]
    else:
        assert res[3] == -1


def test_f_plumbing(matcher):
    """either stream and two runs give the same bytes; family = -1 reads d_ransac_result[4] on the device, both values; d_hyp_code = NULL
    changes nothing else; the host twin gives the device call's bytes; a smaller and then a larger n1 on one handle; a RANSAC status other
    than 0 writes d_result and nothing else; a refusal changes nothing."""
    import torch
    from monoorbslam3_amd import _lib
    sc, m64, m32 = pm.scene_models("plane-300")
    small, _, _ = pm.scene_models("general-9")
    for fam in (0, 1):
        forced, _ = _device_call(matcher, sc, fam)
        rr = sc["ransac_result"].copy()
        rr[4] = fam
        read, _ = _device_call(matcher, sc, -1, stream=_nonblocking_stream(), ransac_result=rr)
        _device_call(matcher, small, small["family"])                      # a smaller n1 in between: the scratch only grows
        again, _ = _device_call(matcher, sc, fam)
        assert forced["result"][1] == fam and forced["result"][2] == (8 if fam else 4)
        for k in forced:
            assert forced[k].tobytes() == read[k].tobytes() == again[k].tobytes(), (fam, k)
        lean, _ = _device_call(matcher, sc, fam, with_code=False)
        assert set(lean) == set(forced) - {"hyp_code"} and all(lean[k].tobytes() == forced[k].tobytes() for k in lean)
        ransac = {k: sc[k] for k in RANSAC_KEYS}
        ransac["result"] = rr
        host = matcher.TwoViewPose(_kps(sc["xy1"]), _kps(sc["xy2"]), sc["matches12"], ransac, pm.K4, -1, SIGMA, MIN_PARALLAX)
        for k in forced:
            assert forced[k].tobytes() == host[k].tobytes(), (fam, k)
        host = matcher.TwoViewPose(_kps(sc["xy1"]), _kps(sc["xy2"]), sc["matches12"], ransac, pm.K4, fam, SIGMA, MIN_PARALLAX, codes=False)
        assert set(host) == set(lean) and all(host[k].tobytes() == forced[k].tobytes() for k in host)
    # the RANSAC refused: status 1, only d_result is written -- the device call, then the host twin
    for status in (1, 2):
        rr = sc["ransac_result"].copy()
        rr[1] = status
        out, before = _device_call(matcher, sc, -1, ransac_result=rr)
        assert out["result"].tolist() == [1, 1, 0, -1] + [0] * 12
        for k in out:
            assert k == "result" or out[k].tobytes() == before[k].tobytes(), k
        hbuf = {k: before[k].copy() for k in before}
        ransac = {k: sc[k] for k in RANSAC_KEYS}
        ransac["result"] = rr
        matcher.TwoViewPose(_kps(sc["xy1"]), _kps(sc["xy2"]), sc["matches12"], ransac, pm.K4, -1, SIGMA, MIN_PARALLAX, out=hbuf)
        assert hbuf["result"].tolist() == [1, 1, 0, -1] + [0] * 12
        for k in hbuf:
            assert k == "result" or hbuf[k].tobytes() == before[k].tobytes(), k
    # a refusal changes nothing
    dev = torch.device("cuda", 0)
    d = _inputs(sc, dev)
    n1, n2 = len(sc["xy1"]), len(sc["xy2"])
    for salt, (k, (dt, shape)) in enumerate(OUT.items()):
        d[k] = _garbage(shape(n1), dt, dev, salt)
    held = {k: d[k].cpu().numpy().copy() for k in d}
    refusals = [dict(sigma=0.0), dict(sigma=-1.0), dict(n1=0), dict(n2=0), dict(n1=-1), dict(n1=65537, code=-4), dict(family=2), dict(family=-2),
                dict(K=(0.0, 460.0, 376.0, 240.0)), dict(K=(460.0, float("inf"), 376.0, 240.0)), dict(K=(float("nan"), 460.0, 376.0, 240.0)),
                dict(drop="pairs"), dict(drop="result"), dict(drop="kps2"), dict(drop="inl_F"), dict(drop="ransac_result"), dict(drop="hyp_good"),
                dict(drop="matches12_out")]
    for bad in refusals:
        dd = {k: v for k, v in d.items() if k != bad.get("drop")}
        with pytest.raises(_lib.OrbxError) as e:
            matcher.TwoViewPoseDevice(dd, bad.get("n1", n1), bad.get("n2", n2), bad.get("K", pm.K4), bad.get("family", -1), bad.get("sigma", SIGMA),
                                      MIN_PARALLAX)
        assert e.value.code == bad.get("code", -1), bad
        torch.cuda.synchronize()
        for k in d:
            assert d[k].cpu().numpy().tobytes() == held[k].tobytes(), (bad, k)


def _described_scene(n, seed):
    """the general scene of two_view_model with descriptors: a random 256-bit descriptor per key point of frame 1, its match in frame 2 the
    same with 6 bits flipped, every other key point of frame 2 a descriptor of its own"""
    sc = tm.make_scene(n, seed)
    r = np.random.RandomState(seed + 500)
    n1, n2 = len(sc["xy1"]), len(sc["xy2"])
    d1 = r.randint(0, 256, (n1, 32)).astype(np.uint8)
    d2 = r.randint(0, 256, (n2, 32)).astype(np.uint8)
    for i in np.flatnonzero(sc["matches12"] >= 0):
        d = d1[i].copy()
        for bit in r.choice(256, 6, replace=False):
            d[bit >> 3] ^= np.uint8(1 << (bit & 7))
        d2[sc["matches12"][i]] = d
    return sc, d1, d2


def test_g_the_chain_search_ransac_pose_on_one_stream(matcher):
    """orbm_search_for_initialization_device -> orbm_two_view_ransac_device -> orbm_two_view_pose_device on ONE non-blocking stream with no
    synchronisation between them and ONE wait, on the 2000-match general scene with descriptors: every output of the pose call equals
    that of the three calls run separately with read-backs, and the RANSAC's own F is accepted."""
    import torch
    from monoorbslam3_amd.frame import FramePost
    from monoorbslam3_amd.matcher import ORBMatcher
    import test_two_view_gpu as tv
    m = ORBMatcher(0.9, True, handle=matcher._hd)
    dev = torch.device("cuda", 0)
    sc, d1, d2 = _described_scene(2000, 10)
    k1, k2 = _kps(sc["xy1"]), _kps(sc["xy2"])
    n1, n2, iters = len(k1), len(k2), 200
    post = FramePost(tm.W, tm.H, tm.FX, tm.FY, tm.CX, tm.CY)
    _, k2u, start, items = post(k2)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kp = lambda k: torch.from_numpy(np.frombuffer(np.ascontiguousarray(k).tobytes(), np.uint8).copy()).to(dev)  # noqa: E731
    pre = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)
    d = dict(kps1=kp(k1), desc1=up(d1), kps2=kp(k2u), desc2=up(d2), cell_start=up(start.astype(np.int32)),
             cell_items=up(np.concatenate([items, np.zeros(1, items.dtype)]).astype(np.int32)), pre=up(pre),
             matches12=torch.full((n1,), 7, dtype=torch.int32, device=dev), result=torch.zeros(8, dtype=torch.int32, device=dev))
    rv = dict(kps1=d["kps1"], kps2=d["kps2"], matches12=d["matches12"])
    for salt, (k, (dt, shape)) in enumerate(tv.OUT.items()):
        rv[k] = _garbage(shape(n1, iters), dt, dev, 50 + salt)
    pv = dict(kps1=d["kps1"], kps2=d["kps2"], matches12=d["matches12"], ransac_result=rv["result"], **{k: rv[k] for k in RANSAC_KEYS})
    for salt, (k, (dt, shape)) in enumerate(OUT.items()):
        pv[k] = _garbage(shape(n1), dt, dev, salt)
    stream = _nonblocking_stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        m.SearchForInitializationDevice(d, n1, n2, post.cols, post.rows, window=100, list_cap=1024, stream=None)
        m.TwoViewRansacDevice(rv, n1, n2, SIGMA, iters)
        m.TwoViewPoseDevice(pv, n1, n2, pm.K4, -1, SIGMA, MIN_PARALLAX)
    stream.synchronize()                                         # the one wait
    chained = {k: pv[k].cpu().numpy() for k in OUT}
    sres = d["result"].cpu().numpy()
    m12 = d["matches12"].cpu().numpy()
    assert sres[1] == 0 and (m12 >= 0).sum() == sres[0] and sres[0] > 1500, sres
    # apart: every stage on what the stage before it returned to the host
    ransac = m.TwoViewRansac(k1, k2u, m12, SIGMA, iters)
    apart = m.TwoViewPose(k1, k2u, m12, ransac, pm.K4, -1, SIGMA, MIN_PARALLAX)
    res = chained["result"]
    print("search %s, RANSAC %s, pose %s, parallax %s" % (sres.tolist(), ransac["result"].tolist(), res.tolist(), chained["hyp_parallax"].round(3).tolist()))
    for k in OUT:
        assert chained[k].tobytes() == apart[k].tobytes(), k
    assert ransac["result"][1] == 0 and ransac["result"][4] == 0 and res[0] == 0 and res[1] == 0
    assert res[6] > 0.9 * res[4] and res[7] == res[6]
