"""orbm_two_view_ransac{,_device} on the GPU against tests/two_view_model.py, each check against a yardstick of its own so that one
cannot hide another: (a) the hypotheses against the float64 model, (b) the scoring against the float64 Check* on the device's own
matrices, (c) the pick against the device's own scores, exactly, (d) the decision, exactly, (e) the winners' scores against the
float64 model's, (f) plumbing, (g) the chain behind orbm_search_for_initialization_device.

Every test prints its measured figures before it asserts."""
import numpy as np
import pytest

import two_view_model as tm

pytestmark = pytest.mark.gpu

SIGMA = 1.0
OUT = dict(pairs=("int32", lambda n1, it: (n1, 2)), H=("float32", lambda n1, it: (9,)), F=("float32", lambda n1, it: (9,)),
           inl_H=("uint8", lambda n1, it: (n1,)), inl_F=("uint8", lambda n1, it: (n1,)), score=("float32", lambda n1, it: (2,)),
           rh=("float32", lambda n1, it: (1,)), hyp=("float32", lambda n1, it: (2, it, 9)), hyp_score=("float32", lambda n1, it: (2, it)),
           result=("int32", lambda n1, it: (8,)))


def _kps(xy):
    from monoorbslam3_amd.extractor import KP_DTYPE
    k = np.zeros(len(xy), KP_DTYPE)
    k["x"], k["y"] = xy[:, 0], xy[:, 1]
    k["size"], k["angle"], k["octave"], k["class_id"] = 31.0, 77.0, 0, -1
    return k


def _garbage(shape, dtype, dev, salt):
    """an output filled with garbage first: a call must write every byte it owns and nothing else"""
    import torch
    r = np.random.RandomState(1000 + salt)
    raw = r.randint(1, 255, int(np.prod(shape)) * np.dtype(dtype).itemsize).astype(np.uint8)
    return torch.from_numpy(raw.view(dtype).reshape(shape).copy()).to(dev)


def _device_call(m, kps1, kps2, matches12, iters, sets=None, stream=None, state=0, with_hyp=True):
    """one orbm_two_view_ransac_device call on garbage-filled outputs; returns (numpy outputs, the garbage they held)"""
    import torch
    dev = torch.device("cuda", 0)
    n1, n2 = len(kps1), len(kps2)
    rec = lambda k: torch.from_numpy(np.frombuffer(np.ascontiguousarray(k).tobytes(), np.uint8).copy()).to(dev)  # noqa: E731
    d = dict(kps1=rec(kps1), kps2=rec(kps2), matches12=torch.from_numpy(np.ascontiguousarray(matches12, np.int32)).to(dev))
    if sets is not None:
        d["sets"] = torch.from_numpy(np.ascontiguousarray(sets, np.int32)).to(dev)
    before = {}
    for salt, (k, (dt, shape)) in enumerate(OUT.items()):
        if not with_hyp and k.startswith("hyp"):
            continue
        d[k] = _garbage(shape(n1, iters), dt, dev, salt)
        before[k] = d[k].cpu().numpy().copy()
    torch.cuda.synchronize()
    if stream is None:
        m.TwoViewRansacDevice(d, n1, n2, SIGMA, iters, state)
        torch.cuda.synchronize()
    else:
        with torch.cuda.stream(stream):
            m.TwoViewRansacDevice(d, n1, n2, SIGMA, iters, state)
        stream.synchronize()
    return {k: d[k].cpu().numpy() for k in before}, before


@pytest.fixture(scope="module")
def matcher():
    from monoorbslam3_amd.matcher import MatcherHandle, ORBMatcher
    return ORBMatcher(handle=MatcherHandle(device=0))


_runs = {}


def _run(matcher, scene):
    """the device's outputs on one entry of tm.SCENES, computed once: the even scenes on the null stream, the odd ones on a non-blocking
    stream of their own"""
    if scene not in _runs:
        import torch
        sc, m64, m32 = tm.scene_models(*scene)
        stream = _nonblocking_stream() if tm.SCENES.index(scene) % 2 else None
        out, _ = _device_call(matcher, _kps(sc["xy1"]), _kps(sc["xy2"]), sc["matches12"], scene[3], stream=stream)
        _runs[scene] = out
    return _runs[scene]


def _nonblocking_stream():
    """a stream of the test's own: torch creates its streams non-blocking, so nothing orders it with stream 0"""
    import torch
    s = torch.cuda.Stream(device=torch.device("cuda", 0))
    assert s.cuda_stream != 0
    return s


def _matched(sc, m64):
    return sc["xy1"][m64["pairs"][:, 0]], sc["xy2"][m64["pairs"][:, 1]]


@pytest.mark.parametrize("scene", tm.SCENES)
def test_a_hypotheses_against_the_float64_model(matcher, scene):
    """e = the sine of the angle between the device's matrix and the float64 model's, sign free, over the hypotheses whose float64
    sample is conditioned ((s8 - s9) / s1 > 1e-3 of the 16 x 9 matrix, s8 / s1 > 1e-3 of the 8 x 9 one): per scene and family, the
    device's largest e is at most 4 x the float32 model's over the same hypotheses -- LAPACK and a fixed-sweep Jacobi round
    differently (the triangulation's bar and reason).  Every hypothesis, gated or not, is finite."""
    sc, m64, m32 = tm.scene_models(*scene)
    out = _run(matcher, scene)
    iters = scene[3]
    assert out["result"][1] in (0, 2) and out["result"][0] == scene[0]
    hyp = out["hyp"].reshape(2, iters, 3, 3)
    assert np.isfinite(hyp).all()
    gate = m64["cond"] > tm.GATE
    for fam, name in ((0, "H"), (1, "F")):
        g = gate[fam]
        if not g.any():
            print("%s %s: no conditioned hypothesis" % (scene, name))
            continue
        e_dev = tm.unit_sine(hyp[fam][g], m64["hyp"][fam][g]).max()
        e_32 = tm.unit_sine(m32["hyp"][fam][g], m64["hyp"][fam][g]).max()
        print("%s %s: %d of %d conditioned, max e device %.3e, float32 model %.3e, ratio %.2f" % (scene, name, g.sum(), iters, e_dev, e_32,
                                                                                               e_dev / e_32 if e_32 else np.inf))
        assert e_dev <= 4 * e_32, (scene, name, e_dev, e_32)


@pytest.mark.parametrize("scene", tm.SCENES)
def test_b_scoring_given_the_devices_own_matrices(matcher, scene):
    """The float64 Check* on each device hypothesis: the inlier flags are equal except for matches with a side whose chi-square lies
    within 1e-3 relative of its threshold; |S_dev - S_64| is at most 4 x the float32 model's largest relative score error on the same
    matrices (times the score), plus 5.991 per banded side of that hypothesis.  The scores are compared for all 2 * iters
    hypotheses; the FLAGS only for the two winners, whose mask rows are the ones a call returns (the other rows stay in handle
    scratch): a wrong bit in another row shows through that row's score alone, by 2.15 or more outside the band."""
    sc, m64, m32 = tm.scene_models(*scene)
    out = _run(matcher, scene)
    n, iters = scene[0], scene[3]
    x1, x2 = _matched(sc, m64)
    hyp = out["hyp"].reshape(2, iters, 3, 3)
    # the float32 model's relative score error on the same matrices: its Check* in float32 against the float64 one
    rel32, s64, banded, flags64 = np.zeros((2, iters)), np.zeros((2, iters)), np.zeros((2, iters), int), np.zeros((2, iters, n), bool)
    band_any = np.zeros((2, iters, n), bool)
    for fam in range(2):
        check = tm.check_fundamental if fam else tm.check_homography
        for it in range(iters):
            b, s, f = tm.banded_sides(fam, hyp[fam, it], x1, x2, SIGMA)
            s32 = check(hyp[fam, it], x1, x2, SIGMA, np.float32)[0]
            s64[fam, it], banded[fam, it], flags64[fam, it], band_any[fam, it] = s, b.sum(), f, b.any(axis=1)
            rel32[fam, it] = abs(float(s32) - s) / s if s > 0 else 0.0
    bar_rel = 4 * rel32.max(axis=1)
    err = np.abs(out["hyp_score"].astype(np.float64) - s64)
    bar = bar_rel[:, None] * s64 + 5.991 * banded
    worst = (err - bar).max()
    print("%s: float32 model's largest relative score error H %.3e F %.3e; device |S - S64| largest %.3e (relative %.3e), banded sides %d; "
          "closest to the bar %.3e" % (scene, rel32[0].max(), rel32[1].max(), err.max(), (err / np.maximum(s64, 1e-30))[s64 > 0].max()
                                       if (s64 > 0).any() else 0.0, banded.sum(), worst))
    assert (err <= bar).all(), (scene, np.argwhere(err > bar)[:5], err.max())
    # the flags: a call returns the mask rows of the two winners (the others stay in handle scratch)
    for fam, key in ((0, "inl_H"), (1, "inl_F")):
        w = out["result"][2 + fam]
        if w < 0:
            continue
        got = out[key][:n].astype(bool)
        differ = got != flags64[fam, w]
        assert not (differ & ~band_any[fam, w]).any(), (scene, key, np.flatnonzero(differ & ~band_any[fam, w])[:8])


@pytest.mark.parametrize("scene", tm.SCENES)
def test_c_pick_and_d_decision_exact(matcher, scene):
    """(c) d_result[2], [3] = np.argmax of the device's own score rows (-1 when the maximum is 0); d_H, d_F and d_score are the bytes of
    that hypothesis's row; the counts are the masks' sums; the masks are 0 from n_matches on; d_pairs is the model's list.
    (d) d_rh = float32(SH) / (float32(SH) + float32(SF)) and d_result[4] = (d_rh > 0.5)."""
    sc, m64, m32 = tm.scene_models(*scene)
    out = _run(matcher, scene)
    n, iters = scene[0], scene[3]
    res = out["result"]
    n1 = len(sc["xy1"])
    assert np.array_equal(out["pairs"][:n], m64["pairs"]) and (out["pairs"][n:] == -1).all()
    for fam, mat, inl in ((0, "H", "inl_H"), (1, "F", "inl_F")):
        row = out["hyp_score"][fam]
        assert not np.isnan(row).any()
        want = int(np.argmax(row)) if row.max() > 0 else -1
        assert res[2 + fam] == want, (scene, fam, res, want)
        if want >= 0:
            assert out[mat].tobytes() == out["hyp"][fam, want].tobytes() and out["score"][fam].tobytes() == row[want].tobytes()
        else:
            assert not out[mat].any() and out["score"][fam] == 0 and not out[inl].any()
        assert set(np.unique(out[inl])) <= {0, 1} and not out[inl][n:].any() and len(out[inl]) == n1
        assert res[5 + fam] == out[inl].sum()
    sh, sf = np.float32(out["score"][0]), np.float32(out["score"][1])
    if sh + sf == 0:
        assert res[1] == 2 and out["rh"][0] == 0
    else:
        assert res[1] == 0 and out["rh"][0].tobytes() == np.float32(sh / np.float32(sh + sf)).tobytes()
    assert res[4] == int(out["rh"][0] > np.float32(0.5)) and res[7] == 0
    print("%s: result %s, RH %.4f (float64 model %.4f)" % (scene, res.tolist(), out["rh"][0], m64["rh"]))


@pytest.mark.parametrize("scene", tm.SCENES)
def test_e_the_winner_scores_what_the_float64_models_winner_scores(matcher, scene):
    """the device's best SF on the general scenes, its best SH on the planar ones, is at least 0.99 x the float64 model's best, on
    every scene: room for a winner that loses a near tie through banded matches worth at most 2.15 each in a score of several
    hundred.  (On the planar scene of 9 matches no homography scores above 0 in either model: the bar is 0 there.)"""
    sc, m64, m32 = tm.scene_models(*scene)
    out = _run(matcher, scene)
    fam = 0 if scene[2] else 1
    print("%s: device best %s %.3f, float64 model %.3f, float32 model %.3f" % (scene, ("SH", "SF")[fam], out["score"][fam], m64["score"][fam],
                                                                             m32["score"][fam]))
    assert out["score"][fam] >= 0.99 * m64["score"][fam]


def test_f_plumbing(matcher):
    """d_sets given or NULL (the same sets) and two runs give the same bytes, on either stream; the host twin gives the device call's
    bytes, with and without the optional outputs; 7 matches: status 1 and only d_result changes; a refusal changes nothing."""
    import torch
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.matcher import two_view_sets
    scene = (65, 8, False, 200)
    sc, m64, m32 = tm.scene_models(*scene)
    k1, k2, m12 = _kps(sc["xy1"]), _kps(sc["xy2"]), sc["matches12"]
    first = _run(matcher, scene)
    sets = two_view_sets(65, 200)
    assert np.array_equal(sets, m64["sets"])
    given, _ = _device_call(matcher, k1, k2, m12, 200, sets=sets)
    again, _ = _device_call(matcher, k1, k2, m12, 200, stream=_nonblocking_stream())
    for k in first:
        assert first[k].tobytes() == given[k].tobytes() == again[k].tobytes(), k
    # another state draws other sets
    other, _ = _device_call(matcher, k1, k2, m12, 200, state=12345)
    assert other["hyp"].tobytes() != first["hyp"].tobytes()
    given, _ = _device_call(matcher, k1, k2, m12, 200, sets=two_view_sets(65, 200, 12345))
    for k in other:
        assert other[k].tobytes() == given[k].tobytes(), k
    # the optional outputs left out: the others do not change
    lean, _ = _device_call(matcher, k1, k2, m12, 200, with_hyp=False)
    for k in lean:
        assert first[k].tobytes() == lean[k].tobytes(), k
    # the host twin
    host = matcher.TwoViewRansac(k1, k2, m12, SIGMA, 200)
    for k in first:
        assert first[k].tobytes() == host[k].tobytes(), k
    host = matcher.TwoViewRansac(k1, k2, m12, SIGMA, 200, sets=sets, all_hypotheses=False)
    assert set(host) == set(lean) and all(first[k].tobytes() == host[k].tobytes() for k in host)
    # 7 matches: status 1, only d_result is written
    few = m12.copy()
    few[np.flatnonzero(few >= 0)[7:]] = -1
    out, before = _device_call(matcher, k1, k2, few, 200)
    assert out["result"].tolist() == [7, 1, -1, -1, 0, 0, 0, 0]
    for k in out:
        assert k == "result" or out[k].tobytes() == before[k].tobytes(), k
    hbuf = {k: before[k].copy() for k in before}
    matcher.TwoViewRansac(k1, k2, few, SIGMA, 200, out=hbuf)
    assert hbuf["result"].tolist() == [7, 1, -1, -1, 0, 0, 0, 0]
    for k in hbuf:
        assert k == "result" or hbuf[k].tobytes() == before[k].tobytes(), k
    # an entry at or above n2 is no match either
    few[np.flatnonzero(few < 0)[:3]] = len(k2)
    out, _ = _device_call(matcher, k1, k2, few, 200)
    assert out["result"][0] == 7 and out["result"][1] == 1
    # a refusal changes nothing: the device entry point on the garbage-filled device buffers, then the host twin
    dev = torch.device("cuda", 0)
    rec = lambda k: torch.from_numpy(np.frombuffer(np.ascontiguousarray(k).tobytes(), np.uint8).copy()).to(dev)  # noqa: E731
    d = dict(kps1=rec(k1), kps2=rec(k2), matches12=torch.from_numpy(m12).to(dev))
    for salt, (k, (dt, shape)) in enumerate(OUT.items()):
        d[k] = _garbage(shape(len(k1), 200), dt, dev, salt)
    held = {k: d[k].cpu().numpy().copy() for k in d}
    refusals = [dict(iters=0), dict(iters=1025), dict(sigma=0.0), dict(sigma=-1.0), dict(n1=0), dict(n2=0), dict(n1=-1), dict(n1=65537, code=-4),
                dict(drop="pairs"), dict(drop="result"), dict(drop="kps2"), dict(drop="inl_F")]
    for bad in refusals:
        dd = {k: v for k, v in d.items() if k != bad.get("drop")}
        with pytest.raises(_lib.OrbxError) as e:
            matcher.TwoViewRansacDevice(dd, bad.get("n1", len(k1)), bad.get("n2", len(k2)), bad.get("sigma", SIGMA), bad.get("iters", 200))
        assert e.value.code == bad.get("code", -1), bad
        torch.cuda.synchronize()
        for k in d:
            assert d[k].cpu().numpy().tobytes() == held[k].tobytes(), (bad, k)
    for bad in (dict(iters=0), dict(iters=1025), dict(sigma=0.0)):
        hbuf = {k: before[k].copy() for k in before}
        with pytest.raises(_lib.OrbxError) as e:
            matcher.TwoViewRansac(k1, k2, m12, bad.get("sigma", SIGMA), bad.get("iters", 200), out=hbuf)
        assert e.value.code == -1
        for k in hbuf:
            assert hbuf[k].tobytes() == before[k].tobytes(), (bad, k)


def test_g_the_chain_behind_search_for_initialization(matcher):
    """orbm_search_for_initialization_device -> orbm_two_view_ransac_device on ONE non-blocking stream with ONE wait, the inputs built
    as tests/test_matcher_gpu.py builds its two views (the crowded scene's generator is imported from there): the result equals that
    of a separate call on the matches read back."""
    import torch
    from monoorbslam3_amd import synth
    from monoorbslam3_amd.extractor import ORBExtractor
    from monoorbslam3_amd.frame import FramePost
    from test_matcher_gpu import _crowd
    from monoorbslam3_amd.matcher import ORBMatcher
    matcher = ORBMatcher(0.9, True, handle=matcher._hd)          # the search's settings there; the same handle
    dev = torch.device("cuda", 0)
    w, h = 752, 480
    canvas = synth.make_canvas(w + 40, h + 20, seed=77)
    f1 = np.ascontiguousarray(canvas[5:5 + h, 10:10 + w])
    f2 = np.ascontiguousarray(canvas[9:9 + h, 22:22 + w])
    ex = ORBExtractor(2000, 1.2, 8, 20, 7)
    cases = [("views",) + ex(f1) + ex(f2), ("crowded",) + _crowd(900, 1) + _crowd(850, 2)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    kp = lambda k: torch.from_numpy(np.frombuffer(np.ascontiguousarray(k).tobytes(), np.uint8).copy()).to(dev)  # noqa: E731
    post = FramePost(w, h, 460.0, 460.0, w / 2.0, h / 2.0)
    stream = _nonblocking_stream()
    iters = 200
    for name, k1, d1, k2, d2 in cases:
        n1, n2 = len(k1), len(k2)
        pre = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32)
        _, k2u, start, items = post(k2)
        d = dict(kps1=kp(k1), desc1=up(d1), kps2=kp(k2u), desc2=up(d2), cell_start=up(start.astype(np.int32)),
                 cell_items=up(np.concatenate([items, np.zeros(1, items.dtype)]).astype(np.int32)), pre=up(pre),
                 matches12=torch.full((n1,), 7, dtype=torch.int32, device=dev), result=torch.zeros(8, dtype=torch.int32, device=dev))
        tv = dict(kps1=d["kps1"], kps2=d["kps2"], matches12=d["matches12"])
        for salt, (k, (dt, shape)) in enumerate(OUT.items()):
            tv[k] = _garbage(shape(n1, iters), dt, dev, salt)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            matcher.SearchForInitializationDevice(d, n1, n2, post.cols, post.rows, window=100, list_cap=1024, stream=None)
            matcher.TwoViewRansacDevice(tv, n1, n2, SIGMA, iters)
        stream.synchronize()                                     # the one wait
        res = d["result"].cpu().numpy()
        m12 = d["matches12"].cpu().numpy()
        assert res[1] == 0 and res[0] > 50 and (m12 >= 0).sum() == res[0], (name, res)
        chained = {k: tv[k].cpu().numpy() for k in OUT}
        apart, _ = _device_call(matcher, k1, k2u, m12, iters)
        print("%s: %d matches, result %s" % (name, res[0], chained["result"].tolist()))
        assert chained["result"][0] == res[0] and chained["result"][1] in (0, 2)
        for k in OUT:
            assert chained[k].tobytes() == apart[k].tobytes(), (name, k)
