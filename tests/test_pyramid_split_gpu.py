"""ORBX_VAR_PYRAMID_SPLIT: the resizes of pyramid levels G.. on the side stream (k_resize, no LDS) beside FAST of levels 0 .. G-1,
FAST of levels G.. as a second launch behind both.

No kernel changes with the switch, only the order and the streams of the launches: every output, every pyramid level and every
level's FAST candidates must be the bytes of the unsplit order (G = 0) and of the oracle.  A FAST launch that read a level before
its resize had finished would show as a different candidate set of that level.  The shapes are the smallest that take the batch
paths (24 frames: the strip form of FAST, one level per resize launch); ORBX_VAR_RESIZE_LDS = 2 forces the pyramid kernel a large
resident batch runs, ORBX_VAR_FAST = 2 the strip form."""
import numpy as np
import pytest

from monoorbslam3_amd import synth

import test_extractor_gpu as xt
import test_pipeline_gpu as tp

pytestmark = pytest.mark.gpu

B = 24
LDS = 8                      # ORBX_PYRAMID_SPLIT_LDS: the side chain on k_resize_lds (the measurement control)
BASE = {"resize_lds": "always", "fast": "strips"}
SHAPES = {(320, 240): 500, (1242, 375): 2000}   # (w, h) -> features
SAMPLED = (0, B // 2, B - 1)

_base = {}   # (w, h, levels) -> the G = 0 run


def _variants(g):
    return dict(BASE, pyramid_split=g)


def _run(ex, imgs, levels, taps=True):
    """one host-API batch: counts, key points and descriptors of every frame, every level and its sorted candidates"""
    n, h, w = imgs.shape
    out = ex.extract_batch(imgs)
    r = dict(out=out, levels={}, cand={})
    if taps:
        for f in range(n):
            for l in range(levels):
                r["levels"][f, l] = ex.tap_level(f, l, w, h)
                xs, ys, rs = ex.tap_candidates(f, l, cap=1 << 16)
                r["cand"][f, l] = np.sort(xs.astype(np.int64) | (ys.astype(np.int64) << 16) | (rs.astype(np.int64) << 32))
    return r


def _imgs(w, h):
    return synth.make_frames(B, w, h, seed=7 * w + h)


def _baseline(oracle_mod, w, h, levels):
    key = (w, h, levels)
    if key not in _base:
        ex, orc = xt._mk(oracle_mod, SHAPES[w, h], w, h, n_levels=levels, batch=B, variants=_variants(0))
        imgs = _imgs(w, h)
        r = _run(ex, imgs, levels)
        for f in SAMPLED:   # the unsplit order itself is the oracle's, stage by stage
            xt._check_frame(ex, orc, imgs[f], r["out"][f][0], r["out"][f][1], frame=f, stages=True)
        assert min(len(k) for k, _ in r["out"]) > 0
        assert all(len(r["cand"][0, l]) > 0 for l in range(levels))
        _base[key] = r
    return _base[key]


def _same(got, want, levels, where):
    assert [len(k) for k, _ in got["out"]] == [len(k) for k, _ in want["out"]], where
    for f, ((kp, desc), (kp0, desc0)) in enumerate(zip(got["out"], want["out"])):
        assert kp.tobytes() == kp0.tobytes(), "%s: key points of frame %d (angle bits included)" % (where, f)
        assert np.array_equal(desc, desc0), "%s: descriptors of frame %d" % (where, f)
    for (f, l), lv in got["levels"].items():
        assert np.array_equal(lv, want["levels"][f, l]), "%s: level %d of frame %d" % (where, l, f)
        assert np.array_equal(got["cand"][f, l], want["cand"][f, l]), "%s: FAST candidates of level %d, frame %d" % (where, l, f)
    assert len(got["levels"]) == len(want["levels"]) == B * levels


@pytest.mark.parametrize("g", [2, 4, 6, LDS + 4, -1], ids=["G2", "G4", "G6", "G4-lds", "auto"])
@pytest.mark.parametrize("w,h", list(SHAPES))
def test_split_gives_the_bytes_of_the_unsplit_order(oracle_mod, w, h, g):
    """24 frames, 8 levels: counts, key points (all seven fields, bit for bit), descriptors, every level and every level's
    candidate set of every frame equal the G = 0 run; sampled frames equal the oracle.  (auto: the default, which splits at level 3
    where the pyramid is k_resize_lds's, as it is forced to be here.)"""
    want = _baseline(oracle_mod, w, h, 8)
    ex, orc = xt._mk(oracle_mod, SHAPES[w, h], w, h, batch=B, variants=_variants(g))
    assert ex.get_variant("pyramid_split") == g
    imgs = _imgs(w, h)
    got = _run(ex, imgs, 8)
    _same(got, want, 8, "%dx%d, pyramid_split=%d" % (w, h, g))
    for f in SAMPLED:
        xt._check_frame(ex, orc, imgs[f], got["out"][f][0], got["out"][f][1], frame=f, stages=False)
    # the same handle again (its events and the side stream are reused from call to call), and switched off again
    again = _run(ex, imgs, 8, taps=False)
    ex.set_variant("pyramid_split", 0)
    off = _run(ex, imgs, 8, taps=False)
    for r in (again, off):
        for (kp, desc), (kp0, desc0) in zip(r["out"], want["out"]):
            assert kp.tobytes() == kp0.tobytes() and np.array_equal(desc, desc0)


@pytest.mark.parametrize("g,groups", [(2, 2), (3, 1), (6, 1), (-1, 1)])
def test_split_level_at_the_edges_of_a_three_level_pyramid(oracle_mod, g, groups):
    """3 levels: G = 2 leaves one level on the side stream, G >= n_levels is the unsplit order (one resize group, one FAST group
    in timing mode 2); the same bytes every way."""
    w, h = 320, 240
    want = _baseline(oracle_mod, w, h, 3)
    ex, orc = xt._mk(oracle_mod, SHAPES[w, h], w, h, n_levels=3, batch=B, variants=_variants(g))
    ex.set_stage_timing(2)
    imgs = _imgs(w, h)
    got = _run(ex, imgs, 3)
    _same(got, want, 3, "3 levels, pyramid_split=%d" % g)
    for f in (0, B - 1):
        xt._check_frame(ex, orc, imgs[f], got["out"][f][0], got["out"][f][1], frame=f, stages=False)
    n = ex.stage_groups_in_step()
    assert n["resize"] == groups and n["fast"] == groups, n


def test_switch_range():
    from monoorbslam3_amd._lib import OrbxError
    from monoorbslam3_amd.extractor import ORBExtractor
    ex = ORBExtractor(500, 1.2, 8, 20, 7, max_width=320, max_height=240, max_batch=1)
    assert ex.get_variant("pyramid_split") == -1   # by call size
    for bad in (-2, 1, 7, LDS, LDS + 1, LDS + 7, 16):
        with pytest.raises(OrbxError):
            ex.set_variant("pyramid_split", bad)
    for ok in (0, 2, 6, LDS + 2, LDS + 6, -1):
        ex.set_variant("pyramid_split", ok)
        assert ex.get_variant("pyramid_split") == ok


def test_stream_wait_fast_orders_behind_both_fast_launches(oracle_mod, monkeypatch):
    """Two overlapped steps in bench.py's layout (extraction on a side stream into two output sets, the resident best-2 match of
    the first step behind orbx_stream_wait_fast of the second) at 32 frames of 640 x 360 with the split on: both archived sets
    equal the oracle on sampled frames, and the match rows the C oracle's popcount scan of frame f against f + 1."""
    from monoorbslam3_amd.extractor import KP_DTYPE
    monkeypatch.setattr(tp, "N_STEPS", 2)
    case = "pyramid-split"
    cfg = dict(w=640, h=360, b=32, lagged=True, resident=1, variants=_variants(4))
    W, H, Bp = cfg["w"], cfg["h"], cfg["b"]
    geom = (W, H, Bp)
    r = tp._run_pipeline(case, cfg)
    arch, cap = r["arch"], r["cap"]
    check = {k: tp._sampled(case, Bp, k) for k in range(2)}
    keys, pairs = set(), set()
    for k, frames in check.items():
        for f in frames:
            q = (k, (f + 1) % Bp)
            keys.update([(k, f), q])
            pairs.add(((k, f), q))
    tp._prefetch(oracle_mod, geom, keys, pairs)
    for k, frames in check.items():
        host = {name: t[frames].cpu().numpy() for name, t in arch[k].items()}
        for j, f in enumerate(frames):
            where = "step %d, frame %d" % (k, f)
            okp, odesc = tp._extract_cache[geom + (k, f)]
            n = int(host["n"][j])
            assert n == len(okp) and n > 0, "%s: n_keypoints %d, oracle %d" % (where, n, len(okp))
            got = np.ascontiguousarray(host["kp"][j, :n]).view(KP_DTYPE).reshape(-1)
            for fld in tp.KP_FIELDS:
                assert np.array_equal(tp._bits(got[fld]), tp._bits(okp[fld])), "%s: key-point field %s" % (where, fld)
            assert np.array_equal(host["desc"][j, :n], odesc), "%s: descriptors" % where
            r_bi, r_bd, r_sd = tp._best2_cache[(geom + (k, f), geom + (k, (f + 1) % Bp))]
            assert np.array_equal(host["bidx"][j, :n], r_bi), "%s: match index" % where
            assert np.array_equal(host["bd"][j, :n].view(np.uint16), r_bd), "%s: best distance" % where
            assert np.array_equal(host["sd"][j, :n].view(np.uint16), r_sd), "%s: second distance" % where
            assert np.all(host["bidx"][j, n:] == -1), "%s: match rows past the count" % where
    # the two steps had different inputs: stale outputs cannot pass
    assert tp._extract_cache[geom + (0, 0)][0].tobytes() != tp._extract_cache[geom + (1, 0)][0].tobytes()


def test_stage_timing_with_the_split_on(oracle_mod):
    """Mode 1 keeps the serial order on one stream; mode 2 keeps the split and brackets the two resize groups (one per stream) and
    the two FAST launches.  Positive, finite times either way, and the bytes of the unsplit order."""
    from monoorbslam3_amd.extractor import STAGES
    w, h = 320, 240
    want = _baseline(oracle_mod, w, h, 8)
    ex, _ = xt._mk(oracle_mod, SHAPES[w, h], w, h, batch=B, variants=_variants(4))
    imgs = _imgs(w, h)
    for mode in (1, 2):
        ex.set_stage_timing(mode)
        got = _run(ex, imgs, 8, taps=(mode == 2))
        if mode == 2:
            _same(got, want, 8, "timing mode 2")
        for (kp, desc), (kp0, desc0) in zip(got["out"], want["out"]):
            assert kp.tobytes() == kp0.tobytes() and np.array_equal(desc, desc0), mode
        st = ex.stage_times_ms() if mode == 1 else ex.stage_times_in_step_ms()
        assert list(st) == list(STAGES)
        assert all(np.isfinite(v) and v >= 0 for v in st.values()), (mode, st)
        for name in ("resize", "fast", "octree", "orient", "desc"):
            assert st[name] > 0, (mode, name, st)
        if mode == 2:
            n = ex.stage_groups_in_step()
            assert n["resize"] == 2 and n["fast"] == 2, n
            assert ex.fast_time_in_step_ms() == (st["fast"], 2)
