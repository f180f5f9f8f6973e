"""The overlapped extract-and-match pipeline that bench.py times, rebuilt in-process from the library's API, with frames that
change every step; and the stage-timing entry points (orbx_set_stage_timing, orbx_stage_times_ms, orbx_stage_times_in_step_ms,
orbx_fast_times_in_step_ms).

bench.py main() runs the extraction of step k on a side stream into output set k % 2 and the best-2 match of a set on a second
stream, either behind the NEXT batch's FAST stage (orbx_stream_wait_fast, k_best2_fp4 as one workgroup per CU) or right behind its
own extraction.  Two events per set order the streams: ev_extracted (the match may read the set) and ev_matched (the next
extraction may overwrite it).  The bench extracts the same resident frames every step, so a missing dependency there rewrites the
same bytes and goes unseen.  Here every step gets an input batch of its own, behind each match the set is copied into a per-step
archive on the match stream, and afterwards every archived step is compared with the C oracle."""
import os
import threading
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from monoorbslam3_amd import synth

pytestmark = pytest.mark.gpu

NF = 2000
WARMUP, STEPS = 1, 6              # one warm-up step, then K timed steps: every one of them is archived and checked
N_STEPS = WARMUP + STEPS
SEED0 = 1000                      # step k extracts synth.make_frames(B, W, H, seed=SEED0 + k)
SENTINEL = 0xA5                   # every output buffer holds this byte before the first step
KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
# bench.py --records: camera and vocabulary of its frame records
CAM = dict(fx=718.856, fy=718.856, dist=(-0.2834, 0.0739, 1.9e-4, 1.8e-5))
LEVELSUP = 4

# what bench.py can run: (width, height, batch, lagged match placement, ORBM_VAR_BEST2_RESIDENT, extractor variants, records,
# timing mode)
CASES = {
    "after-fast": dict(w=1242, h=375, b=64, lagged=True, resident=1),
    "after-fast-timing2": dict(w=1242, h=375, b=64, lagged=True, resident=1, timing=2),
    "eager": dict(w=1242, h=375, b=64, lagged=False, resident=0),
    "streams2": dict(w=1242, h=375, b=64, lagged=True, resident=1, variants={"streams": 2}),
    "records": dict(w=1242, h=375, b=64, lagged=True, resident=1, records=True),
    "config4": dict(w=1920, h=1080, b=1, lagged=False, resident=0),
}

# The inputs and the oracle's answers are the same for every case of one geometry: computed once per session.
_frames_cache = {}     # (w, h, b, step) -> (b, h, w) u8
_extract_cache = {}    # (w, h, b, step, frame) -> (key points, descriptors)
_best2_cache = {}      # ((w, h, b, step, frame), (w, h, b, step, frame)) -> (index, best, second)
_tls = threading.local()


def _frames(w, h, b, step):
    key = (w, h, b, step)
    if key not in _frames_cache:
        _frames_cache[key] = synth.make_frames(b, w, h, seed=SEED0 + step)
    return _frames_cache[key]


def _workers():
    return max(1, min(16, os.cpu_count() or 1))


def _prefetch(oracle_mod, geom, keys, pairs=()):
    """Oracle.extract of every (step, frame) in `keys` and C best2 of every ((step, frame), (step, frame)) in `pairs`, on a thread
    pool (the ctypes calls release the GIL).  Both land in the session caches."""
    w, h, b = geom
    todo = sorted({(w, h, b) + k for k in keys} - set(_extract_cache))
    for k in todo:
        _frames(*k[:4])

    def extract(k):
        if not hasattr(_tls, "orc"):
            _tls.orc = oracle_mod.Oracle(NF, 1.2, 8, 20, 7)
        kps, desc, _ = _tls.orc.extract(_frames(*k[:4])[k[4]])
        return k, (kps, desc)

    with ThreadPoolExecutor(_workers()) as pool:
        for k, r in pool.map(extract, todo):
            _extract_cache[k] = r
        todo = sorted({((w, h, b) + p, (w, h, b) + q) for p, q in pairs} - set(_best2_cache))
        for pq, r in pool.map(lambda pq: (pq, oracle_mod.best2(_extract_cache[pq[0]][1], _extract_cache[pq[1]][1])), todo):
            _best2_cache[pq] = r


def _sampled(case, b, step):
    """the frames of a step whose outputs are checked: the first two, both sides of the middle, the last two, two seeded picks"""
    if b == 1:
        return [0]
    fixed = [0, 1, b // 2 - 1, b // 2, b - 2, b - 1]
    rest = [f for f in range(b) if f not in fixed]
    pick = np.random.RandomState(zlib.crc32(case.encode()) + step).choice(rest, 2, replace=False)
    return sorted(fixed + [int(f) for f in pick])


def _first_diff(a, b):
    d = np.nonzero(np.asarray(a) != np.asarray(b))[0]
    return int(d[0]) if len(d) else -1


def _run_pipeline(case, cfg):
    """bench.py main()'s step() / launch_match() / flush() with a distinct input batch per step, an archive of every step taken on
    the match stream behind its match, and (timing mode 2) the in-step stage times read after every step from the third on.
    Returns the archives (device tensors), the live output sets and the mode-2 readings."""
    import torch
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.extractor import ORBExtractor
    from monoorbslam3_amd.matcher import MatcherHandle, _mlib
    W, H, B = cfg["w"], cfg["h"], cfg["b"]
    dev = torch.device("cuda", 0)
    ex = ORBExtractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B, device=0, variants=cfg.get("variants", {}))
    if cfg.get("timing"):
        ex.set_stage_timing(cfg["timing"])
    cap = ex.max_keypoints(W, H)
    mh = MatcherHandle(device=0)
    mh.set_variant("best2", "fp4")
    mh.set_variant("best2_resident", cfg["resident"])
    ML = _mlib()
    d_in = [torch.from_numpy(_frames(W, H, B, k)).to(dev) for k in range(N_STEPS)]
    z = lambda shape, dt: [torch.empty(shape, dtype=dt, device=dev) for _ in range(2)]  # noqa: E731
    bufs = dict(n=z((B,), torch.int32), kp=z((B, cap, 28), torch.uint8), desc=z((B, cap, 32), torch.uint8),
                bidx=z((B, cap), torch.int32), bd=z((B, cap), torch.int16), sd=z((B, cap), torch.int16))
    fpost = voc = None
    if cfg.get("records"):   # bench.py --records: undistortion + grid (orbf) and bag of words (orbv), chained on the side stream
        from monoorbslam3_amd.frame import FramePost
        from monoorbslam3_amd.vocabulary import ORBVocabulary
        fpost = FramePost(W, H, CAM["fx"], CAM["fy"], W / 2.0, H / 2.0, dist=CAM["dist"], device=0)
        voc = ORBVocabulary.from_arrays(_vocabulary(), device=0)
        bufs.update(kp_un=z((B, cap, 28), torch.uint8), cell_start=z((B, fpost.n_cells + 1), torch.int32),
                    cell_items=z((B, cap), torch.int32), bow_ids=z((B, cap), torch.int32), bow_vals=z((B, cap), torch.float64),
                    n_words=z((B,), torch.int32), fv_nodes=z((B, cap), torch.int32), fv_off=z((B, cap + 1), torch.int32),
                    fv_idx=z((B, cap), torch.int32), n_fv=z((B,), torch.int32))
    for ts in bufs.values():
        for t in ts:
            t.view(torch.uint8).fill_(SENTINEL)
    arch = [{name: torch.empty_like(ts[0]) for name, ts in bufs.items()} for _ in range(N_STEPS)]
    for a in arch:
        for t in a.values():
            t.view(torch.uint8).fill_(SENTINEL)
    p = {name: [t.data_ptr() for t in ts] for name, ts in bufs.items()}
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    mstream = torch.cuda.Stream(device=dev)
    assert side.cuda_stream != 0 and mstream.cuda_stream != 0
    ev_extracted = [torch.cuda.Event() for _ in range(2)]
    ev_matched = [torch.cuda.Event() for _ in range(2)]

    def match(i, st):   # bench.py match(): frame f against f + 1, the last frame against frame 0 (B = 1: the previous step's)
        if B > 1:
            _lib.check(ML.orbm_best2_device(mh._h, B - 1, p["desc"][i], cap, p["n"][i], cap, p["desc"][i] + cap * 32, cap,
                                            p["n"][i] + 4, cap, None, None, p["bidx"][i], p["bd"][i], p["sd"][i], st))
        o = i if B > 1 else (i + 1) % 2
        _lib.check(ML.orbm_best2_device(mh._h, 1, p["desc"][i] + (B - 1) * cap * 32, cap, p["n"][i] + 4 * (B - 1), cap,
                                        p["desc"][o], cap, p["n"][o], cap, None, None, p["bidx"][i] + 4 * (B - 1) * cap,
                                        p["bd"][i] + 2 * (B - 1) * cap, p["sd"][i] + 2 * (B - 1) * cap, st))

    def launch_match(i, k):
        mstream.wait_event(ev_extracted[i])
        match(i, mstream.cuda_stream)
        with torch.cuda.stream(mstream):   # the one addition to the bench's stream graph: archive the set behind its match
            for name, t in arch[k].items():
                t.copy_(bufs[name][i])
        ev_matched[i].record(mstream)

    pending = [None]
    timings = []

    def step(k):
        i = k % 2
        side.wait_event(ev_matched[i])       # set i is free once its previous match (and archive copy) has finished ...
        if B == 1:
            # ... and, one frame per step, once the match of step k - 1 has finished too: that match compares set 1 - i with
            # set i (the previous step's frame), so it READS set i.  bench.py waits on ev_matched[i] only, which was recorded
            # behind the match of step k - 2: extraction k can then overwrite descriptors the match of step k - 1 is reading.
            side.wait_event(ev_matched[1 - i])
        t0 = time.perf_counter()
        ex.extract_batch_device(d_in[k].data_ptr(), B, W, H, W, W * H, p["kp"][i], p["desc"][i], cap, p["n"][i], side.cuda_stream)
        if fpost is not None:
            fpost.post_device(B, p["kp"][i], p["n"][i], cap, p["kp_un"][i], p["cell_start"][i], p["cell_items"][i], side.cuda_stream)
            voc.transform_device(B, p["desc"][i], p["n"][i], cap, LEVELSUP, p["bow_ids"][i], p["bow_vals"][i], p["n_words"][i],
                                 p["fv_nodes"][i], p["fv_off"][i], p["fv_idx"][i], p["n_fv"][i], side.cuda_stream)
        ev_extracted[i].record(side)
        if cfg["lagged"]:
            if pending[0] is not None:
                ex.stream_wait_fast(mstream.cuda_stream)   # the previous batch's match: behind THIS batch's FAST
                launch_match(*pending[0])
            pending[0] = (i, k)
        else:
            launch_match(i, k)
        if cfg.get("timing") == 2 and k >= 2:   # as bench.py reads them: after the step, from the third step on
            st = ex.stage_times_in_step_ms()
            fast = ex.fast_time_in_step_ms()
            timings.append((k, st, fast, (time.perf_counter() - t0) * 1e3))

    for k in range(N_STEPS):
        step(k)
    if pending[0] is not None:   # flush()
        launch_match(*pending[0])
    torch.cuda.synchronize()
    return dict(arch=arch, bufs=bufs, cap=cap, timings=timings)


_voc = []


def _vocabulary():
    if not _voc:   # bench.py --records: a synthetic ORBvoc-sized tree (10 children, 6 levels)
        _voc.append(synth.make_vocabulary(10, 6, seed=1, p_early_leaf=0.0, p_stop=0.0))
    return _voc[0]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("case", list(CASES))
def test_overlapped_steps_as_the_bench_runs_them(oracle_mod, case):
    """Every step of the overlapped pipeline equals the oracle on that step's own input: counts, all seven key-point fields
    bit-exact and the descriptors of sampled frames (every frame of the two live sets), the best-2 rows [0, n) against the C
    oracle's strict-'<' scan of the step's f and f + 1 (the last frame against frame 0; one frame per step: against the previous
    step's frame) and the rows [n, cap) as -1 / 256 / 256; the live sets equal the archives of the last two steps byte for byte.
    Inputs change every step: the oracle's key points of a checked frame differ from those of the same frame one and two steps
    earlier, so stale outputs cannot pass."""
    import torch
    from monoorbslam3_amd.extractor import KP_DTYPE
    cfg = CASES[case]
    W, H, B = cfg["w"], cfg["h"], cfg["b"]
    geom = (W, H, B)
    r = _run_pipeline(case, cfg)
    arch, bufs, cap = r["arch"], r["bufs"], r["cap"]
    live = {(N_STEPS - 1) % 2: N_STEPS - 1, (N_STEPS - 2) % 2: N_STEPS - 2}

    # 1. the live output sets are the last two steps' archives, byte for byte (set 1 included, which bench.py never reads)
    for i, k in sorted(live.items()):
        for name, t in bufs.items():
            assert torch.equal(t[i], arch[k][name]), "%s: live set %d differs from the archive of step %d in %s" % (case, i, k, name)

    # 2. / 3. every step against the oracle: all frames of the live sets' steps, sampled frames of the others
    check = {k: list(range(B)) if k in live.values() else _sampled(case, B, k) for k in range(N_STEPS)}

    def partner(k, f):
        if B > 1:
            return (k, (f + 1) % B)
        return (k - 1, 0) if k > 0 else None   # step 0's partner is the other set before anything was written to it

    keys, pairs = set(), set()
    for k, frames in check.items():
        for f in frames:
            keys.update((k - d, f) for d in (0, 1, 2) if k - d >= 0)
            q = partner(k, f)
            if q is not None:
                keys.add(q)
                pairs.add(((k, f), q))
    _prefetch(oracle_mod, geom, keys, pairs)
    ex_of = lambda k, f: _extract_cache[geom + (k, f)]  # noqa: E731
    ovoc = oracle_mod.Vocabulary(_vocabulary()) if cfg.get("records") else None
    n_checked = 0
    for k in range(N_STEPS):
        frames = check[k]
        sel = torch.tensor(frames, dtype=torch.long, device=arch[k]["n"].device)
        host = {name: t.index_select(0, sel).cpu().numpy() for name, t in arch[k].items()}
        for j, f in enumerate(frames):
            where = "%s: step %d, set %d, frame %d" % (case, k, k % 2, f)
            okp, odesc = ex_of(k, f)
            for back in (1, 2):   # the frame's content really changed from step to step
                if k - back >= 0:
                    prev = ex_of(k - back, f)[0]
                    assert len(prev) != len(okp) or prev.tobytes() != okp.tobytes(), \
                        "%s: the oracle finds the same key points in step %d's input" % (where, k - back)
            n = int(host["n"][j])
            assert n == len(okp), "%s: n_keypoints %d, oracle %d" % (where, n, len(okp))
            want_kp = okp
            if ovoc is not None:   # orbf_frame_post_device scales `size` of the raw records in place
                want_kp, want_un, want_start, want_items = oracle_mod.frame_post(W, H, CAM["fx"], CAM["fy"], W / 2.0, H / 2.0,
                                                                               CAM["dist"], okp)
            got = np.ascontiguousarray(host["kp"][j, :n]).view(KP_DTYPE).reshape(-1)
            for fld in KP_FIELDS:
                bad = _first_diff(_bits(got[fld]), _bits(want_kp[fld]))
                assert bad < 0, "%s: key point %d field %s: %r, oracle %r" % (where, bad, fld, got[fld][bad], want_kp[fld][bad])
            bad = _first_diff(np.any(host["desc"][j, :n] != odesc, axis=1), np.zeros(n, bool))
            assert bad < 0, "%s: descriptor %d differs from the oracle's" % (where, bad)
            q = partner(k, f)
            if q is not None:
                r_bi, r_bd, r_sd = _best2_cache[(geom + (k, f), geom + q)]
                got_m = dict(best_idx=host["bidx"][j], best=host["bd"][j].view(np.uint16), second=host["sd"][j].view(np.uint16))
                for fld, want in (("best_idx", r_bi), ("best", r_bd), ("second", r_sd)):
                    bad = _first_diff(got_m[fld][:n], want)
                    assert bad < 0, "%s: match row %d %s: %d, oracle %d (against step %d frame %d)" % (
                        where, bad, fld, got_m[fld][bad], want[bad], q[0], q[1])
                for fld, want in (("best_idx", -1), ("best", 256), ("second", 256)):
                    bad = _first_diff(got_m[fld][n:], np.full(cap - n, want))
                    assert bad < 0, "%s: match row %d (past the count) %s: %d, want %d" % (where, n + bad, fld, got_m[fld][n + bad], want)
            if ovoc is not None:
                assert host["kp_un"][j, :n].tobytes() == want_un.tobytes(), "%s: undistorted key points" % where
                assert np.array_equal(host["cell_start"][j], want_start), "%s: grid cell_start" % where
                assert np.array_equal(host["cell_items"][j, :want_start[-1]], want_items), "%s: grid cell_items" % where
                bi, bv, (fn, fo, fi) = ovoc.transform(odesc, LEVELSUP)
                nw, nfv = int(host["n_words"][j]), int(host["n_fv"][j])
                assert nw == len(bi), "%s: BoW words %d, oracle %d" % (where, nw, len(bi))
                assert np.array_equal(host["bow_ids"][j, :nw].view(np.uint32), bi), "%s: BoW word ids" % where
                assert host["bow_vals"][j, :nw].tobytes() == bv.tobytes(), "%s: BoW values" % where
                assert nfv == len(fn), "%s: feature-vector nodes %d, oracle %d" % (where, nfv, len(fn))
                assert np.array_equal(host["fv_nodes"][j, :nfv].view(np.uint32), fn), "%s: feature-vector node ids" % where
                assert np.array_equal(host["fv_off"][j, :nfv + 1], fo), "%s: feature-vector offsets" % where
                assert np.array_equal(host["fv_idx"][j, :fo[-1]].view(np.uint32), fi), "%s: feature-vector indices" % where
            n_checked += 1
    assert n_checked >= (2 * B + 8 * (N_STEPS - 2) if B > 1 else N_STEPS)

    # timing mode 2 inside the overlapped steps: as bench.py reads it, every stage within the host span of its step
    if cfg.get("timing") == 2:
        from monoorbslam3_amd.extractor import STAGES
        assert [t[0] for t in r["timings"]] == list(range(2, N_STEPS))
        for k, st, (fast_ms, n_fast), span_ms in r["timings"]:
            assert list(st) == list(STAGES), k
            for name, v in st.items():
                assert np.isfinite(v) and v >= 0, (k, name, v)
                assert v <= span_ms, "step %d: stage %s %.4f ms, host span of the step %.4f ms" % (k, name, v, span_ms)
            assert st["fast"] > 0, (k, st)
            assert fast_ms == st["fast"] and n_fast in (1, 2), (k, fast_ms, n_fast, st)


def test_stream_wait_fast_arguments():
    """orbx_stream_wait_fast refuses a handle that has enqueued no batched call yet, and stream 0 (NULL)"""
    import torch
    from monoorbslam3_amd._lib import OrbxError
    from monoorbslam3_amd.extractor import ORBExtractor
    W, H, B = 320, 240, 2
    ex = ORBExtractor(500, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B, device=0)
    s = torch.cuda.Stream()
    with pytest.raises(OrbxError) as e:
        ex.stream_wait_fast(s.cuda_stream)
    assert e.value.code == -1
    cap = ex.max_keypoints(W, H)
    img = torch.from_numpy(synth.make_frames(B, W, H, seed=3)).cuda()
    kp = torch.empty((B, cap, 28), dtype=torch.uint8, device="cuda")
    desc = torch.empty((B, cap, 32), dtype=torch.uint8, device="cuda")
    n = torch.empty(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(img.data_ptr(), B, W, H, W, W * H, kp.data_ptr(), desc.data_ptr(), cap, n.data_ptr(), s.cuda_stream)
    with pytest.raises(OrbxError) as e:
        ex.stream_wait_fast(0)
    assert e.value.code == -1
    other = torch.cuda.Stream()
    ex.stream_wait_fast(other.cuda_stream)   # and a real stream is accepted
    other.synchronize()
    s.synchronize()
    assert int(n.min()) > 0


def _one_batch(ex, d_img, W, H, B, stream):
    """one extraction of the batch into fresh sentinel-filled buffers; returns (host counts, key points, descriptors, host span ms)"""
    import torch
    cap = ex.max_keypoints(W, H)
    kp = torch.full((B, cap, 28), SENTINEL, dtype=torch.uint8, device=d_img.device)
    desc = torch.full((B, cap, 32), SENTINEL, dtype=torch.uint8, device=d_img.device)
    n = torch.full((B,), -7, dtype=torch.int32, device=d_img.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ex.extract_batch_device(d_img.data_ptr(), B, W, H, W, W * H, kp.data_ptr(), desc.data_ptr(), cap, n.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    span = (time.perf_counter() - t0) * 1e3
    return n.cpu().numpy(), kp.cpu().numpy(), desc.cpu().numpy(), span


def test_stage_timing_does_not_change_results(oracle_mod):
    """Timing modes 0, 1 and 2 give the same bytes on one distinct 64-frame batch at 1242 x 375 (mode 1 runs every kernel on one
    stream without the side blur: a different stream layout), and those bytes are the oracle's for the first and last frame."""
    import torch
    from monoorbslam3_amd.extractor import ORBExtractor, KP_DTYPE
    W, H, B = 1242, 375, 64
    d_img = torch.from_numpy(_frames(W, H, B, 0)).cuda()
    ex = ORBExtractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B, device=0)
    s = torch.cuda.Stream()
    outs = {}
    for mode in (0, 1, 2, 0):
        ex.set_stage_timing(mode)
        outs.setdefault(mode, []).append(_one_batch(ex, d_img, W, H, B, s))
    n0, kp0, desc0, _ = outs[0][0]
    assert n0.min() > 500 and n0.max() <= kp0.shape[1]
    for mode, runs in outs.items():
        for n, kp, desc, _ in runs:
            assert np.array_equal(n, n0), mode
            for f in range(B):
                assert kp[f, :n[f]].tobytes() == kp0[f, :n0[f]].tobytes(), (mode, f, "key points")
                assert desc[f, :n[f]].tobytes() == desc0[f, :n0[f]].tobytes(), (mode, f, "descriptors")
    _prefetch(oracle_mod, (W, H, B), [(0, 0), (0, B - 1)])
    for f in (0, B - 1):
        okp, odesc = _extract_cache[(W, H, B, 0, f)]
        assert n0[f] == len(okp) and kp0[f, :n0[f]].tobytes() == okp.astype(KP_DTYPE).tobytes(), f
        assert np.array_equal(desc0[f, :n0[f]], odesc), f


@pytest.mark.parametrize("desc", ["auto", "separate"])
def test_stage_times_mode1(desc):
    """Timing mode 1: six finite values >= 0; resize, FAST, quadtree, orientation and descriptors take time (with the separate
    blur pass, ORBX_VAR_DESC = separate, so does the blur); the events sit inside the call, so their sum is at most the host-clock
    span of the call plus the synchronisation."""
    import torch
    from monoorbslam3_amd.extractor import ORBExtractor, STAGES
    W, H, B = 1242, 375, 64
    d_img = torch.from_numpy(_frames(W, H, B, 1)).cuda()
    ex = ORBExtractor(NF, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B, device=0, variants={"desc": desc})
    ex.set_stage_timing(1)
    s = torch.cuda.Stream()
    for _ in range(2):   # the first call also sets the handle up; both are timed
        n, _, _, span = _one_batch(ex, d_img, W, H, B, s)
        st = ex.stage_times_ms()
        assert list(st) == list(STAGES)
        assert all(np.isfinite(v) and v >= 0 for v in st.values()), st
        for name in ("resize", "fast", "octree", "orient", "desc"):
            assert st[name] > 0, (name, st)
        if desc == "separate":
            assert st["blur"] > 0, st
        assert sum(st.values()) <= span, (st, span)
        assert n.min() > 500


def test_stage_timing_refusals():
    """stage_times_ms needs a call in mode 1 (a fresh handle, and one switched back to mode 0, refuse); stage_times_in_step_ms
    needs mode 2; mode 2 with the batch split over internal streams (ORBX_VAR_STREAMS = 2, B >= 16) is ORBX_E_UNSUPPORTED"""
    import torch
    from monoorbslam3_amd._lib import OrbxError
    from monoorbslam3_amd.extractor import ORBExtractor
    W, H, B = 640, 360, 16
    d_img = torch.from_numpy(synth.make_frames(B, W, H, seed=11)).cuda()
    s = torch.cuda.Stream()
    ex = ORBExtractor(800, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B, device=0)
    for query in (ex.stage_times_ms, ex.stage_times_in_step_ms, ex.fast_time_in_step_ms):
        with pytest.raises(OrbxError):
            query()
    ex.set_stage_timing(1)
    _one_batch(ex, d_img, W, H, B, s)
    assert ex.stage_times_ms()["fast"] > 0
    with pytest.raises(OrbxError):
        ex.stage_times_in_step_ms()
    ex.set_stage_timing(0)
    with pytest.raises(OrbxError):
        ex.stage_times_ms()
    ex.set_stage_timing(2)
    _one_batch(ex, d_img, W, H, B, s)
    assert ex.stage_times_in_step_ms()["fast"] > 0
    ex2 = ORBExtractor(800, 1.2, 8, 20, 7, max_width=W, max_height=H, max_batch=B, device=0, variants={"streams": 2})
    ex2.set_stage_timing(2)
    n, _, _, _ = _one_batch(ex2, d_img, W, H, B, s)
    assert n.min() > 0
    for query in (ex2.stage_times_in_step_ms, ex2.fast_time_in_step_ms):
        with pytest.raises(OrbxError) as e:
            query()
        assert e.value.code == -4, e.value   # ORBX_E_UNSUPPORTED
