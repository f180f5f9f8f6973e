"""The batch quadtree and k_desc_bins behind the XCD-balanced workgroup mapping (orbx_xcd_map_levels): every frame of a
batch against the CPU oracle, stages included.

The mapping only decides which workgroup takes which (frame, level), so every frame must come out as before -- a wrong
mapping shows as a frame or a level that is missing, done twice or written to another frame's slot.  The shapes are the
smallest that still take the 256-thread batch build (frames x levels > 512; asserted through orbx_dev_octree_plan): frame
counts that are no multiple of 8 (surplus workgroups), level counts that do not divide 8 or lie below it, the one-pass
descriptor path (k_desc_bins, whose levels per frame are the fused levels), and a batch split over two sub-streams (two
launches, each with its own frame count, the second with a frame offset)."""
import ctypes as C

import numpy as np
import pytest

from monoorbslam3_amd import synth

pytestmark = pytest.mark.gpu


def _check_frame(ex, orc, img, kps, desc, frame):
    """tests/test_extractor_gpu.py's check of one frame, every stage"""
    h, w = img.shape
    okps, odesc, ocounts = orc.extract(img)
    pyr = orc.pyramid(img)
    for l in range(orc.n_levels):
        assert np.array_equal(ex.tap_level(frame, l, w, h, blurred=False), pyr[l]), "frame %d: pyramid level %d differs" % (frame, l)
        assert np.array_equal(ex.tap_level(frame, l, w, h, blurred=True), orc.blur(pyr[l])), "frame %d: blurred level %d differs" % (frame, l)
        xs, ys, rs = ex.tap_candidates(frame, l)
        oc = orc.level_candidates(pyr[l])
        got_set = sorted(zip(ys.tolist(), xs.tolist(), rs.tolist()))
        ref_set = sorted(zip(oc["y"].astype(int).tolist(), oc["x"].astype(int).tolist(), oc["response"].astype(int).tolist()))
        assert got_set == ref_set, "frame %d: FAST candidates differ at level %d" % (frame, l)
    assert ex.tap_level_counts(frame).tolist() == ocounts, "frame %d" % frame
    assert len(kps) == len(okps), "frame %d" % frame
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        assert np.array_equal(kps[f], okps[f]), "frame %d: %s" % (frame, f)
    assert np.array_equal(kps["angle"], okps["angle"]), "frame %d" % frame
    assert np.array_equal(desc, odesc), "frame %d" % frame
    return len(okps)


def _plan_kind(nf, sf, levels, w, h, frames):
    from monoorbslam3_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    fn = L.orbx_dev_octree_plan
    fn.restype = C.c_int
    fn.argtypes = [C.POINTER(_lib.OrbxCfg), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int64)]
    cfg = _lib.OrbxCfg(nf, sf, levels, 20, 7, w, h, frames, 0, -1)
    out = (C.c_int64 * 4)()
    assert fn(C.byref(cfg), 0, w, h, frames, 0, levels, out) == 0
    return out[0]


# w, h, levels, scale, features, frames, variants, frames of each launch
CASES = {
    "65_frames_fused_descriptors": (320, 240, 8, 1.2, 500, 65, {"desc": "fused"}, (65,)),
    "12_levels_43_frames": (400, 200, 12, 1.1, 600, 43, {}, (43,)),
    "4_levels_136_frames": (256, 160, 4, 1.5, 300, 136, {}, (136,)),
    "two_sub_streams_65_and_66_frames": (320, 240, 8, 1.2, 500, 131, {"streams": 2}, (65, 66)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_every_frame_of_a_batch_equals_the_oracle(oracle_mod, case):
    import torch
    from monoorbslam3_amd.extractor import ORBExtractor, KP_DTYPE
    w, h, levels, sf, nf, frames, variants, launches = CASES[case]
    assert sum(launches) == frames
    for n in launches:  # every launch takes the batch build, the one behind the mapping
        assert n * levels > 512 and _plan_kind(nf, sf, levels, w, h, n) == 0
    ex = ORBExtractor(nf, sf, levels, 20, 7, max_width=w, max_height=h, max_batch=frames, variants=variants)
    orc = oracle_mod.Oracle(nf, sf, levels, 20, 7)
    imgs = synth.make_frames(frames, w, h, seed=7 * w + frames)
    res = ex.extract_batch(imgs)
    totals = [_check_frame(ex, orc, imgs[f], res[f][0], res[f][1], f) for f in range(frames)]
    assert min(totals) > nf // 2
    if "desc" in variants:
        # the frame's count is written by its level-0 workgroup of k_desc_bins: device entry point, every frame
        cap = ex.max_keypoints(w, h)
        d_img = torch.from_numpy(imgs).cuda()
        d_kp = torch.zeros((frames, cap, 28), dtype=torch.uint8, device="cuda")
        d_desc = torch.zeros((frames, cap, 32), dtype=torch.uint8, device="cuda")
        d_n = torch.full((frames,), -1, dtype=torch.int32, device="cuda")
        ex.extract_batch_device(d_img.data_ptr(), frames, w, h, w, w * h, d_kp.data_ptr(), d_desc.data_ptr(), cap, d_n.data_ptr())
        ex.synchronize()
        n = d_n.cpu().numpy()
        kp, de = d_kp.cpu().numpy(), d_desc.cpu().numpy()
        for f in range(frames):
            assert n[f] == int(ex.tap_level_counts(f).sum()) == totals[f], "frame %d" % f
            assert np.array_equal(kp[f, :n[f]].copy().view(KP_DTYPE).reshape(-1), res[f][0]), "frame %d" % f
            assert np.array_equal(de[f, :n[f]], res[f][1]), "frame %d" % f
