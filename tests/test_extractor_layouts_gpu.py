"""The extractor on the level-0 layouts real callers hand over: pitched rows, gaps between frames, unaligned bases.

include/orbx.h ("Layout of the caller's image"): any stride >= width, any frame stride, any byte alignment; the bytes
between rows and between frames never influence a result, nothing of the caller's image is written, nothing outside
[frame 0's first pixel, the last frame's last pixel] is read.  Level 0 is a special case in every launcher (the caller's
pitch and frame stride instead of the arena's, packed 8- and 16-byte loads on rows that are neither aligned nor padded),
and every other test passes dense rows in a fresh allocation.

Every device case asserts: (a) every stage bit for bit against the oracle run on the dense copy of the frames, (b) the
same bytes whatever fills the pad, (c) the caller's allocation unchanged, (d) the outputs' guards and the records past
each frame's count unchanged, (e) the same bytes as the dense call on the same handle.  The image always lies in the
middle of its allocation with 64 KiB either side: these tests are about results, not about where a load may land.
tests/test_extractor_layouts_cpu.py shows on the oracle that the frames are not vacuous and that the fill, read as
pixels, would change FAST's candidates and the blur.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

from test_extractor_gpu import _check_frame, _mk
from test_extractor_layouts_cpu import layout_frames, layouts

pytestmark = pytest.mark.gpu

GUARD = 65536
OUT_FILL = 0xA5
FILLS = (0x00, 0xFF, "random")
ORBX_E_ARG = -1


class _SharedOracle:
    """The oracle's answers, computed once per input and handed (read-only) to every case that asks again."""
    _memo = {}

    def __init__(self, orc, key):
        self._orc, self._key = orc, key

    @property
    def n_levels(self):
        return self._orc.n_levels

    def _once(self, name, img):
        k = (self._key, name, img.shape, img.tobytes())
        if k not in self._memo:
            r = getattr(self._orc, name)(img)
            for a in (r if isinstance(r, (list, tuple)) else [r]):
                if isinstance(a, np.ndarray):
                    a.setflags(write=False)
            self._memo[k] = r
        return self._memo[k]

    def extract(self, img):
        return self._once("extract", img)

    def pyramid(self, img):
        return self._once("pyramid", img)

    def blur(self, img):
        return self._once("blur", img)

    def level_candidates(self, img):
        return self._once("level_candidates", img)


def _handle(oracle_mod, nf, w, h, batch, variants=None):
    ex, orc = _mk(oracle_mod, nf, w, h, batch=batch, variants=variants)
    return ex, _SharedOracle(orc, nf)


def _laid_out(torch, imgs, stride, frame_gap, base_off, fill):
    """ONE allocation of GUARD + base_off + B * frame_stride + GUARD bytes, all of it `fill`, with the frames written at
    GUARD + base_off, rows `stride` and frames `stride * h + frame_gap` bytes apart.  Returns (tensor, pointer to frame 0's
    first pixel, stride, frame_stride)."""
    B, h, w = imgs.shape
    frame_stride = stride * h + frame_gap
    n = GUARD + base_off + B * frame_stride + GUARD
    if fill == "random":
        g = torch.Generator(device="cuda")
        g.manual_seed(20261020)
        t = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda", generator=g)
    else:
        t = torch.full((n,), fill, dtype=torch.uint8, device="cuda")
    t.as_strided((B, h, w), (frame_stride, stride, 1), GUARD + base_off).copy_(torch.from_numpy(np.ascontiguousarray(imgs)).cuda())
    return t, t.data_ptr() + GUARD + base_off, stride, frame_stride


def _guarded(torch, nbytes):
    t = torch.full((GUARD + nbytes + GUARD,), OUT_FILL, dtype=torch.uint8, device="cuda")
    return t, t.data_ptr() + GUARD


def _device_call(torch, ex, ptr, B, w, h, stride, frame_stride, cap):
    """orbx_extract_batch_device into guarded outputs -> the three whole output allocations as host bytes"""
    kp, kp_p = _guarded(torch, B * cap * 28)
    de, de_p = _guarded(torch, B * cap * 32)
    cn, cn_p = _guarded(torch, B * 4)
    ex.extract_batch_device(ptr, B, w, h, stride, frame_stride, kp_p, de_p, cap, cn_p)
    ex.synchronize()
    torch.cuda.synchronize()
    return kp.cpu().numpy(), de.cpu().numpy(), cn.cpu().numpy()


def _records(out, B, cap, f):
    from monoorbslam3_amd.extractor import KP_DTYPE
    kp, de, cn = out
    n = int(cn[GUARD:GUARD + 4 * B].view(np.int32)[f])
    assert 0 <= n <= cap
    kps = kp[GUARD + f * cap * 28:GUARD + (f * cap + n) * 28].copy().view(KP_DTYPE).reshape(-1)
    return kps, de[GUARD + f * cap * 32:GUARD + (f * cap + n) * 32].reshape(n, 32)


def _assert_outputs_kept_their_fill(out, B, cap):
    kp, de, cn = out
    for a in (kp, de, cn):
        assert (a[:GUARD] == OUT_FILL).all() and (a[-GUARD:] == OUT_FILL).all(), "a guard of an output was written"
    counts = cn[GUARD:GUARD + 4 * B].view(np.int32)
    for f in range(B):
        n = int(counts[f])
        assert (kp[GUARD + (f * cap + n) * 28:GUARD + (f + 1) * cap * 28] == OUT_FILL).all(), "key-point rows past the count written"
        assert (de[GUARD + (f * cap + n) * 32:GUARD + (f + 1) * cap * 32] == OUT_FILL).all(), "descriptor rows past the count written"


def _layout_case(ex, orc, imgs, layout, frames):
    """(a) .. (e) of the module docstring for one handle, one batch of frames and one layout"""
    import torch
    B, h, w = imgs.shape
    cap = ex.max_keypoints(w, h)
    outs = []
    for fill in FILLS:
        t, ptr, stride, frame_stride = _laid_out(torch, imgs, *layout, fill)
        before = t.clone()
        out = _device_call(torch, ex, ptr, B, w, h, stride, frame_stride, cap)
        assert torch.equal(t, before), "the caller's allocation was written (fill %r)" % (fill,)  # (c)
        _assert_outputs_kept_their_fill(out, B, cap)  # (d)
        for f in frames:  # (a), while the caller's buffer -- which the level-0 tap reads -- is alive
            kps, desc = _records(out, B, cap, f)
            _check_frame(ex, orc, imgs[f], kps, desc, frame=f, stages=True)
        outs.append(out)
        del t, before
    for o in outs[1:]:  # (b)
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b), "the pad's contents changed the output"
    d_dense = torch.from_numpy(np.ascontiguousarray(imgs)).cuda()  # (e)
    dense = _device_call(torch, ex, d_dense.data_ptr(), B, w, h, w, w * h, cap)
    for a, b in zip(outs[0], dense):
        assert np.array_equal(a, b), "the dense call gives other bytes"


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", ["L1", "L2", "L3", "L4", "L5"])
def test_layouts_with_the_default_kernels(oracle_mod, name, batch):
    """333 x 251, one frame and three: per-cell FAST, k_resize2, the VALU blur, k_orient and the level-0 tap on every layout"""
    w, h, nf = 333, 251, 300
    ex, orc = _handle(oracle_mod, nf, w, h, batch)
    _layout_case(ex, orc, layout_frames(w, h, batch), layouts(w, h)[name], range(batch))


_PYRAMIDS = {"resize": {"resize2": "never", "resize_lds": "never"}, "resize2": {"resize2": "always"},
             "resize_lds": {"resize_lds": "always", "resize2": "never"}}


@pytest.mark.parametrize("name", ["L2", "L3", "L5"])
@pytest.mark.parametrize("fast,pyramid,blur,desc", list(itertools.product(["strips", "cells"], list(_PYRAMIDS), ["valu", "mfma"],
                                                                          ["separate", "fused"])))
def test_every_kernel_that_reads_the_callers_buffer(oracle_mod, fast, pyramid, blur, desc, name):
    """The nine kernels that read level 0 from the caller's buffer, forced in every combination on three frames of 333 x 251:
    k_fast_strip | k_fast_cells_wave, k_resize | k_resize2 | k_resize_lds, k_blur_cols + k_blur_edges | k_blur_mfma, the
    blur pass + k_orient_desc | k_blur_desc, and k_orient in every one of them."""
    w, h, nf, B = 333, 251, 300, 3
    ex, orc = _handle(oracle_mod, nf, w, h, B, variants=dict({"fast": fast, "blur": blur, "desc": desc}, **_PYRAMIDS[pyramid]))
    _layout_case(ex, orc, layout_frames(w, h, B), layouts(w, h)[name], range(B))


@pytest.mark.parametrize("name", ["L2", "L5"])
@pytest.mark.parametrize("w,h,nf", [(130, 97, 100), (641, 200, 700)])
def test_further_shapes(oracle_mod, w, h, nf, name):
    """130 x 97: the top levels are smaller than a tile; 641 x 200: the last 16-byte chunk of a row holds one pixel"""
    ex, orc = _handle(oracle_mod, nf, w, h, 1)
    _layout_case(ex, orc, layout_frames(w, h, 1), layouts(w, h)[name], [0])


def test_throughput_path_on_a_pitched_ring(oracle_mod):
    """26 frames of 1242 x 375 at stride 1280, two bytes off an aligned base, six bytes between the frames: k_fast_strip, the
    matrix-pipe blur and the batch quadtree, as a host batch of this size runs them; frames 0 and 25"""
    w, h, nf, B = 1242, 375, 2000, 26
    ex, orc = _handle(oracle_mod, nf, w, h, B)
    _layout_case(ex, orc, layout_frames(w, h, B), (1280, 6, 2), [0, B - 1])


@pytest.mark.parametrize("resize2", ["auto", "always"])
@pytest.mark.parametrize("w,h", [(7, 64), (9, 40)])
def test_images_narrower_than_a_load_window(oracle_mod, w, h, resize2):
    """Levels under 8 pixels wide are narrower than the 8-byte window of k_resize and k_resize2: k_resize_narrow builds them
    (7 x 64: from level 0 on; 9 x 40: levels 0 and 1 through k_resize, the rest from 6 columns down).  No key point can come
    from such an image; the pyramid and its blurred levels still equal the oracle's, whatever fills the pad."""
    import torch
    B = 2
    ex, orc = _handle(oracle_mod, 100, w, h, B, variants={"resize2": resize2})
    imgs = np.random.RandomState(w).randint(0, 256, (B, h, w)).astype(np.uint8)
    cap = ex.max_keypoints(w, h)
    outs = []
    for fill in FILLS:
        t, ptr, stride, frame_stride = _laid_out(torch, imgs, w + 1, 3, 0, fill)
        before = t.clone()
        out = _device_call(torch, ex, ptr, B, w, h, stride, frame_stride, cap)
        assert torch.equal(t, before)
        _assert_outputs_kept_their_fill(out, B, cap)
        for f in range(B):
            assert len(_records(out, B, cap, f)[0]) == 0
            pyr = orc.pyramid(imgs[f])
            for l in range(orc.n_levels):
                assert np.array_equal(ex.tap_level(f, l, w, h, blurred=False), pyr[l]), "pyramid level %d differs" % l
                assert np.array_equal(ex.tap_level(f, l, w, h, blurred=True), orc.blur(pyr[l])), "blurred level %d differs" % l
        outs.append(out)
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert np.array_equal(a, b)


def test_stride_below_width_is_refused(oracle_mod):
    """stride < width is ORBX_E_ARG from all three entry points and leaves the record buffers alone (the host entry points
    report zero key points, the device entry point enqueues nothing); stride == width + 1 is accepted by all three."""
    import torch
    from monoorbslam3_amd.extractor import ORBExtractor
    w, h, nf = 333, 251, 300
    ex = ORBExtractor(nf, 1.2, 8, 20, 7)
    orc = _SharedOracle(oracle_mod.Oracle(nf, 1.2, 8, 20, 7), nf)
    img = layout_frames(w, h, 1)[0]
    n_ref = len(orc.extract(img)[0])
    cap = ex.max_keypoints(w, h)
    pitched = np.zeros((h, w + 1), np.uint8)
    pitched[:, :w] = img
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    for stride, src, want in ((w - 1, img, ORBX_E_ARG), (w + 1, pitched, 0)):
        for batch_call in (False, True):
            kps = np.full((cap, 28), OUT_FILL, np.uint8)
            desc = np.full((cap, 32), OUT_FILL, np.uint8)
            if batch_call:
                n = np.full(1, -7, np.int32)
                rc = ex._L.orbx_extract_batch(ex._h, vp(src), 1, w, h, stride, stride * h, vp(kps), vp(desc), cap, vp(n))
                n = int(n[0])
            else:
                n = C.c_int(-7)
                rc = ex._L.orbx_extract(ex._h, vp(src), w, h, stride, vp(kps), vp(desc), cap, C.byref(n))
                n = n.value
            assert rc == want
            if want:
                assert n == 0 and (kps == OUT_FILL).all() and (desc == OUT_FILL).all()
            else:
                assert n == n_ref and (kps[n:] == OUT_FILL).all() and (desc[n:] == OUT_FILL).all()
        t, ptr, _, frame_stride = _laid_out(torch, img[None], max(stride, w), 0, 0, 0x00)
        if want:
            from monoorbslam3_amd._lib import OrbxError
            kp, kp_p = _guarded(torch, cap * 28)
            de, de_p = _guarded(torch, cap * 32)
            cn, cn_p = _guarded(torch, 4)
            with pytest.raises(OrbxError) as e:
                ex.extract_batch_device(ptr, 1, w, h, stride, frame_stride, kp_p, de_p, cap, cn_p)
            assert e.value.code == ORBX_E_ARG
            ex.synchronize()
            torch.cuda.synchronize()
            for a in (kp, de, cn):
                assert bool((a == OUT_FILL).all())
        else:
            out = _device_call(torch, ex, ptr, 1, w, h, stride, frame_stride, cap)
            assert len(_records(out, 1, cap, 0)[0]) == n_ref


# ---- the host entry points on the same layouts ----------------------------------------------------------------------

@pytest.mark.parametrize("wv", [333, 130])
def test_a_crop_of_a_wider_host_image(oracle_mod, wv):
    """ex(big[3:254, 20:20 + wv]) of a 700-wide array: the 2-D copy stages level 0 at a pitch of align_up(width, 64) -- 384
    for 333 columns, 192 for 130 -- and every stage reads it there"""
    from monoorbslam3_amd import synth
    from monoorbslam3_amd.extractor import ORBExtractor
    ex = ORBExtractor(300, 1.2, 8, 20, 7)
    orc = _SharedOracle(oracle_mod.Oracle(300, 1.2, 8, 20, 7), 300)
    view = synth.make_frames(1, 700, 300, seed=11)[0][3:254, 20:20 + wv]
    assert view.strides == (700, 1)
    kps, desc = ex(view)
    assert len(kps) >= 50
    _check_frame(ex, orc, np.ascontiguousarray(view), kps, desc, stages=True)


def test_one_handle_through_dense_and_strided_frames(oracle_mod):
    """dense 800 x 300, strided 333 x 251, dense 333 x 251, strided 480 x 270 on one handle: the staging pitch of a geometry
    stays behind when the next frame is dense (pitch = width) and is replaced when the geometry changes"""
    from monoorbslam3_amd import synth
    from monoorbslam3_amd.extractor import ORBExtractor
    ex = ORBExtractor(500, 1.2, 8, 20, 7)
    orc = _SharedOracle(oracle_mod.Oracle(500, 1.2, 8, 20, 7), 500)
    big = synth.make_frames(1, 700, 300, seed=12)[0]
    for img in (synth.make_frames(1, 800, 300, seed=13)[0], big[3:254, 20:353], layout_frames(333, 251, 1)[0], big[10:280, 100:580]):
        kps, desc = ex(img)
        assert len(kps) >= 50
        _check_frame(ex, orc, np.ascontiguousarray(img), kps, desc, stages=True)


@pytest.mark.parametrize("B", [3, 26])
@pytest.mark.parametrize("kind", ["every_second_frame", "crop"])
def test_host_batches_with_their_own_strides(oracle_mod, kind, B):
    """ORBExtractor.extract_batch passes a uint8 stack's own strides.  stack[::2]: dense rows, frames two frames apart (one
    linear copy per frame); stack[:, 3:-5, 20:353]: a crop (one 2-D copy per frame).  First and last frame, every stage."""
    from monoorbslam3_amd import synth
    if kind == "every_second_frame":
        w, h = 333, 251
        stack = synth.make_frames(2 * B - 1, w, h, seed=40 + B)
        view = stack[::2]
        assert view.strides == (2 * h * w, w, 1)
    else:
        stack = synth.make_frames(B, 700, 300, seed=50 + B)
        view = stack[:, 3:-5, 20:353]
        _, h, w = view.shape
        assert view.strides == (700 * 300, 700, 1) and (w, h) == (333, 292)
    assert view.shape[0] == B and not view.flags["C_CONTIGUOUS"] and view.base is not None
    ex, orc = _handle(oracle_mod, 300, w, h, B)
    res = ex.extract_batch(view)
    assert len(res) == B
    for f in (0, B - 1):
        assert len(res[f][0]) >= 50
        _check_frame(ex, orc, np.ascontiguousarray(view[f]), res[f][0], res[f][1], frame=f, stages=True)


def test_a_crop_of_a_page_locked_buffer(oracle_mod):
    """a strided view of a buffer registered with orbx_host_register: the frame's 2-D copy is asynchronous; three calls with
    the buffer's contents changed in between"""
    from monoorbslam3_amd import synth
    from monoorbslam3_amd.extractor import ORBExtractor
    ex = ORBExtractor(300, 1.2, 8, 20, 7)
    orc = _SharedOracle(oracle_mod.Oracle(300, 1.2, 8, 20, 7), 300)
    buf = np.empty((300, 700), np.uint8)
    view = buf[3:254, 20:353]
    ex.host_register(buf)
    try:
        for seed in (31, 32, 33):
            buf[:] = synth.make_frames(1, 700, 300, seed=seed)[0]
            kps, desc = ex(view)
            assert len(kps) >= 50
            _check_frame(ex, orc, view.copy(), kps, desc, stages=True)
    finally:
        ex.host_unregister(buf)
