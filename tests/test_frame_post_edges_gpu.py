"""orbf_frame_post / orbf_frame_post_device (include/orbf.h) on the MI355X at the edges the friendly cameras of test_frame_post.py
never reach: grid shapes around the kernel's 256 threads, coordinates on cell borders and just outside the image, every exit of
the undistortion loop, short coefficient lists, the unchecked size_scale lookup, clamped counts in padded arrays, and one handle
across call sizes.  Every comparison is with the oracle, bit for bit."""
import numpy as np
import pytest

import test_frame_post as tf
from test_frame_post import EUROC, EUROC_DIST
from test_observations_gpu import _guards_intact, _padded
from test_projection_queries_gpu import _stream, _up

pytestmark = pytest.mark.gpu

NAMES = ("raw", "undistorted", "cell_start", "cell_items")
KP_BYTES = 28
UN_FILL, START_FILL, ITEMS_FILL, RAW_GUARD = 0xA5, -7, -9, 0x5A


def _same(got, want):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), name


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------- 1. grid shapes and borders
@pytest.mark.parametrize("w,h,cells", tf.GRID_SIZES)
def test_grid_shapes_and_border_coordinates(oracle_mod, w, h, cells):
    from monoorbslam3_amd.frame import FramePost
    k, _ = tf.edge_kps(oracle_mod, w, h, 30)
    cam = dict(width=w, height=h, fx=500., fy=500., cx=w / 2, cy=h / 2)
    fp = FramePost(**cam)
    assert fp.n_cells == cells and (fp.cols, fp.rows) == (tf.grid_dim(w), tf.grid_dim(h))
    _same(fp(k), oracle_mod.frame_post(**cam, dist=(), kps=k))


def test_grid_one_cell_too_many_is_refused():
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.frame import FramePost
    assert tf.grid_dim(3840) * tf.grid_dim(3200) == 7680
    with pytest.raises(_lib.OrbxError) as e:
        FramePost(width=3840, height=3200, fx=500., fy=500., cx=1920., cy=1600.)
    assert e.value.code == -1  # ORBX_E_ARG


# ------------------------------------------------------------------------------------------- 2. undistortion branches
def test_undistort_every_exit_of_the_loop(oracle_mod):
    from monoorbslam3_amd.frame import FramePost
    k = tf.uniform_kps(oracle_mod, 3000, 752, 480, 5)
    _, _, exit_at = tf.undistort_model(EUROC, tf.NEG_DIST, k["x"], k["y"])
    print("icdist < 0 at iteration 0..4:", tf.check_undistort_branches(exit_at), "all five ran:", int((exit_at == -1).sum()))
    _same(FramePost(**EUROC, dist=tf.NEG_DIST)(k), oracle_mod.frame_post(**EUROC, dist=tf.NEG_DIST, kps=k))


@pytest.mark.parametrize("n_dist", [1, 2, 5, 8])
def test_undistort_absent_coefficients_are_zeros(oracle_mod, n_dist):
    from monoorbslam3_amd.frame import FramePost
    k = tf.uniform_kps(oracle_mod, 800, 752, 480, 6)
    dist = tf.EUROC_K12[:n_dist]
    want = oracle_mod.frame_post(**EUROC, dist=dist + (0.0,) * (12 - n_dist), kps=k)  # the zeros written out
    assert not np.array_equal(want[1]["x"], k["x"])
    _same(FramePost(**EUROC, dist=dist)(k), want)


@pytest.mark.parametrize("case", ["k1_zero", "k1_minus_zero", "fisheye"])
def test_undistort_is_copy(oracle_mod, case):
    from monoorbslam3_amd.frame import FramePost
    k = tf.uniform_kps(oracle_mod, 500, 752, 480, 7)
    dist, kw = {"k1_zero": ((0.0, 0.1, 0.01, 0.01), {}), "k1_minus_zero": ((-0.0, 0.1, 0.01, 0.01), {}),
                "fisheye": (EUROC_DIST, dict(undistort=False))}[case]
    got = FramePost(**EUROC, dist=dist, **kw)(k)
    assert got[0].tobytes() == k.tobytes() and got[1].tobytes() == k.tobytes()
    _same(got, oracle_mod.frame_post(**EUROC, dist=dist, kps=k, **kw))


def test_size_scale_lookup_truncates(oracle_mod):
    from monoorbslam3_amd.frame import FramePost
    table, k = tf.fisheye_case(oracle_mod)
    got = FramePost(**EUROC, dist=EUROC_DIST, undistort=False, size_scale=table)(k)
    assert np.array_equal(got[0]["size"], k["size"] * table[k["y"].astype(np.int32), k["x"].astype(np.int32)])
    _same(got, oracle_mod.frame_post(**EUROC, dist=EUROC_DIST, kps=k, undistort=False, size_scale=table))


# ------------------------------------------------------------------------------------------- 3. / 4. the batch contract
def _frames(oracle_mod, n_frames, cap, seed):
    """[n_frames][cap] key points over the EuRoC image and a little beyond it: every row is a plausible record, so a frame whose
    count says more than cap, or less than what the array holds, still has something to get wrong"""
    k = tf.uniform_kps(oracle_mod, n_frames * cap, 752 + 8, 480 + 8, seed)
    k["x"] -= 4
    k["y"] -= 4
    return k.reshape(n_frames, cap)


def _post_device(torch, dev, fp, raw, counts, cap, kind):
    """orbf_frame_post_device on padded, sentinel-filled arrays; checks the guards and returns the host copies"""
    B = len(counts)
    raw_b = np.frombuffer(raw.tobytes(), np.uint8)
    pads = dict(raw=_padded(torch, dev, raw_b, RAW_GUARD), un=_padded(torch, dev, np.full(B * cap * KP_BYTES, UN_FILL, np.uint8), 0x3C),
                start=_padded(torch, dev, np.full(B * (fp.n_cells + 1), START_FILL, np.int32), -3),
                items=_padded(torch, dev, np.full(B * cap, ITEMS_FILL, np.int32), -4))
    d_n = _up(torch, dev, np.asarray(counts, np.int32))
    st = _stream(torch, dev, kind)
    fp.post_device(B, pads["raw"][1].data_ptr(), d_n.data_ptr(), cap, pads["un"][1].data_ptr(), pads["start"][1].data_ptr(),
                   pads["items"][1].data_ptr(), st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for name, fill in (("raw", RAW_GUARD), ("un", 0x3C), ("start", -3), ("items", -4)):
        assert _guards_intact(pads[name][0], fill), name
    return dict(raw=pads["raw"][1].cpu().numpy().reshape(B, cap, KP_BYTES), un=pads["un"][1].cpu().numpy().reshape(B, cap, KP_BYTES),
                start=pads["start"][1].cpu().numpy().reshape(B, fp.n_cells + 1), items=pads["items"][1].cpu().numpy().reshape(B, cap))


def _check_batch(oracle_mod, cam, dist, raw, counts, cap, out):
    """every frame against the oracle run on its first min(count, cap) rows, and nothing written beyond the counts"""
    for f, count in enumerate(counts):
        n = min(count, cap)
        w_raw, w_un, w_start, w_items = oracle_mod.frame_post(**cam, dist=dist, kps=raw[f, :n])
        assert out["raw"][f].tobytes() == raw[f].tobytes(), f  # no size_scale: raw is read, never written
        assert out["un"][f, :n].tobytes() == w_un.tobytes(), f
        assert (out["un"][f, n:] == UN_FILL).all(), f
        assert np.array_equal(out["start"][f], w_start), f
        assert np.array_equal(out["items"][f, : w_start[-1]], w_items), f
        assert (out["items"][f, w_start[-1]:] == ITEMS_FILL).all(), f


@pytest.mark.parametrize("kind", ["chain", "null"])
def test_batch_contract_padded(oracle_mod, dev, kind):
    import torch
    from monoorbslam3_amd.frame import FramePost
    cap, counts = 300, [350, 0, 1, 257, 300]
    raw = _frames(oracle_mod, len(counts), cap, 40)
    fp = FramePost(**EUROC, dist=EUROC_DIST)
    out = _post_device(torch, dev, fp, raw, counts, cap, kind)
    _check_batch(oracle_mod, EUROC, EUROC_DIST, raw, counts, cap, out)
    assert (out["start"][1] == 0).all()
    # frame 0 says 350: exactly what a count of 300 gives
    as_300 = oracle_mod.frame_post(**EUROC, dist=EUROC_DIST, kps=raw[0])
    assert out["un"][0].tobytes() == as_300[1].tobytes() and np.array_equal(out["start"][0], as_300[2])
    # the inputs do what they are there for: some key points of every non-empty frame are in no cell, most are in one
    for f in (0, 3, 4):
        assert 0.5 * min(counts[f], cap) < out["start"][f, -1] < min(counts[f], cap)


def test_one_handle_across_sizes(oracle_mod, dev):
    import torch
    from monoorbslam3_amd.frame import FramePost
    fp = FramePost(**EUROC, dist=EUROC_DIST)
    small, big = _frames(oracle_mod, 1, 64, 41), _frames(oracle_mod, 8, 4000, 42)
    big_counts = [4000, 0, 1, 3999, 2500, 257, 4000, 1000]
    host_big, host_small = tf.uniform_kps(oracle_mod, 2500, 752, 480, 43), tf.uniform_kps(oracle_mod, 10, 752, 480, 44)

    def first():
        out = _post_device(torch, dev, fp, small, [64], 64, "chain")
        _check_batch(oracle_mod, EUROC, EUROC_DIST, small, [64], 64, out)
        return b"".join(out[k].tobytes() for k in ("raw", "un", "start", "items"))

    a = first()
    out = _post_device(torch, dev, fp, big, big_counts, 4000, "chain")  # the scratch grows
    _check_batch(oracle_mod, EUROC, EUROC_DIST, big, big_counts, 4000, out)
    b = first()  # and is reused by a smaller call
    _same(fp(host_big), oracle_mod.frame_post(**EUROC, dist=EUROC_DIST, kps=host_big))
    _same(fp(host_small), oracle_mod.frame_post(**EUROC, dist=EUROC_DIST, kps=host_small))
    c = first()
    assert a == b == c
