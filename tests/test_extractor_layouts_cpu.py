"""The frames and layouts of tests/test_extractor_layouts_gpu.py, and what the oracle alone says about them.

The GPU tests hand the extractor level-0 images whose rows are `stride > width` bytes apart, with filled bytes between the
rows and between the frames, and hold the result to the oracle run on the dense copy.  That proves something only if
 (1) the frames give key points, some of them where a wrong right or bottom border would move them, and
 (2) an extractor that took the pitch for the width -- and so treated the fill as pixels -- would come out differently.
Both are shown here on the reference implementation, never on the code under test.
"""
import numpy as np
import pytest

from monoorbslam3_amd import synth

# (width, height, features): the shapes of the layout tests
SHAPES = [(333, 251, 300), (130, 97, 100), (641, 200, 700), (1242, 375, 2000)]
EDGE_BAND = 24  # "near an edge": within this many pixels of it


def layout_frames(w, h, batch):
    """The frames every layout test of this shape uses (frame f is the same for every batch size >= f + 1)."""
    return synth.make_frames(batch, w, h, seed=3 * w + h)


def layouts(w, h):
    """name -> (stride, frame_gap, base_off) of a level-0 image of w x h pixels inside its allocation"""
    return {
        "L1": (w, 0, 1),                      # dense, but every frame at an odd address
        "L2": (w + 1, 3, 0),                  # one byte of pad per row (333, 641: pitch = 2 mod 4), odd frame stride
        "L3": (352, 0, 7),                    # a multiple of 16 that is not align_up(w, 64), unaligned base
        "L4": (384, -(384 * h) % 256, 0),     # what hipMallocPitch gives: frames at multiples of 256
        "L5": (1024, 4097, 5),                # a crop from a much wider image
    }


def fill_bytes(n, fill):
    """n bytes of pad: 0x00, 0xFF or ("random") seeded random bytes"""
    if fill == "random":
        return np.random.RandomState(20261020).randint(0, 256, n).astype(np.uint8)
    return np.full(n, fill, np.uint8)


@pytest.fixture(scope="module")
def orc_mod():
    from oracle import orb_ref_py
    orb_ref_py.build()
    return orb_ref_py


@pytest.mark.parametrize("w,h,nf", SHAPES)
def test_frames_are_not_vacuous(orc_mod, w, h, nf):
    """at least 50 key points, and level-0 key points beside the right and the bottom edge (130 x 97: its level-0 region is
    three cells wide and two high, none beside the bottom edge -- the right edge only)"""
    orc = orc_mod.Oracle(nf, 1.2, 8, 20, 7)
    kps, _, _ = orc.extract(layout_frames(w, h, 1)[0])
    assert len(kps) >= 50
    # the other frames the batches check: 1 and 2 of three, the last of 26
    others = {333: layout_frames(w, h, 3)[1:], 1242: layout_frames(w, h, 26)[25:]}.get(w, [])
    for img in others:
        assert len(orc.extract(img)[0]) >= 50
    l0 = kps[kps["octave"] == 0]
    assert np.count_nonzero(l0["x"] >= w - EDGE_BAND) >= 1
    if (w, h) != (130, 97):
        assert np.count_nonzero(l0["y"] >= h - EDGE_BAND) >= 1


def test_the_fill_would_show_if_it_were_read(orc_mod):
    """The 333 x 251 frame at stride 352 with the random fill, read as a 352-wide image: FAST's candidates left of x = w and
    the blur's last three columns differ from the dense frame's.  A kernel that takes the pitch for the width cannot
    equal the oracle on the dense frame and give the same bytes for every fill."""
    w, h, nf = SHAPES[0]
    stride = layouts(w, h)["L3"][0]
    orc = orc_mod.Oracle(nf, 1.2, 8, 20, 7)
    img = layout_frames(w, h, 1)[0]
    wide = fill_bytes(h * stride, "random").reshape(h, stride)
    wide[:, :w] = img
    dense = orc.level_candidates(img)
    pitched = orc.level_candidates(wide)
    pitched = pitched[pitched["x"].astype(int) + 19 < w]  # candidate coordinates are relative to (19, 19)
    as_set = lambda c: sorted(zip(c["y"].astype(int).tolist(), c["x"].astype(int).tolist(), c["response"].astype(int).tolist()))
    assert as_set(pitched) != as_set(dense)
    b_dense, b_wide = orc.blur(img), orc.blur(wide)[:, :w]
    assert np.array_equal(b_wide[:, :w - 3], b_dense[:, :w - 3])  # the 7-tap window reaches three columns
    assert not np.array_equal(b_wide[:, w - 3:], b_dense[:, w - 3:])
