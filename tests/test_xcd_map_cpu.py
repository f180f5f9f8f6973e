"""The workgroup -> (frame, level) mapping of the batch quadtree and k_desc_bins, through orbx_dev_xcd_map (no GPU).

A grid of (levels, frames) workgroups is dealt to the 8 XCDs by its linear block id, level + n_levels * frame: with 8 levels
every workgroup of one level lands on one XCD, and the kernel waits for the XCD that got level 0.  The mapping keeps the
project's convention -- XCD x takes the frames congruent to x (mod 8) -- so every XCD gets its share of every level."""
import ctypes as C
import itertools

import pytest

PER_FRAME = (1, 3, 4, 7, 8, 12, 16)
N_FRAMES = (1, 7, 8, 9, 43, 64, 65, 512)


@pytest.fixture(scope="module")
def xcd_map():
    import __graft_entry__ as g
    g.build()
    from monoorbslam3_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    fn = L.orbx_dev_xcd_map
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]

    def query(per_frame, n_frames, block):
        f, i = C.c_int(-1), C.c_int(-1)
        rc = fn(per_frame, n_frames, block, C.byref(f), C.byref(i))
        return rc, f.value, i.value
    return query


def _grid(per_frame, n_frames):
    """orbx_xcd_grid: whole groups of 8 frames from 8 frames on (the surplus workgroups return at once)"""
    return n_frames * per_frame if n_frames < 8 else 8 * ((n_frames + 7) // 8) * per_frame


def _balance(blocks, per_frame):
    """largest difference between two XCDs in the number of workgroups of one item value; blocks: (block id, item)"""
    worst = 0
    for item in range(per_frame):
        counts = [0] * 8
        for b, it in blocks:
            if it == item:
                counts[b % 8] += 1
        worst = max(worst, max(counts) - min(counts))
    return worst


@pytest.mark.parametrize("per_frame,n_frames", list(itertools.product(PER_FRAME, N_FRAMES)))
def test_mapping_is_a_bijection_keeps_the_xcd_convention_and_balances_the_levels(xcd_map, per_frame, n_frames):
    grid = _grid(per_frame, n_frames)
    # the export knows the launch's grid: the block behind the last one is refused, as is one before the first
    assert xcd_map(per_frame, n_frames, grid)[0] < 0 and xcd_map(per_frame, n_frames, -1)[0] < 0
    live = []
    for b in range(grid):
        rc, frame, item = xcd_map(per_frame, n_frames, b)
        assert rc in (0, 1), (b, rc)
        if rc == 1:
            assert 0 <= frame < n_frames and 0 <= item < per_frame, (b, frame, item)
            live.append((b, frame, item))
    # bijection onto [0, n_frames) x [0, per_frame)
    assert len(live) == n_frames * per_frame
    assert len({(f, i) for _, f, i in live}) == n_frames * per_frame
    # XCD x takes the frames congruent to x (mod 8)
    if n_frames >= 8:
        for b, frame, _ in live:
            assert frame % 8 == b % 8, (b, frame)
    # every XCD gets the same number of workgroups of every item value, to within one
    assert _balance([(b, i) for b, _, i in live], per_frame) <= 1


def test_a_levels_by_frames_grid_fails_the_balance_with_8_levels():
    """what the mapping replaces: linear block id = level + n_levels * frame puts every level on an XCD of its own"""
    for n_frames in (8, 65, 512):
        blocks = [(level + 8 * frame, level) for frame in range(n_frames) for level in range(8)]
        assert _balance(blocks, 8) == n_frames
