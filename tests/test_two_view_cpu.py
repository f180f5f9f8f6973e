"""orbm_two_view_ransac{,_device} and orbm_two_view_sets without a GPU: the header's declarations, the exports and the wrappers; the
refusals that come before any device call; the draw against the model's; and the conditions that the scenes of
tests/test_two_view_gpu.py have to meet, asserted on the numpy model (tests/two_view_model.py) alone."""
import ctypes as C

import numpy as np
import pytest

import two_view_model as tm
from abi_checks import E_ARG, E_NO_DEVICE, E_UNSUPPORTED, P, built, declared, device_present, exported, returns

NAMES = {"orbm_two_view_ransac_device", "orbm_two_view_ransac", "orbm_two_view_sets"}


@pytest.fixture(scope="module")
def matcher():
    return built("matcher")


def test_header_declares_the_entry_points_the_library_exports_them_and_the_wrappers_bind(matcher):
    assert NAMES <= declared("orbm_", "orbm.h")
    exported(NAMES)
    L = matcher._mlib()
    for name in NAMES:
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is C.c_int, name
    assert callable(matcher.ORBMatcher.TwoViewRansacDevice) and callable(matcher.ORBMatcher.TwoViewRansac) and callable(matcher.two_view_sets)
    from abi_checks import flat
    text = flat("include/orbm.h")
    assert "parity with OpenCV is UNPINNED" in text                 # as oracle/README.md says of OpenCV elsewhere


ARGS = ("h", "kps1", "n1", "kps2", "n2", "matches12", "sigma", "iters", "state", "sets", "pairs", "H", "F", "inl_H", "inl_F", "score", "rh", "hyp",
        "hyp_score", "result")
REQUIRED = ("kps1", "kps2", "matches12", "pairs", "H", "F", "inl_H", "inl_F", "score", "rh", "result")


def _call(L, device, **over):
    """one call with valid arguments (the fake pointer, never dereferenced: abi_checks' rule) except for `over`"""
    a = {k: P for k in ARGS}
    a.update(h=None, n1=100, n2=120, sigma=1.0, iters=200, state=0, sets=None)
    a.update(over)
    vals = [a[k] for k in ARGS]
    return L.orbm_two_view_ransac_device(*vals, None) if device else L.orbm_two_view_ransac(*vals)


def _named(device):
    def call(L, **over):
        return _call(L, device, **over)
    call.__name__ = "orbm_two_view_ransac" + ("_device" if device else "")
    return call


@pytest.mark.parametrize("device", [True, False])
def test_the_refusals_come_before_any_device_call(matcher, device):
    L = matcher._mlib()
    call = _named(device)
    cases = [dict(iters=0), dict(iters=-3), dict(iters=1025), dict(n1=0), dict(n2=0), dict(n1=-1), dict(n2=-5), dict(sigma=0.0), dict(sigma=-1.0),
             dict(sigma=float("nan"))]
    cases += [{k: None} for k in REQUIRED]
    for over in cases:
        returns(E_ARG, call, L, **over)
    # more key points than the masks' scratch is sized for; an argument error wins over the limit
    returns(E_UNSUPPORTED, call, L, n1=65537)
    returns(E_UNSUPPORTED, call, L, n2=65537)
    returns(E_ARG, call, L, n1=65537, iters=0)
    # the optional ones may be NULL, the limits themselves are allowed: such a call passes every check
    for over in (dict(), dict(hyp=None, hyp_score=None), dict(sets=P), dict(iters=1), dict(iters=1024), dict(n1=1, n2=1), dict(n1=65536, n2=65536)):
        returns(E_NO_DEVICE, call, L, **over)


def test_the_sets_function_refuses_what_it_cannot_draw(matcher):
    L = matcher._mlib()
    out = np.zeros((4, 8), np.int32)
    ptr = out.ctypes.data_as(C.c_void_p)
    for args in ((7, 4, 0, ptr), (0, 4, 0, ptr), (9, 0, 0, ptr), (9, 1025, 0, ptr), (9, 4, 0, None)):
        returns(E_ARG, L.orbm_two_view_sets, *args)
    assert not out.any()
    with pytest.raises(Exception):
        matcher.two_view_sets(7)


def test_every_wrapper_fails_loudly_without_a_gpu(matcher):
    if device_present():
        pytest.skip("needs a machine without a GPU")
    from monoorbslam3_amd import _lib
    with pytest.raises(_lib.OrbxError) as e:
        matcher.ORBMatcher()                     # the handle itself
    assert e.value.code == E_NO_DEVICE

    class NoHandle:                              # the wrappers behind a handle that could not exist
        _L, _h = matcher._mlib(), None

    class Fake:
        def data_ptr(self):
            return P

    m = matcher.ORBMatcher(handle=NoHandle())
    names = ("kps1", "kps2", "matches12", "pairs", "H", "F", "inl_H", "inl_F", "score", "rh", "result")
    returns(E_NO_DEVICE, m.TwoViewRansacDevice, {k: Fake() for k in names}, 100, 120)
    sc = tm.make_scene(33, 5)
    from monoorbslam3_amd.extractor import KP_DTYPE
    k1, k2 = np.zeros(len(sc["xy1"]), KP_DTYPE), np.zeros(len(sc["xy2"]), KP_DTYPE)
    returns(E_NO_DEVICE, m.TwoViewRansac, k1, k2, sc["matches12"])


@pytest.mark.parametrize("state", [0, 0x1234567887654321])
@pytest.mark.parametrize("iters", [1, 200, 1024])
@pytest.mark.parametrize("n_matches", [8, 9, 65, 300])
def test_the_draw_equals_the_models(matcher, n_matches, iters, state):
    """orbm_two_view_sets against the model's availableIndices vector (state 0 is cv::RNG's default); every set holds eight distinct
    indices below n_matches, and at eight matches every set is a permutation of 0..7"""
    sets = matcher.two_view_sets(n_matches, iters, state)
    assert sets.shape == (iters, 8) and sets.dtype == np.int32
    assert np.array_equal(sets, tm.draw_sets(n_matches, iters, state))
    assert (sets >= 0).all() and (sets < n_matches).all()
    assert all(len(set(row)) == 8 for row in sets.tolist())
    if n_matches == 8:
        assert (np.sort(sets, axis=1) == np.arange(8)).all()
    if state == 0:
        assert np.array_equal(sets, matcher.two_view_sets(n_matches, iters, tm.RNG_DEFAULT))


@pytest.mark.parametrize("state", [1, 0xFFFFFFFFFFFFFFFF, 0xFFFFFFFF00000000, (4164903690 << 32) - 1, (4164903690 << 32), (4164903690 << 32) + 1,
                                   (4164903689 << 32) | 0xFFFFFFFF, 4164903690, 0x00000001FFFFFFFF])
def test_the_draw_from_edge_states_equals_the_models(matcher, state):
    """the library makes the raw stream on 64 lanes that jump ahead by a modular product; the model steps one by one.  States whose
    carry is not below the multiplier, the modulus itself (the generator's fixed point) and its neighbours, all 1024 sets"""
    assert np.array_equal(matcher.two_view_sets(300, 1024, state), tm.draw_sets(300, 1024, state))


def test_the_generator_is_cv_rngs_multiply_with_carry():
    """the first draws from the default state, worked by hand from state = (uint32) state * 4164903690 + (state >> 32)"""
    s, r = tm.rng_next(0xFFFFFFFF)
    assert s == 0xFFFFFFFF * 4164903690 and r == s & 0xFFFFFFFF
    s2, r2 = tm.rng_next(s)
    assert s2 == (s & 0xFFFFFFFF) * 4164903690 + (s >> 32) and r2 == s2 & 0xFFFFFFFF


@pytest.mark.parametrize("n,seed,planar,iters", tm.SCENES)
def test_the_scenes_meet_their_conditions_on_the_model(n, seed, planar, iters):
    """The scenes the GPU test runs: n1 != n2 and holes in matches12; the sides whose chi-square lies within 1e-3 of its threshold are
    at most 1 % of all sides; the conditioning gate of check (a) keeps at least half of the H hypotheses on every scene and at least
    half of the F hypotheses on the general scenes of 64 matches or more; the float32 model's winner scores within 1 % of the
    float64 model's in the family check (e) looks at."""
    sc, m64, m32 = tm.scene_models(n, seed, planar, iters)
    assert len(sc["xy1"]) != len(sc["xy2"]) and (sc["matches12"] < 0).any()
    assert m64["n_matches"] == n and m64["status"] == 0 and m64["sets"].shape == (iters, 8)
    x1, x2 = sc["xy1"][m64["pairs"][:, 0]], sc["xy2"][m64["pairs"][:, 1]]
    band = sides = 0
    for fam in range(2):
        for it in range(iters):
            b, score, flags = tm.banded_sides(fam, m64["hyp"][fam, it], x1, x2, 1.0)
            band, sides = band + int(b.sum()), sides + b.size
            assert score == m64["hyp_score"][fam, it]
    gate = m64["cond"] > tm.GATE
    print("%d matches, %s, %d sets: banded sides %d of %d, gate keeps H %.2f F %.2f, RH %.3f, winners %s, scores %s" % (
        n, "planar" if planar else "general", iters, band, sides, gate[0].mean(), gate[1].mean(), m64["rh"], m64["win"], m64["score"]))
    assert band <= 0.01 * sides
    assert gate[0].mean() >= 0.5
    if not planar and n >= 64:
        assert gate[1].mean() >= 0.5
    fam = 0 if planar else 1
    assert m32["score"][fam] >= 0.99 * m64["score"][fam]            # every scene; on the planar one of 9 matches both are 0
    assert np.isfinite(m64["hyp"]).all() and np.isfinite(m32["hyp"]).all()
