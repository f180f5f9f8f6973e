"""orbv_transform / orbv_transform_device / orbv_transform_features_device (include/orbv.h) on the MI355X on the trees and batches
that test_vocabulary.py's well-formed vocabularies never produce: a word shared by nodes of different weight, uneven fan-out with
exact sibling ties, a chain, a root-only tree, and the batch contract (clamped and zero counts, ORBV_NO_NODE keys, a frame of
stopped words, padded outputs, one handle across capacities).  Every comparison is with the oracle, bit for bit."""
import numpy as np
import pytest

import test_vocabulary as tv
from monoorbslam3_amd import synth
from test_observations_gpu import _guards_intact, _padded
from test_projection_queries_gpu import _stream, _up
from test_vocabulary import NO_NODE, _same_transform

pytestmark = pytest.mark.gpu

# sentinel the seven outputs are filled with, and the different value of the guards around each
FILLS = dict(bow_ids=(-11, -21), bow_vals=(-123.25, -7.5), n_words=(-12, -22), fv_nodes=(-13, -23), fv_off=(-14, -24),
             fv_idx=(-15, -25), n_fv=(-16, -26))


@pytest.fixture(scope="module")
def dev():
    import torch
    return torch.device("cuda:0")


def _batch(torch, dev, V, desc, counts, cap, levelsup, kind="chain"):
    """orbv_transform_device on padded, sentinel-filled outputs.  desc is [B][cap][32].  Checks the guards and that nothing is
    written beyond n_words, n_fv, fv_off[n_fv] and fv_idx[fv_off[n_fv]]; returns every frame in the form of transform()."""
    B = len(counts)
    assert desc.shape == (B, cap, 32)
    shape = dict(bow_ids=(B * cap, np.int32), bow_vals=(B * cap, np.float64), n_words=(B, np.int32), fv_nodes=(B * cap, np.int32),
                 fv_off=(B * (cap + 1), np.int32), fv_idx=(B * cap, np.int32), n_fv=(B, np.int32))
    pads = {k: _padded(torch, dev, np.full(n, FILLS[k][0], t), FILLS[k][1]) for k, (n, t) in shape.items()}
    d_desc, d_n = _up(torch, dev, desc), _up(torch, dev, np.asarray(counts, np.int32))
    st = _stream(torch, dev, kind)
    V.transform_device(B, d_desc.data_ptr(), d_n.data_ptr(), cap, levelsup,
                       *[pads[k][1].data_ptr() for k in ("bow_ids", "bow_vals", "n_words", "fv_nodes", "fv_off", "fv_idx", "n_fv")], st)
    torch.cuda.synchronize()
    torch.cuda.set_stream(torch.cuda.default_stream(dev))
    for k in shape:
        assert _guards_intact(pads[k][0], FILLS[k][1]), k
    h = {k: pads[k][1].cpu().numpy() for k in shape}
    frames = []
    for f in range(B):
        nw, nf = int(h["n_words"][f]), int(h["n_fv"][f])
        assert 0 <= nw <= min(counts[f], cap) and 0 <= nf <= min(counts[f], cap), f
        ids, vals = h["bow_ids"].reshape(B, cap)[f], h["bow_vals"].reshape(B, cap)[f]
        nodes, off, idx = h["fv_nodes"].reshape(B, cap)[f], h["fv_off"].reshape(B, cap + 1)[f], h["fv_idx"].reshape(B, cap)[f]
        assert (ids[nw:] == FILLS["bow_ids"][0]).all() and (vals[nw:] == FILLS["bow_vals"][0]).all(), f
        assert (nodes[nf:] == FILLS["fv_nodes"][0]).all() and (off[nf + 1:] == FILLS["fv_off"][0]).all(), f
        assert 0 <= off[nf] <= min(counts[f], cap) and (idx[off[nf]:] == FILLS["fv_idx"][0]).all(), f
        frames.append((ids[:nw].view(np.uint32), vals[:nw], (nodes[:nf].view(np.uint32), off[: nf + 1], idx[: off[nf]].view(np.uint32))))
    return frames


def _one(desc, cap=None):
    """a batch of one frame holding desc"""
    cap = cap or len(desc)
    out = np.zeros((1, cap, 32), np.uint8)
    out[0, : len(desc)] = desc
    return out


# ------------------------------------------------------------------------------------- 5. trees orbv_create accepts
@pytest.mark.parametrize("scoring,weighting", tv.WEIGHTINGS_AND_SCORINGS)
def test_word_shared_by_unequal_weights(oracle_mod, dev, scoring, weighting):
    """A childless node without the is_leaf flag shares word 0 with the first real leaf, at its own weight: the BowVector value
    is the sum of every feature's own weight (BowVector::addWeight), 4.5 and not 4 x 1.5 / 2 = 3.0 for DOT_PRODUCT + TF_IDF."""
    import torch
    from monoorbslam3_amd.vocabulary import ORBVocabulary
    voc = tv.unequal_tiny(scoring, weighting)
    V, R = ORBVocabulary.from_arrays(voc), oracle_mod.Vocabulary(voc)
    want = R.transform(tv.UNEQUAL_FEATS, 1)
    if (scoring, weighting) == (5, 0):
        assert list(want[1]) == [4.5, 1.0]
    got = V.transform(tv.UNEQUAL_FEATS, 1)
    print("BowVector", list(got[1]), "oracle", list(want[1]))
    _same_transform(got, want)
    _same_transform(_batch(torch, dev, V, _one(tv.UNEQUAL_FEATS), [5], 5, 1)[0], want)


@pytest.mark.parametrize("scoring,weighting", tv.WEIGHTINGS_AND_SCORINGS)
def test_word_shared_by_unequal_weights_at_scale(oracle_mod, dev, scoring, weighting):
    import torch
    from monoorbslam3_amd.vocabulary import ORBVocabulary
    voc, desc = tv.cleared_leaves_case(scoring, weighting)
    V, R = ORBVocabulary.from_arrays(voc), oracle_mod.Vocabulary(voc)
    assert V.n_words == R.n_words == int(voc["is_leaf"].sum())
    word, _, w = R.transform_features(desc, 0)
    tv.check_word_zero_is_mixed(word, w, 100)
    for levelsup in (1, 0):
        want = R.transform(desc, levelsup)
        got = V.transform(desc, levelsup)
        print("word 0:", got[1][0], "oracle", want[1][0])
        _same_transform(got, want)
        _same_transform(_batch(torch, dev, V, _one(desc), [len(desc)], len(desc), levelsup)[0], want)


def _features_device(torch, dev, V, desc, levelsup):
    n = len(desc)
    d = _up(torch, dev, desc)
    word, node = torch.full((n,), -1, dtype=torch.int32, device=dev), torch.full((n,), -2, dtype=torch.int32, device=dev)
    w = torch.full((n,), -3.0, dtype=torch.float64, device=dev)
    V.transform_features_device(d.data_ptr(), n, levelsup, word.data_ptr(), node.data_ptr(), w.data_ptr())
    torch.cuda.synchronize()
    return word.cpu().numpy().view(np.uint32), node.cpu().numpy().view(np.uint32), w.cpu().numpy()


def test_uneven_fanout_ties_and_upper_half(oracle_mod, dev):
    """1, 4, 5, 6, 11 and 20 children under one tree; exact ties, also across the descent's groups of five, stay with the first
    child; one pair is told apart by bytes 16..31 alone.  fanout_queries() establishes every expectation with plain distances."""
    import torch
    from monoorbslam3_amd.vocabulary import ORBVocabulary
    voc, first = tv.fanout_tree()
    q, want_node = tv.fanout_queries(voc, first)
    V, R = ORBVocabulary.from_arrays(voc), oracle_mod.Vocabulary(voc)
    for levelsup in (0, 1, 2):
        rw, rn, rwt = R.transform_features(q, levelsup)
        if levelsup == 0:
            assert np.array_equal(rn, want_node)
        word, node, w = _features_device(torch, dev, V, q, levelsup)
        assert np.array_equal(word, rw) and np.array_equal(node, rn) and w.tobytes() == rwt.tobytes(), levelsup
        _same_transform(V.transform(q, levelsup), R.transform(q, levelsup))
        _same_transform(_batch(torch, dev, V, _one(q), [len(q)], len(q), levelsup)[0], R.transform(q, levelsup))


@pytest.mark.parametrize("k", [1, 2])
def test_deep_trees(oracle_mod, dev, k):
    """L = 10: a chain and a binary tree; levelsup below, at and above L"""
    import torch
    from monoorbslam3_amd.vocabulary import ORBVocabulary
    voc, desc = tv.deep_tree(k)
    V, R = ORBVocabulary.from_arrays(voc), oracle_mod.Vocabulary(voc)
    saw_no_node = False
    for levelsup in (0, 4, 9, 10, 12):
        rw, rn, rwt = R.transform_features(desc, levelsup)
        saw_no_node |= bool((rn == NO_NODE).any())
        word, node, w = _features_device(torch, dev, V, desc, levelsup)
        assert np.array_equal(word, rw) and np.array_equal(node, rn) and w.tobytes() == rwt.tobytes(), levelsup
        _same_transform(V.transform(desc, levelsup), R.transform(desc, levelsup))
    assert saw_no_node == (k == 2)  # the chain has no early leaf; the binary tree has
    _same_transform(_batch(torch, dev, V, _one(desc), [len(desc)], len(desc), 0)[0], R.transform(desc, 0))


def test_root_only_tree(oracle_mod, dev):
    import torch
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.vocabulary import ORBVocabulary
    V, R = ORBVocabulary.from_arrays(tv.ROOT_ONLY), oracle_mod.Vocabulary(tv.ROOT_ONLY)
    assert (V.n_nodes, V.n_words, R.n_words) == (1, 0, 0)
    want = R.transform(tv.UNEQUAL_FEATS, 2)
    got = V.transform(tv.UNEQUAL_FEATS, 2)
    _same_transform(got, want)
    assert len(got[0]) == len(got[2][0]) == len(got[2][2]) == 0 and list(got[2][1]) == [0]
    desc = np.zeros((2, 5, 32), np.uint8)
    desc[0] = tv.UNEQUAL_FEATS
    for frame in _batch(torch, dev, V, desc, [5, 0], 5, 2):
        _same_transform(frame, want)  # _batch has checked that only the counts and fv_off[0] were written
    d = _up(torch, dev, tv.UNEQUAL_FEATS)
    out = torch.zeros(5, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.OrbxError) as e:
        V.transform_features_device(d.data_ptr(), 5, 2, out.data_ptr(), out.data_ptr(), out.data_ptr())
    assert e.value.code == -1  # ORBX_E_ARG


# ------------------------------------------------------------------------------------------- 6. the batch contract
_contract = {}


def _contract_case(oracle_mod):
    """(vocabulary, oracle, desc [6][300][32], counts): computed once, shared, never changed"""
    if not _contract:
        voc = synth.make_vocabulary(10, 4, seed=71, p_early_leaf=0.2, p_stop=0.1)
        R = oracle_mod.Vocabulary(voc)
        cap, counts = 300, [340, 0, 1, 257, 300, 300]
        desc = synth.make_descriptors_near_words(voc, len(counts) * cap, seed=72).reshape(len(counts), cap, 32).copy()
        # frame 5: descriptors of stopped words only, each one checked with the oracle to end in a word of weight 0
        stopped = voc["desc"][(voc["is_leaf"] > 0) & (voc["weight"] == 0) & (np.arange(len(voc["weight"])) > 0)]
        stopped = stopped[R.transform_features(stopped, 0)[2] == 0]
        assert len(stopped) >= 50
        desc[5] = stopped[np.random.RandomState(73).randint(0, len(stopped), cap)]
        _contract.update(voc=voc, R=R, desc=desc, counts=counts, cap=cap, want={})
    return _contract


def _contract_want(c, levelsup):
    if levelsup not in c["want"]:
        c["want"][levelsup] = [c["R"].transform(c["desc"][f, : min(n, c["cap"])], levelsup) for f, n in enumerate(c["counts"])]
    return c["want"][levelsup]


@pytest.mark.parametrize("kind", ["chain", "null"])
def test_batch_contract_padded(oracle_mod, dev, kind):
    import torch
    from monoorbslam3_amd.vocabulary import ORBVocabulary
    c = _contract_case(oracle_mod)
    V = ORBVocabulary.from_arrays(c["voc"])
    for levelsup in (0, 2, 4, 7):
        want = _contract_want(c, levelsup)
        got = _batch(torch, dev, V, c["desc"], c["counts"], c["cap"], levelsup, kind)
        for f, (g, w) in enumerate(zip(got, want)):
            _same_transform(g, w)
            nodes = g[2][0]
            assert not (nodes[:-1] == NO_NODE).any(), f  # ORBV_NO_NODE is the largest key: it can only be the last row
        # what the case is there for, asked of the oracle's side
        stopped_in_live_frames = sum(min(n, c["cap"]) - w[2][1][-1] for n, w in zip(c["counts"][:5], want[:5]))
        assert stopped_in_live_frames > 20
        assert [len(w[0]) for w in want][5] == 0 and len(want[5][2][0]) == 0 and len(want[1][0]) == 0
        has_no_node = [len(w[2][0]) > 0 and w[2][0][-1] == NO_NODE for w in want]
        if levelsup == 0:
            assert has_no_node[0] and has_no_node[3] and has_no_node[4]  # early leaves end above level L - levelsup = 4
        elif levelsup == 2:
            assert not any(has_no_node) and all(len(want[f][2][0]) > 10 for f in (0, 3, 4))  # no leaf above level 2
        else:
            assert all(list(want[f][2][0]) == [0] for f in (0, 3, 4))  # levelsup >= L: every feature under the root


def test_one_handle_across_capacities(oracle_mod, dev):
    import torch
    from monoorbslam3_amd import _lib
    from monoorbslam3_amd.vocabulary import ORBVocabulary
    c = _contract_case(oracle_mod)
    V, R = ORBVocabulary.from_arrays(c["voc"]), c["R"]
    ones = c["desc"][:3, :1].copy()
    for f, g in enumerate(_batch(torch, dev, V, ones, [1, 0, 5], 1, 2)):  # cap = 1: a count of 5 is one feature
        _same_transform(g, R.transform(ones[f, : [1, 0, 1][f]], 2))
    full = synth.make_descriptors_near_words(c["voc"], 8192, seed=74)
    _same_transform(_batch(torch, dev, V, _one(full), [8192], 8192, 2)[0], R.transform(full, 2))  # the scratch grows
    want = _contract_want(c, 2)
    for g, w in zip(_batch(torch, dev, V, c["desc"], c["counts"], c["cap"], 2), want):  # and is reused by a smaller call
        _same_transform(g, w)
    out = torch.zeros(8, dtype=torch.float64, device=dev)
    with pytest.raises(_lib.OrbxError) as e:
        V.transform_device(1, out.data_ptr(), out.data_ptr(), 8193, 2, *[out.data_ptr()] * 7)
    assert e.value.code == -4  # ORBX_E_UNSUPPORTED: refused before anything is read or launched
