"""The two restatements of the covisibility graph in tests/graph_model.py against each other after every operation, the cases the scenes
were built for, :428-460 literally against its simplification, and the entry points' argument checks through the library.  No GPU."""
import ctypes as C

import numpy as np
import pytest

import graph_model as gm

_cache = {}


def replayed(name):
    """a scene replayed once (the array form and the objects compared after every operation), shared, never changed"""
    if name not in _cache:
        _cache[name] = gm.replay(name)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(gm.SCENES))
def test_the_array_form_and_the_objects_agree_after_every_operation(name):
    """maps, lists, parents and children of the array form equal the KeyFrame objects' after each of the 80 / 400 operations (asserted
    inside the replay); the scene holds every case it was built for; the fuse's targets and rows equal searchInNeighbors on the objects"""
    rep = replayed(name)
    sc = gm.check_scene(rep)
    n_kf = sc["n_kf"]
    print(name, "cases", sorted(rep["tags"]), "lists rebuilt", int(sum(r[gm.U_REBUILT] for r, o in zip(rep["results"], rep["ops"]) if o[0] == "update")))
    kfs = rep["kfs"]
    for k, kf in enumerate(kfs):
        kf.map_points = [(int(p), int(sc["valid"][p])) if 0 <= p < sc["cap_points"] else None for p in sc["slots"][k, :min(max(int(sc["n"][k]), 0), sc["stride"])]]
    targets, rows, res = gm.run_fuse(rep, sc)
    want_targets, want_rows = gm.search_in_neighbors(kfs, kfs[sc["cur"]], stamp=object())
    assert targets.tolist() == want_targets and rows.tolist() == want_rows
    for kf_ in (sc["cur"], int(targets[0])):
        out, n = gm.connected(rep["graph"], n_kf, kf_, True, n_kf, n_kf + 1)
        assert out[:n].tolist() == [kf_] + [o.id for o in kfs[kf_].ordered_connected_kfs] and (out[n:] == -1).all()
        out, n = gm.connected(rep["graph"], n_kf, kf_, False, 3, 5)
        assert out[:n].tolist() == [o.id for o in kfs[kf_].get_best_covisible_kfs(3)] and (out[n:] == -1).all()


def test_the_spanning_tree_loop_is_its_simplification():
    """KeyFrame.cpp:428-460 restated literally leaves every child, linked or not, bad or not, with the erased key frame's parent: on 200
    seeded random trees with random weights"""
    moved = 0
    for seed in range(200):
        kfs, c = gm.random_tree(seed)
        P, kids, others = c.parent, set(c.children_set), {k: k.parent for k in kfs}
        c.set_bad()
        assert all(k.parent is P for k in kids) and c.parent is P and c not in P.children_set
        assert all(k.parent is others[k] for k in kfs if k not in kids)
        moved += len(kids)
    assert moved > 200


@pytest.fixture(scope="module")
def mlib():
    import __graft_entry__ as g
    g.build()
    from monoorbslam3_amd import matcher
    return matcher._mlib(), matcher


def _graph(matcher, cap=64, **over):
    f = dict(cap_kf=cap, d_weight=0x1000, d_ord_kf=0x1000, d_ord_n=0x1000, d_parent=0x1000)
    f.update(over)
    return matcher.CovisGraph(f["cap_kf"], f["d_weight"], f["d_ord_kf"], f["d_ord_n"], f["d_parent"])


def _calls(L, matcher, g, n_kf=32, kf=3, n_recent=4):
    """the four entry points with valid arguments (fake, never dereferenced device pointers) but for the graph, n_kf, the key frame
    and n_recent; -> their return codes"""
    P = 0x1000
    gp = C.byref(g) if g is not None else None
    rec = (C.c_int32 * 40)(*([1] * 40))
    return [L.orbm_update_connections_device(None, gp, n_kf, P, P, kf, -1, 15, P, P, None),
            L.orbm_erase_connections_device(None, gp, n_kf, C.cast(rec, C.c_void_p), n_recent, P, P, P, None),
            L.orbm_fuse_targets_device(None, gp, n_kf, P, P, P, 64, P, 500, kf, 20, 5, 120, 500, P, P, P, P, None),
            L.orbm_connected_keyframes_device(None, gp, n_kf, kf, 1, n_kf, P, 40, P, None)]


def test_the_entry_points_check_their_arguments_before_any_device_call(mlib):
    L, matcher = mlib
    E_ARG, E_NO_DEVICE, E_UNSUPPORTED = -1, -2, -4
    import torch
    assert _calls(L, matcher, None) == [E_ARG] * 4
    assert _calls(L, matcher, _graph(matcher, d_weight=None)) == [E_ARG] * 4
    assert _calls(L, matcher, _graph(matcher), n_kf=65) == [E_ARG] * 4
    got = _calls(L, matcher, _graph(matcher), kf=32)
    assert got[0] == got[2] == got[3] == E_ARG
    got = _calls(L, matcher, _graph(matcher), kf=-1)
    assert got[0] == got[2] == got[3] == E_ARG
    assert _calls(L, matcher, _graph(matcher), n_recent=33)[1] == E_ARG
    assert L.orbx_last_error()
    assert _calls(L, matcher, _graph(matcher, cap=4097)) == [E_UNSUPPORTED] * 4
    assert C.sizeof(matcher.CovisGraph) == 40                        # int32, padding, four pointers: the header's struct
    if not torch.cuda.is_available():
        assert _calls(L, matcher, _graph(matcher)) == [E_NO_DEVICE] * 4
        assert _calls(L, matcher, _graph(matcher, cap=4096), n_kf=4096) == [E_NO_DEVICE] * 4
