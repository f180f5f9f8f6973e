"""Python mirror of the reference's ORBMatcher over the C ABI (include/orbm.h).

Same constructor as modules/ORB/ORBMatcher.h:14 (nnRatio, checkOrientation) and the
Search* entry points of the north-star path, expressed over plain arrays instead of
Frame / KeyFrame objects: a "frame" here is (descriptors[n,32], angles[n] or
keypoints, FeatureVector CSR, map-point mask).  Distances are computed by the HIP
kernels; the library's host code performs the reference's greedy resolution.
"""
import ctypes as C

import numpy as np

from . import _lib
from .extractor import KP_DTYPE

TH_LOW, TH_HIGH, HISTO_LENGTH = 50, 100, 30
# kernel-choice switches of include/orbm.h (ORBM_VAR_*): name -> index
VARIANTS = {"best2": 0, "window": 1, "best2_resident": 2, "init_lanes": 3, "init_max_sweeps": 4}


class _Fv(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("node_ids", C.c_void_p), ("offsets", C.c_void_p), ("indices", C.c_void_p)]


class ProjCamera(C.Structure):
    """orbm_proj_camera (include/orbm.h): the camera of the query builders, every field a float as in the reference's Camera."""
    _fields_ = [("model", C.c_int32), ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
                ("k", C.c_float * 4), ("min_x", C.c_float), ("max_x", C.c_float), ("min_y", C.c_float), ("max_y", C.c_float)]

    @classmethod
    def make(cls, cam, bounds):
        """cam = (fx, fy, cx, cy) -> Pinhole, (fx, fy, cx, cy, k1, k2, k3, k4) -> Fisheye (as ba._cam_tail); bounds = (min_x, max_x,
        min_y, max_y) of isInImage -- for Fisheye (0, width, 0, height)."""
        assert len(cam) in (4, 8) and len(bounds) == 4
        k = tuple(cam[4:]) if len(cam) == 8 else (0.0, 0.0, 0.0, 0.0)
        return cls(1 if len(cam) == 8 else 0, cam[0], cam[1], cam[2], cam[3], (C.c_float * 4)(*k), *bounds)


class KfTable(C.Structure):
    """orbm_kf_table (include/orbm.h): a host struct of device pointers to the key frames the refresh reads."""
    _fields_ = [("n_kf", C.c_int32), ("d_pose_R", C.c_void_p), ("d_pose_t", C.c_void_p), ("d_bad", C.c_void_p), ("d_kps", C.c_void_p),
                ("d_desc", C.c_void_p), ("d_n", C.c_void_p)]

    @classmethod
    def make(cls, pose_R, pose_t, bad, kps, desc, n):
        """torch device tensors: pose_R f64 [n_kf,9], pose_t f64 [n_kf,3], bad u8 [n_kf], n i32 [n_kf]; kps / desc either int64
        [n_kf] tensors of device addresses or lists of per-key-frame tensors (their addresses are uploaded)."""
        import torch
        n_kf = int(n.shape[0])

        def pointers(x):
            if isinstance(x, (list, tuple)):
                assert len(x) == n_kf
                return torch.tensor([t.data_ptr() for t in x], dtype=torch.int64).to(n.device), x
            assert x.dtype == torch.int64 and x.shape[0] == n_kf
            return x, None

        pk, keep_k = pointers(kps)
        pd, keep_d = pointers(desc)
        t = cls(n_kf, pose_R.data_ptr(), pose_t.data_ptr(), bad.data_ptr(), pk.data_ptr(), pd.data_ptr(), n.data_ptr())
        t._keep = (pose_R, pose_t, bad, pk, pd, n, keep_k, keep_d)
        return t


class CovisGraph(C.Structure):
    """orbm_covis_graph (include/orbm.h): a host struct of device pointers to the covisibility graph and the spanning tree."""
    _fields_ = [("cap_kf", C.c_int32), ("d_weight", C.c_void_p), ("d_ord_kf", C.c_void_p), ("d_ord_n", C.c_void_p), ("d_parent", C.c_void_p)]
    CONNECT_TH = 15   # modules/BasicObject/KeyFrame.h:24

    @classmethod
    def make(cls, weight, ord_kf, ord_n, parent):
        """torch device tensors, i32: weight, ord_kf [cap_kf, cap_kf] (weight and ord_n zero-filled once), ord_n, parent [cap_kf]
        (parent filled with -1 once)."""
        cap = int(ord_n.shape[0])
        assert weight.numel() == cap * cap and ord_kf.numel() == cap * cap and parent.numel() == cap
        g = cls(cap, weight.data_ptr(), ord_kf.data_ptr(), ord_n.data_ptr(), parent.data_ptr())
        g._keep = (weight, ord_kf, ord_n, parent)
        return g

    @classmethod
    def empty(cls, cap_kf, device):
        """an empty graph of cap_kf key frames on `device`, initialised as the header asks"""
        import torch
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=device)  # noqa: E731
        return cls.make(z(cap_kf, cap_kf), z(cap_kf, cap_kf), z(cap_kf), torch.full((cap_kf,), -1, dtype=torch.int32, device=device))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


_sigs_done = False


def _mlib():
    global _sigs_done
    L = _lib.lib()
    if not _sigs_done:
        vp, i32, f32, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
        sigs = {
            "orbm_create": (i32, [i32, C.POINTER(vp)]),
            "orbm_destroy": (None, [vp]),
            "orbm_set_variant": (i32, [vp, i32, i32]),
            "orbm_hamming_matrix": (i32, [vp, vp, i32, vp, i32, vp]),
            "orbm_hamming_matrix_device": (i32, [vp, vp, i32, vp, i32, vp, vp]),
            "orbm_best2_device": (i32, [vp, i32, vp, sz, vp, i32, vp, sz, vp, i32, vp, vp, vp, vp, vp, vp]),
            "orbm_best2": (i32, [vp, vp, i32, vp, i32, vp, vp, vp, vp, vp]),
            "orbm_hamming_csr": (i32, [vp, vp, i32, vp, i32, vp, vp, i32, vp, vp]),
            "orbm_search_by_bow": (i32, [vp, f32, i32, vp, vp, vp, i32, C.POINTER(_Fv), vp, vp, vp, i32,
                                         C.POINTER(_Fv), C.POINTER(i32)]),
            "orbm_search_for_triangulation": (i32, [vp, i32, vp, vp, vp, i32, C.POINTER(_Fv), vp, vp, vp, i32,
                                                    C.POINTER(_Fv), vp, C.POINTER(i32)]),
            "orbm_search_for_initialization": (i32, [vp, f32, i32, vp, vp, i32, vp, vp, i32, i32, i32, vp, vp, i32,
                                                     C.POINTER(i32)]),
            "orbm_search_by_projection_frame": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, vp,
                                                      C.POINTER(i32)]),
            "orbm_search_by_projection_points": (i32, [vp, f32, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, vp,
                                                       C.POINTER(i32), vp]),
            "orbm_search_fuse": (i32, [vp, vp, vp, vp, vp, vp, i32, vp, vp, i32, i32, i32, vp, i32, vp, vp, C.POINTER(i32)]),
            "orbm_search_by_projection_frame_device": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32,
                                                             vp, vp, vp]),
            "orbm_search_by_projection_points_device": (i32, [vp, f32, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, i32,
                                                              vp, vp, vp]),
            "orbm_search_by_bow_device": (i32, [vp, f32, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp]),
            "orbm_search_for_initialization_device": (i32, [vp, f32, i32, vp, vp, i32, vp, vp, vp, vp, i32, i32, i32, vp, i32, i32,
                                                            vp, vp, vp]),
            "orbm_search_fuse_device": (i32, [vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, i32, i32, vp, i32, vp, vp, vp, vp]),
            "orbm_search_for_triangulation_device": (i32, [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, vp, vp, vp, vp,
                                                           vp, vp]),
            "orbm_window_lists_device": (i32, [vp, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, i32, vp, i32, vp, vp, vp]),
            "orbm_project_frame_device": (i32, [vp, C.POINTER(ProjCamera), vp, vp, vp, vp, vp, i32, f32, vp, vp, vp, vp, vp, vp, vp]),
            "orbm_project_frustum_device": (i32, [vp, C.POINTER(ProjCamera), vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, f32, f32,
                                                  f32, vp, vp, vp, vp, vp, vp, vp]),
            "orbm_project_fuse_device": (i32, [vp, C.POINTER(ProjCamera), vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, f32, f32, vp, vp, vp,
                                               vp, vp, vp]),
            "orbm_triangulate_matches_device": (i32, [vp, C.POINTER(ProjCamera), vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp,
                                                      i32, f32, C.c_double, C.c_double, f32, vp, i32] + [vp] * 14),
            "orbm_triangulate_matches": (i32, [vp, C.POINTER(ProjCamera), vp, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32,
                                               f32, C.c_double, C.c_double, f32, vp, i32] + [vp] * 13),
            "orbm_refresh_points_device": (i32, [vp, C.POINTER(KfTable), vp, i32, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, f32, i32,
                                                 vp, vp, vp]),
            "orbm_scene_median_depth_device": (i32, [vp, i32, vp, vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp]),
            "orbm_build_observations_device": (i32, [vp, i32, vp, vp, vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]),
            "orbm_cull_keyframes_device": (i32, [vp, C.POINTER(KfTable), vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, i32, i32,
                                                 C.c_double, C.c_double, vp, vp, vp, vp, vp]),
            "orbm_fuse_apply_device": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, vp, vp]),
            "orbm_local_ba_problem_device": (i32, [vp, C.POINTER(KfTable), vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32]
                                             + [vp] * 16),
            "orbm_local_ba_apply_device": (i32, [vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32]
                                           + [vp] * 11),
            "orbm_inertial_window_problem_device": (i32, [vp, C.POINTER(KfTable), vp, i32, vp, vp, i32, vp, vp, vp, i32, vp, i32, vp, i32, i32, i32, i32,
                                                          i32, i32, i32] + [vp] * 20),
            "orbm_inertial_window_velocity_prior_device": (i32, [vp, vp, i32, vp, i32, vp, vp, vp, vp]),
            "orbm_inertial_chain_problem_device": (i32, [vp, i32, vp, vp, i32, vp, i32, i32, i32] + [vp] * 9),
            "orbm_inertial_chain_velocity_priors_device": (i32, [vp, vp, i32, vp, i32, vp, i32, vp, vp]),
            "orbm_apply_scale_rotation_device": (i32, [vp, vp, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, vp, vp, i32, vp, i32, f32, vp, vp]),
            "orbm_update_connections_device": (i32, [vp, C.POINTER(CovisGraph), i32, vp, vp, i32, i32, i32, vp, vp, vp]),
            "orbm_erase_connections_device": (i32, [vp, C.POINTER(CovisGraph), i32, vp, i32, vp, vp, vp, vp]),
            "orbm_fuse_targets_device": (i32, [vp, C.POINTER(CovisGraph), i32, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp,
                                               vp, vp]),
            "orbm_connected_keyframes_device": (i32, [vp, C.POINTER(CovisGraph), i32, i32, i32, i32, vp, i32, vp, vp]),
            "orbm_local_map_device": (i32, [vp, vp, i32, vp, i32, vp, vp, vp, i32, i32, vp, vp, vp, i32, C.POINTER(CovisGraph), vp, i32, i32, i32, i32,
                                            i32, vp, vp, vp, vp, vp, vp, vp]),
            "orbm_track_counters_device": (i32, [vp, vp, i32, vp, i32, vp, i32, i32, vp, vp, vp, vp]),
            "orbm_num_tracked_points_device": (i32, [vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp]),
            "orbm_insert_keyframe_device": (i32, [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, vp, vp, vp]),
            "orbm_register_new_points_device": (i32, [vp, vp, vp, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, vp, vp]),
            "orbm_cull_map_points_device": (i32, [vp, vp, vp, i32, i32, vp, vp, vp, vp, i32, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp]),
            "orbm_distinctive_descriptors": (i32, [vp, vp, vp, i32, vp]),
            "orbm_distinctive_descriptors_device": (i32, [vp, vp, vp, i32, vp, vp]),
            "orbm_three_maxima": (None, [vp, i32, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]),
            "orbm_two_view_ransac_device": (i32, [vp, vp, i32, vp, i32, vp, f32, i32, C.c_uint64] + [vp] * 12),
            "orbm_two_view_ransac": (i32, [vp, vp, i32, vp, i32, vp, f32, i32, C.c_uint64] + [vp] * 11),
            "orbm_two_view_sets": (i32, [i32, i32, C.c_uint64, vp]),
            "orbm_two_view_pose_device": (i32, [vp, f32, f32, f32, f32, vp, i32, vp, i32] + [vp] * 7 + [i32, f32, f32] + [vp] * 12),
            "orbm_two_view_pose": (i32, [vp, f32, f32, f32, f32, vp, i32, vp, i32] + [vp] * 7 + [i32, f32, f32] + [vp] * 11),
            "orbm_two_view_decide": (i32, [i32, vp, vp, i32, f32, vp, vp, vp]),
        }
        for name, (res, args) in sigs.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _sigs_done = True
    return L


def _fv(csr):
    node_ids, offsets, indices = csr
    node_ids = np.ascontiguousarray(node_ids, dtype=np.uint32)
    offsets = np.ascontiguousarray(offsets, dtype=np.int32)
    indices = np.ascontiguousarray(indices, dtype=np.uint32)
    f = _Fv(len(node_ids), node_ids.ctypes.data, offsets.ctypes.data, indices.ctypes.data)
    f._keep = (node_ids, offsets, indices)
    return f


_default = None


def _handle():
    global _default
    if _default is None:
        _default = MatcherHandle()
    return _default


class MatcherHandle:
    """One orbm_t: a HIP stream plus scratch.  Use one per host thread."""

    def __init__(self, device=-1):
        self._L = _mlib()
        self._h = C.c_void_p()
        _lib.check(self._L.orbm_create(device, C.byref(self._h)))

    def set_variant(self, name, value):
        """orbm_set_variant: "best2" = "fp4" | "i8" | "valu" (dense best / second-best kernel), "window" = "device" | "host",
        "best2_resident" = 0 | 1 | 2 (k_best2_fp4 as that many workgroups per CU walking the query blocks), "init_lanes" = 0 | 1 |
        4 | 16 | 64, "init_max_sweeps" = 0 (the default cap, ORBM_INIT_MAX_SWEEPS) | 1 .. 64 (SearchForInitializationDevice)."""
        which = VARIANTS[name]
        val = {"fp4": 0, "i8": 1, "valu": 2, "device": 0, "host": 1}.get(value, value)
        _lib.check(self._L.orbm_set_variant(self._h, which, int(val)))

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._L.orbm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ORBMatcher:
    """ORBMatcher(nnRatio=0.6, checkOrientation=True) (reference modules/ORB/ORBMatcher.h:14)."""

    def __init__(self, nnRatio=0.6, checkOrientation=True, handle=None):
        self.nn_ratio = float(nnRatio)
        self.be_check_orientation = bool(checkOrientation)
        self._hd = handle or _handle()
        self._L = self._hd._L

    # -- DescriptorDistance (ORBMatcher.cpp:17-31) --------------------------------
    @staticmethod
    def DescriptorDistance(a, b):
        return int(ORBMatcher.hamming_matrix(np.asarray(a, np.uint8).reshape(1, 32),
                                             np.asarray(b, np.uint8).reshape(1, 32))[0, 0])

    @staticmethod
    def hamming_matrix(a, b, handle=None):
        hd = handle or _handle()
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, 32)
        out = np.zeros((len(a), len(b)), np.uint16)
        _lib.check(hd._L.orbm_hamming_matrix(hd._h, _vp(a), len(a), _vp(b), len(b), _vp(out)))
        return out

    @staticmethod
    def best2(a, b, row_ok=None, col_ok=None, handle=None):
        """(best index, best distance, second distance) per row of `a` among rows of `b`."""
        hd = handle or _handle()
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, 32)
        bi = np.zeros(len(a), np.int32)
        bd = np.zeros(len(a), np.uint16)
        sd = np.zeros(len(a), np.uint16)
        ro = None if row_ok is None else np.ascontiguousarray(row_ok, dtype=np.uint8)
        co = None if col_ok is None else np.ascontiguousarray(col_ok, dtype=np.uint8)
        _lib.check(hd._L.orbm_best2(hd._h, _vp(a), len(a), _vp(b), len(b), None if ro is None else _vp(ro),
                                    None if co is None else _vp(co), _vp(bi), _vp(bd), _vp(sd)))
        return bi, bd, sd

    @staticmethod
    def hamming_csr(a, b, q_idx, off, c_idx, handle=None):
        hd = handle or _handle()
        a = np.ascontiguousarray(a, dtype=np.uint8).reshape(-1, 32)
        b = np.ascontiguousarray(b, dtype=np.uint8).reshape(-1, 32)
        q_idx = np.ascontiguousarray(q_idx, dtype=np.int32)
        off = np.ascontiguousarray(off, dtype=np.int32)
        c_idx = np.ascontiguousarray(c_idx, dtype=np.int32)
        out = np.zeros(int(off[-1]) if len(off) else 0, np.uint16)
        _lib.check(hd._L.orbm_hamming_csr(hd._h, _vp(a), len(a), _vp(b), len(b), _vp(q_idx), _vp(off), len(q_idx),
                                          _vp(c_idx), _vp(out)))
        return out

    @staticmethod
    def ComputeDistinctiveDescriptors(desc, off, handle=None):
        """MapPoint::computeDescriptor (MapPoint.cpp:103-152) for many map points: desc[off[g]:off[g+1]] are the
        observations of point g; returns the index (inside its group) of each point's new descriptor, -1 if none."""
        hd = handle or _handle()
        desc = np.ascontiguousarray(desc, dtype=np.uint8).reshape(-1, 32)
        off = np.ascontiguousarray(off, dtype=np.int32)
        out = np.zeros(max(len(off) - 1, 0), np.int32)
        _lib.check(hd._L.orbm_distinctive_descriptors(hd._h, _vp(desc), _vp(off), len(off) - 1, _vp(out)))
        return out

    @staticmethod
    def ComputeThreeMaxima(hist_sizes):
        L = _mlib()
        s = np.ascontiguousarray(hist_sizes, dtype=np.int32)
        i1, i2, i3 = C.c_int(-1), C.c_int(-1), C.c_int(-1)
        L.orbm_three_maxima(_vp(s), len(s), C.byref(i1), C.byref(i2), C.byref(i3))
        return i1.value, i2.value, i3.value

    # -- SearchByBow (ORBMatcher.cpp:118-201) --------------------------------------
    def SearchByBow(self, kf_desc, kf_angles, kf_mp_ok, kf_fv, fr_desc, fr_angles, frame_mp, fr_fv):
        """Returns (numMatch, frame_mp'): frame_mp'[j] = key-frame feature whose MapPoint is assigned, -1 = null."""
        d1 = np.ascontiguousarray(kf_desc, dtype=np.uint8)
        d2 = np.ascontiguousarray(fr_desc, dtype=np.uint8)
        a1 = np.ascontiguousarray(kf_angles, dtype=np.float32)
        a2 = np.ascontiguousarray(fr_angles, dtype=np.float32)
        ok = np.ascontiguousarray(kf_mp_ok, dtype=np.uint8)
        mp = np.ascontiguousarray(frame_mp, dtype=np.int32).copy()
        f1, f2 = _fv(kf_fv), _fv(fr_fv)
        n = C.c_int()
        _lib.check(self._L.orbm_search_by_bow(self._hd._h, self.nn_ratio, int(self.be_check_orientation), _vp(d1),
                                              _vp(a1), _vp(ok), len(d1), C.byref(f1), _vp(d2), _vp(a2), _vp(mp),
                                              len(d2), C.byref(f2), C.byref(n)))
        return n.value, mp

    # -- SearchForTriangulation (ORBMatcher.cpp:417-522) -----------------------------
    def SearchForTriangulation(self, desc1, angles1, has_mp1, fv1, desc2, angles2, has_mp2, fv2):
        d1 = np.ascontiguousarray(desc1, dtype=np.uint8)
        d2 = np.ascontiguousarray(desc2, dtype=np.uint8)
        a1 = np.ascontiguousarray(angles1, dtype=np.float32)
        a2 = np.ascontiguousarray(angles2, dtype=np.float32)
        h1 = np.ascontiguousarray(has_mp1, dtype=np.uint8)
        h2 = np.ascontiguousarray(has_mp2, dtype=np.uint8)
        m12 = np.full(len(d1), -1, np.int32)
        f1, f2 = _fv(fv1), _fv(fv2)
        n = C.c_int()
        _lib.check(self._L.orbm_search_for_triangulation(self._hd._h, int(self.be_check_orientation), _vp(d1), _vp(a1),
                                                         _vp(h1), len(d1), C.byref(f1), _vp(d2), _vp(a2), _vp(h2),
                                                         len(d2), C.byref(f2), _vp(m12), C.byref(n)))
        return n.value, m12

    # -- SearchForInitialization (ORBMatcher.cpp:33-116) -----------------------------
    def SearchForInitialization(self, kps1, desc1, kps2, desc2, img_w, img_h, vecPreMatched, windowSize=100):
        k1 = np.ascontiguousarray(kps1, dtype=KP_DTYPE)
        k2 = np.ascontiguousarray(kps2, dtype=KP_DTYPE)
        d1 = np.ascontiguousarray(desc1, dtype=np.uint8)
        d2 = np.ascontiguousarray(desc2, dtype=np.uint8)
        pre = np.ascontiguousarray(vecPreMatched, dtype=np.float32).copy()
        m12 = np.full(len(k1), -1, np.int32)
        n = C.c_int()
        _lib.check(self._L.orbm_search_for_initialization(self._hd._h, self.nn_ratio, int(self.be_check_orientation),
                                                          _vp(k1), _vp(d1), len(k1), _vp(k2), _vp(d2), len(k2), img_w,
                                                          img_h, _vp(pre), _vp(m12), windowSize, C.byref(n)))
        return n.value, m12, pre

    # -- SearchByProjection(lastFrame | lastKF, curFrame, th) (ORBMatcher.cpp:203-348) ----------
    def SearchByProjectionFrame(self, q_desc, q_xy, q_radius, q_octave, q_angle, q_ok, kps2, desc2, img_w, img_h,
                                frame_mp):
        """Queries = features of the last frame with their MapPoint descriptor and projected position (the camera
        maths stays with the caller).  Returns (numMatch, frame_mp')."""
        qd = np.ascontiguousarray(q_desc, dtype=np.uint8)
        qx = np.ascontiguousarray(q_xy, dtype=np.float32)
        qr = np.ascontiguousarray(q_radius, dtype=np.float32)
        qo = np.ascontiguousarray(q_octave, dtype=np.int32)
        qa = np.ascontiguousarray(q_angle, dtype=np.float32)
        qk = np.ascontiguousarray(q_ok, dtype=np.uint8)
        k2 = np.ascontiguousarray(kps2, dtype=KP_DTYPE)
        d2 = np.ascontiguousarray(desc2, dtype=np.uint8)
        mp = np.ascontiguousarray(frame_mp, dtype=np.int32).copy()
        n = C.c_int()
        _lib.check(self._L.orbm_search_by_projection_frame(self._hd._h, int(self.be_check_orientation), _vp(qd), _vp(qx),
                                                           _vp(qr), _vp(qo), _vp(qa), _vp(qk), len(qd), _vp(k2), _vp(d2),
                                                           len(k2), img_w, img_h, _vp(mp), C.byref(n)))
        return n.value, mp

    # -- SearchByProjection(frame, mapPoints, th) (ORBMatcher.cpp:350-415) -----------------------
    def SearchByProjectionPoints(self, q_desc, q_xy, q_radius, q_level, q_ok, kps2, desc2, img_w, img_h, frame_mp):
        """Returns (numMatch, frame_mp', (numOutViewAndBad, fail1, fail2))."""
        qd = np.ascontiguousarray(q_desc, dtype=np.uint8)
        qx = np.ascontiguousarray(q_xy, dtype=np.float32)
        qr = np.ascontiguousarray(q_radius, dtype=np.float32)
        ql = np.ascontiguousarray(q_level, dtype=np.int32)
        qk = np.ascontiguousarray(q_ok, dtype=np.uint8)
        k2 = np.ascontiguousarray(kps2, dtype=KP_DTYPE)
        d2 = np.ascontiguousarray(desc2, dtype=np.uint8)
        mp = np.ascontiguousarray(frame_mp, dtype=np.int32).copy()
        cnt = np.zeros(3, np.int32)
        n = C.c_int()
        _lib.check(self._L.orbm_search_by_projection_points(self._hd._h, self.nn_ratio, _vp(qd), _vp(qx), _vp(qr), _vp(ql),
                                                            _vp(qk), len(qd), _vp(k2), _vp(d2), len(k2), img_w, img_h,
                                                            _vp(mp), C.byref(n), _vp(cnt)))
        return n.value, mp, tuple(cnt.tolist())

    # -- the same two searches on a device-resident frame record, greedy pass on the device -----------------------
    def SearchByProjectionDevice(self, mode, d, nq, n2, grid_cols, grid_rows, list_cap=48, stream=None):
        """mode "frame" | "points".  d: dict of torch device tensors -- q_desc [nq,32] u8, q_xy [nq,2] f32, q_radius f32,
        q_level i32 (octave / predicted level), q_angle f32 (frame only), q_ok u8, kps2 (undistorted records, u8 [*,28]),
        desc2 u8 [*,32], cell_start i32, cell_items i32, frame_mp i32 [n2] (in/out), result i32 [8] (out).  Enqueues on
        `stream`; nothing is copied or synchronised (orbm_search_by_projection_{frame,points}_device)."""
        st = _lib.stream_arg(stream)
        p = lambda k: d[k].data_ptr()  # noqa: E731
        if mode == "frame":
            _lib.check(self._L.orbm_search_by_projection_frame_device(
                self._hd._h, int(self.be_check_orientation), p("q_desc"), p("q_xy"), p("q_radius"), p("q_level"), p("q_angle"),
                p("q_ok"), nq, p("kps2"), p("desc2"), p("cell_start"), p("cell_items"), grid_cols, grid_rows, n2, list_cap,
                p("frame_mp"), p("result"), st))
        else:
            _lib.check(self._L.orbm_search_by_projection_points_device(
                self._hd._h, self.nn_ratio, p("q_desc"), p("q_xy"), p("q_radius"), p("q_level"), p("q_ok"), nq, p("kps2"),
                p("desc2"), p("cell_start"), p("cell_items"), grid_cols, grid_rows, n2, list_cap, p("frame_mp"), p("result"), st))

    # -- the queries of those searches built on the device from a map-point table and a pose (orbm_project_*_device) ----------
    def ProjectFrameDevice(self, cam, d, nq, th, stream=None):
        """orbm_project_frame_device (ORBMatcher.cpp:212-229): cam a ProjCamera.  d: dict of torch device tensors -- pose_R f64 [9],
        pose_t f64 [3] (as pose_optimize_batch_device leaves them), points f32 [nq,3], valid u8, kps1 (the last frame's records, u8
        [*,28]) in; q_xy, q_radius, q_level (the octave), q_angle, q_ok and result i32 [8] out: the keys SearchByProjectionDevice
        ("frame") reads, so the same dict serves both calls.  Enqueues on `stream`; nothing is copied or synchronised."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_project_frame_device(
            self._hd._h, C.byref(cam), p("pose_R"), p("pose_t"), p("points"), p("valid"), p("kps1"), nq, th, p("q_xy"), p("q_radius"),
            p("q_level"), p("q_angle"), p("q_ok"), p("result"), _lib.stream_arg(stream)))

    def ProjectFrustumDevice(self, cam, d, nq, n2, scale_factors, log_scale_factor, th, view_cos_limit=0.5, stream=None):
        """orbm_project_frustum_device (Tracking.cpp:403-412, Frame.cpp:129-166, ORBMatcher.cpp:360-365).  d as for
        ProjectFrameDevice without kps1 / q_angle, plus normals f32 [nq,3], min_dist, max_dist f32 and frame_mp i32 [n2] in (points
        whose index it holds are off) and, optionally, view_cos f32 [nq] out.  scale_factors: host floats, at most 16."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
        _lib.check(self._L.orbm_project_frustum_device(
            self._hd._h, C.byref(cam), p("pose_R"), p("pose_t"), p("points"), p("valid"), p("normals"), p("min_dist"), p("max_dist"), nq,
            p("frame_mp"), n2, _vp(sf), len(sf), log_scale_factor, th, view_cos_limit, p("q_xy"), p("q_radius"), p("q_level"), p("q_ok"),
            p("view_cos") if d.get("view_cos") is not None else None, p("result"), _lib.stream_arg(stream)))

    def ProjectFuseDevice(self, cam, d, nq, scale_factors, log_scale_factor, th, stream=None):
        """orbm_project_fuse_device (ORBMatcher.cpp:534-553): d as for ProjectFrustumDevice without frame_mp / view_cos; `valid`
        carries the caller's three live tests (null, bad, already observed by the key frame).  The outputs are SearchFuseDevice's."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        sf = np.ascontiguousarray(scale_factors, dtype=np.float32)
        _lib.check(self._L.orbm_project_fuse_device(
            self._hd._h, C.byref(cam), p("pose_R"), p("pose_t"), p("points"), p("valid"), p("normals"), p("min_dist"), p("max_dist"), nq,
            _vp(sf), len(sf), log_scale_factor, th, p("q_xy"), p("q_radius"), p("q_level"), p("q_ok"), p("result"),
            _lib.stream_arg(stream)))

    # -- createNewMapPoints between SearchForTriangulation and the fuse (LocalMapping.cpp:171-253) ----------------------------
    def TriangulateMatchesDevice(self, cam, d, n1, n2, cap_points, sigma2, max_scale_factor, ratio_factor, cos_parallax=0.99998,
                                 chi2=5.991, stream=None):
        """orbm_triangulate_matches_device: cam a ProjCamera.  d: dict of torch device tensors -- pose_R1, pose_t1 (key frame 1, the
        older one), pose_R2, pose_t2 f64; kps1, kps2 (orbx_kp records), desc2 u8 [n2,32], matches12 i32 [n1] (as
        SearchForTriangulationDevice leaves it); fisheye_scale f32 [h,w] (Fisheye only); in / out: n_points i32 [1], the table
        points f32 [cap,3], valid u8, normals f32 [cap,3], min_dist, max_dist f32, desc u8 [cap,32], obs i32 [cap,2], the slots mp1
        i32 [n1], mp2 i32 [n2], the flags has_mp1, has_mp2 u8 (the keys SearchForTriangulationDevice reads); out: code i32 [n1]
        (optional), result i32 [8].  sigma2: host floats, at most 16.  Enqueues on `stream`; nothing is copied or synchronised."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        s2 = np.ascontiguousarray(sigma2, dtype=np.float32)
        sc = d.get("fisheye_scale")
        _lib.check(self._L.orbm_triangulate_matches_device(
            self._hd._h, C.byref(cam), sc.data_ptr() if sc is not None else None, sc.shape[1] if sc is not None else 0,
            sc.shape[0] if sc is not None else 0, p("pose_R1"), p("pose_t1"), p("pose_R2"), p("pose_t2"), p("kps1"), n1, p("kps2"), p("desc2"),
            n2, p("matches12"), _vp(s2), len(s2), max_scale_factor, cos_parallax, chi2, ratio_factor, p("n_points"), cap_points, p("points"),
            p("valid"), p("normals"), p("min_dist"), p("max_dist"), p("desc"), p("obs"), p("mp1"), p("mp2"), p("has_mp1"), p("has_mp2"),
            p("code") if d.get("code") is not None else None, p("result"), _lib.stream_arg(stream)))

    def TriangulateMatches(self, cam, t, kps1, kps2, desc2, matches12, pose1, pose2, sigma2, max_scale_factor, ratio_factor,
                           cos_parallax=0.99998, chi2=5.991, fisheye_scale=None):
        """orbm_triangulate_matches on numpy arrays.  t: the table and the key frames' state, a dict of C-contiguous numpy arrays
        changed IN PLACE -- n_points i32 [1], points, valid, normals, min_dist, max_dist, desc, obs, mp1, mp2, has_mp1, has_mp2 (types
        as for TriangulateMatchesDevice).  pose1 / pose2 = (R, t).  Returns (code i32 [n1], result i32 [8])."""
        k1 = np.ascontiguousarray(kps1, dtype=KP_DTYPE)
        k2 = np.ascontiguousarray(kps2, dtype=KP_DTYPE)
        d2 = np.ascontiguousarray(desc2, dtype=np.uint8)
        m12 = np.ascontiguousarray(matches12, dtype=np.int32)
        pose = [np.ascontiguousarray(a, dtype=np.float64) for a in (pose1[0], pose1[1], pose2[0], pose2[1])]
        s2 = np.ascontiguousarray(sigma2, dtype=np.float32)
        sc = None if fisheye_scale is None else np.ascontiguousarray(fisheye_scale, dtype=np.float32)
        types = dict(n_points=np.int32, points=np.float32, valid=np.uint8, normals=np.float32, min_dist=np.float32, max_dist=np.float32,
                     desc=np.uint8, obs=np.int32, mp1=np.int32, mp2=np.int32, has_mp1=np.uint8, has_mp2=np.uint8)
        for k, dt in types.items():
            assert t[k].dtype == dt and t[k].flags["C_CONTIGUOUS"], k
        code, result = np.zeros(len(k1), np.int32), np.zeros(8, np.int32)
        _lib.check(self._L.orbm_triangulate_matches(
            self._hd._h, C.byref(cam), None if sc is None else _vp(sc), 0 if sc is None else sc.shape[1], 0 if sc is None else sc.shape[0],
            _vp(pose[0]), _vp(pose[1]), _vp(pose[2]), _vp(pose[3]), _vp(k1), len(k1), _vp(k2), _vp(d2), len(k2), _vp(m12), _vp(s2), len(s2),
            max_scale_factor, cos_parallax, chi2, ratio_factor, _vp(t["n_points"]), len(t["valid"]), _vp(t["points"]), _vp(t["valid"]),
            _vp(t["normals"]), _vp(t["min_dist"]), _vp(t["max_dist"]), _vp(t["desc"]), _vp(t["obs"]), _vp(t["mp1"]), _vp(t["mp2"]),
            _vp(t["has_mp1"]), _vp(t["has_mp2"]), _vp(code), _vp(result)))
        return code, result

    # -- mp->computeDescriptor(); mp->update(); updateConnections' counts; computeSceneMedianDepth, on the device table ----------
    def RefreshPointsDevice(self, kf, d, n_sel, cap_points, n_obs, max_scale_factor, kf_self=-1, stream=None):
        """orbm_refresh_points_device: kf a KfTable.  d: dict of torch device tensors -- sel i32 [n_sel] (table rows; -1 = none), the
        table points f32 [cap,3], valid u8 in, normals f32 [cap,3], min_dist, max_dist f32, desc u8 [cap,32] in / out (the keys of
        TriangulateMatchesDevice and the builders); obs_off i32 [cap + 1], obs_kf, obs_kp i32 [n_obs] (CSR: its order is the order),
        ref_kf i32 [cap]; out: covis i32 [n_kf] (optional: updateConnections' counts, kf_self left out), result i32 [8].
        Enqueues on `stream`; nothing is copied or synchronised.  There is no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_refresh_points_device(
            self._hd._h, C.byref(kf), p("sel"), n_sel, p("points"), p("valid"), cap_points, p("normals"), p("min_dist"), p("max_dist"),
            p("desc"), p("obs_off"), p("obs_kf"), p("obs_kp"), n_obs, p("ref_kf"), max_scale_factor, kf_self,
            p("covis") if d.get("covis") is not None else None, p("result"), _lib.stream_arg(stream)))

    def SceneMedianDepthDevice(self, d, n_kf, stride, cap_points, cur=-1, stream=None):
        """orbm_scene_median_depth_device: d = dict(pose_R f64 [n_kf,9], pose_t f64 [n_kf,3], slots i32 [n_kf,stride] (map-point rows,
        -1 = none), n i32 [n_kf], points f32 [cap,3]; out: median f32 [n_kf], count i32 [n_kf] and, optionally with cur >= 0, baseline
        f32 [n_kf] = |O_cur - O_k|).  stride <= 8192.  Enqueues on `stream`; nothing is copied or synchronised."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_scene_median_depth_device(
            self._hd._h, n_kf, p("pose_R"), p("pose_t"), p("slots"), p("n"), stride, p("points"), cap_points, cur, p("median"), p("count"),
            p("baseline") if d.get("baseline") is not None else None, _lib.stream_arg(stream)))

    # -- the observation lists behind the refresh, and KeyFrameCulling with its cascade (LocalMapping.cpp:318-372) --------------
    def BuildObservationsDevice(self, d, n_kf, stride, cap_points, cap_obs, stream=None):
        """orbm_build_observations_device: d = dict of torch device tensors -- n i32 [n_kf] (slots per key frame), bad u8 [n_kf], slots
        i32 [n_kf,stride] (map-point rows, -1 = none), valid u8 [cap]; out: obs_off i32 [cap + 1], obs_kf, obs_kp i32 [cap_obs] (the
        refresh's CSR, every list in ascending (key frame, slot)), result i32 [8] ([0] n_obs, [1] overflow: all offsets zero).
        Enqueues on `stream`; nothing is copied or synchronised.  There is no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_build_observations_device(
            self._hd._h, n_kf, p("n"), p("bad"), p("slots"), stride, p("valid"), cap_points, cap_obs, p("obs_off"), p("obs_kf"),
            p("obs_kp"), p("result"), _lib.stream_arg(stream)))

    def CullKeyFramesDevice(self, kf, d, stride, cap_points, n_obs, recent, timestamps, first_kf=-1, th_obs=3, redundant_ratio=0.9,
                            max_gap=1.5, stream=None):
        """orbm_cull_keyframes_device: kf a KfTable (its d_kps and d_n are read).  d: dict of torch device tensors -- in / out: bad u8
        [n_kf] (may be the table's), slots i32 [n_kf,stride], valid u8 [cap], ref_kf i32 [cap]; in: obs_off, obs_kf, obs_kp (the CSR
        BuildObservationsDevice left from these slots); out: code, num_mp, num_redundant i32 [n_recent], result i32 [8].  recent /
        timestamps: host sequences, the key-frame slots of Map::getRecentKeyFrames(25) and their timestamps (at most 32).
        Enqueues on `stream`; nothing is copied or synchronised.  There is no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        rec = np.ascontiguousarray(recent, dtype=np.int32)
        ts = np.ascontiguousarray(timestamps, dtype=np.float64)
        assert rec.ndim == 1 and rec.shape == ts.shape
        _lib.check(self._L.orbm_cull_keyframes_device(
            self._hd._h, C.byref(kf), p("bad"), p("slots"), stride, p("valid"), cap_points, p("obs_off"), p("obs_kf"), p("obs_kp"), n_obs,
            p("ref_kf"), _vp(rec), _vp(ts), len(rec), first_kf, th_obs, redundant_ratio, max_gap, p("code"), p("num_mp"),
            p("num_redundant"), p("result"), _lib.stream_arg(stream)))

    # -- what the fuse does with its hits: addObservation / replace on the slot arrays (ORBMatcher.cpp:574-589) ------------------
    def FuseApplyDevice(self, d, nq, n_kf, kf_target, stride, cap_points, n_obs, stream=None):
        """orbm_fuse_apply_device: d = dict of torch device tensors -- in: best_idx i32 [nq] (as SearchFuseDevice leaves it), rows i32
        [nq] (optional: the table row of every entry; entry j is row j without it), n i32 [n_kf], bad u8 [n_kf], obs_off, obs_kf, obs_kp
        (the CSR BuildObservationsDevice left from these slots), visible i32 [cap] (optional, with found); in / out: slots i32
        [n_kf,stride], valid u8 [cap], found i32 [cap] (optional); work i32 [nq] (the call's work array); out: code, refresh_sel i32
        [nq] (refresh_sel is RefreshPointsDevice's sel behind a rebuilt CSR), result i32 [8] ([0] matches, [1] refusal: nothing
        written).  Enqueues on `stream`; nothing is copied or synchronised.  There is no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        opt = lambda k: d[k].data_ptr() if d.get(k) is not None else None  # noqa: E731
        _lib.check(self._L.orbm_fuse_apply_device(
            self._hd._h, p("best_idx"), opt("rows"), nq, n_kf, kf_target, p("n"), p("bad"), p("slots"), stride, p("valid"), cap_points,
            p("obs_off"), p("obs_kf"), p("obs_kp"), n_obs, opt("found"), opt("visible"), p("work"), p("code"), p("refresh_sel"),
            p("result"), _lib.stream_arg(stream)))

    # -- the covisibility graph and the spanning tree on the device (KeyFrame.cpp:225-362, :402-467; LocalMapping.cpp:263-300) ----
    def UpdateConnectionsDevice(self, graph, d, n_kf, kf_self, first_kf=-1, connect_th=CovisGraph.CONNECT_TH, stream=None):
        """orbm_update_connections_device: graph a CovisGraph (in / out).  d = dict of torch device tensors -- in: bad u8 [n_kf], covis
        i32 [n_kf] (as RefreshPointsDevice leaves it for the same kf_self); work i32 [n_kf] (the call's work array); out: result i32 [8]
        ([0] connections of kf_self, [1] nothing to do, [2] fallback, [3] neighbour lists rebuilt, [4] parent assigned).  Enqueues on
        `stream`; nothing is copied or synchronised.  There is no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_update_connections_device(
            self._hd._h, C.byref(graph), n_kf, p("bad"), p("covis"), kf_self, first_kf, connect_th, p("work"), p("result"),
            _lib.stream_arg(stream)))

    def EraseConnectionsDevice(self, graph, d, n_kf, recent, stream=None):
        """orbm_erase_connections_device: the graph part of KeyFrame::setBad behind CullKeyFramesDevice.  recent: the host sequence the
        culling took (at most 32).  d = dict of torch device tensors -- in: code i32 [n_recent] (the culling's; optional: without it
        every entry of recent is erased); work i32 [n_kf]; out: result i32 [8] ([0] erased, [1] connections erased, [2] children moved,
        [3] without a parent, [4] lists rebuilt).  Enqueues on `stream`; nothing is copied or synchronised."""
        rec = np.ascontiguousarray(recent, dtype=np.int32)
        assert rec.ndim == 1
        code = d.get("code")
        _lib.check(self._L.orbm_erase_connections_device(
            self._hd._h, C.byref(graph), n_kf, _vp(rec), len(rec), code.data_ptr() if code is not None else None, d["work"].data_ptr(),
            d["result"].data_ptr(), _lib.stream_arg(stream)))

    def FuseTargetsDevice(self, graph, d, n_kf, stride, cap_points, cur, cap_targets, cap_rows, n_first=20, n_second=5, stream=None):
        """orbm_fuse_targets_device (LocalMapping.cpp:263-300): d = dict of torch device tensors -- in: n i32 [n_kf], bad u8 [n_kf], slots
        i32 [n_kf,stride], valid u8 [cap]; work i32 [cap] (the call's work array); out: targets i32 [cap_targets], rows i32 [cap_rows]
        (FuseApplyDevice's rows for the direction into `cur`), result i32 [8] ([0] targets, [1] rows, full counts; [2] refusal mask).
        Enqueues on `stream`; nothing is copied or synchronised."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_fuse_targets_device(
            self._hd._h, C.byref(graph), n_kf, p("n"), p("bad"), p("slots"), stride, p("valid"), cap_points, cur, n_first, n_second,
            cap_targets, cap_rows, p("work"), p("targets"), p("rows"), p("result"), _lib.stream_arg(stream)))

    def ConnectedKeyFramesDevice(self, graph, d, n_kf, kf, include_self=True, max_n=None, stream=None):
        """orbm_connected_keyframes_device: d = dict(out i32 [n_out], n_out i32 [1]), torch device tensors.  out = [kf if include_self] +
        the first max_n (default: all) entries of kf's list, then -1: with include_self it is LocalBaProblemDevice's `local` with
        n_local = len(out).  Enqueues on `stream`; nothing is copied or synchronised."""
        _lib.check(self._L.orbm_connected_keyframes_device(
            self._hd._h, C.byref(graph), n_kf, kf, int(bool(include_self)), n_kf if max_n is None else max_n, d["out"].data_ptr(),
            int(d["out"].shape[0]), d["n_out"].data_ptr(), _lib.stream_arg(stream)))

    # -- the tracker's local map, its counters and the reference key frame's tracked points (Tracking.cpp:345-537, KeyFrame.cpp:146-152) --
    def LocalMapDevice(self, graph, d, n2, n_kf, stride, cap_points, n_obs, recent, cap_local_kf, cap_rows, n_neigh=10, max_kf=80, stream=None):
        """orbm_local_map_device (Tracking.cpp:429-537): graph a CovisGraph (read).  recent: the host sequence of key-frame slots of
        Map::getRecentKeyFrames(10), oldest first (at most 32).  d = dict of torch device tensors -- in / out: frame_mp i32 [n2] (slots
        naming a bad row become -1), ref i32 [1] (the reference key frame: written when a key frame got a vote); in: valid u8 [cap],
        obs_off, obs_kf, obs_kp (the CSR BuildObservationsDevice left), n i32 [n_kf], bad u8 [n_kf], slots i32 [n_kf,stride]; work i32
        [cap + n_kf] (the call's work array); out: local_kf i32 [cap_local_kf], rows i32 [cap_rows], local_mask u8 [cap]
        (ProjectFrustumDevice's `valid` with nq = cap), result i32 [16] ([0] key frames, [1] rows, full counts; [2] refusal mask).
        Enqueues on `stream`; nothing is copied or synchronised.  There is no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        rec = np.ascontiguousarray(recent, dtype=np.int32)
        assert rec.ndim == 1
        _lib.check(self._L.orbm_local_map_device(
            self._hd._h, p("frame_mp"), n2, p("valid"), cap_points, p("obs_off"), p("obs_kf"), p("obs_kp"), n_obs, n_kf, p("n"), p("bad"),
            p("slots"), stride, C.byref(graph), _vp(rec), len(rec), n_neigh, max_kf, cap_local_kf, cap_rows, p("work"), p("local_kf"), p("rows"),
            p("local_mask"), p("ref"), p("result"), _lib.stream_arg(stream)))

    def TrackCountersDevice(self, d, n2, cap_points, nq, what, stream=None):
        """orbm_track_counters_device: what = 1 (Tracking.cpp:388-398: frame slots naming a bad row become -1, the others' rows are
        visible) | 2 (:406-408: every query the frustum builder left on is visible) | 4 (:362-364: the frame's rows are found).  d =
        dict of torch device tensors -- in / out: frame_mp i32 [n2], visible, found i32 [cap] (counters: accumulated); in: valid u8
        [cap], q_ok u8 [nq] (ProjectFrustumDevice's; optional without bit 2); out: result i32 [8] ([0] - [2] the three counts, [3] slots
        cleared).  Enqueues on `stream`; nothing is copied or synchronised."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        opt = lambda k: d[k].data_ptr() if d.get(k) is not None else None  # noqa: E731
        _lib.check(self._L.orbm_track_counters_device(
            self._hd._h, p("frame_mp"), n2, p("valid"), cap_points, opt("q_ok"), nq, what, opt("visible"), opt("found"), p("result"),
            _lib.stream_arg(stream)))

    def NumTrackedPointsDevice(self, d, n_kf, stride, cap_points, n_obs, min_obs, stream=None):
        """orbm_num_tracked_points_device (KeyFrame.cpp:146-152): d = dict of torch device tensors -- in: ref i32 [1] (the key frame, as
        LocalMapDevice leaves it: no read-back in between), n i32 [n_kf], bad u8 [n_kf], slots i32 [n_kf,stride], obs_off, obs_kf, obs_kp;
        out: count i32 [4] ([0] the slots whose row has at least min_obs live observations, [1] ref is not a key frame).  Enqueues on
        `stream`; nothing is copied or synchronised."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_num_tracked_points_device(
            self._hd._h, p("ref"), min_obs, n_kf, p("n"), p("bad"), p("slots"), stride, cap_points, p("obs_off"), p("obs_kf"), p("obs_kp"), n_obs,
            p("count"), _lib.stream_arg(stream)))

    # -- a tracked frame becomes a key frame; new map points are registered; MapPointCulling (LocalMapping.cpp:93-105, :117-144, :243-248) --
    def InsertKeyFrameDevice(self, d, K, stride, cap_points, n2, frame_kps, frame_desc, stream=None):
        """orbm_insert_keyframe_device (Tracking.cpp:578-588, LocalMapping.cpp:93-105): d = dict of torch device tensors -- in / out, the
        key-frame table's arrays: pose_R f64 [cap_kf,9], pose_t f64 [cap_kf,3], bad u8 [cap_kf], kps, desc i64 [cap_kf] (device addresses),
        n i32 [cap_kf], slots i32 [cap_kf,stride]; in: valid u8 [cap], frame_mp i32 [n2] (table rows, -1 = none), frame_pose_R f64 [9],
        frame_pose_t f64 [3]; out: result i32 [8] ([0] slots holding a point, [2] cleared: bad row, [3] out of range, [4] second slots of
        a row, [5] n2 beyond stride).  K: the new key frame's slot; frame_kps / frame_desc: the frame's record tensors or their device
        addresses.  Enqueues on `stream`; nothing is copied or synchronised.  There is no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        addr = lambda x: x if isinstance(x, int) else x.data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_insert_keyframe_device(
            self._hd._h, K, int(d["n"].shape[0]), p("pose_R"), p("pose_t"), p("bad"), p("kps"), p("desc"), p("n"), p("slots"), stride, p("valid"),
            cap_points, p("frame_mp"), n2, p("frame_pose_R"), p("frame_pose_t"), addr(frame_kps), addr(frame_desc), p("result"),
            _lib.stream_arg(stream)))

    def RegisterNewPointsDevice(self, d, K, kf_id, cap_points, stream=None):
        """orbm_register_new_points_device (LocalMapping.cpp:243-248, MapPoint.cpp:18, :24-25): d = dict of torch device tensors -- in:
        n_points i32 [1] (as TriangulateMatchesDevice leaves it); in / out: n_registered i32 [1] (rows below it are finished), recent i32
        [cap_recent] with n_recent i32 [1] (recent_map_points as table rows); out, for the rows n_registered .. n_points - 1: ref_kf = K,
        first_kf = kf_id, found = visible = 1 (all i32 [cap]); result i32 [8] ([0] rows registered, [1] refusal: nothing written).
        Enqueues on `stream`; nothing is copied or synchronised."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_register_new_points_device(
            self._hd._h, p("n_points"), p("n_registered"), K, kf_id, cap_points, p("ref_kf"), p("first_kf"), p("found"), p("visible"), p("recent"),
            int(d["recent"].shape[0]), p("n_recent"), p("result"), _lib.stream_arg(stream)))

    def CullMapPointsDevice(self, d, cur_kf_id, n_kf, stride, cap_points, n_obs, stream=None):
        """orbm_cull_map_points_device (LocalMapping.cpp:117-144): d = dict of torch device tensors -- in / out: recent i32 [cap_recent]
        with n_recent i32 [1] (the kept entries, compacted in order), valid u8 [cap], slots i32 [n_kf,stride]; in: first_kf, found,
        visible i32 [cap], n i32 [n_kf], bad u8 [n_kf], obs_off, obs_kf, obs_kp (the CSR BuildObservationsDevice left from these slots);
        out: code i32 [cap_recent] (0 kept, 1 already bad, 2 found ratio, 3 few observations, 4 aged out, -1 not a row), result i32 [8]
        ([0] kept, [1] refusal: a row twice in the list, nothing written).  Enqueues on `stream`; nothing is copied or synchronised."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_cull_map_points_device(
            self._hd._h, p("recent"), p("n_recent"), int(d["recent"].shape[0]), cur_kf_id, p("first_kf"), p("found"), p("visible"), p("valid"),
            cap_points, n_kf, p("n"), p("bad"), p("slots"), stride, p("obs_off"), p("obs_kf"), p("obs_kp"), n_obs, p("code"), p("result"),
            _lib.stream_arg(stream)))

    # -- Optimize::localBundleAdjustment on the slot arrays: the problem assembled, the result applied (Optimize.cpp:766-889, :914-950) --
    def LocalBaProblemDevice(self, kf, d, stride, cap_points, n_obs, n_local, first_kf, cap_poses, cap_local_points, cap_edges, stream=None):
        """orbm_local_ba_problem_device: kf a KfTable.  d: dict of torch device tensors -- in: slots i32 [n_kf,stride], valid u8 [cap],
        points f32 [cap,3], obs_off, obs_kf, obs_kp (the CSR BuildObservationsDevice left from these slots), local i32 [n_local] (the
        current key frame, then its connected ones); work i32 [cap + n_kf] (the call's work array); out, an orbba problem in device
        memory: pose_R f64 [cap_poses,9], pose_t f64 [cap_poses,3], pose_fixed u8 [cap_poses], ba_points f64 [cap_local_points,3],
        edge_pose, edge_point i32 [cap_edges], edge_z f64 [cap_edges,2], edge_inv_sigma2 f64 [cap_edges], and the maps back: edge_kf,
        edge_kp i32 [cap_edges], edge_off i32 [cap_local_points + 1], point_row i32 [cap_local_points], pose_kf i32 [cap_poses]; result
        i32 [16] ([0] n_poses, [1] n_points, [2] n_edges, [3] local key frames, [5] refusal mask).  Enqueues on `stream`; nothing is
        copied or synchronised.  There is no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_local_ba_problem_device(
            self._hd._h, C.byref(kf), p("slots"), stride, p("valid"), p("points"), cap_points, p("obs_off"), p("obs_kf"), p("obs_kp"), n_obs,
            p("local"), n_local, first_kf, cap_poses, cap_local_points, cap_edges, p("work"), p("pose_R"), p("pose_t"), p("pose_fixed"),
            p("ba_points"), p("edge_pose"), p("edge_point"), p("edge_z"), p("edge_inv_sigma2"), p("edge_kf"), p("edge_kp"), p("edge_off"),
            p("point_row"), p("pose_kf"), p("result"), _lib.stream_arg(stream)))

    def LocalBaApplyDevice(self, d, n_kf, stride, cap_points, n_obs, n_local, n_points, n_edges, stream=None):
        """orbm_local_ba_apply_device: d = dict of torch device tensors -- in: n i32 [n_kf], bad u8 [n_kf], obs_off, obs_kf, obs_kp (the
        CSR the assembly read), the assembly's maps pose_kf, point_row, edge_off, edge_kf, edge_kp, and the outputs of
        ba.local_bundle_adjustment_device est_pose_R, est_pose_t, est_points f64, outlier u8; in / out: slots i32 [n_kf,stride], valid
        u8 [cap], ref_kf i32 [cap], points f32 [cap,3], kf_pose_R f64 [n_kf,9], kf_pose_t f64 [n_kf,3] (the key-frame table's); out:
        result i32 [8].  n_local, n_points, n_edges: result[3], [1], [2] of the assembly.  Enqueues on `stream`; nothing is copied or
        synchronised.  There is no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_local_ba_apply_device(
            self._hd._h, n_kf, p("n"), p("bad"), p("slots"), stride, p("valid"), p("ref_kf"), p("points"), cap_points, p("kf_pose_R"),
            p("kf_pose_t"), p("obs_off"), p("obs_kf"), p("obs_kp"), n_obs, n_local, n_points, n_edges, p("pose_kf"), p("point_row"),
            p("edge_off"), p("edge_kf"), p("edge_kp"), p("est_pose_R"), p("est_pose_t"), p("est_points"), p("outlier"), p("result"),
            _lib.stream_arg(stream)))

    # -- Optimize::localFullBundleAdjustment on the slot arrays: the window assembled (Optimize.cpp:1073-1108, :1129-1244) --
    def InertialWindowProblemDevice(self, kf, d, stride, cap_points, n_obs, n_window, n_src, cap_bank, n_priors, max_fixed, cap_states,
                                    cap_local_points, cap_edges, stream=None):
        """orbm_inertial_window_problem_device: kf a KfTable.  d: dict of torch device tensors -- in: slots, valid, points, obs_off,
        obs_kf, obs_kp as LocalBaProblemDevice takes them, window i32 [n_window] (getRecentKeyFrames, oldest first), kf_imu i32 [n_kf,3]
        (state row, record, prior slot); work i32 [cap + 2 n_kf]; out, for the visual window: ba_points f64 [cap_local_points,3],
        point_row i32 [cap_local_points], edge_off i32 [cap_local_points + 1], edge_state, edge_point i32 [cap_edges], edge_z f64
        [cap_edges,2], edge_inv_sigma2 f64 [cap_edges], edge_kf, edge_kp i32 [cap_edges], state_kf i32 [cap_states]; for the inertial
        side: init_jobs i32 [cap_states,3], fixed u8 [cap_states], inertial_edges i32 [n_window - 1,4], prior_jobs i32 [3], recover_jobs
        i32 [n_window,3], bias_ids i32 [n_window], prior_info_jobs i32 [n_window - 1,3]; result i32 [16] ([0] n_states, [1] n_points,
        [2] n_edges, [3] n_solve, [4] n_fixed, [5] refusal mask).  Enqueues on `stream`; nothing is copied or synchronised.  There is
        no host-pointer twin (include/orbm.h)."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_inertial_window_problem_device(
            self._hd._h, C.byref(kf), p("slots"), stride, p("valid"), p("points"), cap_points, p("obs_off"), p("obs_kf"), p("obs_kp"), n_obs,
            p("window"), n_window, p("kf_imu"), n_src, cap_bank, n_priors, max_fixed, cap_states, cap_local_points, cap_edges, p("work"),
            p("ba_points"), p("point_row"), p("edge_off"), p("edge_state"), p("edge_point"), p("edge_z"), p("edge_inv_sigma2"), p("edge_kf"),
            p("edge_kp"), p("state_kf"), p("init_jobs"), p("fixed"), p("inertial_edges"), p("prior_jobs"), p("recover_jobs"), p("bias_ids"),
            p("prior_info_jobs"), p("result"), _lib.stream_arg(stream)))

    def InertialWindowVelocityPriorDevice(self, d, n_priors, n_src, stream=None):
        """orbm_inertial_window_velocity_prior_device: d = dict of torch device tensors -- in / out: priors (the orbi_prior array, 36
        floats a slot); in: src f32 [n_src,15] (the state rows the recover wrote), recover_jobs, prior_jobs (the assembly's); out: result
        i32 [8].  The oldest key frame's velo_priori takes its recovered velocity.  Enqueues on `stream`."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_inertial_window_velocity_prior_device(
            self._hd._h, p("priors"), n_priors, p("src"), n_src, p("recover_jobs"), p("prior_jobs"), p("result"), _lib.stream_arg(stream)))

    # -- Optimize::localInertialBundleAdjustment on the device-resident map: the chain assembled (Optimize.cpp:965-1029, :1044-1053) --
    def InertialChainProblemDevice(self, d, n_kf, n_window, n_src, cap_bank, n_priors, stream=None):
        """orbm_inertial_chain_problem_device: d = dict of torch device tensors -- in: bad u8 [n_kf], window i32 [n_window]
        (getRecentKeyFrames, oldest first), kf_imu i32 [n_kf,3] (state row, record, prior slot); out: init_jobs i32 [n_window,3], fixed
        u8 [n_window], inertial_edges i32 [n_window - 1,4], recover_jobs i32 [n_window,3], bias_ids i32 [n_window], velo_jobs i32
        [n_window,2], state_kf i32 [n_window], result i32 [8] ([0] n_window, [1] refusal mask).  A refused call writes -1 into every
        list and 15 into fixed.  Enqueues on `stream`; nothing is copied or synchronised, and the chain behind it needs no read-back."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_inertial_chain_problem_device(
            self._hd._h, n_kf, p("bad"), p("window"), n_window, p("kf_imu"), n_src, cap_bank, n_priors, p("init_jobs"), p("fixed"),
            p("inertial_edges"), p("recover_jobs"), p("bias_ids"), p("velo_jobs"), p("state_kf"), p("result"), _lib.stream_arg(stream)))

    def InertialChainVelocityPriorsDevice(self, d, n_priors, n_src, n, stream=None):
        """orbm_inertial_chain_velocity_priors_device: d = dict of torch device tensors -- in / out: priors (the orbi_prior array, 36
        floats a slot); in: src f32 [n_src,15] (the state rows the recover wrote), velo_jobs i32 [n,2] (the assembly's); out: result i32
        [8].  velo_priori of every window key frame takes its recovered velocity.  Enqueues on `stream`."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_inertial_chain_velocity_priors_device(
            self._hd._h, p("priors"), n_priors, p("src"), n_src, p("velo_jobs"), n, p("result"), _lib.stream_arg(stream)))

    # -- Map::applyScaleRotation on the device-resident map (Map.cpp:96-124) --
    def ApplyScaleRotationDevice(self, calib, d, n_kf, n_src, n_priors, cap_points, be_first, min_scale=0.1, stream=None):
        """orbm_apply_scale_rotation_device: calib an imu.Calib.  d: dict of torch device tensors -- in / out: pose_R f64 [n_kf,9], pose_t
        f64 [n_kf,3], state f32 [n_src,15], priors (the orbi_prior array), points f32 [cap_points,3]; in: bad u8 [n_kf], kf_imu i32 [n_kf,3]
        (state row, record, prior slot), valid u8 [cap_points], n_points i32 [1], summary f32 [10] (Rwg, scale: imu_init.recover_device's);
        out: result i32 [8] ([0] key frames, [1] out of range, [2] duplicates, [3] refused, [4] points).  With be_first and a scale below
        min_scale nothing but result is written.  Enqueues on `stream`; nothing is copied or synchronised."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_apply_scale_rotation_device(
            self._hd._h, C.addressof(calib), n_kf, p("pose_R"), p("pose_t"), p("bad"), p("kf_imu"), p("state"), n_src, p("priors"), n_priors,
            p("points"), p("valid"), p("n_points"), cap_points, p("summary"), int(bool(be_first)), float(np.float32(min_scale)), p("result"),
            _lib.stream_arg(stream)))

    def SearchForInitializationDevice(self, d, n1, n2, grid_cols, grid_rows, window=100, list_cap=768, stream=None):
        """orbm_search_for_initialization_device on torch device tensors: d = dict(kps1, desc1, kps2 (frame 2's record as
        orbf_frame_post_device leaves it), desc2, cell_start, cell_items, pre (float32 [n1, 2], in / out), matches12 (int32 [n1], out),
        result (int32 x 8, out)).  result[0] is the match count and result[2] the sweeps of the fixed point.  result[1] = 1: the window
        lists overflowed the pool of n1 * list_cap entries; result[1] = 2: the fixed point had not settled within the sweep cap
        (set_variant("init_max_sweeps"), default 64).  In both cases nothing was written -- matches12 is all -1, pre is untouched,
        result[0] is 0 -- and the caller runs the host entry point, SearchForInitialization, instead."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_search_for_initialization_device(
            self._hd._h, self.nn_ratio, int(self.be_check_orientation), p("kps1"), p("desc1"), n1, p("kps2"), p("desc2"),
            p("cell_start"), p("cell_items"), grid_cols, grid_rows, n2, p("pre"), window, list_cap, p("matches12"), p("result"),
            _lib.stream_arg(stream)))

    # -- the H / F RANSAC of TwoViewReconstruction::Reconstruct (TwoViewReconstruction.cpp:14-344) ----------------
    def TwoViewRansacDevice(self, d, n1, n2, sigma=1.0, iters=200, rng_state=0, stream=None):
        """orbm_two_view_ransac_device on torch device tensors: d = dict(kps1, kps2 (orbx_kp records, undistorted), matches12 i32 [n1] (as
        SearchForInitializationDevice leaves it); sets i32 [iters, 8] (optional: the caller's draw); out: pairs i32 [n1, 2], H, F f32 [9],
        inl_H, inl_F u8 [n1], score f32 [2], rh f32 [1], hyp f32 [2, iters, 9] and hyp_score f32 [2, iters] (both optional), result i32
        [8]).  Enqueues on `stream`; nothing is copied or synchronised.  result[1] = 1 (fewer than 8 matches): only result was written."""
        p = lambda k: d[k].data_ptr() if d.get(k) is not None else None  # noqa: E731
        _lib.check(self._L.orbm_two_view_ransac_device(
            self._hd._h, p("kps1"), n1, p("kps2"), n2, p("matches12"), sigma, iters, rng_state, p("sets"), p("pairs"), p("H"), p("F"),
            p("inl_H"), p("inl_F"), p("score"), p("rh"), p("hyp"), p("hyp_score"), p("result"), _lib.stream_arg(stream)))

    def TwoViewRansac(self, kps1, kps2, matches12, sigma=1.0, iters=200, rng_state=0, sets=None, out=None, all_hypotheses=True):
        """orbm_two_view_ransac on numpy arrays.  Returns a dict of the outputs (names as for TwoViewRansacDevice; hyp and hyp_score with
        all_hypotheses); `out`, a dict of C-contiguous arrays of those names and types, is written in place instead."""
        k1 = np.ascontiguousarray(kps1, dtype=KP_DTYPE)
        k2 = np.ascontiguousarray(kps2, dtype=KP_DTYPE)
        m12 = np.ascontiguousarray(matches12, dtype=np.int32)
        st = None if sets is None else np.ascontiguousarray(sets, dtype=np.int32)
        n1, it = len(k1), max(int(iters), 0)
        types = dict(pairs=(np.int32, (n1, 2)), H=(np.float32, (9,)), F=(np.float32, (9,)), inl_H=(np.uint8, (n1,)), inl_F=(np.uint8, (n1,)),
                     score=(np.float32, (2,)), rh=(np.float32, (1,)), hyp=(np.float32, (2, it, 9)), hyp_score=(np.float32, (2, it)),
                     result=(np.int32, (8,)))
        if out is None:
            out = {k: np.zeros(shape, dt) for k, (dt, shape) in types.items() if all_hypotheses or not k.startswith("hyp")}
        for k, a in out.items():
            assert a.dtype == types[k][0] and a.flags["C_CONTIGUOUS"], k
        assert st is None or st.shape == (it, 8)
        q = lambda k: _vp(out[k]) if out.get(k) is not None else None  # noqa: E731
        _lib.check(self._L.orbm_two_view_ransac(
            self._hd._h, _vp(k1), n1, _vp(k2), len(k2), _vp(m12), sigma, iters, rng_state, None if st is None else _vp(st), q("pairs"), q("H"),
            q("F"), q("inl_H"), q("inl_F"), q("score"), q("rh"), q("hyp"), q("hyp_score"), q("result")))
        return out

    # -- ReconstructH / ReconstructF behind the RANSAC (TwoViewReconstruction.cpp:79-83, :346-556, :598-724) ------
    def TwoViewPoseDevice(self, d, n1, n2, K, family=-1, sigma=1.0, min_parallax=1.0, stream=None):
        """orbm_two_view_pose_device on torch device tensors: d = dict(kps1, kps2, matches12 and, as TwoViewRansacDevice left them, pairs, H,
        F, inl_H, inl_F, ransac_result i32 [8]; out: R21 f32 [9], t21 f32 [3], points3D f32 [n1, 3], triangulated u8 [n1], matches12_out
        i32 [n1], hyp_R f32 [8, 9], hyp_t f32 [8, 3], hyp_good i32 [8], hyp_parallax f32 [8], hyp_code u8 [8, n1] (optional), result i32
        [16]).  K = (fx, fy, cx, cy).  family -1: the RANSAC's choice, read on the device; 0 F, 1 H.  Enqueues on `stream`; nothing is
        copied or synchronised.  result[0] = 1 (the RANSAC refused): only result was written."""
        p = lambda k: d[k].data_ptr() if d.get(k) is not None else None  # noqa: E731
        fx, fy, cx, cy = K
        _lib.check(self._L.orbm_two_view_pose_device(
            self._hd._h, fx, fy, cx, cy, p("kps1"), n1, p("kps2"), n2, p("matches12"), p("pairs"), p("H"), p("F"), p("inl_H"), p("inl_F"),
            p("ransac_result"), family, sigma, min_parallax, p("R21"), p("t21"), p("points3D"), p("triangulated"), p("matches12_out"),
            p("hyp_R"), p("hyp_t"), p("hyp_good"), p("hyp_parallax"), p("hyp_code"), p("result"), _lib.stream_arg(stream)))

    def TwoViewPose(self, kps1, kps2, matches12, ransac, K, family=-1, sigma=1.0, min_parallax=1.0, out=None, codes=True):
        """orbm_two_view_pose on numpy arrays; `ransac` is what TwoViewRansac returned (pairs, H, F, inl_H, inl_F, result).  Returns a dict
        of the outputs (names as for TwoViewPoseDevice; hyp_code with `codes`); `out`, a dict of C-contiguous arrays of those names and
        types, is written in place instead."""
        k1 = np.ascontiguousarray(kps1, dtype=KP_DTYPE)
        k2 = np.ascontiguousarray(kps2, dtype=KP_DTYPE)
        m12 = np.ascontiguousarray(matches12, dtype=np.int32)
        n1 = len(k1)
        ins = dict(pairs=(np.int32, (n1, 2)), H=(np.float32, (9,)), F=(np.float32, (9,)), inl_H=(np.uint8, (n1,)), inl_F=(np.uint8, (n1,)),
                   result=(np.int32, (8,)))
        r = {k: np.ascontiguousarray(ransac[k], dtype=dt) for k, (dt, _) in ins.items()}
        for k, (_, shape) in ins.items():
            assert r[k].shape == shape, k
        types = dict(R21=(np.float32, (9,)), t21=(np.float32, (3,)), points3D=(np.float32, (n1, 3)), triangulated=(np.uint8, (n1,)),
                     matches12_out=(np.int32, (n1,)), hyp_R=(np.float32, (8, 9)), hyp_t=(np.float32, (8, 3)), hyp_good=(np.int32, (8,)),
                     hyp_parallax=(np.float32, (8,)), hyp_code=(np.uint8, (8, n1)), result=(np.int32, (16,)))
        if out is None:
            out = {k: np.zeros(shape, dt) for k, (dt, shape) in types.items() if codes or k != "hyp_code"}
        for k, a in out.items():
            assert a.dtype == types[k][0] and a.flags["C_CONTIGUOUS"], k
        q = lambda k: _vp(out[k]) if out.get(k) is not None else None  # noqa: E731
        fx, fy, cx, cy = K
        _lib.check(self._L.orbm_two_view_pose(
            self._hd._h, fx, fy, cx, cy, _vp(k1), n1, _vp(k2), len(k2), _vp(m12), _vp(r["pairs"]), _vp(r["H"]), _vp(r["F"]), _vp(r["inl_H"]),
            _vp(r["inl_F"]), _vp(r["result"]), family, sigma, min_parallax, q("R21"), q("t21"), q("points3D"), q("triangulated"),
            q("matches12_out"), q("hyp_R"), q("hyp_t"), q("hyp_good"), q("hyp_parallax"), q("hyp_code"), q("result")))
        return out

    # -- static SearchByProjection(keyFrame, mapPoints, Map*, th): the fuse (ORBMatcher.cpp:524-592) ------------
    def SearchFuseDevice(self, d, nq, grid_cols, grid_rows, list_cap=48, stream=None):
        """orbm_search_fuse_device on torch device tensors: d = dict(q_desc, q_xy, q_radius, q_level, q_ok, kps, desc, cell_start,
        cell_items, sigma2, best_idx (int32 [nq], out), best_dist (int32 [nq], out), result (int32 x 8, out))."""
        p = lambda k: d[k].data_ptr()  # noqa: E731
        _lib.check(self._L.orbm_search_fuse_device(
            self._hd._h, p("q_desc"), p("q_xy"), p("q_radius"), p("q_level"), p("q_ok"), nq, p("kps"), p("desc"), p("cell_start"),
            p("cell_items"), grid_cols, grid_rows, p("sigma2"), list_cap, p("best_idx"), p("best_dist"), p("result"), _lib.stream_arg(stream)))

    def SearchByBowDevice(self, d, n1, n2, stream=None):
        """orbm_search_by_bow_device on torch device tensors: d = dict(desc1, kps1 (orbx_kp records), kf_mp_ok, fv1=(nodes, off, idx, n), desc2, kps2,
        frame_mp (in / out), fv2=(nodes, off, idx, n), result (int32 x 8))."""
        p = lambda t: t.data_ptr()  # noqa: E731
        _lib.check(self._hd._L.orbm_search_by_bow_device(
            self._hd._h, self.nn_ratio, int(self.be_check_orientation), p(d["desc1"]), p(d["kps1"]), p(d["kf_mp_ok"]), n1,
            p(d["fv1"][0]), p(d["fv1"][1]), p(d["fv1"][2]), p(d["fv1"][3]), p(d["desc2"]), p(d["kps2"]), p(d["frame_mp"]), n2,
            p(d["fv2"][0]), p(d["fv2"][1]), p(d["fv2"][2]), p(d["fv2"][3]), p(d["result"]), _lib.stream_arg(stream)))

    def SearchForTriangulationDevice(self, d, n1, n2, stream=None):
        """orbm_search_for_triangulation_device: d = dict(desc1, kps1, has_mp1, fv1, desc2, kps2, has_mp2, fv2, matches12, result)."""
        p = lambda t: t.data_ptr()  # noqa: E731
        _lib.check(self._hd._L.orbm_search_for_triangulation_device(
            self._hd._h, int(self.be_check_orientation), p(d["desc1"]), p(d["kps1"]), p(d["has_mp1"]), n1, p(d["fv1"][0]), p(d["fv1"][1]),
            p(d["fv1"][2]), p(d["fv1"][3]), p(d["desc2"]), p(d["kps2"]), p(d["has_mp2"]), n2, p(d["fv2"][0]), p(d["fv2"][1]),
            p(d["fv2"][2]), p(d["fv2"][3]), p(d["matches12"]), p(d["result"]), _lib.stream_arg(stream)))

    def SearchFuse(self, q_desc, q_xy, q_radius, q_level, q_ok, kps, desc, img_w, img_h, sigma2):
        """Per-point core of the fuse: (best_idx, best_dist, n_found); the observation rewiring stays with the caller."""
        qd = np.ascontiguousarray(q_desc, dtype=np.uint8)
        qx = np.ascontiguousarray(q_xy, dtype=np.float32)
        qr = np.ascontiguousarray(q_radius, dtype=np.float32)
        ql = np.ascontiguousarray(q_level, dtype=np.int32)
        qk = np.ascontiguousarray(q_ok, dtype=np.uint8)
        k = np.ascontiguousarray(kps, dtype=KP_DTYPE)
        d = np.ascontiguousarray(desc, dtype=np.uint8)
        s2 = np.ascontiguousarray(sigma2, dtype=np.float32)
        bi = np.full(len(qd), -1, np.int32)
        bd = np.zeros(len(qd), np.int32)
        n = C.c_int()
        _lib.check(self._L.orbm_search_fuse(self._hd._h, _vp(qd), _vp(qx), _vp(qr), _vp(ql), _vp(qk), len(qd), _vp(k),
                                            _vp(d), len(k), img_w, img_h, _vp(s2), len(s2), _vp(bi), _vp(bd), C.byref(n)))
        return bi, bd, n.value


TWO_VIEW_RNG_DEFAULT = 0xFFFFFFFF   # ORBM_TWO_VIEW_RNG_DEFAULT: cv::RNG's default state


def two_view_sets(n_matches, iters=200, rng_state=0):
    """orbm_two_view_sets: the eight-point sets of TwoViewReconstruction.cpp:42-58, int32 [iters, 8]; a host function, no GPU needed"""
    sets = np.zeros((max(int(iters), 0), 8), np.int32)
    _lib.check(_mlib().orbm_two_view_sets(n_matches, iters, rng_state, _vp(sets)))
    return sets


def two_view_decide(family, n_good, parallax, n_inlier, min_parallax=1.0):
    """orbm_two_view_decide: the decision of ReconstructF (family 0, four hypotheses) or ReconstructH (family 1, eight) from the
    per-hypothesis nGood and parallax; returns (winner or -1, minGood, reason: 0 accepted, 3 no clear winner or too few good, 4 parallax
    too low); a host function, the code the device runs, no GPU needed"""
    g = np.ascontiguousarray(n_good, dtype=np.int32)
    p = np.ascontiguousarray(parallax, dtype=np.float32)
    assert family not in (0, 1) or (len(g) >= (8 if family else 4) and len(p) >= (8 if family else 4))
    w, mg, why = C.c_int32(-1), C.c_int32(0), C.c_int32(0)
    _lib.check(_mlib().orbm_two_view_decide(family, _vp(g), _vp(p), n_inlier, min_parallax, C.byref(w), C.byref(mg), C.byref(why)))
    return w.value, mg.value, why.value


def local_ba_problem_device(matcher, *args, **kwargs):
    """ORBMatcher.LocalBaProblemDevice (orbm_local_ba_problem_device) under the name include/orbm.h's section uses"""
    return matcher.LocalBaProblemDevice(*args, **kwargs)


def local_ba_apply_device(matcher, *args, **kwargs):
    """ORBMatcher.LocalBaApplyDevice (orbm_local_ba_apply_device)"""
    return matcher.LocalBaApplyDevice(*args, **kwargs)


IW_MAX_SOLVE, IW_MAX_FIXED_DEFAULT = 32, 150   # ORBM_IW_MAX_SOLVE, ORBM_IW_MAX_FIXED_DEFAULT


def inertial_window_problem_device(matcher, *args, **kwargs):
    """ORBMatcher.InertialWindowProblemDevice (orbm_inertial_window_problem_device)"""
    return matcher.InertialWindowProblemDevice(*args, **kwargs)


def inertial_window_velocity_prior_device(matcher, *args, **kwargs):
    """ORBMatcher.InertialWindowVelocityPriorDevice (orbm_inertial_window_velocity_prior_device)"""
    return matcher.InertialWindowVelocityPriorDevice(*args, **kwargs)


def inertial_chain_problem_device(matcher, *args, **kwargs):
    """ORBMatcher.InertialChainProblemDevice (orbm_inertial_chain_problem_device)"""
    return matcher.InertialChainProblemDevice(*args, **kwargs)


def inertial_chain_velocity_priors_device(matcher, *args, **kwargs):
    """ORBMatcher.InertialChainVelocityPriorsDevice (orbm_inertial_chain_velocity_priors_device)"""
    return matcher.InertialChainVelocityPriorsDevice(*args, **kwargs)


def apply_scale_rotation_device(matcher, *args, **kwargs):
    """ORBMatcher.ApplyScaleRotationDevice (orbm_apply_scale_rotation_device)"""
    return matcher.ApplyScaleRotationDevice(*args, **kwargs)
