"""Kernel resources of the visual window of the inertial local bundle adjustment (csrc/orbvw.hip), read from the gfx950 ISA that hipcc
emits for the shipped source (no GPU needed), by the method of tests/test_vi_resources.py: what include/orbvw.h states."""
import os
import re

from test_kernel_resources import _isa, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monoorbslam3_amd", "csrc")
# kernel -> (threads per workgroup, static LDS bytes as include/orbvw.h states them)
STATED = {"k_vw_off_init": (256, 0), "k_vw_off_first": (256, 0), "k_vw_off_scan": (1024, 4096), "k_vw_edge": (256, 32), "k_vw_point": (256, 0),
          "k_vw_state": (1024, 3456), "k_vw_point_inv": (256, 0), "k_vw_base": (256, 64), "k_vw_schur": (256, 1344), "k_vw_solve": (512, 63368),
          "k_vw_backsub": (256, 0), "k_vw_scale": (1024, 160)}


# what csrc/orbi_graph_device.h defines once for orbi_factors.hip, orbvi.hip and orbvw.hip
SHARED_DEVICE = ("dsum3", "dof_fixed", "edge_valid", "pose_rcw", "pose_tcw", "pose_tbc", "pose_jacobian", "huber", "quad_accumulate", "quad_scatter")
SHARED_HOST = ("graph_camera", "graph_check_linearize")
# the constant a kernel's __launch_bounds__ names, where it is not a literal
BOUND = {"k_vw_state": "ST_T", "k_vw_schur": "SC_T", "k_vw_solve": "SW_T", "k_vw_scale": "BS_T"}


def test_the_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Twelve kernels, the ones the header names.  No scratch memory; VGPRs within what a workgroup of that size can have (512 per lane
    and SIMD, a wave per 64 threads, four SIMDs: 128 for 1024 threads, 256 for 512, 512 for 256); static LDS as stated: k_vw_off_scan a
    minimum per thread, k_vw_edge and k_vw_base eight counters (and four wave maxima), k_vw_state sixteen wave slots of 27 sums,
    k_vw_schur four of 42, k_vw_solve fifteen rows of L, the block's own triangle, y and the pivot, k_vw_scale sixteen wave sums and eight counters."""
    k = _kernels(_isa("orbvw"))
    source = open(os.path.join(CSRC, "orbvw.hip")).read()
    header = open(os.path.join(ROOT, "include", "orbvw.h")).read()
    header = re.sub(r"\s*\n \* +", " ", header)
    assert len(k) == len(STATED), sorted(k)
    assert STATED["k_vw_state"][1] == 16 * 27 * 8 and STATED["k_vw_schur"][1] == 4 * 42 * 8 and STATED["k_vw_solve"][1] == (15 * 480 + 15 * 16 + 480 + 1) * 8
    assert STATED["k_vw_off_scan"][1] == 1024 * 4 and STATED["k_vw_base"][1] == 4 * 8 + 8 * 4 and STATED["k_vw_scale"][1] == 16 * 8 + 8 * 4
    for key, (threads, lds_stated) in STATED.items():
        mangled = [m for m in k if re.search(r"\d%sE" % key, m)]
        assert len(mangled) == 1, (key, sorted(k))
        vgpr, scratch, lds = k[mangled[0]]
        print(key, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0 and vgpr <= 512 * 4 * 64 // threads and vgpr <= 512 and lds == lds_stated
        assert "%s %d / 0 / %d B" % (key, vgpr, lds) in header, key
        assert re.search(r"__launch_bounds__\((%d|%s)\) void %s\(" % (threads, BOUND.get(key, "-"), key), source), key


def test_the_camera_is_still_written_once_and_orbvi_is_left_alone():
    """orbvw.hip evaluates csrc/orbba_camera.h like orbba.hip and orbvi.hip and defines neither function itself; the pose derivation, the
    pose Jacobian, the Huber kernel and the quadratic form it has in common with k_vi_linearize are defined once, in
    csrc/orbi_graph_device.h, which the three sources on the inertial graph include, so orbvi.hip still does not know about orbvw"""
    text = open(os.path.join(CSRC, "orbvw.hip")).read()
    for fn in ("ba_project", "ba_proj_jacobian"):
        assert '#include "orbba_camera.h"' in text and re.search(r"\b%s\(" % fn, text), fn
        assert not re.search(r"__forceinline__ \w+ %s\(" % fn, text) and "struct BaCam" not in text, fn
    assert "orbvw" not in open(os.path.join(CSRC, "orbvi.hip")).read()
    assert "orbvw.hip" in open(os.path.join(CSRC, "Makefile")).read()
    consts = dict(re.findall(r"(ST_T|SC_T|SW_T|BS_T) = (\d+)", text))
    assert consts == {"ST_T": "1024", "SC_T": "256", "SW_T": "512", "BS_T": "1024"}, consts
    shared = open(os.path.join(CSRC, "orbi_graph_device.h")).read()
    sources = {src: open(os.path.join(CSRC, src)).read() for src in ("orbvi.hip", "orbvw.hip", "orbi_factors.hip")}
    for fn in SHARED_DEVICE + SHARED_HOST:
        assert len(re.findall(r"^(?:__device__ __forceinline__|inline) \w+ %s\(" % fn, shared, re.M)) == 1, fn
        for src, body in sources.items():
            assert not re.search(r"^\s*(?:__device__ |static |inline )[\w ]*\b%s\(" % fn, body, re.M), (src, fn)
    for src, body in sources.items():
        assert '#include "orbi_graph_device.h"' in body, src
    for fn in SHARED_DEVICE + SHARED_HOST:                        # and every one serves both of EdgeMono's files
        assert re.search(r"\b%s\(" % fn, sources["orbvi.hip"]) and re.search(r"\b%s\(" % fn, text), fn
    workgroup = open(os.path.join(CSRC, "orb_device.h")).read()
    for fn in ("block_sums_put", "block_sums_get"):
        assert len(re.findall(r"__forceinline__ \w+ %s\(" % fn, workgroup)) == 1 and text.count(fn + "(") == 3, fn
    assert "wave_sum(" not in text                                # no kernel of the file finishes its sums by hand
