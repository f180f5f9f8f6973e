"""Kernel resources of the visual window of the inertial local bundle adjustment (csrc/orbvw.hip), read from the gfx950 ISA that hipcc
emits for the shipped source (no GPU needed), by the method of tests/test_vi_resources.py: what include/orbvw.h states."""
import re

from resource_checks import defined_once, defines_itself, source, stated

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
    assert STATED["k_vw_state"][1] == 16 * 27 * 8 and STATED["k_vw_schur"][1] == 4 * 42 * 8 and STATED["k_vw_solve"][1] == (15 * 480 + 15 * 16 + 480 + 1) * 8
    assert STATED["k_vw_off_scan"][1] == 1024 * 4 and STATED["k_vw_base"][1] == 4 * 8 + 8 * 4 and STATED["k_vw_scale"][1] == 16 * 8 + 8 * 4
    stated("orbvw", "orbvw.h", {key: lds for key, (_, lds) in STATED.items()}, lambda key: min(512, 512 * 4 * 64 // STATED[key][0]), match="exact")
    text = source("orbvw.hip")
    for key, (threads, _) in STATED.items():
        assert re.search(r"__launch_bounds__\((%d|%s)\) void %s\(" % (threads, BOUND.get(key, "-"), key), text), key


def test_the_camera_is_still_written_once_and_orbvi_is_left_alone():
    """orbvw.hip evaluates csrc/orbba_camera.h like orbba.hip and orbvi.hip and defines neither function itself; the pose derivation, the
    pose Jacobian, the Huber kernel and the quadratic form it has in common with k_vi_linearize are defined once, in
    csrc/orbi_graph_device.h, which the three sources on the inertial graph include, so orbvi.hip still does not know about orbvw"""
    text = source("orbvw.hip")
    for fn in ("ba_project", "ba_proj_jacobian"):
        assert '#include "orbba_camera.h"' in text and re.search(r"\b%s\(" % fn, text), fn
        assert not re.search(r"__forceinline__ \w+ %s\(" % fn, text) and "struct BaCam" not in text, fn
    assert "orbvw" not in source("orbvi.hip")
    assert "orbvw.hip" in source("Makefile")
    consts = dict(re.findall(r"(ST_T|SC_T|SW_T|BS_T) = (\d+)", text))
    assert consts == {"ST_T": "1024", "SC_T": "256", "SW_T": "512", "BS_T": "1024"}, consts
    shared = source("orbi_graph_device.h")
    sources = {src: source(src) for src in ("orbvi.hip", "orbvw.hip", "orbi_factors.hip")}
    for fn in SHARED_DEVICE + SHARED_HOST:
        assert defined_once(shared, fn, "(?:__device__ __forceinline__|inline)"), fn
        for src, body in sources.items():
            assert not defines_itself(body, fn), (src, fn)
    for src, body in sources.items():
        assert '#include "orbi_graph_device.h"' in body, src
    for fn in SHARED_DEVICE + SHARED_HOST:                        # and every one serves both of EdgeMono's files
        assert re.search(r"\b%s\(" % fn, sources["orbvi.hip"]) and re.search(r"\b%s\(" % fn, text), fn
    workgroup = source("orb_device.h")
    for fn in ("block_sums_put", "block_sums_get"):
        assert len(re.findall(r"__forceinline__ \w+ %s\(" % fn, workgroup)) == 1 and text.count(fn + "(") == 3, fn
    assert "wave_sum(" not in text                                # no kernel of the file finishes its sums by hand
