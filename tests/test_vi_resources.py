"""Kernel resources of the visual edges on the inertial graph and of the damped step (csrc/orbvi.hip), read from the gfx950 ISA that
hipcc emits for the shipped source (no GPU needed), by the method of tests/test_factors_resources.py: what include/orbvi.h states."""
import re

from resource_checks import defined_once, defines_itself, source, stated
from test_vw_resources import SHARED_DEVICE, SHARED_HOST

# kernel (substring of the mangled name) -> static LDS bytes as include/orbvi.h states them
STATED = {"k_counters_clear": 0, "k_vi_linearize": 3952, "k_vi_solve": 30032}


def test_the_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Three kernels, the ones the header names.  No scratch memory; within 128 VGPRs -- k_vi_linearize is a 1024-thread workgroup, which
    has no more; static LDS as stated: k_vi_linearize sixteen wave slots of 29 sums, the derived pose (24 doubles) and twelve counters,
    k_vi_solve the 60 x 61 matrix, a 60-vector, the 60 fixed flags and eight counters."""
    assert STATED["k_vi_linearize"] == 16 * 29 * 8 + 24 * 8 + 12 * 4 and STATED["k_vi_solve"] == 60 * 61 * 8 + 60 * 8 + 60 * 4 + 8 * 4
    stated("orbvi", "orbvi.h", STATED, 128)


def test_the_camera_is_written_once():
    """orbvi.hip and orbba.hip include csrc/orbba_camera.h; neither defines the projection or its Jacobian itself"""
    shared = source("orbba_camera.h")
    for fn in ("ba_project", "ba_proj_jacobian"):
        assert re.search(r"__forceinline__ void %s\(" % fn, shared), fn
        for src in ("orbba.hip", "orbvi.hip"):
            text = source(src)
            assert '#include "orbba_camera.h"' in text and re.search(r"\b%s\(" % fn, text), (src, fn)
            assert not re.search(r"__forceinline__ \w+ %s\(" % fn, text) and "struct BaCam" not in text, (src, fn)
    assert "struct BaCam" in shared
    assert "orbvi.hip" in source("Makefile")


def test_the_edge_math_on_the_inertial_graph_is_written_once():
    """orbvi.hip takes dsum3, dof_fixed, the orbi_edge predicate, the pose entries, the pose Jacobian, the Huber kernel, the quadratic
    form with its scatter and the host checks from csrc/orbi_graph_device.h, which defines each exactly once, and the ordered workgroup
    finish from csrc/orb_device.h"""
    shared, text = source("orbi_graph_device.h"), source("orbvi.hip")
    assert '#include "orbi_graph_device.h"' in text and '#include "orb_device.h"' in text
    for fn in SHARED_DEVICE + SHARED_HOST:
        assert defined_once(shared, fn, "(?:__device__ __forceinline__|inline)"), fn
        assert re.search(r"\b%s\(" % fn, text) and not defines_itself(text, fn), fn
    assert "#pragma clang fp contract(off)" in shared and shared.index("#pragma clang fp contract(off)") < shared.index("namespace {")
    assert "block_sums_put(" in text and "block_sums_get(" in text
