"""Kernel resources of the visual edges on the inertial graph and of the damped step (csrc/orbvi.hip), read from the gfx950 ISA that
hipcc emits for the shipped source (no GPU needed), by the method of tests/test_factors_resources.py: what include/orbvi.h states."""
import os
import re

from test_kernel_resources import _isa, _kernels
from test_vw_resources import SHARED_DEVICE, SHARED_HOST

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monoorbslam3_amd", "csrc")
# kernel (substring of the mangled name) -> static LDS bytes as include/orbvi.h states them
STATED = {"k_counters_clear": 0, "k_vi_linearize": 3952, "k_vi_solve": 30032}


def test_the_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Three kernels, the ones the header names.  No scratch memory; within 128 VGPRs -- k_vi_linearize is a 1024-thread workgroup, which
    has no more; static LDS as stated: k_vi_linearize sixteen wave slots of 29 sums, the derived pose (24 doubles) and twelve counters,
    k_vi_solve the 60 x 61 matrix, a 60-vector, the 60 fixed flags and eight counters."""
    k = _kernels(_isa("orbvi"))
    header = open(os.path.join(ROOT, "include", "orbvi.h")).read()
    header = re.sub(r"\s*\n \* +", " ", header)
    assert len(k) == len(STATED), sorted(k)
    assert STATED["k_vi_linearize"] == 16 * 29 * 8 + 24 * 8 + 12 * 4 and STATED["k_vi_solve"] == 60 * 61 * 8 + 60 * 8 + 60 * 4 + 8 * 4
    for key, lds_stated in STATED.items():
        mangled = [m for m in k if key in m]
        assert len(mangled) == 1, (key, sorted(k))
        vgpr, scratch, lds = k[mangled[0]]
        print(key, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0 and vgpr <= 128 and lds == lds_stated
        assert "%s %d / 0 / %d B" % (key, vgpr, lds) in header, key


def test_the_camera_is_written_once():
    """orbvi.hip and orbba.hip include csrc/orbba_camera.h; neither defines the projection or its Jacobian itself"""
    shared = open(os.path.join(CSRC, "orbba_camera.h")).read()
    for fn in ("ba_project", "ba_proj_jacobian"):
        assert re.search(r"__forceinline__ void %s\(" % fn, shared), fn
        for src in ("orbba.hip", "orbvi.hip"):
            text = open(os.path.join(CSRC, src)).read()
            assert '#include "orbba_camera.h"' in text and re.search(r"\b%s\(" % fn, text), (src, fn)
            assert not re.search(r"__forceinline__ \w+ %s\(" % fn, text) and "struct BaCam" not in text, (src, fn)
    assert "struct BaCam" in shared
    assert "orbvi.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_edge_math_on_the_inertial_graph_is_written_once():
    """orbvi.hip takes dsum3, dof_fixed, the orbi_edge predicate, the pose entries, the pose Jacobian, the Huber kernel, the quadratic
    form with its scatter and the host checks from csrc/orbi_graph_device.h, which defines each exactly once, and the ordered workgroup
    finish from csrc/orb_device.h"""
    shared = open(os.path.join(CSRC, "orbi_graph_device.h")).read()
    text = open(os.path.join(CSRC, "orbvi.hip")).read()
    assert '#include "orbi_graph_device.h"' in text and '#include "orb_device.h"' in text
    for fn in SHARED_DEVICE + SHARED_HOST:
        assert len(re.findall(r"^(?:__device__ __forceinline__|inline) \w+ %s\(" % fn, shared, re.M)) == 1, fn
        assert re.search(r"\b%s\(" % fn, text), fn
        assert not re.search(r"^\s*(?:__device__ |static |inline )[\w ]*\b%s\(" % fn, text, re.M), fn
    assert "#pragma clang fp contract(off)" in shared and shared.index("#pragma clang fp contract(off)") < shared.index("namespace {")
    assert "block_sums_put(" in text and "block_sums_get(" in text
