"""Kernel resources of fullInertialOptimize's shared-bias graph (csrc/orbfi.hip), read from the gfx950 ISA that hipcc emits for the shipped
source (no GPU needed), by the method of tests/test_factors_resources.py: what include/orbfi.h states for them.  Zero scratch is the
condition; the other figures are whatever the build gives, and the header must state them."""
import os
import re

from test_kernel_resources import _isa, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monoorbslam3_amd", "csrc")
# kernel (substring of the mangled name) -> (static LDS bytes as include/orbfi.h states them, threads of its workgroup)
STATED = {"k_fi_edge": (28640, 256), "k_fi_gather": (32, 256), "k_fi_recover": (32, 64), "k_fi_jobs": (32, 64)}


def test_the_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Four kernels, the ones the header names.  No scratch memory anywhere; within 128 VGPRs, the bound of the sister tests; static LDS
    as stated: k_fi_edge holds k_fac_edge's four wave slices of 825 doubles and 140 floats, everything else the eight counters."""
    assert STATED["k_fi_edge"][0] == 4 * (825 * 8 + 140 * 4)
    k = _kernels(_isa("orbfi"))
    header = re.sub(r"\s*\n \* +", " ", open(os.path.join(ROOT, "include", "orbfi.h")).read())
    assert len(k) == len(STATED), sorted(k)
    for key, (lds_stated, threads) in STATED.items():
        mangled = [m for m in k if key in m]
        assert len(mangled) == 1, (key, sorted(k))
        vgpr, scratch, lds = k[mangled[0]]
        print(key, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0 and vgpr <= 128 and threads in (64, 256) and lds == lds_stated
        assert "%s %d / 0 / %d B" % (key, vgpr, lds) in header, key


def test_the_edge_and_the_recovery_are_shared_not_copied():
    """orbfi.hip and orbi_factors.hip take the edge's prologue, widening, rotation residual, chi2 and quadratic form from csrc/orbi_edge.h, the
    fields EdgeInertial adds, ev and ep, the Jacobian's entries and a job of the recovery from csrc/orbi_factors_device.h, the float part from
    csrc/orbi_so3.h, the validity of an edge and the duplicate scan from csrc/orbi_graph_device.h and the flush of the eight counters from
    csrc/orb_device.h, which also has the one clear kernel that csrc/orb_host.h's LAUNCH_COUNTED launches; neither defines them itself"""
    shared = open(os.path.join(CSRC, "orbi_factors_device.h")).read()
    device = open(os.path.join(CSRC, "orb_device.h")).read()
    own = ("jac_entry", "edge_velocity_position", "recover_job", "flush_counts")
    for fn in own:
        where = device if fn == "flush_counts" else shared
        assert len(re.findall(r"^__device__ __forceinline__ \w+ %s\(" % fn, where, re.M)) == 1, fn
    assert "flush_counts(" not in shared and len(re.findall(r"__global__ void k_counters_clear\(", device)) == 1
    assert "define LAUNCH_COUNTED" in open(os.path.join(CSRC, "orb_host.h")).read()
    for src in ("orbfi.hip", "orbi_factors.hip", "orbvi.hip", "orbi_imu.hip"):          # no clear kernel and no launch of one of their own
        text = open(os.path.join(CSRC, src)).read()
        assert not re.search(r"__global__[^\n(]*clear\(", text) and not re.search(r"hipLaunchKernelGGL\([^\n]*clear", text), src
        assert "define LAUNCH_COUNTED" not in text and (src == "orbfi.hip") == ("LAUNCH_COUNTED(" not in text), src
    edge_fns = ("edge_refused", "edge_load", "edge_widen", "edge_rotation", "edge_chi2", "edge_jtwj", "edge_quadratic_form")
    for src in ("orbfi.hip", "orbi_factors.hip"):
        text = open(os.path.join(CSRC, src)).read()
        for header in ("orbi_edge.h", "orbi_factors_device.h", "orbi_graph_device.h", "orbi_so3.h"):
            assert '#include "%s"' % header in text, (src, header)
        for fn in own + edge_fns + ("bias_deltas", "edge_valid", "dof_fixed"):
            assert re.search(r"\b%s(?:<\d+>)?\(" % fn, text), (src, fn)
            assert not re.search(r"^\s*(?:__device__ |static |inline )[\w ]*\b%s\(" % fn, text, re.M), (src, fn)
