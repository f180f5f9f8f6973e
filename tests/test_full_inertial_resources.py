"""Kernel resources of fullInertialOptimize's shared-bias graph (csrc/orbfi.hip), read from the gfx950 ISA that hipcc emits for the shipped
source (no GPU needed), by the method of tests/test_factors_resources.py: what include/orbfi.h states for them.  Zero scratch is the
condition; the other figures are whatever the build gives, and the header must state them."""
import re

from resource_checks import defined_once, source, stated, used_not_defined

# kernel (substring of the mangled name) -> (static LDS bytes as include/orbfi.h states them, threads of its workgroup)
STATED = {"k_fi_edge": (28640, 256), "k_fi_gather": (32, 256), "k_fi_recover": (32, 64), "k_fi_jobs": (32, 64)}


def test_the_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Four kernels, the ones the header names.  No scratch memory anywhere; within 128 VGPRs, the bound of the sister tests; static LDS
    as stated: k_fi_edge holds k_fac_edge's four wave slices of 825 doubles and 140 floats, everything else the eight counters."""
    assert STATED["k_fi_edge"][0] == 4 * (825 * 8 + 140 * 4)
    assert all(threads in (64, 256) for _, threads in STATED.values())
    stated("orbfi", "orbfi.h", {key: lds for key, (lds, _) in STATED.items()}, 128)


def test_the_edge_and_the_recovery_are_shared_not_copied():
    """orbfi.hip and orbi_factors.hip take the edge's prologue, widening, rotation residual, chi2 and quadratic form from csrc/orbi_edge.h, the
    fields EdgeInertial adds, ev and ep, the Jacobian's entries and a job of the recovery from csrc/orbi_factors_device.h, the float part from
    csrc/orbi_so3.h, the validity of an edge and the duplicate scan from csrc/orbi_graph_device.h and the flush of the eight counters from
    csrc/orb_device.h, which also has the one clear kernel that csrc/orb_host.h's LAUNCH_COUNTED launches; neither defines them itself"""
    shared, device = source("orbi_factors_device.h"), source("orb_device.h")
    own = ("jac_entry", "edge_velocity_position", "recover_job", "flush_counts")
    for fn in own:
        assert defined_once(device if fn == "flush_counts" else shared, fn), fn
    assert "flush_counts(" not in shared and len(re.findall(r"__global__ void k_counters_clear\(", device)) == 1
    assert "define LAUNCH_COUNTED" in source("orb_host.h")
    for src in ("orbfi.hip", "orbi_factors.hip", "orbvi.hip", "orbi_imu.hip"):          # no clear kernel and no launch of one of their own
        text = source(src)
        assert not re.search(r"__global__[^\n(]*clear\(", text) and not re.search(r"hipLaunchKernelGGL\([^\n]*clear", text), src
        assert "define LAUNCH_COUNTED" not in text and (src == "orbfi.hip") == ("LAUNCH_COUNTED(" not in text), src
    edge_fns = ("edge_refused", "edge_load", "edge_widen", "edge_rotation", "edge_chi2", "edge_jtwj", "edge_quadratic_form")
    for src in ("orbfi.hip", "orbi_factors.hip"):
        text = source(src)
        for header in ("orbi_edge.h", "orbi_factors_device.h", "orbi_graph_device.h", "orbi_so3.h"):
            assert '#include "%s"' % header in text, (src, header)
        for fn in own + edge_fns + ("bias_deltas", "edge_valid", "dof_fixed"):
            assert used_not_defined(text, fn), (src, fn)
