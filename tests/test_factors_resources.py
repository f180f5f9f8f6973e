"""Kernel resources of the inertial factors (csrc/orbi_factors.hip), read from the gfx950 ISA that hipcc emits for the shipped source
(no GPU needed), by the method of tests/test_imu_resources.py: what include/orbi.h states for them."""
import re

from resource_checks import source, stated

# kernel (substring of the mangled name) -> static LDS bytes as include/orbi.h states them, k_fac_edge under its own name
STATED = {"k_counters_clear": 0, "k_fac_prior_info": 32, "k_fac_init": 32, "k_fac_oplus": 32, "k_fac_recover": 32, "k_fac_edge_info": 5792,
          "k_fac_edgeENS": ("k_fac_edge", 28640), "k_fac_gather": 32}


def test_the_factor_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Eight kernels, the ones the header names.  No scratch memory anywhere; within 128 VGPRs; static LDS as stated: k_fac_edge holds four
    wave slices of 825 doubles and 140 floats (the vertices, the 3x3 temporaries, the 9x30 Jacobian, the 9x9 information, their 9x30
    product), k_fac_edge_info four augmented 9x18 matrices and the two walk blocks, everything else the eight counters."""
    stated("orbi_factors", "orbi.h", STATED, 128)


def test_the_float_helpers_are_shared_not_copied():
    """orbi_factors.hip and orbi_imu.hip include csrc/orbi_so3.h; neither defines ExpSO3f's entry or the Newton step itself"""
    shared = source("orbi_so3.h")
    for fn in ("exp_entry", "rightj_entry", "newton_entry", "so3_scalars", "m3s"):
        assert re.search(r"\b%s\(" % fn, shared), fn
        for src in ("orbi_imu.hip", "orbi_factors.hip"):
            text = source(src)
            assert '#include "orbi_so3.h"' in text and not re.search(r"__forceinline__ \w+ %s\(" % fn, text), (src, fn)
