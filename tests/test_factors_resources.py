"""Kernel resources of the inertial factors (csrc/orbi_factors.hip), read from the gfx950 ISA that hipcc emits for the shipped source
(no GPU needed), by the method of tests/test_imu_resources.py: what include/orbi.h states for them."""
import os
import re

from test_kernel_resources import _isa, _kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# kernel (substring of the mangled name) -> static LDS bytes as include/orbi.h states them
STATED = {"k_counters_clear": 0, "k_fac_prior_info": 32, "k_fac_init": 32, "k_fac_oplus": 32, "k_fac_recover": 32, "k_fac_edge_info": 5792,
          "k_fac_edgeENS": 28640, "k_fac_gather": 32}


def test_the_factor_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Eight kernels, the ones the header names.  No scratch memory anywhere; within 128 VGPRs; static LDS as stated: k_fac_edge holds four
    wave slices of 825 doubles and 140 floats (the vertices, the 3x3 temporaries, the 9x30 Jacobian, the 9x9 information, their 9x30
    product), k_fac_edge_info four augmented 9x18 matrices and the two walk blocks, everything else the eight counters."""
    k = _kernels(_isa("orbi_factors"))
    header = open(os.path.join(ROOT, "include", "orbi.h")).read()
    header = re.sub(r"\s*\n \* +", " ", header)
    assert len(k) == len(STATED), sorted(k)
    for key, lds_stated in STATED.items():
        mangled = [m for m in k if key in m]
        assert len(mangled) == 1, (key, sorted(k))
        vgpr, scratch, lds = k[mangled[0]]
        name = key[:-3] if key.endswith("ENS") else key
        print(name, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0 and vgpr <= 128 and lds == lds_stated
        assert "%s %d / 0 / %d B" % (name, vgpr, lds) in header, name


def test_the_float_helpers_are_shared_not_copied():
    """orbi_factors.hip and orbi_imu.hip include csrc/orbi_so3.h; neither defines ExpSO3f's entry or the Newton step itself"""
    csrc = os.path.join(ROOT, "monoorbslam3_amd", "csrc")
    shared = open(os.path.join(csrc, "orbi_so3.h")).read()
    for fn in ("exp_entry", "rightj_entry", "newton_entry", "so3_scalars", "m3s"):
        assert re.search(r"\b%s\(" % fn, shared), fn
        for src in ("orbi_imu.hip", "orbi_factors.hip"):
            text = open(os.path.join(csrc, src)).read()
            assert '#include "orbi_so3.h"' in text and not re.search(r"__forceinline__ \w+ %s\(" % fn, text), (src, fn)
