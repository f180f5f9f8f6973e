"""Kernel resources of the one-launch pose optimiser (csrc/orbvi_loop.hip), read from the gfx950 ISA that hipcc emits for the shipped source
(no GPU needed), by the method of tests/test_vi_resources.py, and the "written once" rule of its stages (csrc/orbvi_stages.h)."""
import re

from resource_checks import _isa, _kernels, defines_itself, source, stated

# kernel (substring of the mangled name) -> static LDS bytes as include/orbvi_loop.h states them
STATED = {"k_vi_pose_loop": 41576}
STAGES = ("fac_edge_wave", "fac_gather_state", "fac_gather_tail", "fac_oplus_state", "vi_linearize_group", "vi_solve_assemble", "vi_solve_largest", "vi_solve_wave")


def test_the_loop_kernel_uses_no_scratch_memory_and_the_lds_the_header_states():
    """One kernel; no scratch memory; within the VGPRs its workgroup size allows -- 512 threads are eight waves, two per SIMD of 512
    registers: 256 each --; static LDS as stated (the slices of k_fac_edge's wave, k_vi_linearize's and k_vi_solve's LDS, and the loop's
    own: dx, the solve's outputs, the policy's state); and no register is spilled to scratch"""
    text = source("orbvi_loop.hip")
    assert "LOOP_VT = 2, LOOP_T = VI_T / LOOP_VT" in text and "VI_T = 1024" in source("orbvi_stages.h")
    assert "__launch_bounds__(LOOP_T) void k_vi_pose_loop" in text and "dim3(1), dim3(LOOP_T)" in text
    stated("orbvi_loop", "orbvi_loop.h", STATED, 512 // (512 // 64 // 4))
    isa = _isa("orbvi_loop")
    assert len(_kernels(isa)) == 1 and re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa) == ["0"] and "scratch_" not in isa


def test_the_stages_are_written_once():
    """the bodies of k_fac_edge, k_fac_gather, k_fac_oplus, k_vi_linearize and k_vi_solve are device functions of csrc/orbvi_stages.h, defined
    there exactly once; orbi_factors.hip, orbvi.hip and orbvi_loop.hip call them and define none; the loop kernel has no second copy of a
    formula: it includes the header and names no camera, Huber or Cholesky arithmetic of its own"""
    shared = source("orbvi_stages.h")
    texts = {src: source(src) for src in ("orbi_factors.hip", "orbvi.hip", "orbvi_loop.hip")}
    for fn in STAGES:
        assert len(re.findall(r"^__device__ __forceinline__ \w+ %s\(" % fn, shared, re.M)) == 1, fn
        for src, text in texts.items():
            assert not defines_itself(text, fn), (src, fn)
        assert re.search(r"\b%s(?:<\w+>)?\(" % fn, texts["orbvi_loop.hip"]), fn
    for fn in STAGES[:4]:
        assert re.search(r"\b%s\(" % fn, texts["orbi_factors.hip"]), fn
    for fn in STAGES[4:]:
        assert re.search(r"\b%s(?:<\w+>)?\(" % fn, texts["orbvi.hip"]), fn
    for src, text in texts.items():
        assert '#include "orbvi_stages.h"' in text, src
    loop = re.sub(r"//[^\n]*", "", texts["orbvi_loop.hip"])
    for word in ("ba_project", "ba_proj_jacobian", "huber(", "sqrt(", "dexp_so3", "quad_accumulate", "edge_chi2", "__shfl"):
        assert word not in loop, word
    assert "#pragma clang fp contract(off)" in shared and "atomicAdd(&s_cnt" in shared and not re.search(r"atomicAdd\([^)]*double", shared)
    assert "orbvi_loop.hip" in source("Makefile")
