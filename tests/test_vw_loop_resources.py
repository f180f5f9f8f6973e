"""Kernel resources of the window loop's device side (csrc/orbwl.hip), read from the gfx950 ISA that hipcc emits for the shipped source
(no GPU needed), by the method of tests/test_vi_resources.py, and the "written once" rules of the loop: the stages are the library's
staged entry points, which the host driver CALLS; the policy's arithmetic is csrc/orb_lm_policy.h's; no stage formula is restated."""
import re

from resource_checks import _isa, _kernels, defines_itself, source, stated

# kernel -> (threads per workgroup, static LDS bytes as include/orbwl.h states them)
STATED = {"k_vwl_begin": (64, 0), "k_vwl_push": (256, 0), "k_vwl_decide": (256, 4), "k_vwl_end": (64, 0)}
BOUND = {"k_vwl_push": "WL_T", "k_vwl_decide": "WL_T"}
# the staged entry points of one trial chain, in the chain's order, and the classification
STAGES = ("orbi_linearize_device", "orbvw_linearize_device", "orbvw_reduce_device", "orbvw_solve_device", "orbvw_backsub_device", "orbi_graph_oplus_device")
POLICY = ("lm_policy_iteration", "lm_policy_trial", "lm_policy_again", "lm_policy_terminate")


def test_the_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Four kernels, the ones the header names, one workgroup each; no scratch memory, no spilled register; the one static LDS word is the
    decision k_vwl_decide publishes to its workgroup"""
    stated("orbwl", "orbwl.h", {key: lds for key, (_, lds) in STATED.items()}, 128, match="exact")
    isa, text = _isa("orbwl"), source("orbwl.hip")
    assert len(_kernels(isa)) == 4 and set(re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa)) == {"0"} and "scratch_" not in isa
    assert "WL_T = 256" in text
    for key, (threads, _) in STATED.items():
        assert re.search(r"__launch_bounds__\((%d|%s)\) void %s\(" % (threads, BOUND.get(key, "-"), key), text), key
        assert len(re.findall(r"hipLaunchKernelGGL\(%s, dim3\(1\), dim3\((%d|%s)\)" % (key, threads, BOUND.get(key, "-")), text)) == 1, key


def test_the_stages_and_the_policy_are_written_once():
    """orbwl.hip defines none of the stage kernels and names no stage arithmetic; the driver (the window loop's section of orbvw.hip) calls
    every staged entry point by name and launches nothing itself; the trial policy is defined once, in orb_lm_policy.h, which the
    decision kernel uses"""
    loop, policy, host = source("orbwl.hip"), source("orb_lm_policy.h"), source("orbvw.hip")
    code = re.sub(r"//[^\n]*", "", loop)
    assert not re.search(r"\bk_(vw|fac|vi)_\w+", code)
    for word in ("ba_project", "ba_proj_jacobian", "huber(", "sqrt(", "dexp_so3", "quad_accumulate", "edge_chi2", "__shfl", "atomic", "pow("):
        assert word not in code, word
    assert '#include "orb_lm_policy.h"' in loop and "#pragma clang fp contract(off)" in loop and "#pragma clang fp contract(off)" in policy
    for fn in POLICY:
        assert len(re.findall(r"^__host__ __device__ __forceinline__ \w+ %s\(" % fn, policy, re.M)) == 1, fn
        assert not defines_itself(loop, fn) and re.search(r"\b%s\(" % fn, code), fn
    # the cube stands once, behind lm_cube: x * x * x in its device branch, and the header's only pow( is its host branch
    bare = re.sub(r"//[^\n]*", "", policy)
    cube = re.search(r"double lm_cube\(double x\)\s*\{\s*#ifdef __HIP_DEVICE_COMPILE__\s*return x \* x \* x;\s*#else\s*return pow\(x, 3\);\s*#endif\s*\}", bare)
    assert cube and bare.count("pow") == 1 and bare.count("x * x * x") == 1 and "DBL_MAX" in policy and "1e-3" in policy
    # the driver: behind its banner nothing but calls of the staged entry points and of orbwl.hip's four launches
    driver = re.sub(r"//[^\n]*", "", host[host.index('#include "orbwl_kernels.h"'):])
    assert "hipLaunchKernelGGL" not in driver and "__global__" not in driver and "__device__" not in driver
    for fn in STAGES:
        assert re.search(r"\b%s\(" % fn, driver), fn
    at = [driver.index(fn + "(", driver.index("for (int trial")) for fn in STAGES[2:]]
    assert at == sorted(at), at                                    # reduce, solve, back-substitution, update: the chain's order
    for fn in ("wl_launch_begin", "wl_launch_push", "wl_launch_decide", "wl_launch_end"):
        assert re.search(r"\b%s\(" % fn, driver) and re.search(r"^hipError_t %s\(" % fn, loop, re.M), fn
    assert driver.count("hipStreamSynchronize(") == 2              # once per trial, once at the end
    assert "Lease<WlWork> lease(g_wl_work)" in driver and "hipHostMalloc" not in driver and "hipMalloc" not in driver
    before = host[:host.index('#include "orbwl_kernels.h"')]
    assert "orbwl" not in before.split("// The window loop (include/orbwl.h)")[0]      # the stage kernels' part of the file does not know about the loop
    assert "orbwl.hip" in source("Makefile")
