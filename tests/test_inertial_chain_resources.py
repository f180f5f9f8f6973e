"""Kernel resources of localInertialBundleAdjustment on the device (csrc/orbil.hip, csrc/orbm_inertial_chain.hip), read from the gfx950
ISA that hipcc emits for the shipped sources (no GPU needed), by the method of tests/test_vi_loop_resources.py, and the "written once" rule
of the band walk (csrc/orbvi_stages.h)."""
import re

from resource_checks import _isa, _kernels, defines_itself, source, stated

# kernel (substring of the mangled name) -> static LDS bytes as include/orbil.h and include/orbm.h state them
STATED = {"k_il_chain_solve": 15872, "k_il_chain_loop": 59928}
STATED_MAP = {"k_ic_problem": 192, "k_ic_velocity_priors": 32}
CHAIN_STAGES = ("chain_solve_assemble", "chain_solve_largest", "chain_solve_wave")
LOOP_STAGES = ("fac_edge_wave", "fac_gather_state", "fac_gather_tail", "fac_oplus_state")


def test_the_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Two kernels; no scratch memory and no register spilled to it; the solve (four waves) within 128 VGPRs, the loop (512 threads: eight
    waves, two per SIMD of 512 registers) within 256; static LDS as stated.  The solve: the tile of two blocks of 15 rows x 31 doubles, three
    vectors of 300 doubles, 300 fixed flags, eight counters.  The loop: the eight waves' slices of k_fac_edge (825 doubles and 140 floats
    each), over which the solve's LDS lies, and its own: dx, the solve's outputs, the policy's state, the pushed counters.  Both stay below
    the 64 KB that a kernel of this library has always been launched with"""
    assert STATED["k_il_chain_solve"] == (2 * 15 * 31 + 3 * 300) * 8 + 300 * 4 + 8 * 4 and STATED["k_il_chain_loop"] < 64 * 1024
    assert STATED["k_il_chain_loop"] >= 8 * (825 * 8 + 140 * 4) + 300 * 8 and STATED["k_il_chain_loop"] - (8 * (825 * 8 + 140 * 4) + 300 * 8) <= 256
    text = source("orbil.hip")
    assert "__launch_bounds__(IL_T) void k_il_chain_loop" in text and "IL_T = 512" in text and "dim3(1), dim3(IL_T)" in text and "dim3(1), dim3(CS_T)" in text
    stated("orbil", "orbil.h", STATED, lambda key: 256 if key == "k_il_chain_loop" else 128)
    isa = _isa("orbil")
    assert len(_kernels(isa)) == 2 and re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa) == ["0", "0"] and "scratch_" not in isa


def test_the_map_side_kernels_use_no_scratch_memory_and_the_resources_the_header_states():
    """one wave each, within 64 VGPRs; static LDS: the window's 20 key frames and their records and eight counters; eight counters"""
    assert STATED_MAP["k_ic_problem"] == 20 * 4 * 2 + 8 * 4
    stated("orbm_inertial_chain", "orbm.h", STATED_MAP, 64, breaks=r"\s*\n \* ")
    isa = _isa("orbm_inertial_chain")
    assert re.findall(r"\.vgpr_spill_count:\s+(\d+)", isa) == ["0", "0"] and "scratch_" not in isa


def test_the_band_walk_is_written_once_and_both_kernels_call_it():
    """chain_solve_assemble, chain_solve_largest and chain_solve_wave are device functions of csrc/orbvi_stages.h, defined there exactly once;
    orbil.hip calls each from the staged solve's kernel and from the loop's and defines none, nor a Cholesky of its own: it names no sqrt,
    no shuffle and no formula of an edge; the loop's other stages are the functions orbi_factors.hip's kernels run"""
    shared, text = source("orbvi_stages.h"), source("orbil.hip")
    for fn in CHAIN_STAGES + LOOP_STAGES:
        assert len(re.findall(r"^__device__ __forceinline__ \w+ %s\(" % fn, shared, re.M)) == 1, fn
        assert not defines_itself(text, fn), fn
    solve = text[text.index("void k_il_chain_solve"):text.index("// ---- the loop")]
    loop = text[text.index("void k_il_chain_loop"):text.index('extern "C"')]
    for fn in CHAIN_STAGES:
        assert re.search(r"\b%s(?:<\w+>)?\(" % fn, solve) and re.search(r"\b%s(?:<\w+>)?\(" % fn, loop), fn
    for fn in LOOP_STAGES:
        assert re.search(r"\b%s\(" % fn, loop) and re.search(r"\b%s\(" % fn, source("orbi_factors.hip")), fn
    for other in ("orbvi.hip", "orbvi_loop.hip", "orbi_factors.hip"):    # nobody else runs the band walk, and nobody has a copy
        for fn in CHAIN_STAGES:
            assert fn not in source(other), (other, fn)
    code = re.sub(r"//[^\n]*", "", text)
    for word in ("sqrt(", "__shfl", "edge_chi2", "dexp_so3", "jac_entry", "huber(", "lm_cube"):
        assert word not in code, word
    for word in ("lm_policy_iteration(", "lm_policy_trial(", "lm_policy_again(", "lm_policy_terminate(", "lm_trace_row("):
        assert word in loop, word
    assert '#include "orbvi_stages.h"' in text and '#include "orb_lm_policy.h"' in text and "#pragma clang fp contract(off)" in shared
    assert not re.search(r"atomicAdd\([^)]*double", shared) and "orbil.hip" in source("Makefile")
    # the existing stage functions keep their text: the band walk stands behind them, in front of the namespace's end
    assert shared.index("__device__ __forceinline__ bool vi_solve_wave(") < shared.index("// ---- orbil_chain_solve_device") < shared.index("chain_solve_assemble(")
