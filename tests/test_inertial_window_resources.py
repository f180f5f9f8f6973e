"""Kernel resources of the inertial window's assembly and its velocity prior, read from the gfx950 ISA that hipcc emits for the shipped
source (no GPU needed), by the method of tests/test_keyframe_resources.py: what include/orbm.h states for them."""
from resource_checks import stated

# kernel -> static LDS bytes, as include/orbm.h states them
STATED = {"k_iw_problem": 320, "k_iw_velocity_prior": 0}


def test_the_inertial_window_kernels_use_no_scratch_memory_and_the_resources_the_header_states():
    """Two kernels, the ones the header names.  No scratch memory; within 64 VGPRs (the assembly is a workgroup of sixteen waves: 128 is
    all a thread could have); static LDS as stated: the window's 32 key frames, 2 x 16 wave totals and sixteen counters in the assembly,
    none in the velocity prior; the VGPRs the compiler gives are the ones the header prints."""
    stated("orbm_inertial_window", "orbm.h", STATED, 64, breaks=r"\s*\n \* ")
