"""Kernel resources of the two-view RANSAC, read from the gfx950 ISA that hipcc emits for the shipped source (no GPU needed), by the
method of tests/test_keyframe_resources.py: what include/orbm.h states for them."""
from resource_checks import stated

# kernel -> static LDS bytes, as include/orbm.h states them
STATED = {"k_tv_prepare": 33088, "k_tv_hypotheses": 0, "k_tv_pick": 264}


def test_the_two_view_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Three kernels, the ones the header names.  No scratch memory anywhere -- the Jacobi's 9 + 9 registers per lane and the draw's
    eight-entry override list are indexed by constants --; k_tv_prepare and k_tv_pick within 128 VGPRs (workgroups of sixteen
    waves: 128 is all a thread could have), k_tv_hypotheses within 256 (18 doubles a lane and three butterflies in flight; two waves
    per SIMD remain, which is what the 2 * 1024 waves of the largest call put on the device's 1024 SIMDs).  Static LDS as stated: the 8 * 1024 raw draws, the sixteen slots of the scan and the 16 x 4 partial sums of
    Normalize in k_tv_prepare; the per-wave maxima and the two inlier counts in k_tv_pick."""
    stated("orbm_two_view", "orbm.h", STATED, lambda k: 256 if k == "k_tv_hypotheses" else 128)
