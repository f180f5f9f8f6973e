"""Kernel resources of the key-frame insertion, the registration of new map points and the map-point culling, read from the gfx950 ISA
that hipcc emits for the shipped source (no GPU needed), by the method of tests/test_local_map_resources.py: what include/orbm.h states
for them."""
from resource_checks import stated

# kernel -> static LDS bytes, as include/orbm.h states them
STATED = {"k_kf_insert": 32, "k_kf_register": 0, "k_kf_cull_points": 352}


def test_the_keyframe_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Three kernels, the ones the header names.  No scratch memory anywhere; within 64 VGPRs (each is a workgroup of sixteen waves: 128
    is all a thread could have); static LDS as stated: the eight counters, and in k_kf_cull_points also the scan's sixteen slots and the
    words of the workgroup-wide `or` behind the premise's test.  The masks of one bit per table row are dynamic LDS."""
    stated("orbm_keyframe", "orbm.h", STATED, 64, breaks=r"\s*\n \* ")
