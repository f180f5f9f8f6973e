"""Kernel resources of the local map's kernels, read from the gfx950 ISA that hipcc emits for the shipped source (no GPU needed), by
the method of tests/test_graph_resources.py: what include/orbm.h states for them."""
from resource_checks import stated

# kernel -> static LDS bytes, as include/orbm.h states them
STATED = {"k_local_map": 33412, "k_track_counters": 0, "k_num_tracked": 0}


def test_the_local_map_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Three kernels, the ones the header names.  No scratch memory anywhere; within 64 VGPRs (k_local_map is a workgroup of sixteen
    waves: 128 is all a thread could have); static LDS as stated: in k_local_map the 4096 votes and the 4096 list entries (16 KB each),
    their 4096 mark bits, the scan's slots and the counters."""
    stated("orbm_localmap", "orbm.h", STATED, 64, breaks=r"\s*\n \* ")
