"""Kernel resources of the covisibility graph's kernels, read from the gfx950 ISA that hipcc emits for the shipped source (no GPU
needed), by the method of tests/test_kernel_resources.py: what include/orbm.h states for them."""
from resource_checks import stated

# kernel -> static LDS bytes, as include/orbm.h states them
STATED = {"k_graph_update": 32808, "k_graph_erase": 32, "k_graph_resort": 32776, "k_graph_fuse_targets": 16992, "k_graph_connected": 0}


def test_the_graph_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Five kernels, the ones the header names.  No scratch memory anywhere; within 64 VGPRs (workgroups of sixteen waves: 128 is all a
    thread could have); static LDS as stated: the 4096 64-bit sort keys (32 KB) plus counters in k_graph_update and k_graph_resort, the
    4096 targets, their marks and the scan's slots in k_graph_fuse_targets."""
    stated("orbm_graph", "orbm.h", STATED, 64, breaks=r"\s*\n \* ")
