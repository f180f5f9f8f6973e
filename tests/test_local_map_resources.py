"""Kernel resources of the local map's kernels, read from the gfx950 ISA that hipcc emits for the shipped source (no GPU needed), by
the method of tests/test_graph_resources.py: what include/orbm.h states for them."""
import re

from test_kernel_resources import _isa, _kernels

# kernel -> static LDS bytes, as include/orbm.h states them
STATED = {"k_local_map": 33412, "k_track_counters": 0, "k_num_tracked": 0}


def test_the_local_map_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Three kernels, the ones the header names.  No scratch memory anywhere; within 64 VGPRs (k_local_map is a workgroup of sixteen
    waves: 128 is all a thread could have); static LDS as stated: in k_local_map the 4096 votes and the 4096 list entries (16 KB each),
    their 4096 mark bits, the scan's slots and the counters."""
    k = _kernels(_isa("orbm_localmap"))
    header = open(__file__.replace("tests/test_local_map_resources.py", "include/orbm.h")).read()
    header = re.sub(r"\s*\n \* ", " ", header)                       # the comment's line breaks
    assert len(k) == len(STATED), sorted(k)
    for name, lds_stated in STATED.items():
        mangled = [m for m in k if name in m]
        assert len(mangled) == 1, (name, sorted(k))
        vgpr, scratch, lds = k[mangled[0]]
        print(name, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0 and vgpr <= 64 and lds == lds_stated
        assert "%s %d / 0 / %d B" % (name, vgpr, lds) in header, name
