"""Kernel resources of the local bundle adjustment's assembly and apply, read from the gfx950 ISA that hipcc emits for the shipped source
(no GPU needed), by the method of tests/test_fuse_resources.py: what include/orbm.h states for them."""
from resource_checks import _isa, _kernels


def test_the_local_ba_kernels_use_no_scratch_memory_and_fit_sixteen_waves():
    """Two kernels of sixteen waves each (128 VGPRs is all a thread could have).  No scratch memory; within 64 VGPRs, as the header
    states (the compiler gives 63 and 55); static LDS 4288 B in the assembly (the kept local key frames, 2 x 16 wave totals, sixteen
    counters) and 32 B in the apply (eight counters)."""
    k = _kernels(_isa("orbm_localba"))
    assert len(k) == 2, sorted(k)
    lds = {"k_lba_problem": 4288, "k_lba_apply": 32}
    for name, (vgpr, scratch, static_lds) in k.items():
        print(name, "VGPRs", vgpr, "scratch", scratch, "static LDS", static_lds)
        want = next(v for key, v in lds.items() if key in name)
        assert scratch == 0 and static_lds == want and vgpr <= 64
