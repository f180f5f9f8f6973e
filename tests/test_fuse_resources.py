"""Kernel resources of the fuse's hit handling, read from the gfx950 ISA that hipcc emits for the shipped source (no GPU needed), by
the method of tests/test_kernel_resources.py: what include/orbm.h states for it."""
from resource_checks import _isa, _kernels


def test_the_fuse_kernel_uses_no_scratch_memory_and_fits_sixteen_waves():
    """One kernel.  No scratch memory; static LDS 1064 B (one bit per slot of a key frame of 8192 slots, eight counters, the two
    refusal flags) -- the row mask and the slot heads are dynamic LDS --; within 64 VGPRs, as the header states (the compiler gives 40;
    sixteen waves in one workgroup: 128 is all a thread could have)."""
    k = _kernels(_isa("orbm_fuse"))
    assert len(k) == 1 and "k_fuse_apply" in next(iter(k)), sorted(k)
    for name, (vgpr, scratch, lds) in k.items():
        print(name, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0 and lds == 1064 and vgpr <= 64
