"""Kernel resources of the observation kernels, read from the gfx950 ISA that hipcc emits for the shipped source (no GPU needed), by
the method of tests/test_kernel_resources.py: what include/orbm.h states for them."""
from resource_checks import _isa, _kernels


def test_observation_kernels_use_no_scratch_memory():
    """Five kernels build the CSR (the slot walk is one template, counting and scattering) and one culls.  None uses scratch memory;
    static LDS is the scan's 72 B (sixteen wave sums, two counters) and the culling's 40 B (eight counters, numMP, numRedundant) --
    its claim mask is dynamic LDS --, nothing elsewhere; the build stays within 32 VGPRs, the culling within 64 (sixteen waves in one
    workgroup: 128 is all a thread could have)."""
    k = _kernels(_isa("orbm_observations"))
    names = sorted(k)
    keys = ("k_obs_clear", "k_obs_slotsILb0", "k_obs_slotsILb1", "k_obs_scan", "k_obs_sort", "k_cull")
    assert len(k) == 6 and all(any(key in n for n in names) for key in keys), names
    for name, (vgpr, scratch, lds) in k.items():
        print(name, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0
        if "k_cull" in name:
            assert lds == 40 and vgpr <= 64
        elif "k_obs_scan" in name:
            assert lds == 72 and vgpr <= 32
        else:
            assert lds == 0 and vgpr <= 32
