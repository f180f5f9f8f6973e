"""Kernel resources of the refresh kernels, read from the gfx950 ISA that hipcc emits for the shipped source (no GPU needed), by the
method of tests/test_kernel_resources.py."""
from resource_checks import _isa, _kernels


def test_refresh_kernels_use_no_scratch_memory():
    """k_refresh keeps a row's descriptor and its eight counters in registers (constant indices only) and its tile of 64
    descriptors in a per-wave slice of LDS: no scratch, and the static LDS per workgroup is what the header states."""
    k = _kernels(_isa("orbm_refresh"))
    names = sorted(k)
    assert len(k) == 3 and all(any(key in n for n in names) for key in ("k_refresh_clear", "k_refreshE", "k_median_depth")), names
    for name, (vgpr, scratch, lds) in k.items():
        print(name, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0
        if "k_refreshE" in name:
            assert lds == 4 * 64 * 32 and vgpr <= 64          # four waves' tiles; eight waves per SIMD
        if "k_median_depth" in name:
            assert 8192 * 4 <= lds <= 40 * 1024                # the keys of ORBM_MEDIAN_MAX_STRIDE slots, the histogram
