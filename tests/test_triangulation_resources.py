"""Kernel resources of the triangulation kernel, read from the gfx950 ISA that hipcc emits for the shipped source (no GPU needed),
by the method of tests/test_kernel_resources.py."""
from resource_checks import _isa, _kernels


def test_k_triangulate_uses_no_scratch_memory():
    """The 4x4 matrix, V and both poses live in registers through the fully index-constant Jacobi sweeps: no scratch, and at 1024
    threads per workgroup 128 VGPRs is all a thread can have."""
    k = {name: v for name, v in _kernels(_isa("orbm_triangulate")).items() if "k_triangulate" in name}
    assert len(k) == 1, sorted(k)
    for name, (vgpr, scratch, lds) in k.items():
        print(name, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0 and vgpr <= 128


def test_moving_project_into_a_header_left_the_builders_without_scratch():
    k = {name: v for name, v in _kernels(_isa("orbm_project")).items() if "k_project" in name}
    assert len(k) == 3 and all(v[1] == 0 for v in k.values())
