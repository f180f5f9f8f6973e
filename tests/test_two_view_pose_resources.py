"""Kernel resources of the two-view pose recovery, read from the gfx950 ISA that hipcc emits for the shipped source (no GPU needed), by the
method of tests/test_two_view_resources.py: what include/orbm.h states for them."""
from resource_checks import defined_once, source, stated, used_not_defined

# kernel -> static LDS bytes, as include/orbm.h states them
STATED = {"k_tvp_decompose": 0, "k_tvp_check": 1104, "k_tvp_decide": 8}


def test_the_pose_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Three kernels, the ones the header names.  No scratch memory anywhere -- the 3 x 3 and 4 x 4 Jacobi and the eight hypotheses are
    indexed by constants --; k_tvp_check and k_tvp_decide within 128 VGPRs (workgroups of sixteen waves: 128 is all a thread could
    have), k_tvp_decompose, a single wave, within 256.  Static LDS as stated: the 256-bin histogram of the select, the sixteen slots
    of its scan, the two counters and the chosen digit in k_tvp_check; the two counters in k_tvp_decide."""
    stated("orbm_two_view_pose", "orbm.h", STATED, lambda k: 256 if k == "k_tvp_decompose" else 128)


def test_the_jacobi_steps_are_written_once():
    """rotate / dot4 (Triangulate's 4 x 4) and jacobi_cs / rotate3 / dot3 (the 3 x 3 in double) live in csrc/orbm_jacobi.h; the
    triangulation, the RANSAC and the pose recovery use them and define none of their own"""
    shared = source("orbm_jacobi.h")
    for fn in ("rotate", "dot4", "jacobi_cs", "rotate3", "dot3"):
        assert defined_once(shared, fn), fn
    for src, fns in (("orbm_triangulate.hip", ("rotate", "dot4")), ("orbm_two_view.hip", ("jacobi_cs", "rotate3", "dot3")),
                     ("orbm_two_view_pose.hip", ("rotate", "dot4", "rotate3", "dot3"))):
        text = source(src)
        for fn in fns:
            assert used_not_defined(text, fn), (src, fn)
