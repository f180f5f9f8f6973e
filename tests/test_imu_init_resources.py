"""Kernel resources of the IMU initialisation's steps (csrc/orbii.hip) and of the map rescale (csrc/orbm_rescale.hip), read from the gfx950
ISA that hipcc emits for the shipped sources (no GPU needed), by the method of tests/test_vi_resources.py: what include/orbii.h and
include/orbm.h state.  Nothing else is read from the ISA."""
from resource_checks import defined_once, source, stated, used_not_defined

# kernel (substring of the mangled name) -> (static LDS bytes as the header states them, threads of its workgroup)
STATED = {
    "orbii": ("orbii.h", {"k_ii_prior": (5748, 64), "k_ii_init": (256, 256), "k_ii_edge": (20608, 256), "k_ii_assemble": (0, 256), "k_ii_damp": (0, 256),
                          "k_ii_oplus": (0, 256), "k_ii_recover": (256, 256)}),
    "orbm_rescale": ("orbm.h", {"k_rescale_begin": (0, 64), "k_rescale_kf": (768, 256), "k_rescale_points": (4, 256)}),
}


def test_the_kernels_use_no_scratch_memory_and_the_lds_the_headers_state():
    """No scratch memory; at most 128 VGPRs, the bound of the sister tests -- a 64- or 256-thread workgroup puts one wave on a SIMD, whose
    lanes have 512, so four workgroups still fit beside each other; static LDS as stated: k_ii_edge four wave slices of 574 doubles and 140
    floats, k_ii_prior 157 x (two ints and seven floats) and twenty more words, k_rescale_kf four wave slices of 48 floats; k_ii_init and
    k_ii_recover hold the 256 bytes of their workgroup count."""
    assert STATED["orbii"][1]["k_ii_edge"][0] == 4 * (574 * 8 + 140 * 4) and STATED["orbii"][1]["k_ii_prior"][0] == 157 * 9 * 4 + (8 + 3 + 9) * 4 + 16
    assert STATED["orbm_rescale"][1]["k_rescale_kf"][0] == 4 * 48 * 4
    for src, (header_name, table) in STATED.items():
        assert all(threads in (64, 256) for _, threads in table.values())
        stated(src, header_name, {key: lds for key, (lds, _) in table.items()}, 128)


def test_the_so3_code_is_written_once():
    """orbii.hip and orbi_factors.hip take what their edges share behind the cast to double (the prologue, the widening, the rotation
    residual, Omega*e with chi2, the quadratic form) from csrc/orbi_edge.h, which takes LogSO3 and the two Jacobians from csrc/orbi_so3d.h;
    both take ExpSO3 from there, the float part of an edge (bias_deltas) from csrc/orbi_so3.h and the duplicate scan over a job list from
    csrc/orbi_graph_device.h; orbm_rescale.hip and orbi_imu.hip take T_wb = T_cw.inverse() * T_cb from orbi_so3.h.  None defines them
    itself, and no scan is written out."""
    d, f, e, g = source("orbi_so3d.h"), source("orbi_so3.h"), source("orbi_edge.h"), source("orbi_graph_device.h")
    for fn in ("dlog_so3", "dright_jacobian", "dinverse_right_jacobian", "dexp_so3", "dnormalize", "dm3", "dcof"):
        assert defined_once(d, fn), fn
    for fn in ("bias_deltas", "imu_pose_from_camera"):
        assert defined_once(f, fn), fn
    edge_fns = ("edge_refused", "edge_load", "edge_widen", "edge_rotation", "edge_chi2", "edge_jtwj", "edge_quadratic_form")
    for fn in edge_fns:
        assert defined_once(e, fn), fn
    assert defined_once(g, "job_named_before")
    for src, header, fns in (("orbi_edge.h", "orbi_so3d.h", ("dlog_so3", "dright_jacobian", "dinverse_right_jacobian")),
                             ("orbii.hip", "orbi_so3d.h", ("dexp_so3", "bias_deltas")), ("orbi_factors.hip", "orbi_so3d.h", ("dexp_so3", "bias_deltas")),
                             ("orbii.hip", "orbi_edge.h", [fn for fn in edge_fns if fn != "edge_jtwj"]), ("orbi_factors.hip", "orbi_edge.h", edge_fns),
                             ("orbii.hip", "orbi_graph_device.h", ("job_named_before",)), ("orbi_factors.hip", "orbi_graph_device.h", ("job_named_before",)),
                             ("orbm_rescale.hip", "orbi_so3.h", ("imu_pose_from_camera",)), ("orbi_imu.hip", "orbi_so3.h", ("imu_pose_from_camera",))):
        text = source(src)
        assert '#include "%s"' % header in text, src
        for fn in fns:
            assert used_not_defined(text, fn), (src, fn)
    assert "orbii.hip" in source("Makefile")
