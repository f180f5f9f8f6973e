"""Kernel resources of the IMU preintegration and pose prediction, read from the gfx950 ISA that hipcc emits for the shipped source (no
GPU needed), by the method of tests/test_keyframe_resources.py: what include/orbi.h states for them."""
from resource_checks import stated

# kernel (substring of the mangled name) -> (the header's name for it, static LDS bytes as include/orbi.h states them)
STATED = {"k_imuILi0E": ("k_imu<reset>", 32), "k_imuILi1E": ("k_imu<integrate>", 12368), "k_imuILi2E": ("k_imu<set_bias>", 12368),
          "k_imuILi3E": ("k_imu<merge>", 12368), "k_imu_predict": ("k_imu_predict", 688), "k_imu_pose": ("k_imu_pose", 124),
          "k_counters_clear": ("k_counters_clear", 0)}


def test_the_imu_kernels_use_no_scratch_memory_and_the_lds_the_header_states():
    """Seven kernels, the ones the header names.  No scratch memory anywhere; within 128 VGPRs (a workgroup is four waves, one per
    SIMD: nothing competes for the register file, but a spill would put the record's matrices behind global memory); static LDS as
    stated: four wave slices of 768 words (the record's image, the 9x9 intermediate, thirteen 3x3 temporaries, 33 staged samples), the
    calibration's twelve floats and the eight counters.  No dynamic LDS."""
    stated("orbi_imu", "orbi.h", STATED, 128, breaks=r"\s*\n \* ")
