"""tests/abi_checks.py's own: its three codes are include/orbx.h's, and the rule of the fake device pointer holds for every refusal table of
the eight ABI tests -- checked without a GPU, where a call that gets past the argument checks shows as ORBX_E_NO_DEVICE, not as a launch."""
import ctypes as C
import re

import abi_checks as abi
import test_abi
import test_ba_abi
import test_factors_abi
import test_full_inertial_abi
import test_imu_init_abi
import test_inertial_window_abi
import test_vi_abi
import test_vw_abi


def test_with_a_device_assumed_no_fake_pointer_call_passes_the_checks(monkeypatch):
    """The three codes are the header's.  Then the device probe says "present"; every table runs; every entry point of the one library is
    wrapped so that each call, through abi_checks.returns() or past it, leaves its code.  No code is ORBX_E_NO_DEVICE, which is what a call
    that would have launched on the fake pointer returns here, and the calls are exactly the rows that expect ORBX_E_ARG or
    ORBX_E_UNSUPPORTED."""
    import torch
    from monoorbslam3_amd import _lib
    defines = {name: int(value) for name, value in re.findall(r"#define (ORBX_E_[A-Z_]+) \((-\d+)\)", abi.header("orbx.h"))}
    assert (defines["ORBX_E_ARG"], defines["ORBX_E_NO_DEVICE"], defines["ORBX_E_UNSUPPORTED"]) == (abi.E_ARG, abi.E_NO_DEVICE, abi.E_UNSUPPORTED)
    mods = {name: abi.built(name) for name in ("_lib", "ba", "imu", "vi", "vw", "matcher", "imu_init", "full_inertial")}
    tables = [(test_abi.test_bad_arguments_are_rejected_before_touching_the_device, mods["_lib"]),
              (test_ba_abi.test_argument_errors_are_reported_before_the_device_is_looked_for, mods["ba"]),
              (test_factors_abi.test_argument_errors_are_reported_before_the_device_is_looked_for, mods["imu"]),
              (test_factors_abi.test_every_wrapper_fails_loudly_without_a_gpu, mods["imu"]),
              (test_vi_abi.test_argument_errors_are_reported_before_the_device_is_looked_for, mods["vi"]),
              (test_vi_abi.test_every_wrapper_fails_loudly_without_a_gpu, mods["vi"]),
              (test_vw_abi.test_argument_errors_are_reported_before_the_device_is_looked_for, mods["vw"]),
              (test_vw_abi.test_every_wrapper_fails_loudly_without_a_gpu, mods["vw"]),
              (test_inertial_window_abi.test_the_entry_points_check_their_arguments_before_any_device_call, (mods["matcher"]._mlib(), mods["matcher"])),
              (test_imu_init_abi.test_bad_arguments_are_refused_before_the_device_in_the_documented_order, mods["imu_init"]),
              (test_imu_init_abi.test_the_rescale_checks_its_arguments_before_any_device_call, mods["imu_init"]),
              (test_full_inertial_abi.test_bad_arguments_are_refused_before_the_device_in_the_documented_order, mods["full_inertial"])]
    if not torch.cuda.is_available():                           # this one keeps a skip of its own for a machine with a GPU
        tables.append((test_ba_abi.test_a_valid_call_fails_loudly_without_a_gpu, mods["ba"]))
    for name in ("ba", "imu", "vi", "vw", "imu_init", "full_inertial"):
        mods[name]._L()                                         # every signature is set before the entry points are wrapped
    L, codes = _lib.lib(), []
    for name, fn in list(vars(L).items()):
        if isinstance(fn, C._CFuncPtr) and fn.restype is C.c_int:
            monkeypatch.setattr(L, name, lambda *args, _fn=fn, _name=name: codes.append((_name, _fn(*args))) or codes[-1][1])
    rows, outcome = [], abi.outcome                             # the rows that returns() makes: with a device, the refused ones alone
    monkeypatch.setattr(abi, "outcome", lambda *args, **kwargs: rows.append(outcome(*args, **kwargs)) or rows[-1])
    monkeypatch.setattr(abi, "device_present", lambda: True)
    for test, arg in tables:
        test(arg)
    test_abi.test_every_handle_type_fails_loudly_without_a_gpu()
    passed = [(name, code) for name, code in codes if code not in (abi.E_ARG, abi.E_UNSUPPORTED)]
    assert not passed, "calls that got past the argument checks, and launch on the fake pointer where a device is: %s" % passed
    print(len(codes), "calls made")
    assert len(codes) == len(rows) > 0 and [code for _, code in codes] == [code for code, _ in rows]
