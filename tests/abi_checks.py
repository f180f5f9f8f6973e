"""What the no-GPU ABI tests (tests/test_*abi*.py) share: where the headers are and what they declare, the check that a declared name is
exported and mirrored, the library's error codes, and the ONE way to call the library with a fake device pointer.

The rule of the fake pointer.  P is an address no test owns.  An entry point may be given it only in a call that the library refuses
before it looks for the device: ORBX_E_ARG and ORBX_E_UNSUPPORTED come back with or without a GPU.  A call that passes every check goes
on to launch kernels on P wherever a device is present, so such a call is made only where none is, and must then come back with
ORBX_E_NO_DEVICE.  returns() is that rule; every call that carries P, raw or through a wrapper, goes through it, and it has no "any code
but" form.  tests/test_abi_checks.py holds the tests' tables to it without a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_ARG, E_NO_DEVICE, E_UNSUPPORTED = -1, -2, -4            # include/orbx.h's, which tests/test_abi_checks.py reads
P = 0x1000                                                # the fake device pointer


def built(module="_lib"):
    """what every ABI test's fixture does: build, then import the mirror module under test"""
    import importlib
    import __graft_entry__ as g
    g.build()
    return importlib.import_module("monoorbslam3_amd." + module)


def header(name):
    return open(os.path.join(ROOT, "include", name)).read()


def stripped(name):
    """a header without its comments"""
    return re.sub(r"/\*.*?\*/", "", header(name), flags=re.S)


def flat(path):
    """a document, or a header, on one line: the breaks of the text and of a block comment do not split a sentence"""
    return re.sub(r"\s*\n( \*)?\s*", " ", open(os.path.join(ROOT, path)).read())


def declared(prefix, name, follow_includes=False, seen=None):
    """the functions whose names begin with `prefix` (a regular expression) that a header declares, with follow_includes those of the
    headers it includes from its own directory too"""
    seen = set() if seen is None else seen
    if name in seen:
        return set()
    seen.add(name)
    txt = stripped(name)
    out = set(re.findall(r"\b(%s[a-z0-9_]+)\s*\(" % prefix, txt))
    for inc in re.findall(r'#include "([a-z_]+\.h)"', txt) if follow_includes else ():
        if os.path.exists(os.path.join(ROOT, "include", inc)):
            out |= declared(prefix, inc, True, seen)
    return out


def exported(names):
    from monoorbslam3_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    for n in sorted(names):
        assert hasattr(L, n), "liborbx.so does not export %s" % n


def exported_and_mirrored(module, prefix, names, sigs_equal):
    """every declared name is exported by the built library, listed in the mirror module's _SIGS and has a callable wrapper named without
    the prefix; with sigs_equal the module lists nothing else; the module's _L() binds every name of _SIGS (or raises) on the one library"""
    from monoorbslam3_amd import _lib
    exported(names)
    for n in sorted(names):
        assert n in module._SIGS and callable(getattr(module, n[len(prefix):])), n
    assert not sigs_equal or set(module._SIGS) == set(names), sorted(set(module._SIGS) ^ set(names))
    assert module._L() is _lib.lib()


def device_present():
    import torch
    return torch.cuda.is_available()


def outcome(call, *args, **kwargs):
    """(code, message) of a call that fails: a raw entry point returns the code and leaves the message as the library's last error, a
    wrapper raises OrbxError with both"""
    from monoorbslam3_amd import _lib
    try:
        rc = call(*args, **kwargs)
    except _lib.OrbxError as e:
        return e.code, str(e)
    assert isinstance(rc, int), "%r returned %r: a wrapper that does not raise has succeeded" % (call, rc)
    return rc, _lib.lib().orbx_last_error().decode()


def code_of(call, *args, **kwargs):
    return outcome(call, *args, **kwargs)[0]


def returns(want, call, *args, what=None, **kwargs):
    """call(*args, **kwargs) fails with `want`, one of the three codes, and leaves a message.  ORBX_E_NO_DEVICE says that the call passes
    every check: it is made only where no device is present, anywhere else it would launch on P, and the message is the missing device's.
    Returns the message of a call made, None for one not made.  `what` names the case in a failure; by default the call's name and
    the arguments that were overridden."""
    assert want in (E_ARG, E_UNSUPPORTED, E_NO_DEVICE), want
    if want == E_NO_DEVICE and device_present():
        return None
    what = what or (getattr(call, "__name__", call), list(kwargs) or args)
    got, text = outcome(call, *args, **kwargs)
    assert got == want, (what, got, want, text)
    assert text, what
    assert want != E_NO_DEVICE or "no HIP device" in text, (what, text)
    return text
