"""Loader for the in-tree HIP library (monoorbslam3_amd/lib/liborbx.so).

There is no Python or CPU fallback: if the shared library is missing or a symbol
is absent the import fails loudly.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liborbx.so")

MAX_LEVELS = 16


class OrbxCfg(C.Structure):
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("ini_th_fast", C.c_int32), ("min_th_fast", C.c_int32), ("max_width", C.c_int32),
                ("max_height", C.c_int32), ("max_batch", C.c_int32), ("blur_variant", C.c_int32),
                ("device", C.c_int32)]


class OrbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbx error %d: %s" % (code, msg))
        self.code = code


def binder(sigs, load=None):
    """The bind-once accessor of a module's entry points: sigs maps a name to its argtypes (restype c_int) or to (restype, argtypes).
    The first call loads the library (`load`, by default lib()) and sets every signature -- a name the library does not export raises
    AttributeError there, and the next call tries again; every later call returns the same library and sets nothing."""
    bound = []

    def get():
        if not bound:
            L = (load or lib)()
            for name, sig in sigs.items():
                fn = getattr(L, name)  # AttributeError if the library does not export it
                fn.restype, fn.argtypes = sig if isinstance(sig, tuple) else (C.c_int, sig)
            bound.append(L)
        return bound[0]
    return get


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(there is no CPU fallback)" % LIB_PATH)
    # PyTorch-ROCm bundles its own libamdhip64; if liborbx.so (linked against /opt/rocm) is loaded first, the process
    # ends up with two HIP runtimes and the second one sees no device.  Importing torch first makes both share one.
    try:
        import torch  # noqa: F401
    except Exception:  # a pure C/C++ consumer without torch is fine
        pass
    return C.CDLL(LIB_PATH)


_vp, _i32, _f32, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
_SIGS = {
    "orbx_create": (_i32, [C.POINTER(OrbxCfg), C.POINTER(_vp)]),
    "orbx_create_requota": (_i32, [_vp, _i32, C.POINTER(_vp)]),
    "orbx_destroy": (None, [_vp]),
    "orbx_tables": (_i32, [_vp, C.POINTER(_i32), _vp, _vp, _vp, _vp, C.POINTER(_f32), _vp, _vp]),
    "orbx_level_size": (_i32, [_vp, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32)]),
    "orbx_max_keypoints": (_i32, [_vp, _i32, _i32]),
    "orbx_extract": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, C.POINTER(_i32)]),
    "orbx_extract_batch": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _sz, _vp, _vp, _i32, _vp]),
    "orbx_extract_batch_device": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _sz, _vp, _vp, _i32, _vp, _vp]),
    "orbx_synchronize": (_i32, [_vp]),
    "orbx_host_register": (_i32, [_vp, _sz]),
    "orbx_host_unregister": (_i32, [_vp]),
    "orbx_stream_wait_fast": (_i32, [_vp, _vp]),
    "orbx_tap_level": (_i32, [_vp, _i32, _i32, _i32, _vp, _sz]),
    "orbx_tap_candidates": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _i32, C.POINTER(_i32)]),
    "orbx_tap_level_counts": (_i32, [_vp, _i32, _vp]),
    "orbx_tap_sincos": (_i32, [_vp, _vp, _i32, _vp]),
    "orbx_set_variant": (_i32, [_vp, _i32, _i32]),
    "orbx_get_variant": (_i32, [_vp, _i32, C.POINTER(_i32)]),
    "orbx_set_stage_timing": (_i32, [_vp, _i32]),
    "orbx_fast_times_in_step_ms": (_i32, [_vp, C.POINTER(_f32), C.POINTER(_i32)]),
    "orbx_stage_times_ms": (_i32, [_vp, _vp]),
    "orbx_stage_times_in_step_ms": (_i32, [_vp, _vp]),
    "orbx_stage_groups_in_step": (_i32, [_vp, _vp]),
    "orbx_last_error": (C.c_char_p, []),
    "orbx_version": (C.c_char_p, []),
}
lib = binder(_SIGS, _load)


def check(rc):
    if rc != 0:
        raise OrbxError(rc, lib().orbx_last_error().decode("utf-8", "replace"))


def stream_arg(stream=None):
    """The `stream` argument of a *_device entry point for a wrapper call.  An explicit stream (raw hipStream_t as int) is
    passed through.  None follows torch's CURRENT stream when torch is loaded and the GPU is initialised -- inside
    `with torch.cuda.stream(s):` the call is enqueued on s, like the tensor operations around it -- and is NULL otherwise,
    which the C ABI runs on stream 0 (include/orbx.h, "Streams"); torch's default stream IS stream 0."""
    if stream is not None:
        return stream
    import sys
    torch = sys.modules.get("torch")
    if torch is not None and torch.cuda.is_initialized():
        return torch.cuda.current_stream().cuda_stream or None
    return None


def kernels_sha16():
    """First 16 hex digits of the sha256 over the kernel sources (csrc/*.hip, *.h): ties a profile to the code it measured."""
    import glob
    import hashlib
    h = hashlib.sha256()
    for f in sorted(glob.glob(os.path.join(_HERE, "csrc", "*.hip")) + glob.glob(os.path.join(_HERE, "csrc", "*.h"))):
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:16]
