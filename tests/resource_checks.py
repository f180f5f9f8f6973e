"""What the no-GPU kernel-resource tests (tests/test_*_resources.py) share: the gfx950 ISA that hipcc emits for a shipped source, the
figures of its kernels, the check that they are the ones a header states, and the two "written once" patterns."""
import hashlib
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "monoorbslam3_amd", "csrc")
FLAGS = ["-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "--offload-arch=gfx950", "-mllvm",
         "-amdgpu-mfma-vgpr-form=1", "--cuda-device-only", "-S"]


def _isa(source="orbx_kernels"):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not found")
    h = hashlib.sha256()
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h")):
            h.update(open(os.path.join(CSRC, f), "rb").read())
    out_dir = os.path.join(ROOT, "build", "isa")
    os.makedirs(out_dir, exist_ok=True)
    out = os.path.join(out_dir, "%s_%s.s" % (source, h.hexdigest()[:16]))
    if not os.path.exists(out):
        subprocess.run([hipcc] + FLAGS + ["-o", out, os.path.join(CSRC, source + ".hip")], check=True, cwd=CSRC,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def _kernels(isa):
    """mangled name -> (VGPRs, scratch bytes, static LDS bytes)"""
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", isa, re.S):
        body = m.group(2)
        out[m.group(1)] = (int(re.search(r"\.amdhsa_next_free_vgpr (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body).group(1)),
                           int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body).group(1)))
    return out


def source(name):
    return open(os.path.join(CSRC, name)).read()


def stated(src, header_name, table, vgpr_bound, match="substring", breaks=r"\s*\n \* +"):
    """The kernels of csrc/<src>.hip are the keys of `table` (key -> static LDS bytes as include/<header_name> states them, or -> (the
    header's name for the kernel, those bytes)), one mangled name each -- the key a substring of it, or with match="exact" the whole
    identifier --; none uses scratch memory; each stays within vgpr_bound, a number or a function of the key; its static LDS is the stated;
    and the header has the line "<name> <VGPRs> / 0 / <LDS> B", `breaks` being how the header's comment is joined into one line."""
    k = _kernels(_isa(src))
    header = re.sub(breaks, " ", open(os.path.join(ROOT, "include", header_name)).read())
    assert len(k) == len(table), sorted(k)
    for key, lds_stated in table.items():
        name, lds_stated = lds_stated if isinstance(lds_stated, tuple) else (key, lds_stated)
        mangled = [m for m in k if (re.search(r"\d%sE" % key, m) if match == "exact" else key in m)]
        assert len(mangled) == 1, (key, sorted(k))
        vgpr, scratch, lds = k[mangled[0]]
        print(name, "VGPRs", vgpr, "scratch", scratch, "static LDS", lds)
        assert scratch == 0 and vgpr <= (vgpr_bound(key) if callable(vgpr_bound) else vgpr_bound) and lds == lds_stated, key
        assert "%s %d / 0 / %d B" % (name, vgpr, lds) in header, name


def defined_once(text, fn, qualifier="__device__ __forceinline__"):
    """a shared header defines fn exactly once, at the start of a line, with this qualifier"""
    return len(re.findall(r"^%s \w+ %s\(" % (qualifier, fn), text, re.M)) == 1


def defines_itself(text, fn):
    """a source has a definition of fn of its own"""
    return bool(re.search(r"^\s*(?:__device__ |static |inline )[\w ]*\b%s\(" % fn, text, re.M))


def used_not_defined(text, fn):
    """a source calls fn (a template argument list allowed) and has no definition of its own"""
    return bool(re.search(r"\b%s(?:<\d+>)?\(" % fn, text)) and not defines_itself(text, fn)
