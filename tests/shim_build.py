"""The one place that builds what the tests compile for themselves: the host shims (tests/host_shim/<name>_shim.cpp, the shipped
headers compiled by g++ into build/lib<name>_shim.so and loaded with ctypes), the device shims (tests/device_shim/*.hip, compiled
for gfx950 with the product's flags) and the stand-alone check programs that run under the host sanitizers.

One staleness rule for all of them, the one build_hip applies to the product's own units: a target is stale when it is missing, or
older than its source or than ANY *.h of ginger-lib_amd/csrc, include or tests/host_shim.  That is coarser than exact dependencies
on purpose: it needs no list that somebody can forget (tests/test_shim_build.py checks, with the compiler's own -MM, that no
program reads a header from anywhere else), and the device compiles write no depfile.  Every compile goes through
__graft_entry__._run with stamp=, so a source edited while the compiler runs leaves the target stale, and the command and its
output land in build/<target>.log.

The sanitizers run stand-alone programs only: nothing sanitised is ever loaded into python."""
import ctypes
import functools
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
# build() imports this module too; when __graft_entry__.py is the program itself it is __main__ there and is loaded a second time
# under its own name here, which is harmless: only constants and functions without state are taken from it
from __graft_entry__ import BUILD, CSRC, HIPCC_FLAGS, _newer, _run      # noqa: E402

HOST = os.path.join(ROOT, "tests", "host_shim")
DEVICE = os.path.join(ROOT, "tests", "device_shim")
WATCHED = (CSRC, os.path.join(ROOT, "include"), HOST)

# name -> what build() says once it has compiled tests/host_shim/<name>_shim.cpp (aff: .hip, the host half through hipcc)
HOST_SHIMS = {
    "fp29": "host shim", "fp29_lazy": "lazy host shim", "poseidon": "poseidon host shim", "schnorr": "schnorr host shim",
    "pairing": "pairing host shim", "gm17": "gm17 host shim", "points": "points host shim", "r1cs": "r1cs host shim",
    "sap": "sap host shim", "pedersen": "pedersen host shim", "poly": "polynomial host shim", "msm_host": "msm host shim",
    "aff": "affine rounds host shim",
}
# the stand-alone programs of tests/host_shim that run under the host sanitizers -> their compiler
CHECKS = {"points_check.cpp": "g++", "r1cs_check.cpp": "g++", "sap_check.cpp": "g++", "poly_check.cpp": "g++",
          "gm17_sum_check.cpp": "g++", "fp29_lazy_shim.cpp": "g++", "unit_host_check.cpp": "hipcc"}
DEVICE_SHIMS = ("tower_ops.hip", "msm_stages.hip", "msm_reduce.hip")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def headers(dirs=WATCHED):
    return [os.path.join(d, f) for d in dirs for f in sorted(os.listdir(d)) if f.endswith(".h")]


def stale(target, source, dirs=WATCHED):
    return not _newer(target, [source] + headers(dirs))


def _compile(cmd, target):
    """-> seconds spent compiling"""
    os.makedirs(BUILD, exist_ok=True)
    os.makedirs(os.path.dirname(target), exist_ok=True)
    return _run(cmd, os.path.join(BUILD, os.path.basename(target) + ".log"), target)


def host_shim_source(name):
    return os.path.join(HOST, name + ("_shim.hip" if name == "aff" else "_shim.cpp"))


def _host_compiler(source):
    if source.endswith(".hip") or CHECKS.get(os.path.basename(source)) == "hipcc":
        return ["hipcc", "--offload-host-only", "-Wno-unused-result"]
    return ["g++"]


def build_host_shim(name):
    """build/lib<name>_shim.so -> seconds spent compiling (0.0: up to date)"""
    assert name in HOST_SHIMS, name
    src, so = host_shim_source(name), os.path.join(BUILD, "lib%s_shim.so" % name)
    if not stale(so, src):
        return 0.0
    return _compile(_host_compiler(src) + ["-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, src], so)


@functools.lru_cache(maxsize=None)
def host_shim(name):
    """the loaded shim, one per process: every test file that uses it sets the argtypes of what it calls"""
    build_host_shim(name)
    return ctypes.CDLL(os.path.join(BUILD, "lib%s_shim.so" % name))


def device_shim(src, out, extra_flags=(), genco=False):
    """tests/device_shim/<src> for gfx950 with the product's flags: a shared object, or with genco a bare code object
    -> seconds spent compiling (0.0: up to date)"""
    assert src in DEVICE_SHIMS, src
    src = os.path.join(DEVICE, src)
    if not stale(out, src):
        return 0.0
    return _compile(["hipcc"] + HIPCC_FLAGS + list(extra_flags) + ["--genco" if genco else "-shared", src, "-o", out], out)


def sanitized_check(source, exe, defines=()):
    """tests/host_shim/<source> as a program of its own under the address and undefined-behaviour sanitizers, built when stale and
    run once -> the completed process (stdout and stderr as text)"""
    assert source in CHECKS, source
    src = os.path.join(HOST, source)
    if stale(exe, src):
        flags = SANITIZE
        if CHECKS[source] == "hipcc":
            flags = ["--offload-arch=gfx950"] + [x for f in SANITIZE for x in ("-Xarch_host", f)]
        _compile([CHECKS[source], "-O1", "-g", "-std=c++17"] + flags + ["-D" + d for d in defines] + [src, "-o", exe], exe)
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def dependencies(source):
    """the files of this repository that the compiler reads for `source` (-MM; its own toolchain's headers left out)"""
    out = subprocess.run(_host_compiler(source) + ["-std=c++17", "-MM", source], capture_output=True, text=True, check=True).stdout
    words = out.replace("\\\n", " ").split()[1:]
    return [p for p in (os.path.realpath(w) for w in words) if p.startswith(ROOT + os.sep)]
