"""The kernels' .hip sources as host C++ (tests/hip_emu/README.md): the one builder behind every tests/test_*_emulated.py and behind
the stand-alone sanitizer programs tests/hip_emu/*_sanitize_main.cpp.

    python tests/hip_emu_build.py frame_filter [-DFF_EMU_LDS_BYTES=2048] [arguments of the program]

builds tests/hip_emu/frame_filter_sanitize_main.cpp around the emulated kernel with -fsanitize=address,undefined and runs it."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.join(os.path.dirname(HERE), "vsc22-submission_amd")
CSRC = os.path.join(PKG, "csrc")
EMU = os.path.join(HERE, "hip_emu")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

from vsc_hip._lib import SIGNATURES  # noqa: E402

# name -> (sources of one translation unit, the header that stands in for csrc/common.h, the name of the dynamic LDS or None)
KERNELS = {
    "match_segments": (("match_segments.hip",), "common.h", "ms_smem"),
    "match_maps": (("match_maps.hip",), "common.h", None),
    "segment_metric": (("segment_metric.hip",), "common.h", None),
    "score_norm": (("score_norm.hip",), "common.h", None),
    "uap": (("uap.hip",), "common.h", None),
    "global_topk": (("global_topk.hip",), "common.h", None),
    "frame_filter": (("frame_filter.hip",), "frame_filter.h", "ff_smem"),
    "view_decide": (("view_decide.hip",), "view_decide.h", "vd_smem"),
    "frame_inputs": (("frame_inputs.hip",), "frame_inputs.h", "fi_smem"),
    "jpeg_decode": (("jpeg_decode.hip",), "jpeg_decode.h", None),
    "jpeg_split": (("jpeg_decode.hip", "jpeg_split.hip"), "jpeg_decode.h", None),      # both entries, one handle type
}
COUNTERS = ("emu_launches", "emu_blocks", "emu_allocs", "emu_scratch_allocs", "emu_scratch_bytes", "emu_coeff_tables")
# stands where a source had `#pragma clang fp contract(off)`: such a source is compiled with -ffp-contract=off
FP_CONTRACT_OFF = "// (emulated: -ffp-contract=off on the command line)\n"
LDS_LINE = r"^( *)extern __shared__ __align__\(16\) unsigned char (\w+)\[\];\n"


def compiler():
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    assert shutil.which(cxx) or os.path.exists(cxx), "no host C++ compiler (g++ / clang++) for the emulated kernel"
    return cxx


def emulated_source(*kernels, header="common.h", lds=None):
    """csrc/<kernel> for the host, several joined into one translation unit: `#include "common.h"` names tests/hip_emu/<header>,
    the fp-contract pragma becomes a compiler flag, and the dynamic LDS `lds` (None: the kernels declare none) is the shim's
    buffer.  Line numbers stay those of the .hip file."""
    out, found = [], []
    for kernel in kernels:
        src = open(os.path.join(CSRC, kernel)).read()
        src, n = re.subn(r'^#include "common.h"\n', f'#include "{header}"\n', src, flags=re.M)
        assert n == 1, f"{kernel} no longer has the line the emulation replaces"
        src, n = re.subn(r"^#pragma clang fp contract\(off\)\n", FP_CONTRACT_OFF, src, flags=re.M)
        assert n <= 1, kernel
        found += [m[1] for m in re.findall(LDS_LINE, src, flags=re.M)]
        out.append(re.sub(LDS_LINE, r"\1unsigned char *const \2 = emu_lds;\n", src, flags=re.M))
    assert found == ([lds] if lds else []), f"{kernels}: dynamic LDS {found}, expected {lds}"
    return "\n".join(out)


def source(name):
    kernels, header, lds = KERNELS[name]
    return emulated_source(*kernels, header=header, lds=lds)


def _compile(source, src, out, flags, defines):
    """the one compile line, for the file `src` that is or includes the emulated `source`; tests/hip_emu goes in front of csrc,
    whose common.h is the device's"""
    contract = ["-ffp-contract=off"] if FP_CONTRACT_OFF in source else []
    subprocess.check_call([compiler(), "-std=c++20", "-pthread", "-Wno-unknown-pragmas", *contract, *flags, *defines, "-I", EMU, "-I", CSRC,
                           "-o", out, src])
    return out


def build_shared(tmp_path_factory, tag, source, defines=()):
    """-> the emulated kernel as a ctypes.CDLL, its entries bound"""
    work = tmp_path_factory.mktemp("hip_emu_" + tag)
    (work / (tag + ".cpp")).write_text(source)
    return bind(ctypes.CDLL(_compile(source, str(work / (tag + ".cpp")), str(work / f"lib{tag}_emu.so"), ["-O2", "-fPIC", "-shared"], defines)))


def build_sanitized(workdir, source, main_cpp, defines=()):
    """-> the path of a stand-alone program: tests/hip_emu/<name>_sanitize_main.cpp, which includes `source` as <name>_emu.inc,
    under the address and undefined-behaviour sanitizers.  It is run as a process of its own; nothing sanitized is loaded into Python."""
    with open(os.path.join(str(workdir), main_cpp.replace("_sanitize_main.cpp", "_emu.inc")), "w") as f:
        f.write(source)
    # the runtimes inside the program: no load order to get wrong
    static = ["-static-libasan", "-static-libubsan"] if os.path.basename(compiler()).startswith("g++") else []
    return _compile(source, os.path.join(EMU, main_cpp), os.path.join(str(workdir), main_cpp.replace("_sanitize_main.cpp", "_san")),
                    ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", *static, "-I", str(workdir)], defines)


def bind(lib):
    """restype / argtypes of every vsc_* entry the library exports, from the table the real library is bound by, and of the
    emulation's counters"""
    for name, (res, args) in SIGNATURES.items():
        if hasattr(lib, name):
            getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    for name in COUNTERS:
        if hasattr(lib, name):
            getattr(lib, name).restype = ctypes.c_size_t
    lib.emu_scratch_bytes.argtypes = [ctypes.c_int]
    return lib


def guarded(count, dtype=np.uint8, guard=8, fill=0xFF):
    """(buffer, view of `count` elements filled with the byte `fill`) with `guard` elements of 0xFF bytes on both sides: -1 as an
    integer, NaN as a float; an odd guard of bytes puts the view at an odd address"""
    size = np.dtype(dtype).itemsize
    raw = np.full((count + 2 * guard) * size, 0xFF, np.uint8)
    raw[guard * size:(guard + count) * size] = fill
    buf = raw.view(dtype)
    return buf, buf[guard:guard + count]


def guards_intact(buf, guard=8):
    raw, g = buf.view(np.uint8), guard * buf.dtype.itemsize
    return bool((raw[:g] == 0xFF).all() and (raw[len(raw) - g:] == 0xFF).all())


if __name__ == "__main__":
    name, rest = sys.argv[1], sys.argv[2:]
    with tempfile.TemporaryDirectory() as work:
        exe = build_sanitized(work, source(name), name + "_sanitize_main.cpp", [a for a in rest if a.startswith("-D")])
        sys.exit(subprocess.call([exe, *(a for a in rest if not a.startswith("-D"))]))
