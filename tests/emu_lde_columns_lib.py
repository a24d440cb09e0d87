"""Loader for the host index model of ntt_lde_columns / ntt_coset_inverse_columns (tests/emu/emu_lde_columns.cpp) -- test
infrastructure, built the way emu_columns_lib.py builds its library."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_lde_columns.cpp")
OUT = os.path.join(HERE, "emu", "libntt_emu_lde_columns.so")
CSRC = os.path.join(os.path.dirname(HERE), "ntt_aie_amd", "csrc")

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(HERE, "emu", "emu_exec.h")] + [os.path.join(CSRC, f) for f in ("pass.h", "field.h", "plan.h", "launch.h", "sequence.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", OUT])
        L = C.CDLL(OUT)
        u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
        L.emu_lde_columns.argtypes = [C.c_int, C.c_int, u64, vp, vp, u32, vp, u32, u32, u32, C.c_int, u64, u32]
        L.emu_coset_inverse_columns.argtypes = [C.c_int, C.c_int, u64, vp, vp, vp, u32, u32, u32, u64, u32]
        _lib = L
    return _lib
