"""Loader for the host index model of ntt_polymul_dot_pre (tests/emu/emu_product_dot.cpp) -- test infrastructure, built the
way emu_lib.py builds its library."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_product_dot.cpp")
OUT = os.path.join(HERE, "emu", "libntt_emu_product_dot.so")
CSRC = os.path.join(os.path.dirname(HERE), "ntt_aie_amd", "csrc")

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(HERE, "emu", "emu_exec.h")] + [os.path.join(CSRC, f) for f in ("pass.h", "field.h", "plan.h", "launch.h", "sequence.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", OUT])
        L = C.CDLL(OUT)
        u32 = C.c_uint32
        L.emu_polymul_dot.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, u32, u32, C.c_void_p, u32, u32, C.c_int]
        L.emu_polymul_dot_sequence.argtypes = [C.c_int, C.c_int, C.c_uint64, u32, u32, u32, C.c_int, u32, C.POINTER(C.c_int), C.c_int]
        L.emu_polymul_dot_alternatives.argtypes = [C.c_int, C.c_int, C.c_uint64]
        L.emu_polymul_dot_fused.argtypes = [C.c_int, C.c_int, C.c_uint64, u32, u32, C.c_int]
        _lib = L
    return _lib
