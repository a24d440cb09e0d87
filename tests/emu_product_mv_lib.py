"""Loader for the host index model of ntt_polymul_matvec_pre (tests/emu/emu_product_mv.cpp) -- test infrastructure, built the
way emu_lib.py builds its library."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_product_mv.cpp")
OUT = os.path.join(HERE, "emu", "libntt_emu_product_mv.so")
CSRC = os.path.join(os.path.dirname(HERE), "ntt_aie_amd", "csrc")

OUT_EXP = os.path.join(HERE, "emu", "libntt_emu_product_mv_exp.so")

_libs = {}


def lib(experiment=False):
    """experiment: the model of the EXPERIMENT build (-DNTT_EXPERIMENT), which keeps the Goldilocks two-output kernels the product library
    does not use (launch.h: product_mv_unit) -- Goldilocks only, the other fields are the same code in both builds"""
    if experiment not in _libs:
        out, flags = (OUT_EXP, ["-DNTT_EXPERIMENT", "-DEMU_PRODUCT_MV_FIELDS=1"]) if experiment else (OUT, [])
        deps = [SRC, os.path.join(HERE, "emu", "emu_exec.h")] + [os.path.join(CSRC, f) for f in ("pass.h", "field.h", "plan.h", "launch.h", "sequence.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", *flags, SRC, "-o", out])
        L = C.CDLL(out)
        u32 = C.c_uint32
        L.emu_polymul_matvec.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, u32, u32, u32, C.c_void_p, u32, u32, C.c_int, C.c_int]
        L.emu_polymul_matvec_sequence.argtypes = [C.c_int, C.c_int, C.c_uint64, u32, u32, u32, u32, C.c_int, u32, C.c_int, C.POINTER(C.c_int), C.c_int]
        L.emu_polymul_matvec_alternatives.argtypes = [C.c_int, C.c_int, C.c_uint64]
        L.emu_polymul_matvec_fused.argtypes = [C.c_int, C.c_int, C.c_uint64, u32, u32, C.c_int]
        _libs[experiment] = L
    return _libs[experiment]
