"""Loader for the host index model of ntt_polymul_gadget_pre (tests/emu/emu_product_gadget.cpp) -- test infrastructure, built the
way emu_lib.py builds its library."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_product_gadget.cpp")
OUT = os.path.join(HERE, "emu", "libntt_emu_product_gadget.so")
CSRC = os.path.join(os.path.dirname(HERE), "ntt_aie_amd", "csrc")

OUT_EXP = os.path.join(HERE, "emu", "libntt_emu_product_gadget_exp.so")

_libs = {}


def lib(experiment=False):
    """experiment: the model of the EXPERIMENT build (-DNTT_EXPERIMENT), which keeps the Goldilocks and 4-byte digit kernels the product
    library does not use (launch.h: product_gadget_unit) -- those two classes only, the general 64-bit modulus is the same code in both"""
    if experiment not in _libs:
        out, flags = (OUT_EXP, ["-DNTT_EXPERIMENT", "-DEMU_PRODUCT_GADGET_FIELDS=5"]) if experiment else (OUT, [])
        deps = [SRC, os.path.join(HERE, "emu", "emu_exec.h")] + [os.path.join(CSRC, f) for f in ("pass.h", "field.h", "plan.h", "launch.h", "sequence.h")]
        if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", *flags, SRC, "-o", out])
        L = C.CDLL(out)
        u32, u64, i, vp = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p
        L.emu_polymul_gadget.argtypes = [i, i, u64, vp, vp, u32, i, i, i, vp, vp, u32, u32, vp, u32, u32, i, i, i]
        L.emu_polymul_gadget_sequence.argtypes = [i, i, u64, u32, u32, u32, i, i, i, u32, i, u32, i, i, C.POINTER(i), i]
        L.emu_polymul_gadget_alternatives.argtypes = [i, i, u64]
        L.emu_polymul_gadget_fused.argtypes = [i, i, u64, u32, u32, i, i]
        L.emu_gadget_params_ok.argtypes = [u64, i, i, i]
        L.emu_gadget_digits.argtypes = [i, u64, vp, u64, u64, i, i, i, vp]
        _libs[experiment] = L
    return _libs[experiment]
