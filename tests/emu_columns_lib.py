"""Loader for the host index model of ntt_forward_columns / ntt_inverse_columns (tests/emu/emu_columns.cpp) -- test infrastructure,
built the way emu_lde_lib.py builds its library."""
import ctypes as C
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_columns.cpp")
OUT = os.path.join(HERE, "emu", "libntt_emu_columns.so")
CSRC = os.path.join(os.path.dirname(HERE), "ntt_aie_amd", "csrc")

_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(HERE, "emu", "emu_exec.h")] + [os.path.join(CSRC, f) for f in ("pass.h", "field.h", "plan.h", "launch.h", "sequence.h")]
        if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", SRC, "-o", OUT])
        L = C.CDLL(OUT)
        L.emu_columns.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                  C.c_int, C.c_uint32]
        L.emu_column_passes.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int]
        L.emu_columns_geometry.argtypes = [C.c_int, C.c_uint64, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                           C.POINTER(C.c_uint32)]
        _lib = L
    return _lib


def geometry(word_bytes, p, logn, width, pitch, count, target, k, inverse=False):
    """what launch.h's mat_dispatch + pass_geometry_of give for pass k of plan_column_passes(logn) of a columns call on this shape"""
    v = (C.c_uint32 * 8)()
    rc = lib().emu_columns_geometry(word_bytes, p, logn, width, pitch, count, target, k, int(inverse), v)
    assert rc == 0, rc
    return {"grid_x": v[0], "grid_y": v[1], "ppw": v[2], "log_up": v[3], "taper": list(v[4:8])}


def column_passes(logn):
    """[(first stage, stages)] of plan.h's plan_column_passes(logn)"""
    s0, lm = (C.c_int * 8)(), (C.c_int * 8)()
    k = lib().emu_column_passes(logn, s0, lm, 8)
    assert 0 <= k <= 8
    return [(s0[i], lm[i]) for i in range(k)]
