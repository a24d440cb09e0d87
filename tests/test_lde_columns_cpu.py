"""Coset LDE and coset interpolation on matrix columns without a GPU: the virtual-polynomial claim extended to the expanded, scaled
matrix (a Python-integer model, no library), the two coset twins of the matrix column pass in the host index model against the
oracle on the transposed columns, the launcher's refusals, and the part of the error contract that is reported before any launch."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

GOLD = 0xFFFFFFFF00000001
CLASSES = {"gl": (8, GOLD, 7), "m64": (8, 0xFFFFFFFC00000001, 10), "m32": (4, 998244353, 3)}


def _bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def _network(a, T, p):
    """include/ntt_hip.h: stage s = 0.., stride 2^s, (x, y) -> (x + y, (x - y) * T[n / 2^(s+1) + block])"""
    a, n = list(a), len(a)
    t = 1
    while t < n:
        h = n // (2 * t)
        for i in range(h):
            for j in range(2 * i * t, 2 * i * t + t):
                x, y = a[j], a[j + t]
                a[j], a[j + t] = (x + y) % p, (x - y) * T[h + i] % p
        t *= 2
    return a


def _inverse_network(a, Ti, p):
    """stages logn-1 .. 0, (u, v) -> (u + v * Ti, u - v * Ti), unscaled; Ti = the word-wise inverse table"""
    a, n = list(a), len(a)
    t = n // 2
    while t >= 1:
        h = n // (2 * t)
        for i in range(h):
            for j in range(2 * i * t, 2 * i * t + t):
                u, v = a[j], a[j + t] * Ti[h + i] % p
                a[j], a[j + t] = (u + v) % p, (u - v) % p
        t //= 2
    return a


def _virtual_stages(a, logn, w, T, p, inverse=False):
    """stages w .. w + logn - 1 of the size-2^(logn + w) network on `a` (descending and with the inverse butterfly when `inverse`),
    every twiddle taken from the size-2^logn table at the index the column pass forms"""
    a = list(a)
    big = 1 << (logn + w)
    for s in (reversed(range(logn)) if inverse else range(logn)):
        t = 1 << (w + s)
        blocks = big // (2 * t)
        for i in range(blocks):
            for j in range(2 * i * t, 2 * i * t + t):
                if inverse:
                    u, v = a[j], a[j + t] * T[blocks + i] % p
                    a[j], a[j + t] = (u + v) % p, (u - v) % p
                else:
                    x, y = a[j], a[j + t]
                    a[j], a[j + t] = (x + y) % p, (x - y) * T[blocks + i] % p
    return a


@pytest.mark.parametrize("p", [3329, 998244353, GOLD])
def test_the_expanded_matrix_is_one_virtual_polynomial(p):
    """the claim behind ntt_lde_columns: on the matrix [M][2^w] whose row i << beta is in[i] * s[i] (a multiplier per ROW) and whose
    other rows are zero, read as one polynomial of 2^(logn + w) words, stages w .. w + logn - 1 with the size-M table give per column
    the header's ntt_lde definition; and the same for ntt_coset_inverse_columns: the inverse stages, then row r times u[r].  Any
    table (random words, not even roots), any multipliers; logn 2..5, beta 1..min(4, logn - 1), w 0..3"""
    rng = np.random.default_rng(77)
    rnd = lambda k: [int(v) % p for v in rng.integers(0, 2**62, size=k)]
    cases = 0
    for logn in range(2, 6):
        m = 1 << logn
        T = rnd(m)
        Ti = [pow(t, p - 2, p) if t else 0 for t in T]
        for w in range(4):
            cols = 1 << w
            for beta in range(1, min(4, logn - 1) + 1):
                n = m >> beta
                s = rnd(n)
                small = [rnd(cols) for _ in range(n)]
                small[0][0], small[-1][-1] = p - 1, 0
                flat = [0] * (m * cols)
                for i in range(n):
                    for c in range(cols):
                        flat[(i << beta) * cols + c] = small[i][c] * s[i] % p
                got = _virtual_stages(flat, logn, w, T, p)
                for c in range(cols):
                    x = [0] * m
                    for i in range(n):
                        x[i << beta] = small[i][c] * s[i] % p  # include/ntt_hip.h, ntt_lde
                    assert [got[r * cols + c] for r in range(m)] == _network(x, T, p), (logn, w, beta, c)
                cases += 1
            u = rnd(m)
            big = [rnd(cols) for _ in range(m)]
            got = _virtual_stages([big[r][c] for r in range(m) for c in range(cols)], logn, w, Ti, p, inverse=True)
            for c in range(cols):
                want = [v * u[r] % p for r, v in enumerate(_inverse_network([big[r][c] for r in range(m)], Ti, p))]
                assert [got[r * cols + c] * u[r] % p for r in range(m)] == want, (logn, w, c)
    assert cases == 4 * (1 + 2 + 3 + 4)


def test_the_launcher_refuses_what_it_should():
    """launch.h: fill_pass_args refuses a coset twin without its operands, the operands on any other configuration (plain matrix
    twin, CONTIG LDE kernel), either twin on a pass with s0 != mat_w, do_scale with the scaling twin, a blow-up out of range, a
    source pitch below the width; mat_twin_dispatch refuses both operands at once and an operand of the wrong direction; the
    matching launches are accepted; ordinary launches and the plain columns calls never select a twin"""
    import emu_lde_columns_lib as E

    assert E.lib().emu_lde_columns_refusals() == 0x1FFF


def _sweep_cases():
    for logn in (4, 5, 8, 9, 12):
        for width in (1, 3, 16, 17, 33):
            p2 = 1 << (width - 1).bit_length()
            pitches = (width, width + 1, p2 + 16)
            for k, pitch in enumerate(pitches):
                yield logn, width, pitches[(k + 1) % 3], pitch, (1, 3)[(logn + width + k) & 1]


def _three_pass_cases():
    """(logn, width, in_pitch, pitch, count, blow-ups): logn 17 = 6 + 6 + 5 -- a plain in-place matrix pass lies between the fused twin
    and the other end -- with the smallest and the largest blow-up, and logn 18 = 6 + 6 + 6 for the coset inverse alone"""
    for width in (1, 17):
        for in_pitch, pitch in ((width + 1, width), (width, width + 1)):
            yield 17, width, in_pitch, pitch, 1, (1, 4)
    yield 18, 1, 1, 1, 1, ()


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_both_twins_in_the_host_model(oracle, cls):
    """pass.h's PassCfg::MLDE / MCINV kernels stepped on the host (tests/emu/emu_lde_columns.cpp, LDS hazard tracker on) through
    mat_twin_dispatch / pass_geometry_of / fill_pass_args over plan_column_passes: logn {4, 5, 8, 9, 12} x width {1, 3, 16, 17, 33} x
    three pitches (input and output pitch differ for the LDE) x count 1 or 3, the blow-up cycling through every legal value and the
    shift through {1, g, p - 1}, then the three-pass shapes of _three_pass_cases; buffers of exactly (count * rows - 1) * pitch + width
    words; every live word is the oracle's network on the expanded / scaled transposed column, every padding word keeps its sentinel
    (>= p: junk on the input side)"""
    import emu_columns_lib
    import emu_lde_columns_lib as E

    L = E.lib()
    wb, p, g = CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    sent = np.iinfo(dt).max - 10
    assert sent >= p
    rng = np.random.default_rng(41)
    tables, case, ldes = {}, 0, 0

    def flat_of(x, rows, pitch, width, count):
        words = (count * rows - 1) * pitch + width
        live = np.zeros((count * rows, pitch), dtype=bool)
        live[:, :width] = True
        live = live.reshape(-1)[:words]
        a = np.full(words, sent, dtype=dt)
        a[live] = x.reshape(-1)
        return a, live

    for logn, width, in_pitch, pitch, count, betas in [c + (None,) for c in _sweep_cases()] + list(_three_pass_cases()):
        m = 1 << logn
        if logn not in tables:
            tables[logn] = oracle.make_table(1, m, p, g, wb)
        T = tables[logn]
        assert len(emu_columns_lib.column_passes(logn)) == (3 if logn >= 17 else 2 if logn >= 9 else 1)
        shift = (1, g, p - 1)[case % 3]
        target = 2 if case & 2 else 16384
        if betas is None:
            betas = (1 + case % min(4, logn - 1),)
        case += 1
        # ---- lde
        for beta in betas:
            n = m >> beta
            x = (rng.integers(0, 2**63, size=(count, n, width), dtype=np.uint64) % np.uint64(p)).astype(dt)
            x[0, 0, 0], x[-1, -1, -1] = p - 1, 0
            svec = np.array([pow(shift, _bitrev(i, logn - beta), p) for i in range(n)], dtype=dt)
            cols = np.zeros((count * width, m), dtype=dt)
            cols[:, :: 1 << beta] = oracle.pointwise(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(count * width, n), np.broadcast_to(svec, (count * width, n)).copy(), p)
            want = np.ascontiguousarray(oracle.ntt(cols, T, p).reshape(count, width, m).transpose(0, 2, 1))
            a, _ = flat_of(x, n, in_pitch, width, count)
            a0 = a.copy()
            out, live = flat_of(np.full((count, m, width), sent - 2, dtype=dt), m, pitch, width, count)
            out[~live] = sent - 1
            key = (cls, "lde", logn, beta, width, in_pitch, pitch, count, shift, target)
            assert L.emu_lde_columns(wb, logn, p, T.ctypes.data, a.ctypes.data, in_pitch, out.ctypes.data, pitch, width, count, beta, shift, target) == 0, key
            assert np.array_equal(out[live], want.reshape(-1)), key
            assert np.all(out[~live] == sent - 1) and np.array_equal(a, a0), key
            ldes += 1
        # ---- coset inverse, in place and out of place alternating
        y = (rng.integers(0, 2**63, size=(count, m, width), dtype=np.uint64) % np.uint64(p)).astype(dt)
        y[0, 0, 0], y[-1, -1, -1] = p - 1, 0
        inv = oracle.intt(np.ascontiguousarray(y.transpose(0, 2, 1)).reshape(count * width, m), T, p)
        uvec = np.array([pow(pow(shift, p - 2, p), _bitrev(i, logn), p) for i in range(m)], dtype=dt)
        want = np.ascontiguousarray(oracle.pointwise(inv, np.broadcast_to(uvec, inv.shape).copy(), p).reshape(count, width, m).transpose(0, 2, 1))
        a, live = flat_of(y, m, pitch, width, count)
        a0 = a.copy()
        in_place = bool(case & 1)
        out = a if in_place else np.full_like(a, sent - 1)
        key = (cls, "cinv", logn, width, pitch, count, shift, target, in_place)
        assert L.emu_coset_inverse_columns(wb, logn, p, T.ctypes.data, a.ctypes.data, out.ctypes.data, width, pitch, count, shift, target) == 0, key
        assert np.array_equal(out[live], want.reshape(-1)), key
        assert np.all(out[~live] == (sent if in_place else sent - 1)), key
        if not in_place:
            assert np.array_equal(a, a0), key
    assert (case, ldes) == (5 * 5 * 3 + 2 * 2 + 1, 5 * 5 * 3 + 2 * 2 * 2)


def test_error_contract_without_a_device():
    """every NTT_E_* case of the two entry points that is reported before a launch and needs no plan on a device; the binding and
    the header agree"""
    from ntt_aie_amd import _lib

    L = _lib.lib()
    assert {"ntt_lde_columns", "ntt_coset_inverse_columns"} <= set(_lib.EXPORTS)
    assert len(L.ntt_lde_columns.argtypes) == 8 and len(L.ntt_coset_inverse_columns.argtypes) == 7
    assert L.ntt_lde_columns(None, None, 1, None, 1, 1, 1, None) == _lib.NTT_E_ARG
    assert L.ntt_coset_inverse_columns(None, None, None, 1, 1, 1, None) == _lib.NTT_E_ARG
    assert L.ntt_lde_columns(None, None, 0, None, 0, 0, 0, None) == _lib.NTT_E_ARG  # no plan: not even an empty batch
    assert L.ntt_coset_inverse_columns(None, None, None, 0, 0, 0, None) == _lib.NTT_E_ARG
    hdr = open(os.path.join(ROOT, "include", "ntt_hip.h")).read()
    assert re.search(r"int ntt_lde_columns\(ntt_plan_t plan, const void \*d_in, size_t in_pitch, void \*d_out, size_t out_pitch, size_t width, size_t count,\s+void \*stream\);", hdr)
    assert re.search(r"int ntt_coset_inverse_columns\(ntt_plan_t plan, const void \*d_in, void \*d_out, size_t width, size_t pitch, size_t count, void \*stream\);", hdr)
    assert "a coset shift on columns" not in hdr
    import ntt_aie_amd as eng

    for name in ("lde_columns", "coset_inverse_columns"):
        assert hasattr(eng.NTTPlan, name)
