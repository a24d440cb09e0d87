"""Coset interpolation without a GPU: the semantics the header states (a Python-integer model of the network, no library), the
flagged last pass in the host index model against that model and the oracle, and the binding / header agreement."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

GOLD = 0xFFFFFFFF00000001
PRIMES = [(3329, 3), (998244353, 3), (GOLD, 7)]


def _bitrev(i, bits):
    r = 0
    for k in range(bits):
        r |= ((i >> k) & 1) << (bits - 1 - k)
    return r


def _kind1(n, p, g):
    """plan.h make_table kind 1 in Python integers: T[h + i] = w^(bitrev(i) * n / 2h)"""
    w = pow(g, (p - 1) // n, p)
    T = [1] * n
    h, lh = 1, 0
    while h < n:
        for i in range(h):
            T[h + i] = pow(w, _bitrev(i, lh) * (n // (2 * h)), p)
        h, lh = 2 * h, lh + 1
    return T


def _kind0(n, p, g):
    """the reference's rule: T[i] = w^i, w = g^((p - 1) // n) with integer division"""
    w = pow(g, (p - 1) // n, p)
    return [pow(w, i, p) for i in range(n)]


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


def _inv_scaled(a, T, p):
    """the exact inverse of _network: stages descending, (u, v) -> (u + v / T, u - v / T), then * n^-1"""
    a, n = list(a), len(a)
    t = n // 2
    while t >= 1:
        h = n // (2 * t)
        for i in range(h):
            ti = pow(T[h + i], -1, p)
            for j in range(2 * i * t, 2 * i * t + t):
                u, w = a[j], a[j + t] * ti % p
                a[j], a[j + t] = (u + w) % p, (u - w) % p
        t //= 2
    ninv = pow(n, -1, p)
    return [x * ninv % p for x in a]


def coset_inverse_model(a, T, p, shift):
    """include/ntt_hip.h: d_out[i] = InvScaled_M(d_in)[i] * shift^(-bitrev_logM(i)) mod p"""
    n = len(a)
    bits = n.bit_length() - 1
    return [x * pow(shift, -_bitrev(i, bits), p) % p for i, x in enumerate(_inv_scaled(a, T, p))]


@pytest.mark.parametrize("p,g", PRIMES)
def test_model_returns_the_coefficients_in_bit_reversed_order(p, g):
    """N = 2^1 .. 2^6, kind-1 tables: from P's values on shift * <w_N> the stated semantics give coefficient bitrev(i) of P at word i;
    for p = 3329 the inverse model also undoes the forward network of a 2^9-word kind-0 table (defined at network level)."""
    rng = np.random.default_rng(11)
    if (p - 1) % 512:  # p = 3329: no kind-1 table of 2^9 words; the reference's rule gives an invertible table all the same
        T0 = _kind0(512, p, g)
        x = [int(v) % p for v in rng.integers(0, 2**62, size=512)]
        y = _network(x, T0, p)
        assert _inv_scaled(y, T0, p) == x
        assert coset_inverse_model(y, T0, p, g) == [v * pow(g, -_bitrev(i, 9), p) % p for i, v in enumerate(x)]
    for logn in range(1, 7):
        n = 1 << logn
        assert (p - 1) % n == 0
        T = _kind1(n, p, g)
        w = pow(g, (p - 1) // n, p)
        coef = [int(v) % p for v in rng.integers(0, 2**62, size=n)]
        coef[0], coef[-1] = p - 1, 0
        for shift in (1, g, p - 1):
            evals = [sum(c * pow(shift * pow(w, k, p) % p, j, p) for j, c in enumerate(coef)) % p for k in range(n)]
            got = coset_inverse_model(evals, T, p, shift)
            assert got == [coef[_bitrev(i, logn)] for i in range(n)], (logn, shift)
            assert _inv_scaled(_network(evals, T, p), T, p) == evals


@pytest.mark.parametrize("p,g", PRIMES)
def test_identity_with_the_definition_of_lde(p, g):
    """coset_inverse(Forward_M(x))[i << beta] = c[i] and zero elsewhere, x the expanded input of ntt_lde's definition
    (x[i << beta] = c[i] * shift^bitrev_N(i)), for beta = 1 .. 3: the two calls are inverse to each other on the coset."""
    rng = np.random.default_rng(12)
    for logn in range(1, 5):
        n = 1 << logn
        for beta in range(1, 4):
            m = n << beta
            if (p - 1) % m:
                continue
            Tm = _kind1(m, p, g)
            c = [int(v) % p for v in rng.integers(0, 2**62, size=n)]
            c[0] = p - 1
            for shift in (1, g, p - 1):
                x = [0] * m
                for i in range(n):
                    x[i << beta] = c[i] * pow(shift, _bitrev(i, logn), p) % p
                got = coset_inverse_model(_network(x, Tm, p), Tm, p, shift)
                want = [0] * m
                for i in range(n):
                    want[i << beta] = c[i]
                assert got == want, (logn, beta, shift)


CLASSES = [(8, GOLD, 7), (8, 0xFFFFFFFC00000001, 10), (4, 998244353, 3)]


def test_model_agrees_with_the_oracle(oracle):
    """the comparator of the GPU tests -- oracle.intt times pow(shift, -bitrev(i), p) -- is the Python-integer model"""
    rng = np.random.default_rng(13)
    for wb, p, g in CLASSES:
        dt = np.uint32 if wb == 4 else np.uint64
        for logn in (1, 3, 6):
            n = 1 << logn
            T = oracle.make_table(1, n, p, g, wb)
            assert [int(v) for v in T] == _kind1(n, p, g)
            a = (rng.integers(0, 2**63, size=(2, n), dtype=np.uint64) % np.uint64(p)).astype(dt)
            y = oracle.intt(a, T, p)
            for b in range(2):
                want = [int(y[b][i]) * pow(g, -_bitrev(i, logn), p) % p for i in range(n)]
                assert coset_inverse_model([int(v) for v in a[b]], [int(v) for v in T], p, g) == want


@pytest.mark.parametrize("wb,p,g", CLASSES)
def test_flagged_last_pass_in_the_host_model(oracle, wb, p, g):
    """pass.h's PassCfg::CINV kernels stepped on the host (tests/emu/emu_coset_inverse.cpp, LDS hazard tracker on) through
    pass_dispatch / fill_pass_args: every fused logM 5..14, every plan alternative, ppw 1 and > 1 (target_wgs 8192 and 2), ragged
    batches {1, 3, 5, 9} at every size, both layouts, in place and out of place -- the oracle's scaled inverse times shift^-bitrev(i), word for word."""
    import emu_coset_inverse_lib

    L = emu_coset_inverse_lib.lib()
    assert L.emu_cinv_refusals() == 7  # twin without vector, vector without twin, twin on a scaled launch: refused; the pair: accepted
    dt = np.uint32 if wb == 4 else np.uint64
    rng = np.random.default_rng(5)
    case = 0
    for logm in range(1, 15):
        nalt = L.emu_cinv_alternatives(wb, logm, p)
        for alt in range(nalt):
            assert L.emu_cinv_fused(wb, logm, p, alt) == (1 if logm >= 5 else 0), (logm, alt)  # the documented rule of ntt_plan_info 12
        if logm < 5:
            continue
        m = 1 << logm
        T = oracle.make_table(1, m, p, g, wb)
        for alt in range(nalt):
            for batch in (1, 3, 5, 9):
                for target in (8192, 2):
                    shift = (1, g, p - 1)[case % 3]
                    layout = case % 2
                    in_place = (case // 2) % 2
                    case += 1
                    y = (rng.integers(0, 2**63, size=(batch, m), dtype=np.uint64) % np.uint64(p)).astype(dt)
                    y[0, 0], y[-1, -1] = 0, p - 1
                    u = np.array([pow(shift, -_bitrev(i, logm), p) for i in range(m)], dtype=object)
                    want = ((oracle.intt(y, T, p).astype(object) * u[None, :]) % p).astype(dt)
                    a = np.ascontiguousarray(oracle.block16(y) if layout else y.copy())
                    out = a if in_place else np.full((batch, m), 0xEE, dtype=dt)
                    rc = L.emu_coset_inverse(wb, logm, p, T.ctypes.data, shift, a.ctypes.data, out.ctypes.data, batch, layout, target, alt)
                    assert rc == 0 and np.array_equal(out, want), (logm, alt, batch, target, shift, layout, in_place, rc)
    # many polynomials per workgroup AND several groups per workgroup (ppw > 1) with a ragged last group
    for logm in (5, 8):
        m, batch = 1 << logm, (3 << (12 - logm)) + 1
        T = oracle.make_table(1, m, p, g, wb)
        y = (rng.integers(0, 2**63, size=(batch, m), dtype=np.uint64) % np.uint64(p)).astype(dt)
        u = np.array([pow(g, -_bitrev(i, logm), p) for i in range(m)], dtype=object)
        want = ((oracle.intt(y, T, p).astype(object) * u[None, :]) % p).astype(dt)
        out = np.full((batch, m), 0xEE, dtype=dt)
        assert L.emu_coset_inverse(wb, logm, p, T.ctypes.data, g, y.ctypes.data, out.ctypes.data, batch, 0, 2, 0) == 0
        assert np.array_equal(out, want), logm


def test_header_binding_and_info_codes():
    """the two entry points are declared, exported, bound and documented; argument errors that need no device"""
    from ntt_aie_amd import _lib

    L = _lib.lib()
    assert {"ntt_plan_set_coset_inverse", "ntt_coset_inverse"} <= set(_lib.EXPORTS)
    assert L.ntt_plan_set_coset_inverse(None, 7) == _lib.NTT_E_ARG
    assert L.ntt_coset_inverse(None, None, None, 1, 0, None) == _lib.NTT_E_ARG
    assert L.ntt_coset_inverse(None, None, None, 0, 0, None) == _lib.NTT_E_ARG  # no plan: not even batch 0
    assert L.ntt_plan_set_coset_inverse.argtypes is not None and len(L.ntt_coset_inverse.argtypes) == 6
    hdr = open(os.path.join(ROOT, "include", "ntt_hip.h")).read()
    assert re.search(r"int ntt_plan_set_coset_inverse\(ntt_plan_t plan, uint64_t shift\);", hdr)
    assert re.search(r"int ntt_coset_inverse\(ntt_plan_t plan, const void \*d_in, void \*d_out, size_t batch, int in_layout, void \*stream\);", hdr)
    assert re.search(r"\b11 whether a coset-inverse shift is set", hdr) and re.search(r"\b12 whether ntt_coset_inverse on this plan scales inside", hdr)
    api = open(os.path.join(ROOT, "ntt_aie_amd", "csrc", "ntt_api.hip")).read()
    assert "case 11: return pl->cinv_set ? 1 : 0;" in api and "case 12: return cinv_fused(pl) ? 1 : 0;" in api
    import ntt_aie_amd as eng
    from ntt_aie_amd.multi import MultiDevicePlan

    for name in ("set_coset_inverse", "coset_inverse", "coset_inverse_set", "coset_inverse_fused"):
        assert hasattr(eng.NTTPlan, name)
    assert hasattr(MultiDevicePlan, "set_coset_inverse") and hasattr(MultiDevicePlan, "coset_inverse")


def test_the_flag_lives_only_in_inverse_contig_configurations():
    """the rule is in the configuration type and in both launch-side checks; the product library reads no experiment knob"""
    src = open(os.path.join(ROOT, "ntt_aie_amd", "csrc", "pass.h")).read()
    assert re.search(r"static_assert\(!CINV_ \|\| \(INV_ && CONTIG_\)", src)
    inc = open(os.path.join(ROOT, "ntt_aie_amd", "csrc", "pass_kernel.inc")).read()
    assert "if ((e.cinv_u != nullptr) != Cfg::CINV) return hipErrorInvalidValue;" in inc
    launch = open(os.path.join(ROOT, "ntt_aie_amd", "csrc", "launch.h")).read()
    assert "if ((e.cinv_u != nullptr) != Cfg::CINV) return false;" in launch
    api = open(os.path.join(ROOT, "ntt_aie_amd", "csrc", "ntt_api.hip")).read()
    knob = api.index('getenv("NTT_COSET_INV_UNFUSED")')
    assert api.rfind("#if defined(NTT_EXPERIMENT)", 0, knob) > api.rfind("#endif", 0, knob)  # inside the experiment-only block
