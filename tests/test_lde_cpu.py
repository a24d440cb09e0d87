"""Coset low-degree extension without a GPU: the semantics the header states (a Python-integer model of the network, no library),
the fused first pass in the host index model against the oracle, and the error contract that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

GOLD = 0xFFFFFFFF00000001


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


@pytest.mark.parametrize("p,g", [(GOLD, 7), (998244353, 3)])
def test_network_level_definition_is_the_coset_evaluation(oracle, p, g):
    """For N <= 64, blow-up 1..4: Forward_M(x) with x[i * 2^beta] = c[i] * shift^bitrev_N(i), zero elsewhere, where c = the oracle's
    scaled inverse network of the evaluations (kind-1 table of size N) -- equals P(shift * w_M^k) at natural k, P being the
    polynomial with those evaluations on <w_N>.  Pure Python integers; pins what include/ntt_hip.h says ntt_lde computes."""
    rng = np.random.default_rng(1)
    dt = np.uint64 if p > 2**32 else np.uint32
    for logn in range(1, 7):
        n = 1 << logn
        Tn = _kind1(n, p, g)
        assert [int(v) for v in oracle.make_table(1, n, p, g, 8 if p > 2**32 else 4)] == Tn
        for beta in range(1, 5):
            m = n << beta
            Tm = _kind1(m, p, g)
            wn, wm = pow(g, (p - 1) // n, p), pow(g, (p - 1) // m, p)
            coef = [int(v) % p for v in rng.integers(0, 2**62, size=n)]  # P, natural order
            coef[0], coef[-1] = p - 1, 0
            evals = [sum(c * pow(wn, j * k, p) for j, c in enumerate(coef)) % p for k in range(n)]
            assert _network([coef[_bitrev(i, logn)] for i in range(n)], Tn, p) == evals  # bit-reversed in, natural out
            c_br = [int(v) for v in oracle.intt(np.array([evals], dtype=dt), np.array(Tn, dtype=dt), p)[0]]
            assert c_br == [coef[_bitrev(i, logn)] for i in range(n)]
            for shift in (1, g, p - 1):
                x = [0] * m
                for i in range(n):
                    x[i << beta] = c_br[i] * pow(shift, _bitrev(i, logn), p) % p
                got = _network(x, Tm, p)
                xs = [shift * pow(wm, k, p) % p for k in range(m)]
                want = [sum(c * pow(xk, j, p) for j, c in enumerate(coef)) % p for xk in xs]
                assert got == want, (logn, beta, shift)


CLASSES = [(8, GOLD, 7), (8, 0xFFFFFFFC00000001, 10), (4, 998244353, 3)]


@pytest.mark.parametrize("wb,p,g", CLASSES)
def test_fused_first_pass_in_the_host_model(oracle, wb, p, g):
    """pass.h's PassCfg::LDE kernels stepped on the host (tests/emu/emu_lde.cpp, LDS hazard tracker on) for logM 5..13, blow-up
    1..4, ragged batches, both layouts, every plan alternative: the oracle's network of the expanded input, word for word."""
    import emu_lde_lib

    L = emu_lde_lib.lib()
    dt = np.uint32 if wb == 4 else np.uint64
    rng = np.random.default_rng(5)
    case = 0
    for logm in range(5, 14):
        m = 1 << logm
        T = oracle.make_table(1, m, p, g, wb)
        for beta in range(1, 5):
            n = m >> beta
            for alt in range(L.emu_lde_alternatives(wb, logm, p)):
                for batch in ((1, 3, 37) if logm <= 10 else (3,)):
                    shift = (1, g, p - 1)[case % 3]
                    layout = case % 2
                    case += 1
                    a = (rng.integers(0, 2**63, size=(batch, n), dtype=np.uint64) % np.uint64(p)).astype(dt)
                    a[0, 0], a[-1, -1] = 0, p - 1
                    s = np.array([pow(shift, _bitrev(i, logm - beta), p) for i in range(n)], dtype=object)
                    x = np.zeros((batch, m), dtype=dt)
                    x[:, :: 1 << beta] = ((a.astype(object) * s[None, :]) % p).astype(dt)
                    want = oracle.ntt(x, T, p)
                    if layout:
                        want = oracle.block16(want)
                    out = np.full((batch, m), np.iinfo(dt).max, dtype=dt)  # words >= p: the fused pass is handed `out` as its input and must not read it
                    rc = L.emu_lde(wb, logm, p, T.ctypes.data, beta, shift, a.ctypes.data, out.ctypes.data, batch, layout, 8192, alt)
                    assert rc == 0 and np.array_equal(out, want), (logm, beta, alt, batch, shift, layout, rc)


def test_lde_error_contract_without_a_device():
    """argument errors that are reported before any device is touched, and the binding / header agreement"""
    from ntt_aie_amd import _lib

    L = _lib.lib()
    assert {"ntt_plan_set_coset", "ntt_lde"} <= set(_lib.EXPORTS)
    assert L.ntt_plan_set_coset(None, 3, 7) == _lib.NTT_E_ARG
    assert L.ntt_lde(None, None, None, 1, 0, None) == _lib.NTT_E_ARG
    assert L.ntt_lde(None, None, None, 0, 0, None) == _lib.NTT_E_ARG  # no plan: not even batch 0
    hdr = open(os.path.join(ROOT, "include", "ntt_hip.h")).read()
    assert re.search(r"int ntt_plan_set_coset\(ntt_plan_t plan, int log_blowup, uint64_t shift\);", hdr)
    assert re.search(r"int ntt_lde\(ntt_plan_t plan, const void \*d_in, void \*d_out, size_t batch, int out_layout, void \*stream\);", hdr)
    import ntt_aie_amd as eng

    assert callable(eng.lde_from_evals) and hasattr(eng.NTTPlan, "set_coset") and hasattr(eng.NTTPlan, "lde")
    from ntt_aie_amd.multi import MultiDevicePlan

    assert hasattr(MultiDevicePlan, "lde") and hasattr(MultiDevicePlan, "set_coset")


def test_fused_expansion_is_never_a_dma_or_prefetch_kernel():
    """the rule is in the configuration type, and the launcher refuses a mismatch: PassCfg::DMA and ::PREFETCH both carry !LDE_,
    launch_cfg returns an error when the coset operand meets a kernel that is not its own (and the other way round); the shared
    argument fill behind it (launch.h: fill_pass_args, also the host model's) refuses the same mismatch"""
    src = open(os.path.join(ROOT, "ntt_aie_amd", "csrc", "pass.h")).read()
    assert re.search(r"static constexpr bool DMA = ALLOW_DMA_ && !LDE_ &&", src)
    assert re.search(r"static constexpr bool PREFETCH = NTT_PREFETCH_M32_WIDE && ALLOW_DMA_ && !LDE_ &&", src)
    inc = open(os.path.join(ROOT, "ntt_aie_amd", "csrc", "pass_kernel.inc")).read()
    assert "if ((e.lde_beta != 0) != Cfg::LDE) return hipErrorInvalidValue;" in inc
