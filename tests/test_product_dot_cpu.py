"""ntt_polymul_dot_pre in the host index model (tests/emu/emu_product_dot.cpp): the product's fused middle pass summed over the terms of
an inner product (pass.h: run_product_dot_pass -- per term the inverse rounds of a[k] and acc += x . b^[k], one scaling, the forward
rounds) and the launches around it (sequence.h: seq_polymul_dot), against the sum over the terms of the oracle pipeline; terms == 1
against seq_polymul_pre's words; the launch list itself, dumped without running anything, against what the header promises; and the
argument rules of the C-ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import emu_product_dot_lib
import emu_product_pre_lib
import product_dot_ref as R

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
# three word classes; every fused unit size (8-byte words 2^7 .. 2^12, 4-byte words 2^6 .. 2^13) as a single-pass size, the fallback
# size below the smallest unit, one two-pass size and (Goldilocks) one three-pass size, 8 + 8 + 7 stages
CASES = ([(8, GOLD, 7, l) for l in (6, 7, 8, 9, 10, 11, 12, 13, 23)] + [(8, M64, 3, l) for l in (6, 7, 8, 9, 10, 11, 12, 14)] +
         [(4, 998244353, 3, l) for l in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14)] + [(4, 2013265921, 31, 9), (4, 3221225473, 5, 7), (4, 3221225473, 5, 12)])
# (terms, broadcast, out is a[0]): every term count, both operand shapes and both placements of out in every case ...
SCHEDULE = [(1, False, False), (2, True, True), (3, False, True), (5, True, False)]
# ... and their whole product at the smallest unit of every class
CROSS = [(8, GOLD, 7, 7), (8, M64, 3, 7), (4, 998244353, 3, 6)]

# what a pointer of a step is (emu_polymul_dot_sequence)
NULL, A, OUT, BHAT, TW_FWD, TW_INV, TW_SC = range(7)
PASS, PRODUCT, ROW_SUM = 0, 2, 3
KEYS = ("family", "inverse", "contig", "log_m", "n", "s0", "variant", "do_scale", "batch", "in", "out", "tw", "tw2", "tw_sc", "in2", "mask", "terms",
        "a_stride", "b_stride", "zero")


def _batch(logn):
    # target_wgs 8: batch 37 makes workgroups hold several polynomials (a ragged last group) and stream several groups
    return 37 if logn <= 9 else 5 if logn <= 14 else 1


def _run(oracle, wb, p, g, logn, alt, combos, seed=None):
    L = emu_product_dot_lib.lib()
    batch, kmax = _batch(logn), max(c[0] for c in combos)
    a, b, T, bhat = R.operands(oracle, wb, p, g, logn, batch, kmax, seed)
    for terms, bcast, alias in combos:
        rows = 1 if bcast else batch
        bh = np.ascontiguousarray(bhat[:terms, :rows])
        want = R.want(oracle, a[:terms], b[:terms], T, p, bcast)
        sa, keep = np.ascontiguousarray(a[:terms]).copy(), bh.copy()
        out = sa[0] if alias else np.full((batch, 1 << logn), 0xFFFFFFFF, dtype=a.dtype)
        rc = L.emu_polymul_dot(wb, logn, p, T.ctypes.data, sa.ctypes.data, bh.ctypes.data, rows, terms, out.ctypes.data, batch, 8, alt)
        assert rc == 0, (wb, p, logn, alt, terms, bcast, alias)
        assert np.array_equal(out, want), (wb, p, logn, alt, terms, bcast, alias)
        assert np.array_equal(bh, keep), "b^ was written"


@pytest.mark.parametrize("wb,p,g,logn", CASES)
def test_values_against_the_summed_oracle_pipeline(oracle, wb, p, g, logn):
    """Every plan alternative of the size (the pinned ones that have no fused middle take the fallback)."""
    nalt = emu_product_dot_lib.lib().emu_polymul_dot_alternatives(wb, logn, p)
    assert nalt >= 1
    for alt in range(nalt):
        _run(oracle, wb, p, g, logn, alt, [(2, False, True)] if logn == 23 else SCHEDULE)  # (2^23: one polynomial, one call)


@pytest.mark.parametrize("wb,p,g,logn", CROSS)
def test_every_term_count_operand_shape_and_placement_of_out(oracle, wb, p, g, logn):
    _run(oracle, wb, p, g, logn, -1, [(k, bc, al) for k in (1, 2, 3, 5) for bc in (False, True) for al in (False, True)], seed=99)


@pytest.mark.parametrize("wb,p,g,logn", [(8, GOLD, 7, 6), (8, GOLD, 7, 9), (8, GOLD, 7, 13), (8, M64, 3, 12), (4, 998244353, 3, 5), (4, 998244353, 3, 13), (4, 3221225473, 5, 7)])
@pytest.mark.parametrize("bcast", [False, True])
def test_one_term_is_the_prepared_product_word_for_word(oracle, wb, p, g, logn, bcast):
    batch = _batch(logn)
    a, b, T, bhat = R.operands(oracle, wb, p, g, logn, batch, 1)
    rows = 1 if bcast else batch
    bh = np.ascontiguousarray(bhat[0, :rows])
    sa, pre = a[0].copy(), np.zeros_like(a[0])
    assert emu_product_pre_lib.lib().emu_polymul_pre(wb, logn, p, T.ctypes.data, sa.ctypes.data, bh.ctypes.data, rows, pre.ctypes.data, batch, 8, -1) == 0
    sa, dot = a.copy(), np.zeros_like(a[0])
    assert emu_product_dot_lib.lib().emu_polymul_dot(wb, logn, p, T.ctypes.data, sa.ctypes.data, bh.ctypes.data, rows, 1, dot.ctypes.data, batch, 8, -1) == 0
    assert np.array_equal(dot, pre)


def test_a_long_sum_of_maximal_words(oracle):
    """17 terms of all p - 1 (Goldilocks 2^7, batch 5): the accumulator's reduction at every step"""
    a, b, T, bhat = R.operands(oracle, 8, GOLD, 7, 7, 5, 17, all_max=True)
    want = R.want(oracle, a, b, T, GOLD)
    sa, out = a.copy(), np.zeros_like(a[0])
    assert emu_product_dot_lib.lib().emu_polymul_dot(8, 7, GOLD, T.ctypes.data, sa.ctypes.data, bhat.ctypes.data, 5, 17, out.ctypes.data, 5, 8, -1) == 0
    assert np.array_equal(out, want)


def _steps(wb, logn, p, batch, rows, terms, alt=-1, target_wgs=8192):
    buf = (C.c_int * (20 * 16))()
    n = emu_product_dot_lib.lib().emu_polymul_dot_sequence(wb, logn, p, batch, rows, terms, alt, target_wgs, buf, 16)
    assert n >= 0
    return [dict(zip(KEYS, buf[20 * i:20 * i + 20])) for i in range(n)]


def _passes(wb, logn, p, alt):
    tri, mb = (C.c_int * 24)(), C.c_uint64()
    n = emu_lib.lib().emu_plan_alt(logn, wb, C.c_uint64(p), alt, tri, C.byref(mb))
    assert n > 0
    return [(tri[3 * i], tri[3 * i + 1], tri[3 * i + 2]) for i in range(n)]


@pytest.mark.parametrize("wb,p,logn,batch", [(8, GOLD, 13, 5), (8, GOLD, 16, 5), (8, GOLD, 23, 2), (8, M64, 14, 3), (4, 998244353, 14, 5), (4, 3221225473, 16, 33),
                                             (4, 3221225473, 23, 2)])
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("terms", [1, 4])
def test_fused_size_runs_the_column_passes_over_all_terms_and_one_middle_step(wb, p, logn, batch, broadcast, terms):
    passes = _passes(wb, logn, p, 0)
    assert len(passes) >= 2
    rows = 1 if broadcast else batch
    steps = _steps(wb, logn, p, batch, rows, terms, alt=0)
    k = len(passes) - 1
    assert len(steps) == 2 * k + 1  # whatever `terms`: no loop of launches anywhere
    for i, st in enumerate(steps[:k]):  # a's inverse column passes, highest first, in place on a, ONE launch over terms * batch rows
        contig, s0, log_m = passes[len(passes) - 1 - i]
        assert (st["family"], st["inverse"], st["contig"], st["s0"], st["log_m"]) == (PASS, 1, 0, s0, log_m)
        assert (st["in"], st["out"], st["tw"], st["in2"], st["batch"], st["do_scale"], st["mask"], st["terms"]) == (A, A, TW_INV, NULL, terms * batch, 0, 0, 0)
    mid = steps[k]
    assert (mid["family"], mid["contig"], mid["s0"], mid["log_m"], mid["batch"]) == (PRODUCT, 1, 0, passes[0][2], batch)
    assert (mid["in"], mid["out"], mid["in2"], mid["tw"], mid["tw2"]) == (A, OUT, BHAT, TW_INV, TW_FWD)
    assert mid["mask"] == (1 | 4 | (2 if broadcast else 0))
    assert (mid["terms"], mid["a_stride"], mid["b_stride"]) == (terms, batch, rows)
    for i, st in enumerate(steps[k + 1:]):  # the forward column passes in place on out, over batch rows
        contig, s0, log_m = passes[1 + i]
        assert (st["family"], st["inverse"], st["contig"], st["s0"], st["log_m"]) == (PASS, 0, 0, s0, log_m)
        assert (st["in"], st["out"], st["tw"], st["in2"], st["batch"], st["mask"], st["terms"]) == (OUT, OUT, TW_FWD, NULL, batch, 0, 0)


@pytest.mark.parametrize("wb,p,logn", [(8, GOLD, 7), (8, GOLD, 10), (8, GOLD, 12), (8, M64, 9), (8, M64, 11), (4, 998244353, 6), (4, 998244353, 12), (4, 2013265921, 9)])
@pytest.mark.parametrize("broadcast", [False, True])
def test_single_pass_size_is_exactly_one_step(wb, p, logn, broadcast):
    steps = _steps(wb, logn, p, 37, 1 if broadcast else 37, 5)
    assert len(steps) == 1
    st = steps[0]
    assert (st["family"], st["log_m"], st["n"], st["batch"], st["in"], st["out"], st["in2"]) == (PRODUCT, logn, logn, 37, A, OUT, BHAT)
    assert (st["mask"], st["terms"], st["a_stride"], st["b_stride"]) == (1 | 4 | (2 if broadcast else 0), 5, 37, 1 if broadcast else 37)


@pytest.mark.parametrize("wb,p,logn,alt", [(8, GOLD, 13, 1), (8, GOLD, 6, 0), (4, 998244353, 5, 0), (4, 998244353, 14, 1), (8, M64, 10, 0), (4, 998244353, 13, 0)])
@pytest.mark.parametrize("broadcast", [False, True])
def test_sizes_without_a_fused_middle_take_the_fallback(wb, p, logn, alt, broadcast):
    """a pinned 13-stage alternative at Goldilocks 2^13 (and the 14-stage one of a lazy 4-byte prime, the sizes below the smallest
    unit, and the two units whose summed kernel is not built -- general 64-bit 2^10, 4-byte 2^13: launch.h, product_dot_unit, where
    the prepared product IS fused): the unscaled inverse of all terms * batch rows in place, the row sum as a launch of its own into term 0's block, ONE plain
    forward transform from there.  No product-middle step, and no launch per term."""
    assert emu_product_dot_lib.lib().emu_polymul_dot_fused(wb, logn, p, 5, 8192, alt) == 0
    assert emu_product_pre_lib.lib().emu_polymul_pre_fused(wb, logn, p, 5, 8192, alt) == (1 if (wb, logn) in ((8, 10), (4, 13)) and p != GOLD else 0)
    steps = _steps(wb, logn, p, 5, 1 if broadcast else 5, 4, alt=alt)
    assert [st["family"] for st in steps] == [PASS, ROW_SUM, PASS]
    inv, row_sum, fwd = steps
    assert (inv["inverse"], inv["log_m"], inv["in"], inv["out"], inv["do_scale"], inv["tw_sc"], inv["batch"]) == (1, logn, A, A, 0, NULL, 20)
    assert (row_sum["in"], row_sum["out"], row_sum["in2"], row_sum["terms"], row_sum["a_stride"], row_sum["b_stride"]) == (A, A, BHAT, 4, 5, 1 if broadcast else 5)
    assert (fwd["inverse"], fwd["log_m"], fwd["in"], fwd["out"], fwd["batch"], fwd["in2"], fwd["mask"]) == (0, logn, A, OUT, 5, NULL, 0)


def test_the_model_refuses_what_the_c_abi_refuses():
    L = emu_product_dot_lib.lib()
    buf = np.zeros(4 * 64, dtype=np.uint64)
    T = np.ones(64, dtype=np.uint64)
    args = (8, 6, GOLD, T.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    assert L.emu_polymul_dot(*args, 2, 1, buf.ctypes.data, 4, 8, -1) == -1  # bhat_rows is neither 1 nor batch
    assert L.emu_polymul_dot(*args, 1, 0, buf.ctypes.data, 4, 8, -1) == -1  # no terms
    assert L.emu_polymul_dot(*args, 1, 1 << 30, buf.ctypes.data, 4, 8, -1) == -1  # terms * batch beyond the row limit


def test_c_abi_rules_that_need_no_device():
    """The symbol is exported with the header's signature, and a null plan is NTT_E_ARG before anything else is looked at."""
    import __graft_entry__ as ge
    import os

    if not os.path.exists(os.path.join(ge.ROOT, "ntt_aie_amd", "libntt_hip.so")):
        ge.build()
    from ntt_aie_amd import _lib

    L = _lib.lib()
    assert "ntt_polymul_dot_pre" in _lib.EXPORTS
    assert L.ntt_polymul_dot_pre(None, None, None, 1, 1, None, 0, None) == _lib.NTT_E_ARG
    assert L.ntt_polymul_dot_pre(None, None, None, 1, 1, None, 1, None) == _lib.NTT_E_ARG
