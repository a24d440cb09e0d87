"""ntt_polymul_matvec_pre in the host index model (tests/emu/emu_product_mv.cpp): several inner products of ONE operand a -- the two-output
summed middle pass (pass.h: run_product_mv_pass -- per term the inverse rounds of a[k] ONCE and acc_j += x . b^[j][k] for two outputs, then
per output one scaling and the forward rounds) and the launches around it (sequence.h: seq_polymul_matvec), against the reference of
ntt_polymul_dot_pre (product_dot_ref.want) per output; one output against emu_polymul_dot's words; the launch list itself, dumped without
running anything, against what the header promises; and the argument rules of the C-ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import emu_product_dot_lib
import emu_product_mv_lib
import product_dot_ref as R

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
# three word classes; every fused unit size (8-byte words 2^7 .. 2^12, 4-byte words 2^6 .. 2^13) as a single-pass size, the fallback
# size below the smallest unit, one two-pass size and (Goldilocks) one three-pass size, 8 + 8 + 7 stages
CASES = ([(8, GOLD, 7, l) for l in (6, 7, 8, 9, 10, 11, 12, 13, 23)] + [(8, M64, 3, l) for l in (6, 7, 8, 9, 10, 11, 12, 14)] +
         [(4, 998244353, 3, l) for l in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14)])
# (outs, terms, broadcast): every output count (a summed launch alone, a pair, a pair and a summed launch, two pairs), every term count
# and both operand shapes in every case ...
SCHEDULE = [(1, 2, False), (2, 5, True), (3, 1, True), (4, 2, False)]
# ... and their whole product at the smallest unit of every class
CROSS = [(8, GOLD, 7, 7), (8, M64, 3, 7), (4, 998244353, 3, 6)]
OUTS, TERMS = (1, 2, 3, 4), (1, 2, 5)

# what a pointer of a step is (emu_polymul_matvec_sequence)
NULL, A, OUT, BHAT, TW_FWD, TW_INV, TW_SC = range(7)
PASS, PRODUCT, ROW_SUMS = 0, 2, 3
KEYS = ("family", "inverse", "contig", "log_m", "n", "s0", "variant", "do_scale", "batch", "in", "out", "tw", "tw2", "tw_sc", "in2", "mask", "terms",
        "a_stride", "b_stride", "mv_outs", "mv_b_stride", "mv_o_stride", "out_at", "in2_at")


def _batch(logn):
    # target_wgs 8: batch 37 makes workgroups hold several polynomials (a ragged last group) and stream several groups
    return 37 if logn <= 9 else 5 if logn <= 14 else 1


class _Ref:
    """operands of one shape and, per (output, term, operand shape), that term's product from the oracle pipeline -- computed when first
    asked for, shared by every combination and plan alternative, never changed; want() adds the terms mod p"""

    def __init__(self, oracle, wb, p, g, logn, batch, outs, terms, seed=None, all_max=False):
        self.oracle, self.p = oracle, p
        a, b, self.T, bhat = R.operands(oracle, wb, p, g, logn, batch, outs * terms, seed, all_max)
        n = 1 << logn
        self.a = np.ascontiguousarray(a[:terms])
        self.b, self.bhat = b.reshape(outs, terms, batch, n), bhat.reshape(outs, terms, batch, n)
        self._c = {}

    def want(self, outs, terms, bcast):
        res = []
        for j in range(outs):
            acc = None
            for k in range(terms):
                if (j, k, bcast) not in self._c:
                    self._c[(j, k, bcast)] = R.want(self.oracle, self.a[k:k + 1], self.b[j, k:k + 1], self.T, self.p, bcast)
                c = self._c[(j, k, bcast)]
                acc = c if acc is None else R.addmod(acc, c, self.p)
            res.append(acc)
        return np.stack(res)


def _run(ref, wb, p, logn, alt, combos, single=0, experiment=False):
    L = emu_product_mv_lib.lib(experiment)
    batch = ref.a.shape[1]
    for outs, terms, bcast in combos:
        rows = 1 if bcast else batch
        bh = np.ascontiguousarray(ref.bhat[:outs, :terms, :rows])
        sa, keep = np.ascontiguousarray(ref.a[:terms]).copy(), bh.copy()
        out = np.full((outs, batch, 1 << logn), 0xFFFFFFFF, dtype=sa.dtype)
        rc = L.emu_polymul_matvec(wb, logn, p, ref.T.ctypes.data, sa.ctypes.data, bh.ctypes.data, rows, terms, outs, out.ctypes.data, batch, 8, alt, single)
        assert rc == 0, (wb, p, logn, alt, outs, terms, bcast)
        assert np.array_equal(out, ref.want(outs, terms, bcast)), (wb, p, logn, alt, outs, terms, bcast)
        assert np.array_equal(bh, keep), "b^ was written"


@pytest.mark.parametrize("wb,p,g,logn", CASES)
def test_values_against_the_summed_oracle_pipeline_per_output(oracle, wb, p, g, logn):
    """Every plan alternative of the size (the pinned ones that have no fused middle take the fallback)."""
    nalt = emu_product_mv_lib.lib().emu_polymul_matvec_alternatives(wb, logn, p)
    assert nalt >= 1
    big = logn == 23  # one polynomial, one call: a pair
    ref = _Ref(oracle, wb, p, g, logn, _batch(logn), 2 if big else max(OUTS), 2 if big else max(TERMS))
    for alt in range(nalt):
        _run(ref, wb, p, logn, alt, [(2, 2, False)] if big else SCHEDULE)


@pytest.mark.parametrize("wb,p,g,logn", CROSS)
def test_every_output_count_term_count_and_operand_shape(oracle, wb, p, g, logn):
    ref = _Ref(oracle, wb, p, g, logn, _batch(logn), max(OUTS), max(TERMS), seed=99)
    _run(ref, wb, p, logn, -1, [(j, k, bc) for j in OUTS for k in TERMS for bc in (False, True)])


@pytest.mark.parametrize("wb,p,g,logn", [(8, GOLD, 7, 10), (8, M64, 3, 9), (4, 998244353, 3, 13), (4, 3221225473, 5, 12), (4, 2013265921, 31, 9)])
def test_one_summed_launch_per_output_gives_the_same_words(oracle, wb, p, g, logn):
    """the experiment build's switch (NTT_MATVEC_SINGLE): the sequence without the two-output kernel, and two more 4-byte streams"""
    ref = _Ref(oracle, wb, p, g, logn, _batch(logn), 3, 2, seed=5)
    for single in (0, 1):
        _run(ref, wb, p, logn, -1, [(3, 2, False), (2, 2, True)], single)


@pytest.mark.parametrize("wb,p,g,logn", [(8, GOLD, 7, 6), (8, GOLD, 7, 9), (8, GOLD, 7, 13), (8, M64, 3, 12), (4, 998244353, 3, 5), (4, 998244353, 3, 13), (4, 3221225473, 5, 7)])
@pytest.mark.parametrize("bcast", [False, True])
def test_one_output_is_the_inner_product_word_for_word(oracle, wb, p, g, logn, bcast):
    batch = _batch(logn)
    a, b, T, bhat = R.operands(oracle, wb, p, g, logn, batch, 3)
    rows = 1 if bcast else batch
    bh = np.ascontiguousarray(bhat[:, :rows])
    sa, dot = a.copy(), np.zeros_like(a[0])
    assert emu_product_dot_lib.lib().emu_polymul_dot(wb, logn, p, T.ctypes.data, sa.ctypes.data, bh.ctypes.data, rows, 3, dot.ctypes.data, batch, 8, -1) == 0
    sa, mv = a.copy(), np.zeros_like(a[:1])
    assert emu_product_mv_lib.lib().emu_polymul_matvec(wb, logn, p, T.ctypes.data, sa.ctypes.data, bh.ctypes.data, rows, 3, 1, mv.ctypes.data, batch, 8, -1, 0) == 0
    assert np.array_equal(mv[0], dot)


@pytest.mark.parametrize("wb,p,g,logn", [(8, GOLD, 7, 7), (8, M64, 3, 7), (8, 0xFFFFFFFC00000001, 10, 7), (4, 998244353, 3, 6), (4, 3221225473, 5, 7)])
def test_a_long_sum_of_maximal_words_for_two_outputs(oracle, wb, p, g, logn):
    """17 terms of all p - 1 (batch 5), two outputs.  Where the library pairs the outputs (every class here but Goldilocks, which runs the
    summed kernel twice: launch.h, product_mv_unit) both accumulators of run_product_mv_pass, `keep` and `pre`, reduce at every step;
    0xFFFFFFFC00000001 is above 2^63 and 3221225473 above 2^31, so canonical sums wrap the word"""
    assert emu_product_mv_lib.lib().emu_polymul_matvec_fused(wb, logn, p, 5, 8, -1) == (1 if p == GOLD else 2)
    ref = _Ref(oracle, wb, p, g, logn, 5, 2, 17, all_max=True)
    _run(ref, wb, p, logn, -1, [(2, 17, False), (2, 17, True)])


@pytest.mark.parametrize("logn", [7, 8, 9, 10, 11, 12, 13])
def test_the_goldilocks_two_output_kernels_of_the_experiment_build(oracle, logn):
    """The product library does not pair outputs for Goldilocks, the experiment build (tools/bench_polymul_matvec.py, leg Ax) does: the
    model compiled as that build runs every Goldilocks unit of run_product_mv_pass, as a single-pass size and (2^13) behind column passes"""
    assert emu_product_mv_lib.lib().emu_polymul_matvec_fused(8, logn, GOLD, _batch(logn), 8, 0) == 1
    assert emu_product_mv_lib.lib(True).emu_polymul_matvec_fused(8, logn, GOLD, _batch(logn), 8, 0) == 2
    ref = _Ref(oracle, 8, GOLD, 7, logn, _batch(logn), max(OUTS), max(TERMS), seed=3)
    _run(ref, 8, GOLD, logn, 0, SCHEDULE, experiment=True)
    if logn == 7:
        ref = _Ref(oracle, 8, GOLD, 7, 7, 5, 2, 17, all_max=True)
        _run(ref, 8, GOLD, 7, -1, [(2, 17, False), (2, 17, True)], experiment=True)


def _steps(wb, logn, p, batch, rows, terms, outs, alt=-1, target_wgs=8192, single=0):
    buf = (C.c_int * (24 * 16))()
    n = emu_product_mv_lib.lib().emu_polymul_matvec_sequence(wb, logn, p, batch, rows, terms, outs, alt, target_wgs, single, buf, 16)
    assert n >= 0
    return [dict(zip(KEYS, buf[24 * i:24 * i + 24])) for i in range(n)]


def _passes(wb, logn, p, alt):
    tri, mb = (C.c_int * 24)(), C.c_uint64()
    n = emu_lib.lib().emu_plan_alt(logn, wb, C.c_uint64(p), alt, tri, C.byref(mb))
    assert n > 0
    return [(tri[3 * i], tri[3 * i + 1], tri[3 * i + 2]) for i in range(n)]


def _check_middles(mids, paired, log_m, batch, rows, terms, outs, broadcast):
    """the middle launches: one per pair of outputs and a summed one for the last of an odd count, or -- not paired -- a summed one each"""
    j = 0
    for mid in mids:
        two = paired and j + 1 < outs
        assert (mid["family"], mid["contig"], mid["s0"], mid["log_m"], mid["batch"]) == (PRODUCT, 1, 0, log_m, batch)
        assert (mid["in"], mid["out"], mid["in2"], mid["tw"], mid["tw2"]) == (A, OUT, BHAT, TW_INV, TW_FWD)
        assert mid["mask"] == (1 | 4 | (2 if broadcast else 0))
        assert (mid["terms"], mid["a_stride"], mid["b_stride"]) == (terms, batch, rows)
        assert (mid["out_at"], mid["in2_at"]) == (j * batch, j * terms * rows)  # rebased to output j's blocks
        assert (mid["mv_outs"], mid["mv_b_stride"], mid["mv_o_stride"]) == ((2, terms * rows, batch) if two else (0, 0, 0))
        j += 2 if two else 1
    assert j == outs


@pytest.mark.parametrize("wb,p,logn,batch", [(8, GOLD, 13, 5), (8, GOLD, 16, 5), (8, GOLD, 23, 2), (8, M64, 14, 3), (4, 998244353, 14, 5), (4, 3221225473, 16, 33),
                                             (4, 3221225473, 23, 2)])
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("terms", [1, 4])
@pytest.mark.parametrize("outs", [1, 2, 3, 4])
def test_fused_size_shares_the_column_passes_and_pairs_the_outputs(wb, p, logn, batch, broadcast, terms, outs):
    passes = _passes(wb, logn, p, 0)
    assert len(passes) >= 2
    # the two-output kernel is what the library uses for the general 64-bit and the 4-byte class; Goldilocks runs one summed launch per
    # output after the shared column passes (launch.h: product_mv_unit, decided by profiles/polymul_matvec_ab.txt)
    paired = p != GOLD
    assert emu_product_mv_lib.lib().emu_polymul_matvec_fused(wb, logn, p, batch, 8192, 0) == (2 if paired else 1)
    rows = 1 if broadcast else batch
    steps = _steps(wb, logn, p, batch, rows, terms, outs, alt=0)
    k, m = len(passes) - 1, (outs + 1) // 2 if paired else outs
    assert len(steps) == 2 * k + m  # whatever `terms`: no loop of launches over terms, and a is transformed once
    for i, st in enumerate(steps[:k]):  # a's inverse column passes, highest first, in place on a, ONE launch over terms * batch rows
        contig, s0, log_m = passes[len(passes) - 1 - i]
        assert (st["family"], st["inverse"], st["contig"], st["s0"], st["log_m"]) == (PASS, 1, 0, s0, log_m)
        assert (st["in"], st["out"], st["tw"], st["in2"], st["batch"], st["do_scale"], st["mask"], st["terms"]) == (A, A, TW_INV, NULL, terms * batch, 0, 0, 0)
    _check_middles(steps[k:k + m], paired, passes[0][2], batch, rows, terms, outs, broadcast)
    for i, st in enumerate(steps[k + m:]):  # the forward column passes in place on out, ONE launch over outs * batch rows
        contig, s0, log_m = passes[1 + i]
        assert (st["family"], st["inverse"], st["contig"], st["s0"], st["log_m"]) == (PASS, 0, 0, s0, log_m)
        assert (st["in"], st["out"], st["tw"], st["in2"], st["batch"], st["mask"], st["terms"], st["out_at"]) == (OUT, OUT, TW_FWD, NULL, outs * batch, 0, 0, 0)
    # the switch of the experiment build: one summed launch per output, the column passes still shared
    steps = _steps(wb, logn, p, batch, rows, terms, outs, alt=0, single=1)
    assert len(steps) == 2 * k + outs
    _check_middles(steps[k:k + outs], False, passes[0][2], batch, rows, terms, outs, broadcast)
    assert [st["batch"] for st in steps[:k]] == [terms * batch] * k and [st["batch"] for st in steps[k + outs:]] == [outs * batch] * k


@pytest.mark.parametrize("wb,p,logn", [(8, GOLD, 7), (8, GOLD, 10), (8, GOLD, 12), (8, M64, 9), (8, M64, 11), (4, 998244353, 6), (4, 998244353, 12), (4, 2013265921, 9)])
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("outs", [1, 2, 3, 4])
def test_single_pass_size_is_the_middle_launches_alone(wb, p, logn, broadcast, outs):
    rows = 1 if broadcast else 37
    steps = _steps(wb, logn, p, 37, rows, 5, outs)
    paired = p != GOLD  # (launch.h: product_mv_unit)
    assert len(steps) == ((outs + 1) // 2 if paired else outs)
    assert all(st["n"] == logn for st in steps)
    _check_middles(steps, paired, logn, 37, rows, 5, outs, broadcast)


@pytest.mark.parametrize("wb,p,logn,alt", [(8, GOLD, 13, 1), (8, GOLD, 6, 0), (4, 998244353, 5, 0), (4, 998244353, 14, 1), (8, M64, 10, 0), (4, 998244353, 13, 0)])
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("outs", [1, 3])
def test_sizes_without_a_fused_middle_take_the_fallback(wb, p, logn, alt, broadcast, outs):
    """the sizes seq_polymul_dot sends to its fallback: the unscaled inverse of all terms * batch rows in place, ONE launch that writes the
    scaled sums of every output, ONE plain forward transform over outs * batch rows in place on out.  No product-middle step, no launch
    per term or per output."""
    assert emu_product_mv_lib.lib().emu_polymul_matvec_fused(wb, logn, p, 5, 8192, alt) == 0
    assert emu_product_dot_lib.lib().emu_polymul_dot_fused(wb, logn, p, 5, 8192, alt) == 0
    rows = 1 if broadcast else 5
    steps = _steps(wb, logn, p, 5, rows, 4, outs, alt=alt)
    assert [st["family"] for st in steps] == [PASS, ROW_SUMS, PASS]
    inv, sums, fwd = steps
    assert (inv["inverse"], inv["log_m"], inv["in"], inv["out"], inv["do_scale"], inv["tw_sc"], inv["batch"]) == (1, logn, A, A, 0, NULL, 20)
    assert (sums["in"], sums["out"], sums["in2"], sums["terms"], sums["a_stride"], sums["b_stride"]) == (A, OUT, BHAT, 4, 5, rows)
    assert (sums["mv_outs"], sums["mv_b_stride"], sums["mv_o_stride"]) == (outs, 4 * rows, 5)
    assert (fwd["inverse"], fwd["log_m"], fwd["in"], fwd["out"], fwd["batch"], fwd["in2"], fwd["mask"], fwd["out_at"]) == (0, logn, OUT, OUT, outs * 5, NULL, 0, 0)


def test_the_model_refuses_what_the_c_abi_refuses():
    L = emu_product_mv_lib.lib()
    buf, out = np.zeros(4 * 64, dtype=np.uint64), np.zeros(8 * 64, dtype=np.uint64)
    T = np.ones(64, dtype=np.uint64)
    args = (8, 6, GOLD, T.ctypes.data, buf.ctypes.data, buf.ctypes.data)
    mv = lambda rows, terms, outs, o=out.ctypes.data: L.emu_polymul_matvec(*args, rows, terms, outs, o, 4, 8, -1, 0)  # noqa: E731
    assert mv(2, 1, 1) == -1  # bhat_rows is neither 1 nor batch
    assert mv(1, 0, 1) == -1  # no terms
    assert mv(1, 1, 0) == -1  # no outputs
    assert mv(1, 1 << 30, 1) == -1  # terms * batch beyond the row limit
    assert mv(1, 1, 1 << 30) == -1  # outs * batch beyond the row limit
    assert mv(1, 1, 1, buf.ctypes.data) == -1  # out is a: refused, unlike the inner product's


def test_c_abi_rules_that_need_no_device():
    """The symbol is exported with the header's signature, and a null plan is NTT_E_ARG before anything else is looked at."""
    import __graft_entry__ as ge
    import os

    if not os.path.exists(os.path.join(ge.ROOT, "ntt_aie_amd", "libntt_hip.so")):
        ge.build()
    from ntt_aie_amd import _lib

    L = _lib.lib()
    assert "ntt_polymul_matvec_pre" in _lib.EXPORTS
    assert L.ntt_polymul_matvec_pre(None, None, None, 1, 1, 1, None, 0, None) == _lib.NTT_E_ARG
    assert L.ntt_polymul_matvec_pre(None, None, None, 1, 1, 1, None, 1, None) == _lib.NTT_E_ARG
