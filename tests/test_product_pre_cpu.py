"""ntt_polymul_negacyclic_pre in the host index model (tests/emu/emu_product_pre.cpp): the product's fused middle pass with operand b
prepared (pass.h: run_product_pass, PRE = true -- this thread's E words of b^ = InvU(b) loaded in the round-0 layout, no second
inverse) and the launches around it (sequence.h: seq_polymul_pre), against the oracle pipeline; the launch list itself, dumped without
running anything, against what the header promises."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import emu_product_pre_lib

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
CASES = ([(8, GOLD, 7, l) for l in (6, 7, 9, 10, 12, 13, 16, 18)] + [(8, M64, 3, l) for l in (7, 12, 14)] +
         [(4, 998244353, 3, l) for l in (5, 6, 8, 12, 13, 14, 16)] + [(4, 2013265921, 31, 9), (4, 3221225473, 5, 7), (4, 3221225473, 5, 12)])

# what a pointer of a step is (emu_polymul_pre_sequence)
NULL, A, OUT, BHAT, TW_FWD, TW_INV, TW_SC = range(7)
PASS, PRODUCT, ROW_PRODUCT = 0, 2, 3
KEYS = ("family", "inverse", "contig", "log_m", "n", "s0", "variant", "do_scale", "batch", "in", "out", "tw", "tw2", "tw_sc", "in2", "mask")


def _operands(oracle, wb, p, g, logn, batch):
    """a, b (full-range residues, the edge words in row 0), the kind-2 table and b^ = InvU(b) of every row"""
    dt = np.uint32 if wb == 4 else np.uint64
    n = 1 << logn
    T = oracle.make_table(2, n, p, g, wb)
    rng = np.random.default_rng(logn)
    a = (rng.integers(0, 2**63, size=(batch, n), dtype=np.uint64) % np.uint64(p)).astype(dt)
    b = (rng.integers(0, 2**63, size=(batch, n), dtype=np.uint64) % np.uint64(p)).astype(dt)
    a[0, :3] = [p - 1, 0, 1]
    b[0, :3] = [p - 1, p - 1, 0]
    B = oracle.intt(b, T, p, nthreads=4)
    bhat = oracle.pointwise(B, np.ones_like(B), p, n % p)  # the UNSCALED inverse
    return a, b, T, bhat


def _want(oracle, a, b, T, p):
    n = a.shape[1]
    A, B = oracle.intt(a, T, p, nthreads=4), oracle.intt(b, T, p, nthreads=4)
    return oracle.ntt(oracle.pointwise(A, B, p, n % p), T, p, nthreads=4)


@pytest.mark.parametrize("wb,p,g,logn", CASES)
def test_values_against_the_oracle_pipeline(oracle, wb, p, g, logn):
    """Per row and broadcast, out of place and with out aliasing a; target_wgs 8 makes workgroups stream several polynomials and hold
    several per workgroup (batch 37: a ragged last group).  b^ must come back bit-identical."""
    L = emu_product_pre_lib.lib()
    batch = 37 if logn <= 12 else 3
    a, b, T, bhat = _operands(oracle, wb, p, g, logn, batch)
    for rows in (batch, 1):
        bh = np.ascontiguousarray(bhat[:rows])
        want = _want(oracle, a, b if rows == batch else np.repeat(b[:1], batch, axis=0), T, p)
        for alias in (False, True):
            sa, keep = a.copy(), bh.copy()
            out = sa if alias else np.full_like(a, 0xFFFFFFFF)
            rc = L.emu_polymul_pre(wb, logn, p, T.ctypes.data, sa.ctypes.data, bh.ctypes.data, rows, out.ctypes.data, batch, 8, -1)
            assert rc == 0, (wb, p, logn, rows, alias)
            assert np.array_equal(out, want), (wb, p, logn, rows, alias)
            assert np.array_equal(bh, keep), "b^ was written"


@pytest.mark.parametrize("wb,p,g,logn", [(8, GOLD, 7, 9), (8, GOLD, 7, 13), (8, M64, 3, 12), (4, 998244353, 3, 13), (4, 3221225473, 5, 7), (4, 998244353, 3, 16)])
def test_prepared_product_is_the_fused_product_word_for_word(oracle, wb, p, g, logn):
    """prepare(b) = the model's own unscaled inverse (what ntt_polymul_prepare launches), then emu_polymul_pre == emu_polymul_fused(a, b)"""
    batch = 37 if logn <= 12 else 3
    a, b, T, bhat = _operands(oracle, wb, p, g, logn, batch)
    prep = np.zeros_like(b)
    assert emu_lib.lib().emu_transform(wb, logn, p, T.ctypes.data, b.ctypes.data, prep.ctypes.data, batch, 1, 0, 0, 8, 0) == 0
    assert np.array_equal(prep, bhat)
    sa, sb, fused = a.copy(), b.copy(), np.zeros_like(a)
    assert emu_lib.lib().emu_polymul_fused(wb, logn, p, T.ctypes.data, sa.ctypes.data, sb.ctypes.data, fused.ctypes.data, batch, 8) == 0
    sa, out = a.copy(), np.zeros_like(a)
    assert emu_product_pre_lib.lib().emu_polymul_pre(wb, logn, p, T.ctypes.data, sa.ctypes.data, prep.ctypes.data, batch, out.ctypes.data, batch, 8, -1) == 0
    assert np.array_equal(out, fused)


def _steps(wb, logn, p, batch, rows, alt=-1, target_wgs=8192):
    buf = (C.c_int * (16 * 16))()
    n = emu_product_pre_lib.lib().emu_polymul_pre_sequence(wb, logn, p, batch, rows, alt, target_wgs, buf, 16)
    assert n >= 0
    return [dict(zip(KEYS, buf[16 * i:16 * i + 16])) for i in range(n)]


def _passes(wb, logn, p, alt):
    tri, mb = (C.c_int * 24)(), C.c_uint64()
    n = emu_lib.lib().emu_plan_alt(logn, wb, C.c_uint64(p), alt, tri, C.byref(mb))
    assert n > 0
    return [(tri[3 * i], tri[3 * i + 1], tri[3 * i + 2]) for i in range(n)]


@pytest.mark.parametrize("wb,p,logn,batch", [(8, GOLD, 13, 5), (8, GOLD, 16, 5), (8, GOLD, 23, 2), (8, M64, 14, 3), (4, 998244353, 14, 5), (4, 3221225473, 16, 33),
                                             (4, 3221225473, 23, 2)])
@pytest.mark.parametrize("broadcast", [False, True])
def test_fused_size_runs_one_operand_s_column_passes_and_one_middle_step(wb, p, logn, batch, broadcast):
    passes = _passes(wb, logn, p, 0)
    assert len(passes) >= 2
    steps = _steps(wb, logn, p, batch, 1 if broadcast else batch, alt=0)
    k = len(passes) - 1
    assert len(steps) == 2 * k + 1
    for i, st in enumerate(steps[:k]):  # a's inverse column passes, highest first, in place on a, over `batch` rows -- never 2 * batch
        contig, s0, log_m = passes[len(passes) - 1 - i]
        assert (st["family"], st["inverse"], st["contig"], st["s0"], st["log_m"]) == (PASS, 1, 0, s0, log_m)
        assert (st["in"], st["out"], st["tw"], st["in2"], st["batch"], st["do_scale"], st["mask"]) == (A, A, TW_INV, NULL, batch, 0, 0)
    mid = steps[k]
    assert (mid["family"], mid["contig"], mid["s0"], mid["log_m"], mid["batch"]) == (PRODUCT, 1, 0, passes[0][2], batch)
    assert (mid["in"], mid["out"], mid["in2"], mid["tw"], mid["tw2"]) == (A, OUT, BHAT, TW_INV, TW_FWD)
    assert mid["mask"] == (1 | 4 | (2 if broadcast else 0))
    for i, st in enumerate(steps[k + 1:]):  # the forward column passes in place on out
        contig, s0, log_m = passes[1 + i]
        assert (st["family"], st["inverse"], st["contig"], st["s0"], st["log_m"]) == (PASS, 0, 0, s0, log_m)
        assert (st["in"], st["out"], st["tw"], st["in2"], st["batch"], st["mask"]) == (OUT, OUT, TW_FWD, NULL, batch, 0)
    assert sum(st["family"] == PRODUCT for st in steps) == 1


@pytest.mark.parametrize("wb,p,logn", [(8, GOLD, 7), (8, GOLD, 12), (8, M64, 9), (4, 998244353, 6), (4, 998244353, 13), (4, 2013265921, 9)])
@pytest.mark.parametrize("broadcast", [False, True])
def test_single_pass_size_is_exactly_one_step(wb, p, logn, broadcast):
    steps = _steps(wb, logn, p, 37, 1 if broadcast else 37)
    assert len(steps) == 1
    st = steps[0]
    assert (st["family"], st["log_m"], st["n"], st["batch"], st["in"], st["out"], st["in2"]) == (PRODUCT, logn, logn, 37, A, OUT, BHAT)
    assert st["mask"] == (1 | 4 | (2 if broadcast else 0))


@pytest.mark.parametrize("wb,p,logn,alt", [(8, GOLD, 13, 1), (8, GOLD, 6, 0), (4, 998244353, 5, 0), (4, 998244353, 14, 1)])
def test_sizes_without_a_fused_middle_take_the_fallback(wb, p, logn, alt):
    """a pinned 13-stage alternative at Goldilocks 2^13 (and the 14-stage one of a lazy 4-byte prime, and the sizes below the smallest
    unit): a's unscaled inverse in place, then the forward transform with b^ folded into its first pass -- or, the broadcast, the row
    product as a launch of its own and the plain forward transform.  No product-middle step anywhere."""
    assert emu_product_pre_lib.lib().emu_polymul_pre_fused(wb, logn, p, 5, 8192, alt) == 0
    per_row, bcast = _steps(wb, logn, p, 5, 5, alt=alt), _steps(wb, logn, p, 5, 1, alt=alt)
    assert [st["family"] for st in per_row] == [PASS, PASS] and [st["family"] for st in bcast] == [PASS, ROW_PRODUCT, PASS]
    for steps in (per_row, bcast):
        inv, fwd = steps[0], steps[-1]
        assert (inv["inverse"], inv["log_m"], inv["in"], inv["out"], inv["do_scale"], inv["tw_sc"], inv["batch"]) == (1, logn, A, A, 0, NULL, 5)
        assert (fwd["inverse"], fwd["log_m"], fwd["in"], fwd["out"], fwd["batch"]) == (0, logn, A, OUT, 5)
    assert (per_row[1]["in2"], per_row[1]["mask"]) == (BHAT, 4)
    assert (bcast[2]["in2"], bcast[2]["mask"]) == (NULL, 0)
    assert (bcast[1]["in"], bcast[1]["out"], bcast[1]["in2"]) == (A, A, BHAT)
