"""The launch list of every entry point (ntt_aie_amd/csrc/sequence.h), dumped step by step without running anything (tests/emu/emu.cpp:
emu_sequence) and compared, whole, with what the header's contract says: forward passes ascending, inverse passes descending, only the
first step reads the caller's input, an operand rides on the one pass that holds stage 0.  The expectations are written here from
that contract and the planner's own answers (emu_plan_alt, emu_column_passes), not from the sequencer."""
import ctypes as C

import pytest

GOLD = 0xFFFFFFFF00000001
M32 = 998244353  # a lazy 4-byte prime: N = 2^14 has a one-pass alternative

# what a pointer of a step is (emu_sequence)
NULL, IN, OUT, B, TW_FWD, TW_INV, TW_SC, LDE_S, CINV_U = range(9)
PASS, MAT, PRODUCT = 0, 1, 2
FORWARD, INVERSE, LDE, COSET_INVERSE, FORWARD_COLUMNS, INVERSE_COLUMNS, LDE_COLUMNS, COSET_INVERSE_COLUMNS, POLYMUL, POLYMUL_CONTIGUOUS = range(10)


def _steps(call, wb, logn, p, batch, alt=-1, scale=0, beta=0, width=0):
    import emu_lib

    L = emu_lib.lib()
    buf = (C.c_int * (16 * 16))()
    n = L.emu_sequence(call, wb, logn, p, batch, alt, scale, beta, width, buf, 16)
    assert n >= 0, (call, wb, logn, batch, alt)
    keys = ("family", "inverse", "contig", "log_m", "n", "s0", "variant", "do_scale", "batch", "in", "out", "tw", "tw2", "tw_sc", "in2", "coset")
    return [dict(zip(keys, buf[16 * i:16 * i + 16])) for i in range(n)]


def _alternatives(wb, logn, p):
    """[(contig, s0, log_m, variant)] of every plan alternative, from the planner"""
    import emu_lib

    L = emu_lib.lib()
    out = []
    for alt in range(8):
        tri, mb = (C.c_int * 24)(), C.c_uint64()
        n = L.emu_plan_alt(logn, wb, C.c_uint64(p), alt, tri, C.byref(mb))
        if n < 0:
            break
        out.append([(tri[3 * i], tri[3 * i + 1], tri[3 * i + 2], L.emu_plan_alt_variant(logn, wb, C.c_uint64(p), alt, i)) for i in range(n)])
    return out


def _selected(wb, logn, p, batch):
    import emu_lib

    return _alternatives(wb, logn, p)[emu_lib.lib().emu_select_alt(logn, wb, C.c_uint64(p), C.c_uint64(batch))]


def _column_passes(logn):
    import emu_columns_lib

    s0, m = (C.c_int * 8)(), (C.c_int * 8)()
    n = emu_columns_lib.lib().emu_column_passes(logn, s0, m, 8)
    return [(s0[i], m[i]) for i in range(n)]


def _step(family, inverse, pd, n, batch, src, **kw):
    """one ordinary step on `pd` = (contig, s0, log_m, variant): the table of the direction, in place on the output unless `src` says
    otherwise, no operand; kw overrides"""
    contig, s0, log_m, variant = pd
    d = {"family": family, "inverse": int(inverse), "contig": contig, "log_m": log_m, "n": n, "s0": s0, "variant": variant, "do_scale": 0,
         "batch": batch, "in": src, "out": OUT, "tw": TW_INV if inverse else TW_FWD, "tw2": NULL, "tw_sc": NULL, "in2": NULL, "coset": 0}
    d.update(kw)
    return d


@pytest.mark.parametrize("scale", [1, 0])
def test_inverse_runs_descending_and_scales_on_stage_0_only(scale):
    passes = _selected(8, 16, GOLD, 4)
    assert len(passes) == 2 and passes[0][0] == 1 and passes[0][1] == 0
    want = [_step(PASS, True, passes[1], 16, 4, IN),
            _step(PASS, True, passes[0], 16, 4, OUT, do_scale=scale, tw_sc=TW_SC if scale else NULL)]
    assert _steps(INVERSE, 8, 16, GOLD, 4, scale=scale) == want


def test_lde_first_step_carries_the_coset_operands_and_is_handed_the_output():
    passes = _selected(8, 16, GOLD, 4)
    want = [_step(PASS, False, passes[0], 16, 4, OUT, coset=1 | 2 | (2 << 8)), _step(PASS, False, passes[1], 16, 4, OUT)]
    assert _steps(LDE, 8, 16, GOLD, 4, beta=2) == want


@pytest.mark.parametrize("wb,logn,p", [(8, 16, GOLD), (4, 14, M32)])
def test_coset_inverse_vector_rides_on_the_last_step_unscaled(wb, logn, p):
    alts = _alternatives(wb, logn, p)
    assert len(alts) == (2 if wb == 4 else 1)
    for alt, passes in enumerate(alts):
        order = passes[::-1]
        want = [_step(PASS, True, pd, logn, 3, IN if k == 0 else OUT, coset=4 if k == len(order) - 1 else 0) for k, pd in enumerate(order)]
        got = _steps(COSET_INVERSE, wb, logn, p, 3, alt=alt)
        assert got == want and all(s["do_scale"] == 0 for s in got), alt


@pytest.mark.parametrize("wb,p", [(8, GOLD), (4, M32)])
def test_columns_three_steps_over_the_virtual_polynomial(wb, p):
    logn, width, count, beta = 17, 17, 2, 3
    w = max(4 if wb == 8 else 5, (width - 1).bit_length())  # the column tile is 16 words of 8 bytes / 32 of 4 wide at least
    cols = _column_passes(logn)
    assert [m for _, m in cols] == [6, 6, 5] and cols[0][0] == 0
    n = logn + w

    def mat(inverse, k, order, **kw):
        s0, m = order[k]
        return _step(MAT, inverse, (0, s0 + w, m, 0), n, count, IN if k == 0 else OUT, **kw)

    fwd, inv = cols, cols[::-1]
    assert _steps(FORWARD_COLUMNS, wb, logn, p, count, width=width) == [mat(False, k, fwd) for k in range(3)]
    for scale in (0, 1):
        want = [mat(True, k, inv, do_scale=scale if inv[k][0] == 0 else 0) for k in range(3)]
        assert want[2]["s0"] == w and _steps(INVERSE_COLUMNS, wb, logn, p, count, scale=scale, width=width) == want
    # the fused expansion is the step with stage 0, which runs first and is handed the output as its ordinary input
    want = [mat(False, 0, fwd, coset=16 | 32 | (beta << 8), **{"in": OUT}), mat(False, 1, fwd), mat(False, 2, fwd)]
    assert _steps(LDE_COLUMNS, wb, logn, p, count, beta=beta, width=width) == want
    # the interpolation vector is on that step of the inverse, which runs last; N^-1 is inside the vector
    want = [mat(True, 0, inv), mat(True, 1, inv), mat(True, 2, inv, coset=64)]
    got = _steps(COSET_INVERSE_COLUMNS, wb, logn, p, count, width=width)
    assert got == want and all(s["do_scale"] == 0 for s in got)
    # the plain middle step runs in place
    assert all(s[1]["in"] == OUT and s[1]["out"] == OUT and s[1]["coset"] == 0 for s in (got, want))


@pytest.mark.parametrize("contiguous", [False, True])
def test_polymul_inverse_columns_then_middle_then_forward_columns(contiguous):
    passes = _selected(8, 16, GOLD, 4)
    first, col = passes
    mid = _step(PRODUCT, False, first, 16, 4, IN, tw=TW_INV, tw2=TW_FWD, in2=B)
    if contiguous:
        head = [_step(PASS, True, col, 16, 8, IN, out=IN)]
    else:
        head = [_step(PASS, True, col, 16, 4, IN, out=IN), _step(PASS, True, col, 16, 4, B, out=B)]
    want = head + [mid, _step(PASS, False, col, 16, 4, OUT)]
    assert _steps(POLYMUL_CONTIGUOUS if contiguous else POLYMUL, 8, 16, GOLD, 4) == want


def test_polymul_of_a_single_pass_size_is_one_step():
    (first,) = _selected(8, 9, GOLD, 4)
    assert _steps(POLYMUL, 8, 9, GOLD, 4) == [_step(PRODUCT, False, first, 9, 4, IN, tw=TW_INV, tw2=TW_FWD, in2=B)]


@pytest.mark.parametrize("wb,logn,p,nalt", [(4, 14, M32, 2), (8, 13, GOLD, 2), (8, 12, GOLD, 2)])
def test_forward_steps_are_the_alternative_s_passes_with_its_variant(wb, logn, p, nalt):
    alts = _alternatives(wb, logn, p)
    assert len(alts) == nalt
    for alt, passes in enumerate(alts):
        want = [_step(PASS, False, pd, logn, 5, IN if k == 0 else OUT) for k, pd in enumerate(passes)]
        assert _steps(FORWARD, wb, logn, p, 5, alt=alt) == want, alt
    if logn == 12:
        assert [a[0][3] for a in alts] == [1, 0]  # the wide variant below the threshold, the default kernel above
