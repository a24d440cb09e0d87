"""The balanced gadget decomposition and ntt_polymul_gadget_pre without a GPU: the identities of the definition (include/ntt_hip.h) in
Python integers, the argument rule, the host index model (tests/emu/emu_product_gadget.cpp: the digit variants of the summed middle
passes, pass.h run_product_dot_pass / run_product_mv_pass with GAD, and the library's own seq_polymul_gadget) against the reference
(gadget_ref.want: product_dot_ref.want of the reference digits), and the launch list itself, dumped without running anything."""
import ctypes as C

import numpy as np
import pytest

import emu_product_gadget_lib
import emu_product_mv_lib
import gadget_ref as G
import product_dot_ref as R

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
# (word bytes, p, log_base, levels, low_bits)
PARAMS = [(8, GOLD, 16, 4, 0), (8, GOLD, 8, 3, 40), (8, GOLD, 22, 3, 0), (8, GOLD, 1, 5, 0), (8, GOLD, 16, 1, 0), (8, GOLD, 8, 1, 40),
          (8, M64, 16, 4, 0), (8, M64, 10, 3, 32), (4, 998244353, 10, 3, 0), (4, 998244353, 7, 2, 16), (4, 3221225473, 8, 4, 0),
          (4, 3329, 4, 3, 0), (4, 3329, 6, 2, 0)]
# the digit sets the model runs per word class: levels 3 and levels 1
DIGITS = {GOLD: ((8, 3, 40), (16, 1, 0)), M64: ((10, 3, 32), (16, 1, 0)), 998244353: ((10, 3, 0), (7, 1, 16)), 3221225473: ((8, 3, 8), (12, 1, 4)),
          2013265921: ((10, 3, 0), (7, 1, 16))}

NULL, A, OUT, BHAT, TW_FWD, TW_INV, TW_SC, WORK = range(8)
PASS, PRODUCT, ROW_SUMS, DECOMPOSE = 0, 2, 3, 4
KEYS = ("family", "inverse", "contig", "log_m", "n", "s0", "variant", "do_scale", "batch", "in", "out", "tw", "tw2", "tw_sc", "in2", "mask", "terms",
        "a_stride", "b_stride", "mv_outs", "mv_b_stride", "mv_o_stride", "out_at", "in2_at", "log_base", "levels", "low_bits", "zero")


@pytest.mark.parametrize("wb,p,w,K,l", PARAMS)
def test_the_three_identities_in_python_integers(wb, p, w, K, l):
    """Row 0 holds the edge words (gadget_ref.edge_words: 0, 1, around p / 2, p - 1, around the rounding point, and the words whose u has
    every lower digit at B/2 - 1 and at B/2 with both signs, so a carry runs through all levels), the rest is random."""
    assert G.params_ok(p, w, K, l)
    edge = G.edge_words(p, w, K, l)
    n = 256
    assert len(edge) <= n
    a = G.operand(wb, p, w, K, l, 1, 9, n, seed=w + K)[0]
    assert all(int(x) in set(int(v) for v in a[0]) for x in edge)
    s, m, u, e = G.parts_int(a, p, w, K, l)
    B = 1 << w
    assert (sum(ek * B**k for k, ek in enumerate(e)) == u).all()
    assert (2 * abs(s * m - s * u * (1 << l)) <= (1 << l)).all()  # |s m - s u 2^l| <= 2^(l - 1)
    for ek in e[:-1]:
        assert (ek >= -(B // 2)).all() and (ek < B // 2).all()
    assert (e[-1] >= 0).all() and (abs(e[-1]) < p).all()
    d = G.digits_int(a, p, w, K, l)
    neg = ((p - a.astype(object)) % p).astype(a.dtype)
    assert np.array_equal(G.digits_int(neg, p, w, K, l), ((p - d.astype(object)) % p).astype(a.dtype))  # digit_k(p - a) = -digit_k(a)
    assert (d.astype(object) < p).all()
    # the uint64 steps of the reference and of the library's gadget_digit (the host model calls it) are those integers
    assert np.array_equal(G.digits(a, p, w, K, l), d)
    got = np.zeros((K,) + a.shape, dtype=a.dtype)
    assert emu_product_gadget_lib.lib().emu_gadget_digits(wb, p, a.ctypes.data, 1, a.size, w, K, l, got.ctypes.data) == 0
    assert np.array_equal(got, d)
    if l == 0:  # exact: the digits recompose a mod p
        back = sum(d[k].astype(object) * B**k for k in range(K)) % p
        assert (back == a.astype(object)).all()


def test_the_argument_rule():
    """Each condition violated alone is refused, the boundary values are accepted; the library's rule (pass.h: gadget_params_ok, which the
    C-ABI and the launchers call) against the reference's.  The fourth condition, (u_max >> (K - 1) w) + 1 < p, cannot be violated alone:
    for odd p >= 3 and any l, u_max <= (p - 1) / 2, so u_max + 1 <= (p + 1) / 2 < p -- the grid below includes p = 3 and finds no such input."""
    ok = emu_product_gadget_lib.lib().emu_gadget_params_ok
    table = [
        (GOLD, 0, 3, 0, False), (GOLD, 1, 3, 0, True), (GOLD, 31, 1, 0, True), (GOLD, 31, 3, 1, True), (GOLD, 32, 1, 0, False),   # 1 <= w <= 31
        (GOLD, 8, 0, 0, False), (GOLD, 8, 1, 0, True),                                                                       # K >= 1
        (GOLD, 8, 3, -1, False), (GOLD, 8, 3, 0, True),                                                                      # 0 <= l
        (GOLD, 21, 4, 0, True), (GOLD, 16, 4, 15, True), (GOLD, 16, 4, 16, False), (GOLD, 16, 5, 0, False), (GOLD, 8, 1, 63, True), (GOLD, 8, 1, 64, False),  # l + (K - 1) w <= 63
        (3329, 12, 1, 0, True), (3329, 13, 1, 0, False), (3, 1, 1, 0, True), (3, 2, 1, 0, True), (3, 3, 1, 0, False),          # 2^(w - 1) < p
        (GOLD, 16, 4, 0, True), (GOLD, 8, 3, 40, True),                                                                      # the two settings the header names
    ]
    for p, w, K, l, want in table:
        assert G.params_ok(p, w, K, l) == want, (p, w, K, l)
        assert bool(ok(p, w, K, l)) == want, (p, w, K, l)
    for p in (3, 5, 3329, 998244353, M64, GOLD, 0xFFFFFFFFFFFFFFC5):
        for w in (1, 2, 7, 16, 31):
            for K in (1, 2, 5):
                for l in (0, 1, 17, 62, 63):
                    assert bool(ok(p, w, K, l)) == G.params_ok(p, w, K, l), (p, w, K, l)
                    h = (1 << (l - 1)) if l > 0 else 0
                    assert ((((p - 1) // 2 + h) >> l) >> ((K - 1) * w)) + 1 < p  # condition four holds whatever the others say


class _Ref:
    """operands of one shape and digit set; per (output, term, operand shape) that term's product from the oracle pipeline on the
    REFERENCE digits -- computed when first asked for, shared by every combination and plan alternative, never changed"""

    def __init__(self, oracle, wb, p, g, logn, batch, polys, dig, outs, seed):
        self.oracle, self.p, self.dig = oracle, p, dig
        w, K, l = dig
        n = 1 << logn
        self.a = G.operand(wb, p, w, K, l, polys, batch, n, seed)
        self.d = G.decompose(self.a, p, w, K, l)  # [polys, K, batch, n]
        _, b, self.T, bhat = R.operands(oracle, wb, p, g, logn, batch, outs * polys * K, seed)
        self.b, self.bhat = b.reshape(outs, polys * K, batch, n), bhat.reshape(outs, polys * K, batch, n)
        self._c = {}

    def want(self, polys, outs, bcast):
        K = self.dig[1]
        d = self.d.reshape(-1, *self.d.shape[2:])
        res = []
        for j in range(outs):
            acc = None
            for t in range(polys * K):
                if (j, t, bcast) not in self._c:
                    self._c[(j, t, bcast)] = R.want(self.oracle, d[t:t + 1], self.b[j, t:t + 1], self.T, self.p, bcast)
                c = self._c[(j, t, bcast)]
                acc = c if acc is None else R.addmod(acc, c, self.p)
            res.append(acc)
        return np.stack(res)


def _exp(p):
    """The product library uses the digit kernels for the general 64-bit modulus only (launch.h: product_gadget_unit, decided by
    profiles/polymul_gadget_ab.txt); the other two classes are stepped in the model compiled as the experiment build, which keeps them"""
    return p != M64


def _run(ref, wb, p, logn, alt, combos, unfused=0, single=0):
    L = emu_product_gadget_lib.lib(_exp(p))
    w, K, l = ref.dig
    for polys, outs, batch, bcast in combos:
        rows = 1 if bcast else batch
        a = np.ascontiguousarray(ref.a[:polys, :batch])
        bh = np.ascontiguousarray(ref.bhat[:outs, :polys * K, :rows])
        keep_a, keep_b = a.copy(), bh.copy()
        work = np.full((polys * K, batch, 1 << logn), 0xEEEEEEEE, dtype=a.dtype)
        out = np.full((outs, batch, 1 << logn), 0xFFFFFFFF, dtype=a.dtype)
        rc = L.emu_polymul_gadget(wb, logn, p, ref.T.ctypes.data, a.ctypes.data, polys, w, K, l, work.ctypes.data, bh.ctypes.data, rows, outs, out.ctypes.data, batch, 8,
                                  alt, unfused, single)
        assert rc == 0, (wb, p, logn, alt, polys, outs, batch, bcast)
        assert np.array_equal(out, ref.want(polys, outs, bcast)[:, :batch]), (wb, p, logn, alt, polys, outs, batch, bcast, ref.dig)
        assert np.array_equal(a, keep_a), "a was written"
        assert np.array_equal(bh, keep_b), "b^ was written"
        fused = L.emu_polymul_gadget_fused(wb, logn, p, batch, 8, alt, unfused)
        if fused:  # (the other path leaves the transformed digits there: unspecified contents)
            assert (work == work.dtype.type(0xEEEEEEEE)).all(), "the fused path touched work"


# every fused unit size per word class as a single-pass size (8-byte words 2^7 .. 2^12, 4-byte words 2^6 .. 2^12), the two units without
# a summed kernel (general 64-bit 2^10, 4-byte 2^13), the size below the smallest unit and one two-pass size
CASES = ([(8, GOLD, 7, l) for l in (6, 7, 8, 9, 10, 11, 12, 13)] + [(8, M64, 3, l) for l in (7, 8, 9, 10, 11, 12, 14)] +
         [(4, 998244353, 3, l) for l in (5, 6, 7, 8, 9, 10, 11, 12, 13, 14)] + [(4, 2013265921, 31, 9), (4, 3221225473, 5, 7)])
NO_DIGIT_KERNEL = {(GOLD, 6), (GOLD, 13), (M64, 10), (M64, 14), (998244353, 5), (998244353, 13), (998244353, 14)}


@pytest.mark.parametrize("wb,p,g,logn", CASES)
def test_values_against_the_reference(oracle, wb, p, g, logn):
    """Both digit sets of the class, every plan alternative (a pinned one without a middle takes the decomposition kernel).  Batch 33 makes
    workgroups hold several polynomials with a ragged last group and stream several groups (target_wgs 8); the large units run batch 5,
    where the model steps every lane of 5 x 6 terms."""
    L = emu_product_gadget_lib.lib(_exp(p))
    top = 33 if logn <= 9 else 5
    has_kernel = (p if p in (GOLD, M64) else 998244353, logn) not in NO_DIGIT_KERNEL
    assert (L.emu_polymul_gadget_fused(wb, logn, p, top, 8, 0, 0) != 0) == has_kernel
    assert (emu_product_gadget_lib.lib().emu_polymul_gadget_fused(wb, logn, p, top, 8, 0, 0) != 0) == (has_kernel and p == M64)  # what the product library does
    for dig in DIGITS[p]:
        ref = _Ref(oracle, wb, p, g, logn, top, 2, dig, 3, seed=100 * logn + dig[1])
        # (polys, outs, batch, broadcast): a summed launch alone, a pair, a pair and a summed launch; one and two polynomials; per row and broadcast
        combos = [(2, 3, top, False), (2, 2, top, True), (1, 1, top, True), (1, 3, 1, False)]
        for alt in range(L.emu_polymul_gadget_alternatives(wb, logn, p)):
            _run(ref, wb, p, logn, alt, combos if alt == 0 else combos[:2])


@pytest.mark.parametrize("wb,p,g,logn", [(8, GOLD, 7, 7), (8, M64, 3, 7), (4, 998244353, 3, 6)])
def test_every_polynomial_level_output_count_batch_and_operand_shape(oracle, wb, p, g, logn):
    for dig in DIGITS[p]:
        ref = _Ref(oracle, wb, p, g, logn, 33, 2, dig, 3, seed=77)
        _run(ref, wb, p, logn, -1, [(q, j, b, bc) for q in (1, 2) for j in (1, 2, 3) for b in (1, 5, 33) for bc in (False, True)])


@pytest.mark.parametrize("wb,p,g,logn", [(8, GOLD, 7, 10), (8, M64, 3, 9), (4, 998244353, 3, 11), (4, 3221225473, 5, 12)])
def test_the_switches_of_the_experiment_build_give_the_same_words(oracle, wb, p, g, logn):
    """NTT_GADGET_UNFUSED (the decomposition kernel and the digits' product at a size with digit kernels) and NTT_MATVEC_SINGLE (one summed
    digit launch per output): the reference's words on every path, which is the bit-for-bit contract of the header"""
    ref = _Ref(oracle, wb, p, g, logn, 5, 2, DIGITS[p][0], 3, seed=5)
    for unfused, single in ((0, 0), (1, 0), (0, 1)):
        _run(ref, wb, p, logn, -1, [(2, 3, 5, False), (2, 2, 5, True)], unfused, single)


def _steps(wb, logn, p, batch, rows, polys, dig, outs, alt=-1, target_wgs=8192, unfused=0, single=0, experiment=False):
    buf = (C.c_int * (28 * 24))()
    n = emu_product_gadget_lib.lib(experiment).emu_polymul_gadget_sequence(wb, logn, p, batch, rows, polys, *dig, outs, alt, target_wgs, unfused, single, buf, 24)
    assert n >= 0
    return [dict(zip(KEYS, buf[28 * i:28 * i + 28])) for i in range(n)]


def _mv_steps(wb, logn, p, batch, rows, terms, outs, alt=-1, target_wgs=8192, single=0):
    buf = (C.c_int * (24 * 24))()
    n = emu_product_mv_lib.lib().emu_polymul_matvec_sequence(wb, logn, p, batch, rows, terms, outs, alt, target_wgs, single, buf, 24)
    assert n >= 0
    return [dict(zip(KEYS[:24], buf[24 * i:24 * i + 24])) for i in range(n)]


@pytest.mark.parametrize("wb,p,logn", [(8, GOLD, 7), (8, GOLD, 10), (8, GOLD, 12), (8, M64, 9), (8, M64, 11), (4, 998244353, 6), (4, 998244353, 12), (4, 2013265921, 9)])
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("outs", [1, 2, 3, 4])
def test_the_fused_path_is_the_digit_launches_alone(wb, p, logn, broadcast, outs):
    """no decomposition step and no pass over work: one digit launch per pair of outputs plus one for an odd last output where the
    two-output kernel is used, else one per output; each reads a itself.  The general 64-bit modulus in the product build; Goldilocks and
    4-byte words in the experiment build, which keeps their digit kernels and pairs outputs for every class"""
    dig, polys, batch = (8, 3, 0), 2, 37
    rows, terms = (1 if broadcast else batch), 6
    steps = _steps(wb, logn, p, batch, rows, polys, dig, outs, experiment=_exp(p))
    paired = True
    assert emu_product_gadget_lib.lib(_exp(p)).emu_polymul_gadget_fused(wb, logn, p, batch, 8192, -1, 0) == 2
    assert emu_product_gadget_lib.lib().emu_polymul_gadget_fused(wb, logn, p, batch, 8192, -1, 0) == (2 if p == M64 else 0)
    assert len(steps) == ((outs + 1) // 2 if paired else outs)
    j = 0
    for mid in steps:
        two = paired and j + 1 < outs
        assert (mid["family"], mid["contig"], mid["s0"], mid["log_m"], mid["n"], mid["batch"]) == (PRODUCT, 1, 0, logn, logn, batch)
        assert (mid["in"], mid["out"], mid["in2"], mid["tw"], mid["tw2"]) == (A, OUT, BHAT, TW_INV, TW_FWD)
        assert mid["mask"] == (1 | 4 | (2 if broadcast else 0))
        assert (mid["terms"], mid["a_stride"], mid["b_stride"]) == (terms, batch, rows)
        assert (mid["out_at"], mid["in2_at"]) == (j * batch, j * terms * rows)
        assert (mid["mv_outs"], mid["mv_b_stride"], mid["mv_o_stride"]) == ((2, terms * rows, batch) if two else (0, 0, 0))
        assert (mid["log_base"], mid["levels"], mid["low_bits"]) == dig
        j += 2 if two else 1
    assert j == outs
    assert all(WORK not in (st["in"], st["out"], st["in2"]) and st["family"] != DECOMPOSE for st in steps)


@pytest.mark.parametrize("wb,p,logn,alt,unfused", [(8, GOLD, 13, 0, 0), (8, GOLD, 13, 1, 0), (8, GOLD, 6, 0, 0), (8, GOLD, 16, 0, 0), (8, M64, 10, 0, 0), (4, 998244353, 13, 0, 0),
                                                  (4, 998244353, 14, 0, 0), (4, 998244353, 5, 0, 0), (8, M64, 12, 0, 1), (8, M64, 9, 0, 1), (8, GOLD, 12, 0, 0), (8, GOLD, 7, 0, 0),
                                                  (4, 998244353, 12, 0, 0), (4, 2013265921, 9, 0, 0)])
@pytest.mark.parametrize("broadcast", [False, True])
@pytest.mark.parametrize("outs", [1, 3])
def test_every_other_case_is_the_decomposition_and_exactly_the_matvec_steps(wb, p, logn, alt, unfused, broadcast, outs):
    """a multi-pass size, a size without a fused middle, a unit without a digit kernel, a pinned alternative without a middle, the
    experiment build's switch, and -- in the product library -- every size of the two word classes it does not use the digit kernels for: ONE decomposition step a -> work, then the launch list of seq_polymul_matvec on work, step for step"""
    dig, polys, batch = (8, 3, 0), 2, 5
    rows, terms = (1 if broadcast else batch), 6
    assert emu_product_gadget_lib.lib().emu_polymul_gadget_fused(wb, logn, p, batch, 8192, alt, unfused) == 0
    steps = _steps(wb, logn, p, batch, rows, polys, dig, outs, alt=alt, unfused=unfused)
    dec = steps[0]
    assert (dec["family"], dec["in"], dec["out"], dec["batch"], dec["terms"], dec["n"]) == (DECOMPOSE, A, WORK, batch, terms, logn)
    assert (dec["log_base"], dec["levels"], dec["low_bits"]) == dig
    mv = _mv_steps(wb, logn, p, batch, rows, terms, outs, alt=alt)
    assert len(steps) == 1 + len(mv)
    for got, want in zip(steps[1:], mv):
        assert (got["log_base"], got["levels"], got["low_bits"]) == (0, 0, 0)  # no digit parameters on any of them
        assert A not in (got["in"], got["out"], got["in2"])  # a itself is never passed on
        mapped = {k: (A if k in ("in", "out") and got[k] == WORK else got[k]) for k in KEYS[:24]}
        assert mapped == want


def test_the_model_refuses_what_the_c_abi_refuses():
    L = emu_product_gadget_lib.lib()
    n = 64
    a, work, bh, out = (np.zeros(k * n, dtype=np.uint64) for k in (2 * 4, 6 * 4, 2 * 6 * 4, 2 * 4))
    T = np.ones(n, dtype=np.uint64)

    def call(a_=a, work_=work, bh_=bh, out_=out, rows=4, polys=2, dig=(8, 3, 0), outs=2):
        return L.emu_polymul_gadget(8, 6, GOLD, T.ctypes.data, a_.ctypes.data, polys, *dig, work_.ctypes.data, bh_.ctypes.data, rows, outs, out_.ctypes.data, 4, 8, -1, 0, 0)

    assert call(rows=2) == -1       # bhat_rows is neither 1 nor batch
    assert call(polys=0) == -1
    assert call(outs=0) == -1
    assert call(polys=1 << 28) == -1  # polys * levels * batch beyond the row limit
    assert call(outs=1 << 30) == -1
    for dig in ((0, 3, 0), (8, 0, 0), (8, 3, -1), (16, 5, 0)):
        assert call(dig=dig) == -1
    for x, y in (("a_", "work_"), ("a_", "bh_"), ("a_", "out_"), ("work_", "bh_"), ("work_", "out_"), ("bh_", "out_")):  # every overlap pair
        big = np.zeros(2 * 6 * 4 * n, dtype=np.uint64)
        assert call(**{x: big, y: big}) == -1


def test_c_abi_rules_that_need_no_device():
    """The symbols are exported with the header's signatures, and a null plan is NTT_E_ARG before anything else is looked at."""
    import os

    import __graft_entry__ as ge

    if not os.path.exists(os.path.join(ge.ROOT, "ntt_aie_amd", "libntt_hip.so")):
        ge.build()
    from ntt_aie_amd import _lib

    L = _lib.lib()
    assert "ntt_gadget_decompose" in _lib.EXPORTS and "ntt_polymul_gadget_pre" in _lib.EXPORTS
    assert L.ntt_gadget_decompose(None, None, 1, 1, 8, 3, 0, None, None) == _lib.NTT_E_ARG
    assert L.ntt_gadget_decompose(None, None, 1, 0, 8, 3, 0, None, None) == _lib.NTT_E_ARG
    assert L.ntt_polymul_gadget_pre(None, None, 1, 8, 3, 0, None, None, 1, 1, None, 0, None) == _lib.NTT_E_ARG
    assert L.ntt_polymul_gadget_pre(None, None, 1, 8, 3, 0, None, None, 1, 1, None, 1, None) == _lib.NTT_E_ARG
