"""ntt_gadget_decompose and ntt_polymul_gadget_pre on a real MI355X, through NTTPlan, bit-exact against gadget_ref (the definition of
the digits in integers, then the reference of ntt_polymul_dot_pre on them) and equal to polymul_matvec_pre(gadget_decompose(a)) run on
the device.  The smallest shapes that reach each kernel: per word class the size below the smallest unit (the decomposition kernel and
the row sums), the smallest unit (several polynomials per workgroup), the first 512-thread unit, one unit per workgroup, a two-pass size
and a pinned alternative without a middle (the decomposition kernel, then the matrix-vector product), the two units without a summed
kernel, the digit kernels the product library uses (the general 64-bit modulus: 2^8, 2^9 and the multi-wave two-output ones at 2^11 and
2^12; Goldilocks and 4-byte words take the decomposition kernel at every size: launch.h, product_gadget_unit) and the three
4-byte instruction streams -- each with 1, 2 and 3 outputs, 1 and 2 polynomials, 1 and 3 levels, batches 1, 5 and 33, per row and
broadcast, the edge words of the decomposition in row 0.  ntt_plan_info 15 is asserted per shape, so a change of launch.h's
product_gadget_unit cannot silently take the digit kernels out of this file."""
import os

import numpy as np
import pytest

import gadget_ref as G
import product_dot_ref as R

pytestmark = pytest.mark.gpu

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
OUTS, POLYS, BATCHES = (1, 2, 3), (1, 2), (1, 5, 33)
# digit sets per modulus: levels 3 and levels 1
DIGITS = {GOLD: ((8, 3, 40), (16, 1, 0)), M64: ((10, 3, 32), (16, 1, 0)), 998244353: ((10, 3, 0), (7, 1, 16)), 2013265921: ((10, 3, 0), (7, 1, 16)),
          3221225473: ((8, 3, 8), (12, 1, 4)), 3329: ((4, 3, 0), (6, 1, 0))}
# (word bytes, p, g, logn, pinned alternative or None, ntt_plan_info 15)
SHAPES = [
    (8, GOLD, 7, 6, None, 0),    # no product unit below 2^7
    (8, GOLD, 7, 7, None, 0),    # the smallest unit, 16 polynomials per workgroup: Goldilocks takes the decomposition kernel (launch.h: product_gadget_unit)
    (8, GOLD, 7, 10, None, 0),   # the first 512-thread unit
    (8, GOLD, 7, 12, None, 0),   # one unit per workgroup
    (8, GOLD, 7, 13, None, 0),   # 7 + 6: two passes, so the decomposition kernel
    (8, GOLD, 7, 13, 1, 0),      # the 13-stage alternative pinned: no middle
    (8, M64, 3, 8, None, 1),     # the digit kernels the product library uses: the general 64-bit modulus
    (8, M64, 3, 9, None, 1),
    (8, M64, 3, 10, None, 0),    # no summed kernel for this unit
    (8, M64, 3, 11, None, 1),    # the multi-wave two-output digit kernels
    (8, M64, 3, 12, None, 1),
    (4, 998244353, 3, 6, None, 0),  # 4-byte words take the decomposition kernel too
    (4, 998244353, 3, 10, None, 0),
    (4, 998244353, 3, 11, None, 0),
    (4, 998244353, 3, 12, None, 0),
    (4, 998244353, 3, 13, None, 0),  # no summed kernel for this unit
    (4, 2013265921, 31, 11, None, 0),  # a 31-bit prime
    (4, 3221225473, 5, 12, None, 0),   # above 2^31
    (4, 3329, 3, 7, None, 0),          # 3 generates Z_3329^*, and 2N = 256 divides 3328
]


@pytest.fixture(scope="module")
def eng():
    import torch

    import ntt_aie_amd as E

    assert torch.cuda.is_available()
    assert os.path.exists(E.LIB_PATH), "native library missing: the GPU tests must not pass without it"
    torch.cuda.set_device(0)
    return E


def _plan(eng, oracle, wb, p, g, logn, alt=None):
    pl = eng.NTTPlan(logn, p, wb, 0)
    pl.generate_twiddles(2, g)
    T = oracle.make_table(2, 1 << logn, p, g, wb)
    assert np.array_equal(pl.get_twiddles(), T)
    if alt is not None:
        pl.set_policy(alt)
    return pl, T


class _Ref:
    """one reference per shape and digit set, at the largest batch, polynomial and output count: rows are independent, so a smaller batch
    is the first rows of the same arrays, fewer polynomials the first terms.  Per (output, term, operand shape) the term's product from the
    oracle pipeline on the reference digits, computed once and never changed"""

    def __init__(self, oracle, wb, p, g, logn, dig, seed):
        self.oracle, self.p, self.dig = oracle, p, dig
        w, K, l = dig
        n, top, polys, outs = 1 << logn, max(BATCHES), max(POLYS), max(OUTS)
        self.a = G.operand(wb, p, w, K, l, polys, top, n, seed)
        self.d = G.decompose(self.a, p, w, K, l)
        _, b, self.T, bhat = R.operands(oracle, wb, p, g, logn, top, outs * polys * K, seed)
        self.b, self.bhat = b.reshape(outs, polys * K, top, n), bhat.reshape(outs, polys * K, top, n)
        self._c = {}

    def want(self, polys, outs, bcast):
        d = self.d.reshape(-1, *self.d.shape[2:])
        res = []
        for j in range(outs):
            acc = None
            for t in range(polys * self.dig[1]):
                if (j, t, bcast) not in self._c:
                    self._c[(j, t, bcast)] = R.want(self.oracle, d[t:t + 1], self.b[j, t:t + 1], self.T, self.p, bcast)
                acc = self._c[(j, t, bcast)] if acc is None else R.addmod(acc, self._c[(j, t, bcast)], self.p)
            res.append(acc)
        return np.stack(res)


@pytest.mark.parametrize("wb,p,g,logn,alt,fused", SHAPES)
def test_bit_exact_against_the_reference_and_the_unfused_composition(eng, oracle, wb, p, g, logn, alt, fused):
    from ntt_aie_amd import _lib

    pl, T = _plan(eng, oracle, wb, p, g, logn, alt)
    assert _lib.lib().ntt_plan_info(pl._h, 15) == fused
    n = 1 << logn
    for dig in DIGITS[p]:
        w, K, l = dig
        ref = _Ref(oracle, wb, p, g, logn, dig, seed=1000 * wb + logn + K)
        assert np.array_equal(ref.T, T)
        for batch in BATCHES:
            for polys in POLYS:
                a = np.ascontiguousarray(ref.a[:polys, :batch])
                d_a = eng.to_device(a, "cuda:0")
                # the decomposition alone, against the reference digits
                d_dig = pl.gadget_decompose(d_a, w, K, l)
                assert np.array_equal(eng.to_host(d_dig), ref.d[:polys, :, :batch]), (logn, dig, batch, polys)
                for outs in OUTS:
                    for bcast, bh in ((False, ref.bhat[:outs, :polys * K, :batch]), (True, ref.bhat[:outs, :polys * K, :1]), (True, ref.bhat[:outs, :polys * K, 0])):
                        bh = np.ascontiguousarray(bh)
                        d_bh = eng.to_device(bh, "cuda:0")
                        out = eng.to_device(np.zeros((outs, batch, n), dtype=a.dtype), "cuda:0")
                        work = eng.to_device(np.zeros((polys * K, batch, n), dtype=a.dtype), "cuda:0")
                        got = pl.polymul_gadget_pre(d_a, w, K, l, d_bh, work, out)
                        assert got is out
                        host = eng.to_host(out)
                        assert np.array_equal(host, ref.want(polys, outs, bcast)[:, :batch]), (logn, dig, batch, polys, outs, bh.shape)
                        # ... and the matrix-vector product of the decomposition kernel's digits, on the device (it overwrites its a: a copy)
                        mv = pl.polymul_matvec_pre(d_dig.clone().view(polys * K, batch, n), d_bh)
                        assert np.array_equal(host, eng.to_host(mv)), (logn, dig, batch, polys, outs, bh.shape)
                        assert np.array_equal(eng.to_host(d_bh), bh), "b^ was written"
                assert np.array_equal(eng.to_host(d_a), a), "a was written"


@pytest.mark.parametrize("wb,p,g,logn", [(8, GOLD, 7, 13), (4, 998244353, 3, 14)])
def test_the_same_words_whatever_the_decomposition_and_on_a_clone(eng, oracle, wb, p, g, logn):
    pl, _ = _plan(eng, oracle, wb, p, g, logn)
    w, K, l = DIGITS[p][0]
    a = G.operand(wb, p, w, K, l, 2, 5, 1 << logn, seed=3)
    _, _, _, bhat = R.operands(oracle, wb, p, g, logn, 5, 2 * 2 * K, seed=4)
    d_a, d_bh = eng.to_device(a, "cuda:0"), eng.to_device(bhat.reshape(2, 2 * K, 5, -1), "cuda:0")
    first = eng.to_host(pl.polymul_gadget_pre(d_a, w, K, l, d_bh))  # work and out allocated by the call
    other = pl.clone()
    other.set_policy(1)
    assert np.array_equal(eng.to_host(other.polymul_gadget_pre(d_a, w, K, l, d_bh)), first)
    assert np.array_equal(eng.to_host(d_a), a)


@pytest.mark.parametrize("wb,p,g,logn,batch", [(8, GOLD, 7, 7, 5), (4, 998244353, 3, 6, 33), (8, M64, 3, 8, 5), (8, GOLD, 7, 6, 5)])
@pytest.mark.parametrize("broadcast", [False, True])
def test_nothing_outside_the_callers_words_is_touched(eng, oracle, wb, p, g, logn, batch, broadcast):
    """a, work, b^ and out each in the middle of an allocation of its own, one polynomial of sentinel words on both sides, three outputs, a
    ragged last polynomial group (batch 5 of 16 per workgroup, 33 of 64): the digit launches read a itself and must not need anything
    beyond its last polynomial's last row, nor beyond the last output's last term of b^ -- of a broadcast, that term's single row"""
    import torch

    pl, T = _plan(eng, oracle, wb, p, g, logn)
    n, polys, outs = 1 << logn, 2, 3
    w, K, l = DIGITS[p][0]
    a = G.operand(wb, p, w, K, l, polys, batch, n, seed=11)
    _, b, _, bhat = R.operands(oracle, wb, p, g, logn, batch, outs * polys * K, seed=12)
    b, bhat = b.reshape(outs, polys * K, batch, n), bhat.reshape(outs, polys * K, batch, n)
    rows = 1 if broadcast else batch
    bhat = np.ascontiguousarray(bhat[:, :, :rows])
    want = np.stack([G.want(oracle, a, b[j], T, p, w, K, l, broadcast) for j in range(outs)])
    tdt = torch.int32 if wb == 4 else torch.int64
    sentinel = 0x5A5A5A5A if wb == 4 else 0x5A5A5A5A5A5A5A5A

    def framed(words):
        flat = words.reshape(-1, n)
        buf = torch.full((flat.shape[0] + 2, n), sentinel, dtype=tdt, device="cuda:0")
        buf[1:-1].copy_(eng.to_device(flat, "cuda:0"))
        return buf

    fa, fw, fb, fo = framed(a), framed(np.zeros((polys * K, batch, n), dtype=a.dtype)), framed(bhat), framed(np.zeros_like(want))
    pl.polymul_gadget_pre(fa[1:-1].view(polys, batch, n), w, K, l, fb[1:-1].view(outs, polys * K, rows, n), fw[1:-1].view(polys * K, batch, n), fo[1:-1].view(outs, batch, n))
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(fo[1:-1]).reshape(outs, batch, n), want)
    for buf in (fa, fw, fb, fo):
        assert bool((buf[0] == sentinel).all()) and bool((buf[-1] == sentinel).all())
    assert np.array_equal(eng.to_host(fa[1:-1]), a.reshape(-1, n))
    assert np.array_equal(eng.to_host(fb[1:-1]), bhat.reshape(-1, n))


def test_c_abi_errors(eng, oracle):
    import torch

    from ntt_aie_amd import _lib

    L = _lib.lib()
    pl, _ = _plan(eng, oracle, 8, GOLD, 7, 7)
    n, row = 128, 128 * 8
    a = torch.zeros((2, 5, n), dtype=torch.int64, device="cuda:0")
    work = torch.zeros((6, 5, n), dtype=torch.int64, device="cuda:0")
    bh = torch.zeros((2, 6, 5, n), dtype=torch.int64, device="cuda:0")
    out = torch.zeros((2, 5, n), dtype=torch.int64, device="cuda:0")
    A, W, B, O = a.data_ptr(), work.data_ptr(), bh.data_ptr(), out.data_ptr()

    def gp(a_=A, polys=2, dig=(8, 3, 40), w_=W, b_=B, rows=5, outs=2, o_=O, batch=5, plan=pl):
        return L.ntt_polymul_gadget_pre(plan._h, a_, polys, *dig, w_, b_, rows, outs, o_, batch, None)

    assert gp() == 0
    assert gp(rows=1) == 0
    # every overlap pair: the second range begins in the last row of the first
    assert gp(w_=A + 9 * row) == -1 and gp(a_=W + 29 * row) == -1      # a / work
    assert gp(b_=A + 9 * row) == -1 and gp(a_=B + 59 * row) == -1      # a / b^
    assert gp(o_=A + 9 * row) == -1 and gp(a_=O + 9 * row) == -1       # a / out
    assert gp(b_=W + 29 * row) == -1 and gp(w_=B + 59 * row) == -1     # work / b^
    assert gp(o_=W + 29 * row) == -1 and gp(w_=O + 9 * row) == -1      # work / out
    assert gp(o_=B + 59 * row) == -1 and gp(b_=O + 9 * row) == -1      # b^ / out
    assert gp(o_=B + 11 * row, rows=1) == -1                           # ... of a broadcast: the last term's single row
    assert gp(o_=B + 12 * row, rows=1) == 0                            # ... and the words after it are not b^'s
    for name in ("a_", "w_", "b_", "o_"):                              # null and misaligned pointers
        assert gp(**{name: None}) == -1
        assert gp(**{name: {"a_": A, "w_": W, "b_": B, "o_": O}[name] + 8}) == -1
    assert gp(rows=2) == -1                                            # bhat_rows is 1 or batch
    assert gp(polys=0) == -1
    assert gp(outs=0) == -1
    assert gp(polys=(1 << 31) // 15 + 1) == -1                         # polys * levels * batch beyond the row limit
    assert gp(outs=(1 << 31) // 5 + 1) == -1                           # outs * batch beyond the row limit
    for dig in ((0, 3, 40), (32, 1, 0), (8, 0, 40), (8, 3, -1), (8, 3, 48), (16, 5, 0)):  # the decomposition's rules
        assert gp(dig=dig) == -1, dig
    assert gp(dig=(8, 3, 47)) == 0 and gp(dig=(31, 1, 0)) == 0 and gp(dig=(1, 3, 0)) == 0  # ... and their boundary values
    small = eng.NTTPlan(7, 3329, 4, 0)
    small.generate_twiddles(2, 3)
    assert gp(plan=small, dig=(13, 1, 0)) == -1 and gp(plan=small, dig=(12, 1, 0), rows=1, batch=1) == 0  # 2^(w - 1) < p
    assert L.ntt_polymul_gadget_pre(pl._h, None, 0, 0, 0, 0, None, None, 3, 0, None, 0, None) == 0  # batch == 0
    bare = eng.NTTPlan(7, GOLD, 8, 0)  # no tables
    assert gp(plan=bare) == -4
    # ntt_gadget_decompose: needs no table, the same digit rules, ranges apart
    dec = lambda a_=A, polys=2, batch=5, dig=(8, 3, 40), d_=W, plan=bare: L.ntt_gadget_decompose(plan._h, a_, polys, batch, *dig, d_, None)  # noqa: E731
    assert dec() == 0
    assert dec(d_=A + 9 * row) == -1 and dec(a_=W + 29 * row) == -1
    assert dec(a_=None) == -1 and dec(d_=None) == -1 and dec(a_=A + 8) == -1 and dec(d_=W + 8) == -1
    assert dec(polys=0) == -1 and dec(polys=(1 << 31) // 15 + 1) == -1
    assert dec(dig=(8, 3, 48)) == -1 and dec(dig=(0, 3, 0)) == -1
    assert dec(a_=None, d_=None, batch=0) == 0
    torch.cuda.synchronize()
    # the NTTPlan wrappers
    for bad in (bh[:, :5], bh[:, :, :2], bh.reshape(12, 5, n), bh[0]):
        with pytest.raises(ValueError):
            pl.polymul_gadget_pre(a, 8, 3, 40, bad)
    with pytest.raises(ValueError):
        pl.polymul_gadget_pre(a[0], 8, 3, 40, bh)
    with pytest.raises(ValueError):
        pl.polymul_gadget_pre(a, 8, 0, 40, bh)
    with pytest.raises(ValueError):
        pl.polymul_gadget_pre(a, 8, 3, 40, bh, work[:5])
    with pytest.raises(ValueError):
        pl.polymul_gadget_pre(a, 8, 3, 40, bh, work, out[:1])
    with pytest.raises(ValueError):
        pl.gadget_decompose(a[0], 8, 3, 40)
    with pytest.raises(ValueError):
        pl.gadget_decompose(a, 8, 3, 40, out=work)
    with pytest.raises(_lib.NTTError):
        pl.polymul_gadget_pre(a, 8, 3, 48, bh)  # the library's NTT_E_ARG, raised by the wrapper
