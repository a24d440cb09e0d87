"""ntt_polymul_dot_pre on a real MI355X, through NTTPlan.polymul_dot_pre, against the sum mod p over the terms of the oracle pipeline
Fwd(Inv(a_k) . Inv(b_k) . N) with the kind-2 table the plan generates on the device.  Bit-exact: all arithmetic is integer and every
word canonical.  The smallest shapes that reach each path (as tests/test_gpu_product_pre.py chose them): the fallback below the smallest
fused unit, the smallest unit (several polynomials per workgroup), the first 512-thread unit, one unit per workgroup, one column pass
each way, a pinned alternative without a fused middle, the three 4-byte instruction streams -- 1, 2 and 5 terms, per row and broadcast,
out of place and with out = a[0], batches 1, 5 and 33.  The multi-wave units (2^10, 2^12, 2^13) are the ones on which a missing barrier
between two terms would show: the host model steps threads one after the other and cannot see it."""
import os

import numpy as np
import pytest

import product_dot_ref as R

pytestmark = pytest.mark.gpu

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
TERMS = (1, 2, 5)
# (word bytes, p, g, logn, pinned alternative or None, batches)
SHAPES = [
    (8, GOLD, 7, 6, None, (1, 5, 33)),    # fallback: no product unit below 2^7
    (8, GOLD, 7, 7, None, (1, 5, 33)),    # the smallest fused unit, 16 polynomials per workgroup
    (8, GOLD, 7, 10, None, (1, 5, 33)),   # the first 512-thread unit
    (8, GOLD, 7, 12, None, (1, 5, 33)),   # one unit per workgroup, uniform top-round twiddles
    (8, GOLD, 7, 13, None, (1, 5, 33)),   # 7 + 6: one column pass each way
    (8, GOLD, 7, 13, 1, (1, 5, 33)),      # the 13-stage alternative pinned: fallback
    (8, GOLD, 7, 16, None, (5,)),
    (8, M64, 3, 7, None, (1, 5, 33)),
    (8, M64, 3, 13, None, (1, 5, 33)),
    (4, 998244353, 3, 5, None, (1, 5, 33)),   # fallback: the 2^5 unit is not taken
    (4, 998244353, 3, 6, None, (1, 5, 33)),
    (4, 998244353, 3, 13, None, (1, 5, 33)),  # the 512-thread unit
    (4, 998244353, 3, 14, None, (1, 5, 33)),
    (4, 2013265921, 31, 9, None, (1, 5, 33)),
    (4, 3221225473, 5, 12, None, (1, 5, 33)),
    (4, 3329, 3, 7, None, (1, 5, 33)),        # 3 generates Z_3329^*, and 2N = 256 divides 3328
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


def _prefix_sums(oracle, a, b, T, p, broadcast):
    """want[k - 1] = the reference of the first k terms: one pipeline run per term, shared by every term count and batch"""
    out, acc = [], None
    for k in range(a.shape[0]):
        c = R.want(oracle, a[k:k + 1], b[k:k + 1], T, p, broadcast)
        acc = c if acc is None else R.addmod(acc, c, p)
        out.append(acc)
    return out


@pytest.mark.parametrize("wb,p,g,logn,alt,batches", SHAPES)
def test_against_the_summed_oracle_pipeline(eng, oracle, wb, p, g, logn, alt, batches):
    pl, T = _plan(eng, oracle, wb, p, g, logn, alt)
    top, kmax = max(batches), max(TERMS)
    # one reference per shape: rows are independent, so a smaller batch is the first rows of the same arrays, fewer terms the first terms
    a, b, T2, bhat = R.operands(oracle, wb, p, g, logn, top, kmax, seed=1000 * wb + logn)
    assert np.array_equal(T, T2)
    want_rows, want_bcast = _prefix_sums(oracle, a, b, T, p, False), _prefix_sums(oracle, a, b, T, p, True)
    if logn <= 8:  # ... and the reference itself against the sum of schoolbook products mod (x^N + 1, p)
        for k in TERMS:
            for i in (0, top - 1):
                assert np.array_equal(want_rows[k - 1][i], R.schoolbook(oracle, a[:k], b[:k], p, i))
                assert np.array_equal(want_bcast[k - 1][i], R.schoolbook(oracle, a[:k], b[:k], p, i, True))
    for batch in batches:
        for terms in TERMS:
            ak = np.ascontiguousarray(a[:terms, :batch])
            for bh, want in ((bhat[:terms, :batch], want_rows[terms - 1][:batch]), (bhat[:terms, :1], want_bcast[terms - 1][:batch]),
                             (bhat[:terms, 0], want_bcast[terms - 1][:batch])):
                bh = np.ascontiguousarray(bh)
                d_bh = eng.to_device(bh, "cuda:0")
                out = eng.to_device(np.zeros_like(a[0, :batch]), "cuda:0")
                got = pl.polymul_dot_pre(eng.to_device(ak, "cuda:0"), d_bh, out)
                assert got is out
                assert np.array_equal(eng.to_host(out), want), (logn, batch, terms, bh.shape, "out of place")
                d_a = eng.to_device(ak, "cuda:0")
                got = pl.polymul_dot_pre(d_a, d_bh)  # the result is term 0's block of a
                assert got.data_ptr() == d_a.data_ptr() and tuple(got.shape) == (batch, 1 << logn)
                assert np.array_equal(eng.to_host(got), want), (logn, batch, terms, bh.shape, "in place")
                assert np.array_equal(eng.to_host(d_bh), bh), "b^ was written"


def test_seventeen_terms_of_maximal_words(eng, oracle):
    pl, T = _plan(eng, oracle, 8, GOLD, 7, 7)
    a, b, _, bhat = R.operands(oracle, 8, GOLD, 7, 7, 5, 17, all_max=True)
    got = pl.polymul_dot_pre(eng.to_device(a, "cuda:0"), eng.to_device(bhat, "cuda:0"))
    assert np.array_equal(eng.to_host(got), R.want(oracle, a, b, T, GOLD))


@pytest.mark.parametrize("wb,p,g,logn,alt", [(8, GOLD, 7, 7, None), (8, GOLD, 7, 13, None), (8, GOLD, 7, 13, 1), (8, M64, 3, 13, None), (4, 998244353, 3, 5, None),
                                             (4, 998244353, 3, 14, None), (4, 3221225473, 5, 12, None)])
def test_equals_the_prepared_product_and_its_sums_bit_for_bit(eng, oracle, wb, p, g, logn, alt):
    pl, T = _plan(eng, oracle, wb, p, g, logn, alt)
    a, b, _, bhat = R.operands(oracle, wb, p, g, logn, 5, 3, seed=7)
    d_bh = eng.to_device(bhat, "cuda:0")
    pre = [eng.to_host(pl.polymul_negacyclic_pre(eng.to_device(a[k], "cuda:0"), d_bh[k])) for k in range(3)]
    one = eng.to_host(pl.polymul_dot_pre(eng.to_device(a[:1], "cuda:0"), d_bh[:1]))
    assert np.array_equal(one, pre[0])
    total = R.addmod(R.addmod(pre[0], pre[1], p), pre[2], p)
    three = eng.to_host(pl.polymul_dot_pre(eng.to_device(a, "cuda:0"), d_bh))
    assert np.array_equal(three, total)
    # the same words whatever the decomposition: a clone with another policy
    if logn == 13 and wb == 8:
        other = pl.clone()
        other.set_policy(0 if alt else 1)
        assert np.array_equal(eng.to_host(other.polymul_dot_pre(eng.to_device(a, "cuda:0"), d_bh)), total)


@pytest.mark.parametrize("wb,p,g,logn,batch", [(8, GOLD, 7, 7, 5), (4, 998244353, 3, 6, 33)])
@pytest.mark.parametrize("broadcast", [False, True])
def test_nothing_outside_the_callers_words_is_touched(eng, oracle, wb, p, g, logn, batch, broadcast):
    """a, b^ and out each in the middle of an allocation of its own, one polynomial of sentinel words on both sides: a ragged last
    polynomial group (batch 5 of 16 per workgroup, 33 of 64) must neither write beyond a / out nor need anything beyond the last
    term of b^ -- of a broadcast, that term's single row"""
    import torch

    pl, T = _plan(eng, oracle, wb, p, g, logn)
    n, terms = 1 << logn, 3
    a, b, _, bhat = R.operands(oracle, wb, p, g, logn, batch, terms, seed=11)
    rows = 1 if broadcast else batch
    bhat = np.ascontiguousarray(bhat[:, :rows])
    want = R.want(oracle, a, b, T, p, broadcast)
    tdt = torch.int32 if wb == 4 else torch.int64
    sentinel = 0x5A5A5A5A if wb == 4 else 0x5A5A5A5A5A5A5A5A

    def framed(words):
        flat = words.reshape(-1, n)
        buf = torch.full((flat.shape[0] + 2, n), sentinel, dtype=tdt, device="cuda:0")
        buf[1:-1].copy_(eng.to_device(flat, "cuda:0"))
        return buf

    fa, fb, fo = framed(a), framed(bhat), framed(np.zeros_like(a[0]))
    pl.polymul_dot_pre(fa[1:-1].view(terms, batch, n), fb[1:-1].view(terms, rows, n), fo[1:-1])
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(fo[1:-1]), want)
    for buf in (fa, fb, fo):
        assert bool((buf[0] == sentinel).all()) and bool((buf[-1] == sentinel).all())
    assert np.array_equal(eng.to_host(fb[1:-1]), bhat.reshape(-1, n))


def test_c_abi_errors(eng, oracle):
    import torch

    from ntt_aie_amd import _lib

    L = _lib.lib()
    pl, _ = _plan(eng, oracle, 8, GOLD, 7, 7)
    n, row = 128, 128 * 8
    a = torch.zeros((3, 5, n), dtype=torch.int64, device="cuda:0")
    bh = torch.zeros((3, 5, n), dtype=torch.int64, device="cuda:0")
    out = torch.zeros((5, n), dtype=torch.int64, device="cuda:0")
    dot = lambda *args: L.ntt_polymul_dot_pre(pl._h, *args, None)  # noqa: E731
    A, B, O = a.data_ptr(), bh.data_ptr(), out.data_ptr()
    assert dot(A, B, 5, 3, O, 5) == 0
    assert dot(A, B, 1, 3, O, 5) == 0
    assert dot(A, B, 5, 3, A, 5) == 0                          # out is term 0's block of a
    assert dot(A, B, 5, 3, A + 5 * row, 5) == -1               # out is a[1]
    assert dot(A, B, 5, 3, A + 2 * row, 5) == -1               # out straddles a[0] and a[1]
    assert dot(A, B, 5, 3, B + 10 * row, 5) == -1              # out overlaps the last term of b^
    assert dot(A, B, 1, 3, B + 2 * row, 5) == -1               # ... of a broadcast: its single row
    assert dot(A, B, 1, 3, B + 3 * row, 5) == 0                # ... and the words after it are not b^'s
    assert dot(B, B, 1, 3, O, 5) == -1                         # a overlaps b^
    assert dot(A, B, 2, 3, O, 5) == -1                         # bhat_rows is 1 or batch
    assert dot(A, B, 5, 0, O, 5) == -1                         # no terms
    assert dot(A, B, 5, (1 << 31) // 5 + 1, O, 5) == -1        # terms * batch beyond the row limit
    assert dot(A, B + 8, 5, 3, O, 5) == -1                     # misaligned b^
    assert dot(A + 8, B, 5, 3, O, 5) == -1
    assert dot(A, B, 5, 3, O + 8, 5) == -1
    assert dot(A, None, 5, 3, O, 5) == -1
    assert dot(None, B, 5, 3, O, 5) == -1
    assert dot(A, B, 5, 3, None, 5) == -1
    assert dot(None, None, 3, 0, None, 0) == 0                 # batch == 0
    bare = eng.NTTPlan(7, GOLD, 8, 0)  # no tables
    assert L.ntt_polymul_dot_pre(bare._h, A, B, 5, 3, O, 5, None) == -4
    torch.cuda.synchronize()
    for bad in (bh[:2], bh[:, :2], bh.reshape(15, n), bh[0]):
        with pytest.raises(ValueError):
            pl.polymul_dot_pre(a, bad)
    with pytest.raises(ValueError):
        pl.polymul_dot_pre(a[0], bh)
    with pytest.raises(ValueError):
        pl.polymul_dot_pre(a, bh, out[:4])
