"""ntt_polymul_prepare / ntt_polymul_negacyclic_pre on a real MI355X, through NTTPlan.polymul_prepare / polymul_negacyclic_pre, against
the oracle pipeline Fwd(Inv(a) . Inv(b) . N) with the kind-2 table the plan generates on the device.  Bit-exact: all arithmetic is
integer.  The smallest shapes that reach each path: the fallback below the smallest fused unit, the smallest unit (several polynomials
per workgroup), the first 512-thread unit, one unit per workgroup, one column pass each way, a pinned alternative without a fused middle,
the three 4-byte instruction streams -- per row and broadcast, out of place and with out aliasing a, batches 1, 5 and 33."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
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


def _operands(wb, p, logn, batch):
    dt = np.uint32 if wb == 4 else np.uint64
    rng = np.random.default_rng(1000 * wb + logn)
    a = (rng.integers(0, 2**63, size=(batch, 1 << logn), dtype=np.uint64) % np.uint64(p)).astype(dt)
    b = (rng.integers(0, 2**63, size=(batch, 1 << logn), dtype=np.uint64) % np.uint64(p)).astype(dt)
    a[0, :3] = [p - 1, 0, 1]
    b[0, :3] = [p - 1, p - 1, 0]
    return a, b


def _pipeline(oracle, a, b, T, p):
    n = a.shape[1]
    return oracle.ntt(oracle.pointwise(oracle.intt(a, T, p, nthreads=4), oracle.intt(b, T, p, nthreads=4), p, n % p), T, p, nthreads=4)


def _bhat(oracle, b, T, p):
    B = oracle.intt(b, T, p, nthreads=4)
    return oracle.pointwise(B, np.ones_like(B), p, b.shape[1] % p)  # the UNSCALED inverse


@pytest.mark.parametrize("wb,p,g,logn,alt,batches", SHAPES)
def test_against_the_oracle_pipeline(eng, oracle, wb, p, g, logn, alt, batches):
    pl, T = _plan(eng, oracle, wb, p, g, logn, alt)
    top = max(batches)
    a, b = _operands(wb, p, logn, top)
    # one reference per shape: rows are independent, so a smaller batch is the first rows of the same arrays
    want_rows = _pipeline(oracle, a, b, T, p)
    want_bcast = _pipeline(oracle, a, np.repeat(b[:1], top, axis=0), T, p)
    bhat = _bhat(oracle, b, T, p)
    if logn <= 8:  # ... and the reference itself against the schoolbook product mod (x^N + 1, p)
        for i in (0, top - 1):
            assert np.array_equal(want_rows[i], oracle.negacyclic_schoolbook(a[i], b[i], p).astype(a.dtype))
            assert np.array_equal(want_bcast[i], oracle.negacyclic_schoolbook(a[i], b[0], p).astype(a.dtype))
    for batch in batches:
        for bh, want in ((bhat[:batch], want_rows[:batch]), (bhat[:1], want_bcast[:batch]), (bhat[0], want_bcast[:batch])):
            d_bh = eng.to_device(bh, "cuda:0")
            out = eng.to_device(np.zeros_like(a[:batch]), "cuda:0")
            got = pl.polymul_negacyclic_pre(eng.to_device(a[:batch], "cuda:0"), d_bh, out)
            assert got is out
            assert np.array_equal(eng.to_host(out), want), (logn, batch, bh.shape, "out of place")
            d_a = eng.to_device(a[:batch], "cuda:0")
            got = pl.polymul_negacyclic_pre(d_a, d_bh)  # the result aliases a
            assert got is d_a
            assert np.array_equal(eng.to_host(d_a), want), (logn, batch, bh.shape, "in place")
            assert np.array_equal(eng.to_host(d_bh), bh), "b^ was written"


@pytest.mark.parametrize("wb,p,g,logn,alt", [(8, GOLD, 7, 7, None), (8, GOLD, 7, 13, None), (8, GOLD, 7, 13, 1), (8, M64, 3, 13, None), (4, 998244353, 3, 5, None),
                                             (4, 998244353, 3, 14, None), (4, 3221225473, 5, 12, None)])
def test_prepare_is_the_unscaled_inverse_and_pre_is_the_product_bit_for_bit(eng, oracle, wb, p, g, logn, alt):
    pl, T = _plan(eng, oracle, wb, p, g, logn, alt)
    a, b = _operands(wb, p, logn, 5)
    d_b = eng.to_device(b, "cuda:0")
    prep = pl.polymul_prepare(d_b)
    assert np.array_equal(eng.to_host(d_b), b)
    assert np.array_equal(eng.to_host(prep), eng.to_host(pl.inverse(eng.to_device(b, "cuda:0"), scale=False)))
    assert np.array_equal(eng.to_host(prep), _bhat(oracle, b, T, p))
    in_place = eng.to_device(b, "cuda:0")
    assert pl.polymul_prepare(in_place, in_place) is in_place and np.array_equal(eng.to_host(in_place), eng.to_host(prep))
    ref = eng.to_host(pl.polymul_negacyclic(eng.to_device(a, "cuda:0"), eng.to_device(b, "cuda:0")))
    got = eng.to_host(pl.polymul_negacyclic_pre(eng.to_device(a, "cuda:0"), prep))
    assert np.array_equal(got, ref)
    # the prepared form does not depend on the decomposition: a clone with another policy takes it as it is
    if logn == 13 and wb == 8:
        other = pl.clone()
        other.set_policy(0 if alt else 1)
        assert np.array_equal(eng.to_host(other.polymul_negacyclic_pre(eng.to_device(a, "cuda:0"), prep)), ref)


@pytest.mark.parametrize("wb,p,g,logn,batch", [(8, GOLD, 7, 7, 5), (4, 998244353, 3, 6, 33)])
@pytest.mark.parametrize("broadcast", [False, True])
def test_nothing_outside_the_callers_words_is_touched(eng, oracle, wb, p, g, logn, batch, broadcast):
    """a, b^ and out each in the middle of an allocation of its own, one polynomial of sentinel words on both sides: a ragged last
    polynomial group (batch 5 of 16 per workgroup, 33 of 64) must neither write beyond a / out nor need anything beyond b^"""
    import torch

    pl, T = _plan(eng, oracle, wb, p, g, logn)
    n = 1 << logn
    a, b = _operands(wb, p, logn, batch)
    rows = 1 if broadcast else batch
    bhat = _bhat(oracle, b, T, p)[:rows]
    want = _pipeline(oracle, a, np.repeat(b[:1], batch, axis=0) if broadcast else b, T, p)
    tdt = torch.int32 if wb == 4 else torch.int64
    sentinel = 0x5A5A5A5A if wb == 4 else 0x5A5A5A5A5A5A5A5A

    def framed(words):
        buf = torch.full((words.shape[0] + 2, n), sentinel, dtype=tdt, device="cuda:0")
        buf[1:-1].copy_(eng.to_device(words, "cuda:0"))
        return buf

    fa, fb, fo = framed(a), framed(bhat), framed(np.zeros_like(a))
    pl.polymul_negacyclic_pre(fa[1:-1], fb[1:-1], fo[1:-1])
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(fo[1:-1]), want)
    for buf in (fa, fb, fo):
        assert bool((buf[0] == sentinel).all()) and bool((buf[-1] == sentinel).all())
    assert np.array_equal(eng.to_host(fb[1:-1]), bhat)


def test_c_abi_errors(eng, oracle):
    import torch

    from ntt_aie_amd import _lib

    L = _lib.lib()
    pl, _ = _plan(eng, oracle, 8, GOLD, 7, 7)
    n = 128
    a = torch.zeros((5, n), dtype=torch.int64, device="cuda:0")
    bh = torch.zeros((6, n), dtype=torch.int64, device="cuda:0")
    out = torch.zeros((5, n), dtype=torch.int64, device="cuda:0")
    pre = lambda *args: L.ntt_polymul_negacyclic_pre(pl._h, *args, None)  # noqa: E731
    assert pre(a.data_ptr(), bh.data_ptr(), 5, out.data_ptr(), 5) == 0
    assert pre(a.data_ptr(), bh.data_ptr(), 1, out.data_ptr(), 5) == 0
    assert pre(a.data_ptr(), bh.data_ptr(), 2, out.data_ptr(), 5) == -1                   # bhat_rows is 1 or batch
    assert pre(a.data_ptr(), bh.data_ptr(), 5, bh.data_ptr() + 4 * n * 8, 5) == -1        # out overlaps the last row of b^
    assert pre(bh.data_ptr(), bh.data_ptr(), 1, out.data_ptr(), 5) == -1                  # a overlaps b^
    assert pre(a.data_ptr(), bh.data_ptr() + 8, 5, out.data_ptr(), 5) == -1               # misaligned b^
    assert pre(a.data_ptr(), None, 5, out.data_ptr(), 5) == -1
    assert pre(None, None, 3, None, 0) == 0                                               # batch == 0
    assert L.ntt_polymul_prepare(pl._h, None, None, 0, None) == 0
    assert L.ntt_polymul_prepare(pl._h, bh.data_ptr() + 8, out.data_ptr(), 5, None) == -1
    bare = eng.NTTPlan(7, GOLD, 8, 0)  # no tables
    assert L.ntt_polymul_negacyclic_pre(bare._h, a.data_ptr(), bh.data_ptr(), 5, out.data_ptr(), 5, None) == -4
    assert L.ntt_polymul_prepare(bare._h, a.data_ptr(), out.data_ptr(), 5, None) == -4
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        pl.polymul_negacyclic_pre(a, bh)  # six rows for a batch of five
