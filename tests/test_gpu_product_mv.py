"""ntt_polymul_matvec_pre on a real MI355X, through NTTPlan.polymul_matvec_pre, bit-exact per output against the reference of
ntt_polymul_dot_pre: the sum mod p over the terms of the oracle pipeline Fwd(Inv(a_k) . Inv(b_jk) . N) with the kind-2 table the plan
generates on the device.  The smallest shapes that reach each path (as tests/test_gpu_product_dot.py chose them): the fallback below the
smallest fused unit, the smallest unit (several polynomials per workgroup), the first 512-thread unit, one unit per workgroup, one column
pass each way, a pinned alternative without a fused middle, a unit without a summed kernel (general 64-bit 2^10, 4-byte 2^13: fallback),
the three 4-byte instruction streams -- 1, 2 and 3 outputs (a summed launch alone, a pair, a pair and a summed launch), 1 and 3 terms, per
row and broadcast, batches 1, 5 and 33.
A missing barrier between the two forward units of a pair shows only where the TWO-OUTPUT kernel runs on several waves side by side: the
host model steps threads one after the other and cannot see it.  The product library pairs outputs for the general 64-bit modulus and
4-byte words, not for Goldilocks (launch.h: product_mv_unit), so the Goldilocks shapes here run summed launches and guard values and
sequencing only.  A unit is spread over several waves from 2^10 words of 8 bytes and 2^11 of 4 bytes on (pass.h: WAVE_LOCAL), so the
multi-wave pair kernels the library ships are general 64-bit 2^11 and 2^12 (512 threads, one workgroup per CU under the family's register
bound; 2^10 has no summed kernel) and 4-byte 2^11 and 2^12 (2^13 has none).  They are run as single-pass sizes with 2 and 3 outputs and
batches 1, 5 and 33: the general 64-bit modulus, and 4-byte words with a lazy prime (998244353), a 31-bit one (2013265921) and, at 2^12,
one above 2^31 (3221225473).  General 64-bit 2^8 and 2^9 and 4-byte 2^10 add the remaining wave-local pair kernels."""
import os

import numpy as np
import pytest

import product_dot_ref as R

pytestmark = pytest.mark.gpu

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
OUTS, TERMS = (1, 2, 3), (1, 3)
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
    (8, M64, 3, 8, None, (1, 5, 33)),     # the two-output kernel on the other wave-local units ...
    (8, M64, 3, 9, None, (1, 5, 33)),
    (8, M64, 3, 10, None, (1, 5, 33)),    # no summed kernel for this unit: fallback
    (8, M64, 3, 11, None, (1, 5, 33)),    # ... and on the multi-wave 512-thread units: one workgroup per CU, eight waves at the barrier between the two forwards
    (8, M64, 3, 12, None, (1, 5, 33)),
    (8, M64, 3, 13, None, (1, 5, 33)),
    (4, 998244353, 3, 5, None, (1, 5, 33)),   # fallback: the 2^5 unit is not taken
    (4, 998244353, 3, 6, None, (1, 5, 33)),
    (4, 998244353, 3, 13, None, (1, 5, 33)),  # no summed kernel for this unit: fallback
    (4, 998244353, 3, 14, None, (1, 5, 33)),
    (4, 2013265921, 31, 9, None, (1, 5, 33)),
    (4, 998244353, 3, 10, None, (1, 5, 33)),  # wave-local; then the multi-wave 4-byte units 2^11 and 2^12 in the lazy stream ...
    (4, 998244353, 3, 11, None, (1, 5, 33)),
    (4, 998244353, 3, 12, None, (1, 5, 33)),
    (4, 2013265921, 31, 11, None, (1, 5, 33)),  # ... with a 31-bit prime ...
    (4, 2013265921, 31, 12, None, (1, 5, 33)),
    (4, 3221225473, 5, 12, None, (1, 5, 33)),   # ... and above 2^31
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


def _operands(oracle, wb, p, g, logn, batch, outs, terms, seed):
    """a [terms, batch, N], b and b^ [outs, terms, batch, N]: product_dot_ref's operands (row 0 of every block all p - 1), outs * terms of them"""
    a, b, T, bhat = R.operands(oracle, wb, p, g, logn, batch, outs * terms, seed=seed)
    n = 1 << logn
    return np.ascontiguousarray(a[:terms]), b.reshape(outs, terms, batch, n), bhat.reshape(outs, terms, batch, n), T


def _prefix_sums(oracle, a, b, T, p, broadcast):
    """want[j][k - 1] = the reference of output j over the first k terms: one pipeline run per output and term, shared by every output
    count, term count and batch"""
    res = []
    for j in range(b.shape[0]):
        out, acc = [], None
        for k in range(a.shape[0]):
            c = R.want(oracle, a[k:k + 1], b[j, k:k + 1], T, p, broadcast)
            acc = c if acc is None else R.addmod(acc, c, p)
            out.append(acc)
        res.append(out)
    return res


@pytest.mark.parametrize("wb,p,g,logn,pairs", [(8, M64, 3, 11, 1), (8, M64, 3, 12, 1), (4, 998244353, 3, 11, 1), (4, 998244353, 3, 12, 1), (4, 2013265921, 31, 11, 1),
                                               (4, 2013265921, 31, 12, 1), (4, 3221225473, 5, 12, 1), (8, M64, 3, 10, 0), (4, 998244353, 3, 13, 0),
                                               (8, GOLD, 7, 10, 0), (8, GOLD, 7, 12, 0), (8, GOLD, 7, 6, 0)])
def test_which_shapes_run_the_two_output_kernel(eng, oracle, wb, p, g, logn, pairs):
    """ntt_plan_info 14: the multi-wave shapes of SHAPES really run the two-output kernel, Goldilocks and the units without a summed kernel
    do not -- so a change of launch.h's product_mv_unit cannot silently take the pair kernels out of this file"""
    from ntt_aie_amd import _lib

    pl, _ = _plan(eng, oracle, wb, p, g, logn)
    assert _lib.lib().ntt_plan_info(pl._h, 14) == pairs


@pytest.mark.parametrize("wb,p,g,logn,alt,batches", SHAPES)
def test_every_output_against_the_summed_oracle_pipeline(eng, oracle, wb, p, g, logn, alt, batches):
    pl, T = _plan(eng, oracle, wb, p, g, logn, alt)
    top, jmax, kmax = max(batches), max(OUTS), max(TERMS)
    # one reference per shape: rows are independent, so a smaller batch is the first rows of the same arrays, fewer terms the first terms
    a, b, bhat, T2 = _operands(oracle, wb, p, g, logn, top, jmax, kmax, seed=1000 * wb + logn)
    assert np.array_equal(T, T2)
    want = {False: _prefix_sums(oracle, a, b, T, p, False), True: _prefix_sums(oracle, a, b, T, p, True)}
    if logn <= 7:  # ... and the reference itself against the sum of schoolbook products mod (x^N + 1, p)
        for i in (0, top - 1):
            assert np.array_equal(want[False][jmax - 1][kmax - 1][i], R.schoolbook(oracle, a, b[jmax - 1], p, i))
            assert np.array_equal(want[True][jmax - 1][kmax - 1][i], R.schoolbook(oracle, a, b[jmax - 1], p, i, True))
    for batch in batches:
        for terms in TERMS:
            for outs in OUTS:
                for bcast, bh in ((False, bhat[:outs, :terms, :batch]), (True, bhat[:outs, :terms, :1]), (True, bhat[:outs, :terms, 0])):
                    bh = np.ascontiguousarray(bh)
                    d_bh = eng.to_device(bh, "cuda:0")
                    out = eng.to_device(np.zeros_like(bhat[:outs, 0, :batch]), "cuda:0")
                    got = pl.polymul_matvec_pre(eng.to_device(np.ascontiguousarray(a[:terms, :batch]), "cuda:0"), d_bh, out)
                    assert got is out
                    host = eng.to_host(out)
                    for j in range(outs):
                        assert np.array_equal(host[j], want[bcast][j][terms - 1][:batch]), (logn, batch, terms, outs, j, bh.shape)
                    assert np.array_equal(eng.to_host(d_bh), bh), "b^ was written"


@pytest.mark.parametrize("wb,p,g,logn,alt", [(8, GOLD, 7, 7, None), (8, GOLD, 7, 12, None), (8, GOLD, 7, 13, None), (8, GOLD, 7, 13, 1), (8, M64, 3, 13, None),
                                             (4, 998244353, 3, 5, None), (4, 998244353, 3, 14, None), (4, 3221225473, 5, 12, None)])
@pytest.mark.parametrize("broadcast", [False, True])
def test_each_output_is_the_inner_product_of_a_fresh_copy_bit_for_bit(eng, oracle, wb, p, g, logn, alt, broadcast):
    pl, T = _plan(eng, oracle, wb, p, g, logn, alt)
    a, b, bhat, _ = _operands(oracle, wb, p, g, logn, 5, 3, 3, seed=7)
    bhat = np.ascontiguousarray(bhat[:, :, :1] if broadcast else bhat)
    d_bh = eng.to_device(bhat, "cuda:0")
    dots = [eng.to_host(pl.polymul_dot_pre(eng.to_device(a, "cuda:0"), d_bh[j])) for j in range(3)]
    got = eng.to_host(pl.polymul_matvec_pre(eng.to_device(a, "cuda:0"), d_bh))  # out allocated by the call
    assert got.shape == (3, 5, 1 << logn)
    for j in range(3):
        assert np.array_equal(got[j], dots[j]), j
    # the same words whatever the decomposition: a clone with another policy
    if logn == 13 and wb == 8:
        other = pl.clone()
        other.set_policy(0 if alt else 1)
        again = eng.to_host(other.polymul_matvec_pre(eng.to_device(a, "cuda:0"), d_bh))
        assert np.array_equal(again, got)


@pytest.mark.parametrize("wb,p,g,logn,batch", [(8, GOLD, 7, 7, 5), (4, 998244353, 3, 6, 33)])
@pytest.mark.parametrize("broadcast", [False, True])
def test_nothing_outside_the_callers_words_is_touched(eng, oracle, wb, p, g, logn, batch, broadcast):
    """a, b^ and out each in the middle of an allocation of its own, one polynomial of sentinel words on both sides, three outputs: a
    ragged last polynomial group (batch 5 of 16 per workgroup, 33 of 64) must neither write beyond a / out nor need anything beyond the
    last output's last term of b^ -- of a broadcast, that term's single row"""
    import torch

    pl, T = _plan(eng, oracle, wb, p, g, logn)
    n, terms, outs = 1 << logn, 3, 3
    a, b, bhat, _ = _operands(oracle, wb, p, g, logn, batch, outs, terms, seed=11)
    rows = 1 if broadcast else batch
    bhat = np.ascontiguousarray(bhat[:, :, :rows])
    want = np.stack([R.want(oracle, a, b[j], T, p, broadcast) for j in range(outs)])
    tdt = torch.int32 if wb == 4 else torch.int64
    sentinel = 0x5A5A5A5A if wb == 4 else 0x5A5A5A5A5A5A5A5A

    def framed(words):
        flat = words.reshape(-1, n)
        buf = torch.full((flat.shape[0] + 2, n), sentinel, dtype=tdt, device="cuda:0")
        buf[1:-1].copy_(eng.to_device(flat, "cuda:0"))
        return buf

    fa, fb, fo = framed(a), framed(bhat), framed(np.zeros_like(want))
    pl.polymul_matvec_pre(fa[1:-1].view(terms, batch, n), fb[1:-1].view(outs, terms, rows, n), fo[1:-1].view(outs, batch, n))
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(fo[1:-1]).reshape(outs, batch, n), want)
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
    bh = torch.zeros((2, 3, 5, n), dtype=torch.int64, device="cuda:0")
    out = torch.zeros((2, 5, n), dtype=torch.int64, device="cuda:0")
    mv = lambda *args: L.ntt_polymul_matvec_pre(pl._h, *args, None)  # noqa: E731
    A, B, O = a.data_ptr(), bh.data_ptr(), out.data_ptr()
    assert mv(A, B, 5, 3, 2, O, 5) == 0
    assert mv(A, B, 1, 3, 2, O, 5) == 0
    assert mv(A, B, 5, 3, 2, A, 5) == -1                          # out is a: refused, unlike ntt_polymul_dot_pre
    assert mv(A, B, 5, 3, 1, A, 5) == -1                          # ... even for one output
    assert mv(A, B, 5, 3, 2, A + 14 * row, 5) == -1               # out begins in the last row of a
    assert mv(O + 9 * row, B, 5, 1, 2, O, 5) == -1                # a begins in the last row of out
    assert mv(A, B, 5, 3, 2, B + 29 * row, 5) == -1               # out overlaps the last output's last term of b^
    assert mv(A, B, 1, 3, 2, B + 5 * row, 5) == -1                # ... of a broadcast: its single row
    assert mv(A, B, 1, 3, 2, B + 6 * row, 5) == 0                 # ... and the words after it are not b^'s
    assert mv(B, B, 1, 3, 2, O, 5) == -1                          # a overlaps b^
    assert mv(A, B, 2, 3, 2, O, 5) == -1                          # bhat_rows is 1 or batch
    assert mv(A, B, 5, 0, 2, O, 5) == -1                          # no terms
    assert mv(A, B, 5, 3, 0, O, 5) == -1                          # no outputs
    assert mv(A, B, 5, (1 << 31) // 5 + 1, 2, O, 5) == -1         # terms * batch beyond the row limit
    assert mv(A, B, 5, 3, (1 << 31) // 5 + 1, O, 5) == -1         # outs * batch beyond the row limit
    assert mv(A, B + 8, 5, 3, 2, O, 5) == -1                      # misaligned b^
    assert mv(A + 8, B, 5, 3, 2, O, 5) == -1
    assert mv(A, B, 5, 3, 2, O + 8, 5) == -1
    assert mv(A, None, 5, 3, 2, O, 5) == -1
    assert mv(None, B, 5, 3, 2, O, 5) == -1
    assert mv(A, B, 5, 3, 2, None, 5) == -1
    assert mv(None, None, 3, 0, 0, None, 0) == 0                  # batch == 0
    bare = eng.NTTPlan(7, GOLD, 8, 0)  # no tables
    assert L.ntt_polymul_matvec_pre(bare._h, A, B, 5, 3, 2, O, 5, None) == -4
    torch.cuda.synchronize()
    for bad in (bh[:, :2], bh[:, :, :2], bh.reshape(6, 5, n), bh[0]):
        with pytest.raises(ValueError):
            pl.polymul_matvec_pre(a, bad)
    with pytest.raises(ValueError):
        pl.polymul_matvec_pre(a[0], bh)
    with pytest.raises(ValueError):
        pl.polymul_matvec_pre(a, bh, out[:1])
    with pytest.raises(ValueError):
        pl.polymul_matvec_pre(a, bh, out[0])
