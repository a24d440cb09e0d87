"""Row-major matrix batches on the GPU (ntt_forward_columns / ntt_inverse_columns, NTTPlan.forward_columns / inverse_columns).

Every result is compared word for word with the ORACLE -- oracle.ntt / oracle.intt on the transposed columns, which is what
include/ntt_hip.h states -- and plan.forward on the transposed copy is only a second witness."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = 0xFFFFFFFF00000001
# the four word classes every coset / column GPU file started from; the reference's own modulus has kind-1 tables up to 2^8 only, larger sizes
# take the reference's kind-0 rule (the entry points are defined at network level, for any invertible table)
CLASSES = {"gl": (8, GOLD, 7), "m64": (8, 0xFFFFFFFC00000001, 10), "m32": (4, 998244353, 3), "kyber": (4, 3329, 3)}
# 4-byte words run one of three instruction streams, chosen per launch from the modulus (pass_kernel.inc): 0 "lazy" below 2^30 -- both
# 4-byte classes above --, 1 "small" in [2^30, 2^31), 2 "any" from 2^31 on.  These classes take the coset and column kernels through the
# other two; every helper of the coset / column GPU files resolves a class name in ALL_CLASSES, and this is the one definition
STREAM_CLASSES = {"bb31": (4, 2013265921, 31),   # 15*2^27 + 1, stream 1, two-adicity 27
                  "kb31": (4, 2130706433, 3),    # 2^31 - 2^24 + 1, stream 1 at its upper edge, two-adicity 24
                  "top32": (4, 4293918721, 19)}  # 2^32 - 2^20 + 1, stream 2 where almost every sum carries, two-adicity 20
ALL_CLASSES = {**CLASSES, **STREAM_CLASSES}
# (logn, width, pitch, count): one pass with several matrices per workgroup (width 17 gives w = 5: 16 matrices of 4-byte words, 8 of
# 8-byte words) and a count that leaves the last group partly empty; 5 + 4; 7 + 6; 8 + 8 (wave-uniform twiddles) at a line-aligned and
# at an odd pitch
SHAPES = [(4, 17, 18, 19), (9, 3, 3, 3), (13, 33, 48, 1), (16, 100, 128, 1), (16, 100, 101, 1)]


@functools.lru_cache(maxsize=None)
def _table_cached(logn, cls):
    import oracle_py

    wb, p, g = ALL_CLASSES[cls]
    n = 1 << logn
    T = oracle_py.make_table(1, n, p, g, wb) if (p - 1) % n == 0 else oracle_py.make_roots(n, p, g, wb)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def _case(cls, logn, width, count):
    """inputs [count][N][width] and the oracle's three transforms of their columns, computed once and shared (read-only)"""
    import oracle_py

    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    n = 1 << logn
    T = _table_cached(logn, cls)
    rng = np.random.default_rng(1000 * logn + width)
    x = (rng.integers(0, 2**63, size=(count, n, width), dtype=np.uint64) % np.uint64(p)).astype(dt)
    x[0, 0, 0], x[-1, -1, -1], x[0, n // 2, width // 2] = 0, p - 1, p - 1
    cols = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(count * width, n)
    back = lambda c: np.ascontiguousarray(c.reshape(count, width, n).transpose(0, 2, 1))
    inv = oracle_py.intt(cols, T, p, nthreads=8)
    res = {"x": x, "fwd": back(oracle_py.ntt(cols, T, p, nthreads=8)), "inv": back(inv),
           "invu": back(oracle_py.pointwise(inv, np.full_like(inv, n % p), p))}
    for v in res.values():
        v.setflags(write=False)
    return res


def _plan(logn, cls):
    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    pl = eng.NTTPlan(logn, p, wb, 0)
    pl.set_twiddles(np.array(_table_cached(logn, cls)))
    return pl


def test_columns_decomposition_is_reported(oracle):
    import ntt_aie_amd as eng

    for logn, want in ((3, []), (4, [(0, 4)]), (9, [(0, 5), (5, 4)]), (13, [(0, 7), (7, 6)]), (16, [(0, 8), (8, 8)]), (17, [(0, 6), (6, 6), (12, 5)])):
        pl = eng.NTTPlan(logn, GOLD, 8, 0)
        assert pl.column_passes == want
        pl.close()


@pytest.mark.parametrize("cls", sorted(ALL_CLASSES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "n%d_w%d_p%d_c%d" % s)
def test_columns_against_the_oracle_with_guard_words(oracle, cls, shape):
    """forward, scaled and unscaled inverse, out of place and in place.  Input and output each sit in the middle of one allocation:
    one matrix of sentinel on each side, sentinel in every padding column; the input's padding holds non-canonical junk.  All
    sentinels are intact afterwards, the input is read only, every live word is the oracle's."""
    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    wb, p, g = ALL_CLASSES[cls]
    logn, width, pitch, count = shape
    n = 1 << logn
    tdt = torch.int32 if wb == 4 else torch.int64
    ref = _case(cls, logn, width, count)
    pl = _plan(logn, cls)
    L = _lib.lib()
    junk, s_out = (-3, -5)  # all-ones patterns: >= p for every class
    mat_words = n * pitch
    big_in = torch.full(((count + 2) * mat_words,), junk, dtype=tdt, device="cuda:0")
    big_out = torch.full(((count + 2) * mat_words,), s_out, dtype=tdt, device="cuda:0")
    v_in = big_in[mat_words: (count + 1) * mat_words].view(count, n, pitch)
    v_out = big_out[mat_words: (count + 1) * mat_words].view(count, n, pitch)
    dx = eng.to_device(ref["x"], "cuda:0")

    def guards_intact(big, s):
        torch.cuda.synchronize()
        mid = big[mat_words: (count + 1) * mat_words].view(count, n, pitch)
        return bool((big[:mat_words] == s).all()) and bool((big[(count + 1) * mat_words:] == s).all()) and bool((mid[:, :, width:] == s).all())

    for name, call in (("fwd", lambda a, b: L.ntt_forward_columns(pl._h, a, b, width, pitch, count, None)),
                       ("inv", lambda a, b: L.ntt_inverse_columns(pl._h, a, b, width, pitch, count, 1, None)),
                       ("invu", lambda a, b: L.ntt_inverse_columns(pl._h, a, b, width, pitch, count, 0, None))):
        v_in[:, :, :width].copy_(dx)
        v_out[:, :, :width].fill_(-7)
        torch.cuda.synchronize()
        assert call(v_in.data_ptr(), v_out.data_ptr()) == 0
        assert guards_intact(big_in, junk) and guards_intact(big_out, s_out), (cls, shape, name)
        assert np.array_equal(eng.to_host(v_out[:, :, :width]), ref[name]), (cls, shape, name, "out of place")
        assert np.array_equal(eng.to_host(v_in[:, :, :width]), ref["x"]), (cls, shape, name, "input is read only")
        assert call(v_in.data_ptr(), v_in.data_ptr()) == 0
        assert guards_intact(big_in, junk), (cls, shape, name, "in place")
        assert np.array_equal(eng.to_host(v_in[:, :, :width]), ref[name]), (cls, shape, name, "in place")
    pl.close()


@pytest.mark.parametrize("cls", ["gl", "m32", "bb31"])
def test_wrapper_round_trip_on_a_strided_view(oracle, cls):
    """NTTPlan.forward_columns / inverse_columns on big[:, :, :width] of a larger tensor: accepted as it is, in place and with an
    allocated result; inverse(forward(x)) == x; plan.forward on the transposed copy agrees (second witness)"""
    import torch

    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    logn, width, count = 13, 33, 1
    n = 1 << logn
    ref = _case(cls, logn, width, count)
    pl = _plan(logn, cls)
    tdt = torch.int32 if wb == 4 else torch.int64
    big = torch.full((count, n, 48), -3, dtype=tdt, device="cuda:0")
    view = big[:, :, :width]
    view.copy_(eng.to_device(ref["x"], "cuda:0"))
    out = pl.forward_columns(view)  # a fresh contiguous result; the view is untouched
    assert out.is_contiguous() and np.array_equal(eng.to_host(out), ref["fwd"])
    assert np.array_equal(eng.to_host(view), ref["x"]) and bool((big[:, :, width:] == -3).all())
    assert pl.forward_columns(view, out=view) is view
    assert np.array_equal(eng.to_host(view), ref["fwd"]) and bool((big[:, :, width:] == -3).all())
    witness = pl.forward(eng.to_device(ref["x"], "cuda:0").transpose(1, 2).contiguous().view(count * width, n))
    assert np.array_equal(eng.to_host(witness).reshape(count, width, n).transpose(0, 2, 1), ref["fwd"])
    assert pl.inverse_columns(view, out=view) is view
    assert np.array_equal(eng.to_host(view), ref["x"])
    two_d = big[0, :, :width]  # [N][width]
    assert np.array_equal(eng.to_host(pl.inverse_columns(two_d, scale=False)), ref["invu"][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = pl.inverse_columns(view, stream=side)
    side.synchronize()
    assert np.array_equal(eng.to_host(got), ref["inv"])
    pl.close()


def test_wrapper_value_errors(oracle):
    import torch

    import ntt_aie_amd as eng

    pl = _plan(9, "gl")
    n = 512
    ok = torch.zeros((2, n, 8), dtype=torch.int64, device="cuda:0")
    bad = [
        torch.zeros((n, 8), dtype=torch.int64),                                   # not on the device
        torch.zeros((n, 8), dtype=torch.int32, device="cuda:0"),                  # word size
        torch.zeros((n // 2, 8), dtype=torch.int64, device="cuda:0"),             # rows != N
        torch.zeros((n * 8,), dtype=torch.int64, device="cuda:0"),                # one dimension
        torch.zeros((8, n), dtype=torch.int64, device="cuda:0").t(),              # last stride != 1
        torch.zeros((n, 8), dtype=torch.int64, device="cuda:0").expand(2, n, 8),  # matrix stride != N * pitch
        torch.zeros((3, n, 8), dtype=torch.int64, device="cuda:0")[::2],          # matrix stride != N * pitch
    ]
    for t in bad:
        with pytest.raises(ValueError):
            pl.forward_columns(t)
        with pytest.raises(ValueError):
            pl.inverse_columns(t)
    with pytest.raises(ValueError):
        pl.forward_columns(ok, out=torch.zeros((2, n, 4), dtype=torch.int64, device="cuda:0"))  # shape
    with pytest.raises(ValueError):
        pl.forward_columns(ok, out=torch.zeros((2, n, 16), dtype=torch.int64, device="cuda:0")[:, :, :8])  # another pitch
    assert pl.forward_columns(torch.zeros((n, 0), dtype=torch.int64, device="cuda:0")).shape == (n, 0)
    assert pl.forward_columns(ok).shape == ok.shape
    pl.close()


def test_columns_error_contract(oracle):
    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    L = _lib.lib()
    E = _lib
    n = 256
    x = torch.zeros((2 * n * 8,), dtype=torch.int64, device="cuda:0")
    y = torch.zeros((2 * n * 8,), dtype=torch.int64, device="cuda:0")
    a, b = x.data_ptr(), y.data_ptr()
    fwd = lambda pl, i, o, w, pi, c: L.ntt_forward_columns(pl, i, o, w, pi, c, None)
    inv = lambda pl, i, o, w, pi, c: L.ntt_inverse_columns(pl, i, o, w, pi, c, 1, None)
    small = eng.NTTPlan(3, GOLD, 8, 0)
    small.generate_twiddles(1, 7)
    assert small.column_passes == []
    pl = eng.NTTPlan(8, GOLD, 8, 0)
    for call in (fwd, inv):
        assert call(None, a, b, 8, 8, 1) == E.NTT_E_ARG
        assert call(small._h, a, b, 8, 8, 1) == E.NTT_E_LOGN
        assert call(pl._h, a, b, 8, 8, 1) == E.NTT_E_NOTABLE
    T = np.array(_table_cached(8, "gl"))
    broken = T.copy()
    broken[200] = 0
    pl.set_twiddles(broken)
    assert inv(pl._h, a, b, 8, 8, 1) == E.NTT_E_NOTINVERTIBLE and fwd(pl._h, a, b, 8, 8, 1) == 0
    pl.set_twiddles(T)
    for call in (fwd, inv):
        assert call(pl._h, a, b, 0, 8, 1) == 0 and call(pl._h, a, b, 8, 8, 0) == 0 and call(pl._h, None, None, 0, 0, 0) == 0
        assert call(pl._h, None, b, 8, 8, 1) == E.NTT_E_ARG and call(pl._h, a, None, 8, 8, 1) == E.NTT_E_ARG
        assert call(pl._h, a + 8, b, 8, 8, 1) == E.NTT_E_ARG and call(pl._h, a, b + 8, 8, 8, 1) == E.NTT_E_ARG  # misaligned
        assert call(pl._h, a, b, 9, 8, 1) == E.NTT_E_ARG                                                        # width > pitch
        assert call(pl._h, a, a + 16, 8, 8, 2) == E.NTT_E_ARG                                                   # partial overlap
        assert call(pl._h, a, a + 8 * ((2 * n - 1) * 8 + 6), 7, 8, 2) == E.NTT_E_ARG                            # ... by the last live word alone
        assert call(pl._h, a, b, 8, (1 << 20) + 1, 1) == E.NTT_E_ARG                                            # N * pitch > 2^28 words
        assert call(pl._h, a, b, (1 << 20) + 1, 1 << 21, 1) == E.NTT_E_ARG                                      # logn + w > 28
        assert call(pl._h, a, b, 8, 8, 2**31) == E.NTT_E_ARG
        assert call(pl._h, a, b, 8, 8, 2) == 0 and call(pl._h, a, a, 8, 8, 2) == 0
    torch.cuda.synchronize()
    small.close()
    pl.close()
