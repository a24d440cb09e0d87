"""Coset LDE and coset interpolation on matrix columns on the GPU (ntt_lde_columns / ntt_coset_inverse_columns,
NTTPlan.lde_columns / coset_inverse_columns).

Every result is compared word for word with the ORACLE's network on the expanded (or scaled), transposed columns -- what
include/ntt_hip.h states -- never with the library's other paths alone."""
import functools

import numpy as np
import pytest

from test_gpu_columns import ALL_CLASSES, CLASSES, GOLD, STREAM_CLASSES  # noqa: F401

pytestmark = pytest.mark.gpu

# the seven word classes of tests/test_gpu_columns.py (four, and three more 4-byte moduli for the other two instruction streams);
# kind-0 tables where kind-1 does not exist
# (logm, beta, width, in_pitch, out_pitch, count): one pass, several matrices per workgroup, ragged group, two live rows per thread;
# beta = 4: one live word per thread; 5 + 4; 7 + 6; 8 + 8 with wave-uniform twiddles and an odd source pitch
LDE_SHAPES = [(4, 3, 17, 18, 19, 19), (5, 4, 3, 3, 5, 3), (9, 1, 33, 40, 48, 2), (13, 3, 33, 48, 33, 1), (16, 2, 100, 101, 128, 1)]
CINV_SHAPES = [(4, 17, 18, 19), (9, 3, 3, 3), (13, 33, 48, 1), (16, 100, 101, 1)]


def _bitrev_array(n_bits):
    i = np.arange(1 << n_bits, dtype=np.uint64)
    r = np.zeros_like(i)
    for b in range(n_bits):
        r |= ((i >> np.uint64(b)) & np.uint64(1)) << np.uint64(n_bits - 1 - b)
    return r


def _powers(base, exps, p, dt):
    return np.array([pow(base, int(e), p) for e in exps], dtype=dt)


def _shift(cls, k):
    wb, p, g = ALL_CLASSES[cls]
    return (1, g, p - 1)[k % 3]


@functools.lru_cache(maxsize=None)
def _table_cached(logn, cls):
    import oracle_py

    wb, p, g = ALL_CLASSES[cls]
    n = 1 << logn
    T = oracle_py.make_table(1, n, p, g, wb) if (p - 1) % n == 0 else oracle_py.make_roots(n, p, g, wb)
    T.setflags(write=False)
    return T


@functools.lru_cache(maxsize=None)
def _lde_case(cls, logm, beta, width, count, shift):
    """inputs [count][N][width] (holding 0 and p - 1) and the oracle's network on the expanded, scaled columns; computed once, read-only"""
    import oracle_py

    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    m, n = 1 << logm, (1 << logm) >> beta
    rng = np.random.default_rng(1000 * logm + 10 * beta + width)
    x = (rng.integers(0, 2**63, size=(count, n, width), dtype=np.uint64) % np.uint64(p)).astype(dt)
    x[0, 0, 0], x[-1, -1, -1], x[0, n // 2, width // 2] = 0, p - 1, p - 1
    s = _powers(shift, _bitrev_array(logm - beta), p, dt)
    small = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(count * width, n)
    cols = np.zeros((count * width, m), dtype=dt)
    cols[:, :: 1 << beta] = oracle_py.pointwise(small, np.broadcast_to(s, small.shape).copy(), p)
    want = np.ascontiguousarray(oracle_py.ntt(cols, _table_cached(logm, cls), p, nthreads=8).reshape(count, width, m).transpose(0, 2, 1))
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@functools.lru_cache(maxsize=None)
def _cinv_case(cls, logn, width, count, shift):
    import oracle_py

    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    n = 1 << logn
    rng = np.random.default_rng(2000 * logn + width)
    x = (rng.integers(0, 2**63, size=(count, n, width), dtype=np.uint64) % np.uint64(p)).astype(dt)
    x[0, 0, 0], x[-1, -1, -1], x[0, n // 2, width // 2] = 0, p - 1, p - 1
    inv = oracle_py.intt(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(count * width, n), _table_cached(logn, cls), p, nthreads=8)
    u = _powers(pow(shift, p - 2, p), _bitrev_array(logn), p, dt)
    want = np.ascontiguousarray(oracle_py.pointwise(inv, np.broadcast_to(u, inv.shape).copy(), p).reshape(count, width, n).transpose(0, 2, 1))
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


def _plan(logn, cls):
    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    pl = eng.NTTPlan(logn, p, wb, 0)
    pl.set_twiddles(np.array(_table_cached(logn, cls)))
    return pl


class _Guarded:
    """`count` matrices [rows][pitch] in the middle of one allocation: a sentinel matrix (at least) on each side, sentinel in every padding
    column.  The leading guard is rounded up to whole 16-byte units, so that the first matrix starts where the interface wants it: a
    2 x 3 matrix of 4-byte words is 24 bytes"""

    def __init__(self, rows, pitch, width, count, sentinel, tdt):
        import torch

        self.words, self.count, self.width, self.s = rows * pitch, count, width, sentinel
        unit = 16 // torch.empty((), dtype=tdt).element_size()
        self.lead = -(-self.words // unit) * unit
        self.big = torch.full((self.lead + (count + 1) * self.words,), sentinel, dtype=tdt, device="cuda:0")
        self.view = self.big[self.lead: self.lead + count * self.words].view(count, rows, pitch)
        self.live = self.view[:, :, :width]
        assert self.view.data_ptr() % 16 == 0

    def intact(self):
        import torch

        torch.cuda.synchronize()
        end = self.lead + self.count * self.words
        return bool((self.big[:self.lead] == self.s).all()) and bool((self.big[end:] == self.s).all()) and bool((self.view[:, :, self.width:] == self.s).all())


@pytest.mark.parametrize("cls", sorted(ALL_CLASSES))
@pytest.mark.parametrize("shape", LDE_SHAPES, ids=lambda s: "m%d_b%d_w%d_ip%d_op%d_c%d" % s)
def test_lde_columns_against_the_oracle_with_guard_words(oracle, cls, shape):
    """the guards are intact (the input's padding is non-canonical junk), the input is unchanged, every live word is the oracle's"""
    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    wb, p, g = ALL_CLASSES[cls]
    logm, beta, width, in_pitch, out_pitch, count = shape
    m = 1 << logm
    shift = _shift(cls, LDE_SHAPES.index(shape))
    tdt = torch.int32 if wb == 4 else torch.int64
    x, want = _lde_case(cls, logm, beta, width, count, shift)
    pl = _plan(logm, cls)
    pl.set_coset(beta, shift)
    gin, gout = _Guarded(m >> beta, in_pitch, width, count, -3, tdt), _Guarded(m, out_pitch, width, count, -5, tdt)
    gin.live.copy_(eng.to_device(x, "cuda:0"))
    gout.live.fill_(-7)
    torch.cuda.synchronize()
    assert _lib.lib().ntt_lde_columns(pl._h, gin.view.data_ptr(), in_pitch, gout.view.data_ptr(), out_pitch, width, count, None) == 0
    assert gin.intact() and gout.intact(), (cls, shape)
    assert np.array_equal(eng.to_host(gin.live), x), (cls, shape, "input is read only")
    assert np.array_equal(eng.to_host(gout.live), want), (cls, shape)
    pl.close()


@pytest.mark.parametrize("cls", sorted(ALL_CLASSES))
@pytest.mark.parametrize("shape", CINV_SHAPES, ids=lambda s: "n%d_w%d_p%d_c%d" % s)
def test_coset_inverse_columns_against_the_oracle_with_guard_words(oracle, cls, shape):
    """out of place and in place, with the same guards"""
    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    wb, p, g = ALL_CLASSES[cls]
    logn, width, pitch, count = shape
    shift = _shift(cls, CINV_SHAPES.index(shape) + 1)
    tdt = torch.int32 if wb == 4 else torch.int64
    x, want = _cinv_case(cls, logn, width, count, shift)
    pl = _plan(logn, cls)
    pl.set_coset_inverse(shift)
    gin, gout = _Guarded(1 << logn, pitch, width, count, -3, tdt), _Guarded(1 << logn, pitch, width, count, -5, tdt)
    gin.live.copy_(eng.to_device(x, "cuda:0"))
    gout.live.fill_(-7)
    torch.cuda.synchronize()
    call = lambda a, b: _lib.lib().ntt_coset_inverse_columns(pl._h, a, b, width, pitch, count, None)
    assert call(gin.view.data_ptr(), gout.view.data_ptr()) == 0
    assert gin.intact() and gout.intact(), (cls, shape)
    assert np.array_equal(eng.to_host(gin.live), x), (cls, shape, "input is read only")
    assert np.array_equal(eng.to_host(gout.live), want), (cls, shape, "out of place")
    assert call(gin.view.data_ptr(), gin.view.data_ptr()) == 0
    assert gin.intact(), (cls, shape, "in place")
    assert np.array_equal(eng.to_host(gin.live), want), (cls, shape, "in place")
    pl.close()


@pytest.mark.parametrize("cls", ["gl", "m32", "bb31", "top32"])
def test_round_trip_and_sampled_evaluations(oracle, cls):
    """kind-1 tables, logm 13, beta 3, width 33: coset_inverse_columns(lde_columns(x)) has row j << beta equal to x[j] and every other
    row zero; and for 8 sampled (k, c), lde_columns(x)[k][c] is the column's polynomial -- row j holds coefficient bitrev_N(j) --
    evaluated at shift * w_M^k with Python integers"""
    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    logm, beta, width = 13, 3, 33
    m, n = 1 << logm, (1 << logm) >> beta
    assert (p - 1) % m == 0
    shift = g
    x, _ = _lde_case(cls, logm, beta, width, 1, shift)
    pl = _plan(logm, cls)
    pl.set_coset(beta, shift)
    pl.set_coset_inverse(shift)
    ext = pl.lde_columns(eng.to_device(x[0], "cuda:0"))
    assert tuple(ext.shape) == (m, width)
    back = eng.to_host(pl.coset_inverse_columns(ext))
    assert np.array_equal(back[:: 1 << beta], x[0])
    mask = np.ones(m, dtype=bool)
    mask[:: 1 << beta] = False
    assert not back[mask].any()
    got = eng.to_host(ext)
    w_m = pow(g, (p - 1) // m, p)
    br = _bitrev_array(logm - beta)
    rng = np.random.default_rng(5)
    for k, c in zip(rng.integers(0, m, size=8), rng.integers(0, width, size=8)):
        coeff = [0] * n
        for j in range(n):
            coeff[int(br[j])] = int(x[0, j, c])
        z, acc = shift * pow(w_m, int(k), p) % p, 0
        for a in reversed(coeff):
            acc = (acc * z + a) % p
        assert int(got[k, c]) == acc, (cls, int(k), int(c))
    pl.close()


def test_wrappers_on_strided_views_and_value_errors(oracle):
    import torch

    import ntt_aie_amd as eng

    cls, logm, beta, width, count = "gl", 9, 1, 33, 2
    wb, p, g = ALL_CLASSES[cls]
    m, n = 1 << logm, (1 << logm) >> beta
    shift = g
    x, want = _lde_case(cls, logm, beta, width, count, shift)
    y, want_inv = _cinv_case(cls, logm, 3, 3, shift)
    pl = _plan(logm, cls)
    with pytest.raises(ValueError):
        pl.lde_columns(torch.zeros((n, 4), dtype=torch.int64, device="cuda:0"))  # set_coset() first
    with pytest.raises(ValueError):
        pl.coset_inverse_columns(torch.zeros((m, 4), dtype=torch.int64, device="cuda:0"))  # set_coset_inverse() first
    pl.set_coset(beta, shift)
    pl.set_coset_inverse(shift)
    big_in = torch.full((count, n, 40), -3, dtype=torch.int64, device="cuda:0")
    big_out = torch.full((count, m, 48), -5, dtype=torch.int64, device="cuda:0")
    vin, vout = big_in[:, :, :width], big_out[:, :, :width]
    vin.copy_(eng.to_device(x, "cuda:0"))
    got = pl.lde_columns(vin)  # allocated: contiguous [count][M][width]
    assert got.is_contiguous() and tuple(got.shape) == (count, m, width) and np.array_equal(eng.to_host(got), want)
    assert pl.lde_columns(vin, out=vout) is vout
    assert np.array_equal(eng.to_host(vout), want) and bool((big_out[:, :, width:] == -5).all()) and bool((big_in[:, :, width:] == -3).all())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    got = pl.lde_columns(vin[0], stream=side)  # [N][width] -> [M][width]
    side.synchronize()
    assert tuple(got.shape) == (m, width) and np.array_equal(eng.to_host(got), want[0])
    big = torch.full((3, m, 8), -3, dtype=torch.int64, device="cuda:0")
    view = big[:, :, :3]
    view.copy_(eng.to_device(y, "cuda:0"))
    assert np.array_equal(eng.to_host(pl.coset_inverse_columns(view)), want_inv)  # a fresh contiguous result
    side.wait_stream(torch.cuda.current_stream())
    assert pl.coset_inverse_columns(view, out=view, stream=side) is view
    side.synchronize()
    assert np.array_equal(eng.to_host(view), want_inv) and bool((big[:, :, 3:] == -3).all())
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
            pl.lde_columns(t)
    for t in bad[:2] + [torch.zeros((n, 8), dtype=torch.int64, device="cuda:0"), torch.zeros((8, m), dtype=torch.int64, device="cuda:0").t()]:
        with pytest.raises(ValueError):
            pl.coset_inverse_columns(t)
    ok = torch.zeros((2, n, 8), dtype=torch.int64, device="cuda:0")
    with pytest.raises(ValueError):
        pl.lde_columns(ok, out=torch.zeros((2, m, 4), dtype=torch.int64, device="cuda:0"))  # shape
    with pytest.raises(ValueError):
        pl.lde_columns(ok, out=torch.zeros((2, n, 8), dtype=torch.int64, device="cuda:0"))  # rows of the output
    assert pl.lde_columns(torch.zeros((n, 0), dtype=torch.int64, device="cuda:0")).shape == (m, 0)
    pl.close()


def test_error_contract(oracle):
    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    L, E = _lib.lib(), _lib
    logm, beta = 8, 2
    m, n = 1 << logm, (1 << logm) >> beta
    x = torch.zeros((2 * m * 8,), dtype=torch.int64, device="cuda:0")
    y = torch.zeros((2 * m * 8,), dtype=torch.int64, device="cuda:0")
    a, b = x.data_ptr(), y.data_ptr()
    lde = lambda pl, i, o, w, ip, op, c: L.ntt_lde_columns(pl, i, ip, o, op, w, c, None)
    cinv = lambda pl, i, o, w, ip, op, c: L.ntt_coset_inverse_columns(pl, i, o, w, op, c, None)
    small = eng.NTTPlan(3, GOLD, 8, 0)
    small.generate_twiddles(1, 7)
    small.set_coset(1, 7)
    small.set_coset_inverse(7)
    pl = eng.NTTPlan(logm, GOLD, 8, 0)
    for call in (lde, cinv):
        assert call(None, a, b, 8, 8, 8, 1) == E.NTT_E_ARG
        assert call(small._h, a, b, 8, 8, 8, 1) == E.NTT_E_LOGN
        assert call(pl._h, a, b, 8, 8, 8, 1) == E.NTT_E_NOTABLE
    T = np.array(_table_cached(logm, "gl"))
    broken = T.copy()
    broken[200] = 0
    pl.set_twiddles(broken)
    assert cinv(pl._h, a, b, 8, 8, 8, 1) == E.NTT_E_NOTINVERTIBLE
    pl.set_twiddles(T)
    for call in (lde, cinv):
        assert call(pl._h, a, b, 8, 8, 8, 1) == E.NTT_E_ARG  # no coset / no coset-inverse shift set
        assert call(pl._h, a, b, 0, 8, 8, 1) == E.NTT_E_ARG  # ... a configuration error, reported for an empty call too
    pl.set_coset(beta, 7)
    pl.set_coset_inverse(7)
    for call in (lde, cinv):
        assert call(pl._h, a, b, 0, 8, 8, 1) == 0 and call(pl._h, a, b, 8, 8, 8, 0) == 0 and call(pl._h, None, None, 0, 0, 0, 0) == 0
        assert call(pl._h, None, b, 8, 8, 8, 1) == E.NTT_E_ARG and call(pl._h, a, None, 8, 8, 8, 1) == E.NTT_E_ARG
        assert call(pl._h, a + 8, b, 8, 8, 8, 1) == E.NTT_E_ARG and call(pl._h, a, b + 8, 8, 8, 8, 1) == E.NTT_E_ARG  # misaligned
        assert call(pl._h, a, b, 9, 8, 8, 1) == E.NTT_E_ARG                                                          # width > pitch
        assert call(pl._h, a, b, 8, 8, (1 << 20) + 1, 1) == E.NTT_E_ARG                                              # M * pitch > 2^28 words
        assert call(pl._h, a, b, (1 << 20) + 1, 1 << 21, 1 << 21, 1) == E.NTT_E_ARG                                  # logn + w > 28
        assert call(pl._h, a, b, 8, 8, 8, 2**31) == E.NTT_E_ARG
        assert call(pl._h, a, b, 8, 8, 8, 2) == 0
    assert lde(pl._h, a, b, 8, 7, 8, 1) == E.NTT_E_ARG  # width > in_pitch
    assert lde(pl._h, a, a, 8, 8, 8, 1) == E.NTT_E_ARG  # d_in == d_out: out of place only
    assert cinv(pl._h, a, a, 8, 8, 8, 2) == 0           # in place
    assert cinv(pl._h, a, a + 16, 8, 8, 8, 2) == E.NTT_E_ARG  # partial overlap
    # overlap by the last live word alone: the output's last live word is the input's first / the input's last is the output's first
    assert cinv(pl._h, a, a + 8 * ((2 * m - 1) * 8 + 6), 7, 8, 8, 2) == E.NTT_E_ARG
    assert lde(pl._h, a + 8 * ((2 * m - 1) * 8 + 6), a, 7, 8, 8, 2) == E.NTT_E_ARG
    assert lde(pl._h, a, a + 8 * ((2 * n - 1) * 8 + 6), 7, 8, 8, 2) == E.NTT_E_ARG
    assert lde(pl._h, a, a + 8 * ((2 * n - 1) * 8 + 8), 7, 8, 8, 1) == 0  # one 16-byte step further: apart (count 1 keeps it inside x)
    torch.cuda.synchronize()
    small.close()
    pl.close()
