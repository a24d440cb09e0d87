"""Coset interpolation on the GPU (ntt_plan_set_coset_inverse / ntt_coset_inverse, NTTPlan.coset_inverse,
MultiDevicePlan.coset_inverse).

Every result is compared word for word with the ORACLE: oracle.intt (the scaled inverse network, halving per stage) times the
Python-integer vector pow(shift, -bitrev(i), p) -- include/ntt_hip.h states exactly this -- never with the library's own unfused
path alone."""
import functools

import numpy as np
import pytest

from test_gpu_columns import ALL_CLASSES, CLASSES, GOLD, STREAM_CLASSES  # noqa: F401

pytestmark = pytest.mark.gpu

# the word classes of tests/test_gpu_lde.py, defined once in tests/test_gpu_columns.py.  CLASSES: Goldilocks, a general 64-bit NTT prime above 2^63, a lazy 4-byte NTT prime, the
# reference's own modulus (p - 1 = 2^8 * 13: kind-1 tables exist up to 2^8 only, larger sizes take the reference's kind-0 rule --
# ntt_coset_inverse is defined at network level, for any invertible table).  STREAM_CLASSES: three more 4-byte moduli for the other two
# instruction streams of 4-byte words
FUSED_FROM = 5  # the documented rule of ntt_plan_info 12


def _bitrev_np(bits):
    i = np.arange(1 << bits, dtype=np.uint64)
    r = np.zeros_like(i)
    for k in range(bits):
        r |= ((i >> np.uint64(k)) & np.uint64(1)) << np.uint64(bits - 1 - k)
    return r.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _vector(logm, shift, p, wb):
    """pow(shift, -bitrev(i), p) for i < 2^logm in Python integers (a running product of shift^-1, read in bit-reversed order)"""
    m = 1 << logm
    sinv = pow(shift, -1, p)
    pw = [1] * m
    for e in range(1, m):
        pw[e] = pw[e - 1] * sinv % p
    assert pw[m - 1] == pow(shift, -(m - 1), p)
    br = _bitrev_np(logm)
    v = np.array([pw[int(b)] for b in br], dtype=np.uint32 if wb == 4 else np.uint64)
    v.setflags(write=False)
    return v


def _table(oracle, logm, wb, p, g):
    m = 1 << logm
    if (p - 1) % m == 0:
        return oracle.make_table(1, m, p, g, wb)
    return oracle.make_roots(m, p, g, wb)


def _expected(oracle, y, T, p, shift):
    """the header's definition, through the oracle: y in natural order"""
    batch, m = y.shape
    u = _vector(m.bit_length() - 1, shift, p, y.dtype.itemsize)
    c = oracle.intt(y, T, p, nthreads=8)
    return oracle.pointwise(c, np.ascontiguousarray(np.broadcast_to(u, (batch, m))), p)


def _inputs(batch, n, p, dt, seed):
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, 2**63, size=(batch, n), dtype=np.uint64) % np.uint64(p)).astype(dt)
    flat = a.reshape(-1)
    flat[0] = 0
    flat[-1] = p - 1
    flat[flat.size // 2] = p - 1
    if flat.size > 3:
        flat[1] = 0
    return a


def _plan(oracle, logm, cls):
    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    T = _table(oracle, logm, wb, p, g)
    pl = eng.NTTPlan(logm, p, wb, 0)
    pl.set_twiddles(T)
    return pl, T


def test_pointwise_comparator_is_python_integers(oracle):
    """the oracle's pointwise product used by _expected, against Python integers (so the comparator is what the issue states)"""
    for cls in sorted(CLASSES):
        wb, p, g = ALL_CLASSES[cls]
        dt = np.uint32 if wb == 4 else np.uint64
        y = _inputs(2, 64, p, dt, 1)
        T = _table(oracle, 6, wb, p, g)
        c = oracle.intt(y, T, p)
        br = [int(b) for b in _bitrev_np(6)]
        want = [[int(c[b][i]) * pow(g, -br[i], p) % p for i in range(64)] for b in range(2)]
        assert _expected(oracle, y, T, p, g).tolist() == want


@pytest.mark.parametrize("cls", sorted(ALL_CLASSES))
@pytest.mark.parametrize("logm", [1, 2, 3, 4, 5, 6, 9, 11, 13, 14, 16])
def test_coset_inverse_sweep(oracle, cls, logm):
    """word classes x sizes (unfused below 2^5; single-pass; two-pass) x batch 1 / 5 / 33 x both input layouts from 2^4, shift
    cycling through {1, g, p - 1}, inputs holding 0 and p - 1, every launch-time alternative pinned in turn at batch 5, out of place
    and in place; ntt_plan_info 12 follows the documented rule; the other transforms of the plan are unaffected by the setting"""
    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    m = 1 << logm
    pl, T = _plan(oracle, logm, cls)
    assert not pl.coset_inverse_set and not pl.coset_inverse_fused
    case = 0
    for batch in (1, 5, 33):
        y = _inputs(batch, m, p, dt, 100 * logm + batch)
        for layout in ([eng.LAYOUT_NATURAL, eng.LAYOUT_AIE_BLOCK16] if logm >= 4 else [eng.LAYOUT_NATURAL]):
            shift = (1, g, p - 1)[case % 3]
            case += 1
            pl.set_coset_inverse(shift)  # (replaces the previous setting)
            assert pl.coset_inverse_set and pl.coset_inverse_fused == (logm >= FUSED_FROM)
            want = _expected(oracle, y, T, p, shift)
            a = oracle.block16(y) if layout == eng.LAYOUT_AIE_BLOCK16 else y
            d = eng.to_device(a, "cuda:0")
            for alt in [-1] + (list(range(len(pl.alternatives))) if batch == 5 else []):
                pl.set_policy(alt)
                assert pl.coset_inverse_fused == (logm >= FUSED_FROM)
                out = pl.coset_inverse(d, layout=layout)
                assert np.array_equal(eng.to_host(out), want), (cls, logm, batch, shift, layout, alt, "out of place")
                assert np.array_equal(eng.to_host(d), a)  # the input is read only
                d2 = d.clone()
                assert pl.coset_inverse(d2, d2, layout=layout) is d2
                assert np.array_equal(eng.to_host(d2), want), (cls, logm, batch, shift, layout, alt, "in place")
            pl.set_policy(-1)
    # ntt_inverse / ntt_forward / ntt_lde on the same plan are unaffected by the setting (and the setting by ntt_plan_set_coset)
    x = _inputs(3, m, p, dt, 7)
    dx = eng.to_device(x, "cuda:0")
    assert np.array_equal(eng.to_host(pl.forward(dx)), oracle.ntt(x, T, p))
    assert np.array_equal(eng.to_host(pl.inverse(dx)), oracle.intt(x, T, p))
    assert np.array_equal(eng.to_host(pl.forward(pl.inverse(dx, scale=False))), oracle.pointwise(x, np.full_like(x, m % p), p))
    if logm >= 2:
        import test_gpu_lde as lde_tests

        pl.set_coset(1, g)
        c = _inputs(3, m >> 1, p, dt, 8)
        assert np.array_equal(eng.to_host(pl.lde(eng.to_device(c, "cuda:0"))), lde_tests._expected(oracle, c, T, p, 1, g))
        assert pl.coset_inverse_set and pl.log_blowup == 1
        assert np.array_equal(eng.to_host(pl.coset_inverse(dx)), _expected(oracle, x, T, p, shift))
    pl.close()


@pytest.mark.parametrize("p,g", [(3221225473, 5), (2013265921, 31)], ids=["p3221225473", "bb31"])
def test_coset_inverse_three_pass_plan(oracle, p, g):
    """a three-pass decomposition: 4-byte words, p >= 2^30 (above 2^31, and BabyBear below it), 2^22 = 8 + 7 + 7 (pinned), batch 2 --
    the shape of test_lde_three_pass_plan"""
    import ntt_aie_amd as eng

    logm, batch = 22, 2
    T = oracle.make_table(1, 1 << logm, p, g, 4)
    pl = eng.NTTPlan(logm, p, 4, 0)
    pl.set_twiddles(T)
    alts = [stages for stages, _ in pl.alternatives]
    assert [8, 7, 7] in alts
    pl.set_coset_inverse(g)
    pl.set_policy(alts.index([8, 7, 7]))
    assert len(pl.passes_for(batch)) == 3 and pl.coset_inverse_fused
    y = _inputs(batch, 1 << logm, p, np.uint32, 22)
    want = _expected(oracle, y, T, p, g)
    d = eng.to_device(y, "cuda:0")
    assert np.array_equal(eng.to_host(pl.coset_inverse(d)), want)
    pl.coset_inverse(d, d)
    assert np.array_equal(eng.to_host(d), want)
    pl.close()


@pytest.mark.parametrize("cls,logn,beta", [("gl", 9, 2), ("m32", 8, 4), ("bb31", 8, 4), ("top32", 9, 2)])
def test_round_trip_with_lde(oracle, cls, logn, beta):
    """coset_inverse(lde(c)) is the zero-interleaved c, both layouts between the two calls: the prover's pair is closed"""
    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    logm = logn + beta
    pl, T = _plan(oracle, logm, cls)
    pl.set_coset(beta, g)
    pl.set_coset_inverse(g)
    for batch, layout in ((5, eng.LAYOUT_NATURAL), (33, eng.LAYOUT_AIE_BLOCK16)):
        c = _inputs(batch, 1 << logn, p, dt, logm + batch)
        want = np.zeros((batch, 1 << logm), dtype=dt)
        want[:, :: 1 << beta] = c
        ev = pl.lde(eng.to_device(c, "cuda:0"), layout=layout)
        back = pl.coset_inverse(ev, layout=layout)
        assert np.array_equal(eng.to_host(back), want), (cls, layout)
        # ... and the oracle agrees about the middle: the evaluations are what it makes of the expanded, scaled coefficients
        nat = eng.to_host(pl.lde(eng.to_device(c, "cuda:0")))
        assert np.array_equal(_expected(oracle, nat, T, p, g), want)
    pl.close()


@pytest.mark.parametrize("logm,cls", [pytest.param(logm, cls, id="%d-%s" % (logm, cls)) for cls, sizes in
                                      (("gl", (5, 8, 12, 13)), ("m32", (5, 8, 12, 13)), ("bb31", (12, 13)), ("top32", (12, 13))) for logm in sizes])
def test_coset_inverse_stays_inside_the_callers_buffers(oracle, cls, logm):
    """memory safety on hardware: d_in and d_out each carved out of a larger allocation with sentinel words directly before and
    after, ragged batches (a last polynomial group that is part empty where a workgroup holds several polynomials); the sentinels
    are intact afterwards and the words are the oracle's, out of place and in place"""
    import torch

    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    tdt = torch.int32 if wb == 4 else torch.int64
    pl, T = _plan(oracle, logm, cls)
    pl.set_coset_inverse(g)
    m = 1 << logm
    pad = 64  # words: keeps the carved-out rows 16-byte aligned
    s_in, s_out = (0x5A5A5A5A, 0x3C3C3C3C) if wb == 4 else (0x5A5A5A5A5A5A5A5A, 0x3C3C3C3C3C3C3C3C)
    for batch in (1, 3, 17, 257):
        y = _inputs(batch, m, p, dt, batch + logm)
        want = _expected(oracle, y, T, p, g)
        big_in = torch.full((pad + batch * m + pad,), s_in, dtype=tdt, device="cuda:0")
        big_out = torch.full((pad + batch * m + pad,), s_out, dtype=tdt, device="cuda:0")
        d_in = big_in[pad: pad + batch * m].view(batch, m)
        d_out = big_out[pad: pad + batch * m].view(batch, m)
        d_in.copy_(eng.to_device(y, "cuda:0"))

        def intact():
            torch.cuda.synchronize()
            return (bool((big_in[:pad] == s_in).all()) and bool((big_in[pad + batch * m:] == s_in).all())
                    and bool((big_out[:pad] == s_out).all()) and bool((big_out[pad + batch * m:] == s_out).all()))

        for alt in range(len(pl.alternatives)):
            pl.set_policy(alt)
            d_out.fill_(-1)
            pl.coset_inverse(d_in, d_out)
            assert intact(), (cls, logm, batch, alt)
            assert np.array_equal(eng.to_host(d_out), want) and np.array_equal(eng.to_host(d_in), y), (cls, logm, batch, alt)
        pl.set_policy(-1)
        pl.coset_inverse(d_in, d_in)
        assert intact(), (cls, logm, batch, "in place")
        assert np.array_equal(eng.to_host(d_in), want), (cls, logm, batch, "in place")
    pl.close()


def test_coset_inverse_error_contract(oracle):
    import ctypes as C

    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    L = _lib.lib()
    pl = eng.NTTPlan(8, GOLD, 8, 0)
    x = torch.zeros((2, 256), dtype=torch.int64, device="cuda:0")
    y = torch.zeros((2, 256), dtype=torch.int64, device="cuda:0")
    st = C.c_void_p(0)
    # plan configuration
    for shift in (0, GOLD, 2**64 - 1):
        assert L.ntt_plan_set_coset_inverse(pl._h, shift) == _lib.NTT_E_ARG
    assert L.ntt_plan_set_coset_inverse(None, 7) == _lib.NTT_E_ARG
    assert not pl.coset_inverse_set
    comp = eng.NTTPlan(4, 15, 4, 0)  # a composite modulus: 3 and 5 share a factor with it, 2 is a unit
    assert L.ntt_plan_set_coset_inverse(comp._h, 3) == _lib.NTT_E_NOTINVERTIBLE
    assert L.ntt_plan_set_coset_inverse(comp._h, 10) == _lib.NTT_E_NOTINVERTIBLE
    assert L.ntt_plan_set_coset_inverse(comp._h, 15) == _lib.NTT_E_ARG and not comp.coset_inverse_set
    assert L.ntt_plan_set_coset_inverse(comp._h, 2) == 0 and comp.coset_inverse_set and not comp.coset_inverse_fused
    # the call: before the twiddles, before the setting
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), y.data_ptr(), 1, 0, st) == _lib.NTT_E_NOTABLE
    pl.set_coset_inverse(7)  # (legal before the tables: it needs none)
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), y.data_ptr(), 1, 0, st) == _lib.NTT_E_NOTABLE
    T = oracle.make_table(1, 256, GOLD, 7, 8)
    bad = T.copy()
    bad[200] = 0  # not a unit: there is no inverse network
    pl.set_twiddles(bad)
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), y.data_ptr(), 1, 0, st) == _lib.NTT_E_NOTINVERTIBLE
    assert L.ntt_inverse(pl._h, x.data_ptr(), y.data_ptr(), 1, 0, 1, st) == _lib.NTT_E_NOTINVERTIBLE
    fresh = eng.NTTPlan(8, GOLD, 8, 0)
    fresh.set_twiddles(T)
    assert L.ntt_coset_inverse(fresh._h, x.data_ptr(), y.data_ptr(), 1, 0, st) == _lib.NTT_E_ARG  # no shift set
    with pytest.raises(eng.NTTError):
        fresh.coset_inverse(x)
    pl.set_twiddles(T)
    assert (pl.coset_inverse_set, pl.coset_inverse_fused) == (True, True)
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), y.data_ptr(), 0, 0, st) == 0  # batch 0
    assert L.ntt_coset_inverse(pl._h, None, None, 0, 0, st) == 0
    assert L.ntt_coset_inverse(pl._h, None, y.data_ptr(), 1, 0, st) == _lib.NTT_E_ARG
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), None, 1, 0, st) == _lib.NTT_E_ARG
    assert L.ntt_coset_inverse(pl._h, x.data_ptr() + 8, y.data_ptr(), 1, 0, st) == _lib.NTT_E_ARG  # misaligned
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), y.data_ptr() + 8, 1, 0, st) == _lib.NTT_E_ARG
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), y.data_ptr(), 2**31, 0, st) == _lib.NTT_E_ARG   # batch out of range
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), y.data_ptr(), 1, 7, st) == _lib.NTT_E_ARG       # no such layout
    small = eng.NTTPlan(3, GOLD, 8, 0)
    small.generate_twiddles(1, 7)
    small.set_coset_inverse(7)
    assert not small.coset_inverse_fused
    assert L.ntt_coset_inverse(small._h, x.data_ptr(), y.data_ptr(), 1, eng.LAYOUT_AIE_BLOCK16, st) == _lib.NTT_E_LAYOUT
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), y.data_ptr(), 2, 0, st) == 0
    assert L.ntt_coset_inverse(pl._h, x.data_ptr(), x.data_ptr(), 2, 0, st) == 0  # in place is allowed
    torch.cuda.synchronize()
    for q in (pl, comp, fresh, small):
        q.close()


def test_coset_inverse_clone_graph_and_multi_device(oracle):
    """ntt_plan_clone carries the setting and the vector; a coset_inverse captured in a graph on one stream (a single branch) replays
    to the same words; MultiDevicePlan.coset_inverse shards by rows over the visible devices (and over clones on device 0)"""
    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import MultiDevicePlan

    p, g, logm = GOLD, 7, 14
    m = 1 << logm
    T = oracle.make_table(1, m, p, g, 8)
    pl = eng.NTTPlan(logm, p, 8, 0)
    pl.set_twiddles(T)
    pl.set_coset_inverse(g)
    y = _inputs(37, m, p, np.uint64, 3)
    want = _expected(oracle, y, T, p, g)
    d = eng.to_device(y, "cuda:0")
    cl = pl.clone()
    assert (cl.coset_inverse_set, cl.coset_inverse_fused) == (True, True)
    pl.set_coset_inverse(1)  # the clone owns its own vector: changing the source does not reach it
    assert np.array_equal(eng.to_host(cl.coset_inverse(d)), want)
    assert np.array_equal(eng.to_host(pl.coset_inverse(d)), oracle.intt(y, T, p, nthreads=8))  # shift 1: the scaled inverse itself
    pl.set_coset_inverse(g)
    # graph capture
    out = torch.empty((37, m), dtype=torch.int64, device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pl.coset_inverse(d, out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        pl.coset_inverse(d, out)
    for _ in range(2):
        out.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert np.array_equal(eng.to_host(out), want)
    del gr
    # multi-device: every visible device, and three clones on device 0 (ragged rows, one configuration order each)
    for devices, order in ((list(range(torch.cuda.device_count())), 0), ([0, 0, 0], 1)):
        md = MultiDevicePlan(logm, p, 8, devices=devices)
        if order == 0:
            md.set_coset_inverse(g)
            md.set_twiddles(T)
        else:
            md.set_twiddles(T)
            md.set_coset_inverse(g)
        assert all(q.coset_inverse_set for q in md.plans)
        shards = md.scatter(y)
        assert np.array_equal(md.gather(md.coset_inverse(shards)), want)
        md.close()
    pl.close()
    cl.close()
