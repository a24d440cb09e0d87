"""Coset low-degree extension on the GPU (ntt_plan_set_coset / ntt_lde, NTTPlan.lde, lde_from_evals, MultiDevicePlan.lde).

Every result is compared word for word with the ORACLE's network applied to the expanded input
    x[b][i << beta] = in[b][i] * shift^bitrev_logN(i) mod p,   zero elsewhere
(include/ntt_hip.h states exactly this) -- never with the library's own unfused path alone."""
import numpy as np
import pytest

from test_gpu_columns import ALL_CLASSES, CLASSES, GOLD, STREAM_CLASSES  # noqa: F401

pytestmark = pytest.mark.gpu

# word class -> (word bytes, p, generator), defined once in tests/test_gpu_columns.py.  CLASSES: Goldilocks, a general 64-bit NTT prime above 2^63, a lazy 4-byte NTT prime, the
# reference's own modulus (p - 1 = 2^8 * 13: kind-1 tables exist up to 2^8 only, larger sizes take the reference's kind-0 rule --
# ntt_lde is defined at network level, for any table).  STREAM_CLASSES: three more 4-byte moduli, in [2^30, 2^31) and above 2^31, which
# take the kernels through the other two instruction streams of 4-byte words


def _bitrev(i, bits):
    r = 0
    for k in range(bits):
        r |= ((i >> k) & 1) << (bits - 1 - k)
    return r


def _table(oracle, logm, wb, p, g):
    m = 1 << logm
    if (p - 1) % m == 0:
        return oracle.make_table(1, m, p, g, wb)
    return oracle.make_roots(m, p, g, wb)


def _coset_vector(logn, shift, p):
    return [pow(shift, _bitrev(i, logn), p) for i in range(1 << logn)]


def _expected(oracle, a, T, p, beta, shift, layout=0):
    """the header's definition, through the oracle"""
    batch, n = a.shape
    x = np.zeros((batch, n << beta), dtype=a.dtype)
    if p < 2**32:  # products fit 64 bits
        s = np.array(_coset_vector(n.bit_length() - 1, shift, p), dtype=np.uint64)
        x[:, :: 1 << beta] = ((a.astype(np.uint64) * s[None, :]) % np.uint64(p)).astype(a.dtype)
    else:
        s = np.array(_coset_vector(n.bit_length() - 1, shift, p), dtype=object)
        x[:, :: 1 << beta] = ((a.astype(object) * s[None, :]) % p).astype(a.dtype)
    y = oracle.ntt(x, T, p, nthreads=8)
    return oracle.block16(y) if layout else y


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


@pytest.mark.parametrize("cls", sorted(ALL_CLASSES))
@pytest.mark.parametrize("logm", [3, 4, 5, 6, 9, 11, 13, 14, 16])
def test_lde_sweep(oracle, cls, logm):
    """word classes x sizes (unfused below 2^5; single-pass; two-pass) x blow-up 1..4 x batch 1 / 5 / 33 x both layouts, shift
    cycling through {1, g, p - 1}, inputs holding 0 and p - 1, every launch-time alternative of the plan pinned in turn"""
    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    pl, T = _plan(oracle, logm, cls)
    assert pl.log_blowup == 0 and not pl.lde_fused
    case = 0
    for beta in range(1, min(4, logm - 1) + 1):
        n = 1 << (logm - beta)
        for batch in (1, 5, 33):
            shift = (1, g, p - 1)[case % 3]
            layout = eng.LAYOUT_AIE_BLOCK16 if (logm >= 4 and case % 2) else eng.LAYOUT_NATURAL
            case += 1
            pl.set_coset(beta, shift)  # (replaces the previous setting)
            assert pl.log_blowup == beta and pl.lde_fused == (logm >= 5)
            a = _inputs(batch, n, p, dt, 100 * logm + case)
            want = _expected(oracle, a, T, p, beta, shift, layout)
            d = eng.to_device(a, "cuda:0")
            for alt in [-1] + (list(range(len(pl.alternatives))) if batch == 5 else []):
                pl.set_policy(alt)
                out = pl.lde(d, layout=layout)
                assert out.shape == (batch, 1 << logm)
                assert np.array_equal(eng.to_host(out), want), (cls, logm, beta, batch, shift, layout, alt)
            pl.set_policy(-1)
            assert np.array_equal(eng.to_host(d), a)  # the input is read only
    # ntt_forward on a plan with a coset set is unaffected
    x = _inputs(3, 1 << logm, p, dt, 7)
    assert np.array_equal(eng.to_host(pl.forward(eng.to_device(x, "cuda:0"))), oracle.ntt(x, T, p))
    pl.close()


@pytest.mark.parametrize("p,g", [(3221225473, 5), (2013265921, 31)], ids=["p3221225473", "bb31"])
def test_lde_three_pass_plan(oracle, p, g):
    """a three-pass decomposition: 4-byte words, p >= 2^30 (above 2^31, and BabyBear below it: plan.h offers the alternative to every
    non-lazy 4-byte modulus), 2^22 = 8 + 7 + 7 (alternative 1, pinned) and the two-pass default"""
    import ntt_aie_amd as eng

    logm = 22
    T = oracle.make_table(1, 1 << logm, p, g, 4)
    pl = eng.NTTPlan(logm, p, 4, 0)
    pl.set_twiddles(T)
    alts = [stages for stages, _ in pl.alternatives]
    assert [8, 7, 7] in alts
    for beta, batch, shift in ((1, 1, g), (3, 5, p - 1), (4, 2, 1)):
        pl.set_coset(beta, shift)
        a = _inputs(batch, 1 << (logm - beta), p, np.uint32, beta)
        want = _expected(oracle, a, T, p, beta, shift)
        d = eng.to_device(a, "cuda:0")
        for alt in range(len(alts)):
            pl.set_policy(alt)
            assert len(pl.passes_for(batch)) == len(alts[alt])
            assert np.array_equal(eng.to_host(pl.lde(d)), want), (beta, batch, alt)
    pl.close()


@pytest.mark.parametrize("cls,logm", [("gl", 5), ("gl", 10), ("gl", 11), ("gl", 13), ("gl", 16), ("m64", 9), ("m32", 5), ("m32", 10),
                                      ("m32", 12), ("m32", 14), ("kyber", 7), ("gl", 4), ("m32", 3), ("bb31", 12), ("kb31", 14),
                                      ("top32", 5), ("top32", 10)])
def test_lde_stays_inside_the_callers_buffers(oracle, cls, logm):
    """memory safety on hardware: d_out carved out of a larger allocation with sentinel words directly before and after, d_in an
    allocation of exactly batch * N words, ragged batches (a last polynomial group that is part empty at the sizes where a
    workgroup holds several polynomials); the sentinels are intact afterwards and the words are the oracle's"""
    import torch

    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    tdt = torch.int32 if wb == 4 else torch.int64
    pl, T = _plan(oracle, logm, cls)
    m = 1 << logm
    pad = 64  # words: keeps the carved-out rows 16-byte aligned
    sentinel = 0x5A5A5A5A if wb == 4 else 0x5A5A5A5A5A5A5A5A
    for beta in sorted({1, min(4, logm - 1)}):
        n = m >> beta
        pl.set_coset(beta, g)
        for batch in (1, 3, 7, 37):
            a = _inputs(batch, n, p, dt, batch + beta)
            d_in = eng.to_device(a.reshape(-1), "cuda:0")  # exactly batch * N words
            big = torch.full((pad + batch * m + pad,), sentinel, dtype=tdt, device="cuda:0")
            out = big[pad: pad + batch * m].view(batch, m)
            for alt in range(len(pl.alternatives)):
                pl.set_policy(alt)
                out.fill_(-1)
                pl.lde(d_in, out)
                torch.cuda.synchronize()
                assert bool((big[:pad] == sentinel).all()) and bool((big[pad + batch * m:] == sentinel).all()), (cls, logm, beta, batch, alt)
                assert np.array_equal(eng.to_host(out), _expected(oracle, a, T, p, beta, g)), (cls, logm, beta, batch, alt)
            pl.set_policy(-1)
    pl.close()


def test_lde_error_contract():
    import ctypes as C

    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    L = _lib.lib()
    pl = eng.NTTPlan(8, GOLD, 8, 0)
    x = torch.zeros((2, 256), dtype=torch.int64, device="cuda:0")
    y = torch.zeros((2, 256), dtype=torch.int64, device="cuda:0")
    st = C.c_void_p(0)
    assert L.ntt_lde(pl._h, x.data_ptr(), y.data_ptr(), 1, 0, st) == _lib.NTT_E_NOTABLE
    pl.generate_twiddles(1, 7)
    assert L.ntt_lde(pl._h, x.data_ptr(), y.data_ptr(), 1, 0, st) == _lib.NTT_E_ARG  # no coset set
    with pytest.raises(ValueError):
        pl.lde(x)
    for beta, shift in ((0, 7), (5, 7), (-1, 7), (2, 0), (2, GOLD), (2, 2**64 - 1)):
        assert L.ntt_plan_set_coset(pl._h, beta, shift) == _lib.NTT_E_ARG
    assert L.ntt_plan_set_coset(None, 1, 7) == _lib.NTT_E_ARG
    small = eng.NTTPlan(3, GOLD, 8, 0)
    assert L.ntt_plan_set_coset(small._h, 3, 7) == _lib.NTT_E_ARG and L.ntt_plan_set_coset(small._h, 2, 7) == 0  # beta <= logM - 1
    pl.set_coset(2, 7)
    assert (pl.log_blowup, pl.lde_fused) == (2, True) and small.log_blowup == 2 and not small.lde_fused
    assert L.ntt_lde(pl._h, x.data_ptr(), y.data_ptr(), 0, 0, st) == 0  # batch 0
    assert L.ntt_lde(pl._h, None, y.data_ptr(), 1, 0, st) == _lib.NTT_E_ARG
    assert L.ntt_lde(pl._h, x.data_ptr(), None, 1, 0, st) == _lib.NTT_E_ARG
    assert L.ntt_lde(pl._h, x.data_ptr() + 8, y.data_ptr(), 1, 0, st) == _lib.NTT_E_ARG  # misaligned
    assert L.ntt_lde(pl._h, x.data_ptr(), y.data_ptr(), 1, 7, st) == _lib.NTT_E_ARG      # no such layout
    # overlapping byte ranges: in place, input inside the output, output starting inside the input
    assert L.ntt_lde(pl._h, y.data_ptr(), y.data_ptr(), 1, 0, st) == _lib.NTT_E_ARG
    assert L.ntt_lde(pl._h, y.data_ptr() + 256 * 8, y.data_ptr(), 2, 0, st) == _lib.NTT_E_ARG
    assert L.ntt_lde(pl._h, x.data_ptr(), x.data_ptr() + 64 * 8 - 16, 1, 0, st) == _lib.NTT_E_ARG
    # adjacent is fine: 1 row of 64 input words directly in front of the output row
    buf = torch.zeros((64 + 256,), dtype=torch.int64, device="cuda:0")
    assert L.ntt_lde(pl._h, buf.data_ptr(), buf.data_ptr() + 64 * 8, 1, 0, st) == 0
    torch.cuda.synchronize()
    pl.close()
    small.close()


def test_lde_real_shape_properties(oracle):
    """N = 2^16 -> M = 2^19, Goldilocks, batch 512 (2 GiB out).  shift = 1: out[b][8 k] is the original evaluation for EVERY row
    and k (the extension passes through the points it was made from); shift = g: 8 seeded rows word for word against the oracle
    (its inverse network, the expansion, its forward network); lde_from_evals is the two-step recipe."""
    import torch

    import ntt_aie_amd as eng

    p, g, logn, beta, batch = GOLD, 7, 16, 3, 512
    n, m = 1 << logn, 1 << (logn + beta)
    Tn, Tm = oracle.make_table(1, n, p, g, 8), oracle.make_table(1, m, p, g, 8)
    small, big = eng.NTTPlan(logn, p, 8, 0), eng.NTTPlan(logn + beta, p, 8, 0)
    small.generate_twiddles(1, g)
    big.generate_twiddles(1, g)
    assert np.array_equal(big.get_twiddles(), Tm)
    rng = np.random.default_rng(2024)
    evals = rng.integers(0, 2**63, size=(batch, n), dtype=np.uint64) % np.uint64(p)
    evals[0, :4] = (0, p - 1, 1, p - 2)
    d = eng.to_device(evals, "cuda:0")
    big.set_coset(beta, 1)
    assert big.lde_fused
    out = eng.lde_from_evals(small, big, d)
    assert out.shape == (batch, m)
    assert torch.equal(out.view(batch, n, 1 << beta)[:, :, 0], d)  # every row, every k
    assert torch.equal(d, eng.to_device(evals, "cuda:0"))          # lde_from_evals leaves the evaluations alone
    del out
    big.set_coset(beta, g)
    coeffs = small.inverse(d)
    out = big.lde(coeffs)
    rows = sorted({0, batch - 1} | {int(r) for r in np.random.default_rng(7).choice(batch, size=8, replace=False)})
    c_or = oracle.intt(evals[rows], Tn, p, nthreads=8)
    assert np.array_equal(eng.to_host(coeffs[rows]), c_or)
    want = _expected(oracle, c_or, Tm, p, beta, g)
    assert np.array_equal(eng.to_host(out[rows]), want)
    # the same words from the helper, and evaluations of the polynomial on the coset: P(g * w_M^k) by Horner for a few k of row 0
    out2 = eng.lde_from_evals(small, big, d, out=torch.empty_like(out))
    assert torch.equal(out2, out)
    del out2
    coef_nat = [int(c_or[0][_bitrev(j, logn)]) for j in range(n)] if rows[0] == 0 else None
    if coef_nat is not None:
        w = pow(g, (p - 1) // m, p)
        host0 = eng.to_host(out[0:1])[0]
        for k in (0, 1, 12345, m - 1):
            x, acc = g * pow(w, k, p) % p, 0
            for cj in reversed(coef_nat):
                acc = (acc * x + cj) % p
            assert int(host0[k]) == acc
    small.close()
    big.close()


def test_lde_clone_graph_and_multi_device(oracle):
    """ntt_plan_clone carries the coset; an lde captured in a graph on one stream replays to the same words; MultiDevicePlan.lde
    shards by rows over the visible devices (and over clones on device 0)"""
    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import MultiDevicePlan

    p, g, logm, beta = GOLD, 7, 14, 3
    n, m = 1 << (logm - beta), 1 << logm
    T = oracle.make_table(1, m, p, g, 8)
    pl = eng.NTTPlan(logm, p, 8, 0)
    pl.set_twiddles(T)
    pl.set_coset(beta, g)
    a = _inputs(37, n, p, np.uint64, 3)
    want = _expected(oracle, a, T, p, beta, g)
    d = eng.to_device(a, "cuda:0")
    cl = pl.clone()
    assert (cl.log_blowup, cl.lde_fused) == (beta, True)
    pl.set_coset(1, 1)  # the clone owns its own vector: changing the source does not reach it
    assert np.array_equal(eng.to_host(cl.lde(d)), want)
    pl.set_coset(beta, g)
    # graph capture
    out = torch.empty((37, m), dtype=torch.int64, device="cuda:0")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pl.lde(d, out)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        pl.lde(d, out)
    out.zero_()
    gr.replay()
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(out), want)
    out.zero_()
    gr.replay()
    torch.cuda.synchronize()
    assert np.array_equal(eng.to_host(out), want)
    del gr
    # multi-device: every visible device, and three clones on device 0 (ragged rows, one configuration order each)
    for devices, order in ((list(range(torch.cuda.device_count())), 0), ([0, 0, 0], 1)):
        md = MultiDevicePlan(logm, p, 8, devices=devices)
        if order == 0:
            md.set_coset(beta, g)
            md.set_twiddles(T)
        else:
            md.set_twiddles(T)
            md.set_coset(beta, g)
        assert all(q.log_blowup == beta for q in md.plans)
        shards = md.scatter(a)
        assert np.array_equal(md.gather(md.lde(shards)), want)
        md.close()
    md = MultiDevicePlan(logm, p, 8, devices=[0, 0, 0])  # more devices than rows: empty shards give empty [0][M] results
    md.set_twiddles(T)
    md.set_coset(beta, g)
    res = md.lde(md.scatter(a[:2]))
    assert [tuple(r.shape) for r in res] == [(1, m), (1, m), (0, m)]
    assert np.array_equal(md.gather(res), want[:2])
    md.close()
    pl.close()
    cl.close()
