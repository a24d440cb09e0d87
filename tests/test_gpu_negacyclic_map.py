"""ntt_negacyclic_map, ntt_gadget_decompose_map and ntt_polymul_gadget_map_pre on a real MI355X, through NTTPlan: bit-exact against
negacyclic_map_ref (the maps by scatter from the ring definition, then gadget_ref's digits and the reference of the prepared products, then
the addend) and equal ON THE DEVICE to the composition of the separate calls -- gadget_decompose(negacyclic_map(a)) and
polymul_gadget_pre(negacyclic_map(a)) plus the addend.  The map and decomposition shapes are the CPU sweep's with logn 1, 2, 6, 10, 13; the
product shapes per word class the size below the smallest unit, one single-pass unit (2^8: for the general 64-bit modulus a size where
polymul_gadget_pre decomposes inside its middle launch, ntt_plan_info 15 = 1, and the results must still match) and the two-pass 2^13.  Every
output lies in front of one row of guard words, and the operand and the exponents are compared with their copies after the calls.
One reference per shape at the largest batch and polynomial count: rows are independent, so a smaller batch is the first rows.  At the
two-pass product size the oracle's pipeline is run on row 0 and the last row of every batch only (it costs seconds per mapped operand
there); every row of every output is still compared with the composition, whose two calls are each held against the reference in full."""
import os

import numpy as np
import pytest

import gadget_ref as G
import negacyclic_map_ref as M
import product_dot_ref as R

pytestmark = pytest.mark.gpu

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
BATCHES, POLYS, OUTS = (1, 5, 33), (1, 2), (1, 2, 3)
# tests/test_gpu_product_gadget.py's DIGITS for these moduli: one 3-level and one 1-level set
DIGITS = {GOLD: ((8, 3, 40), (16, 1, 0)), M64: ((10, 3, 32), (16, 1, 0)), 998244353: ((10, 3, 0), (7, 1, 16)), 2013265921: ((10, 3, 0), (7, 1, 16)),
          3221225473: ((8, 3, 8), (12, 1, 4)), 3329: ((4, 3, 0), (6, 1, 0))}
MODULI = [(4, 3329), (4, 3221225473), (8, GOLD), (8, M64)]
SENTINEL = {4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}


@pytest.fixture(scope="module")
def eng():
    import torch

    import ntt_aie_amd as E

    assert torch.cuda.is_available()
    assert os.path.exists(E.LIB_PATH), "native library missing: the GPU tests must not pass without it"
    torch.cuda.set_device(0)
    return E


def _guarded(shape, wb):
    """a device buffer of `shape` filled with sentinel words, in front of one more row of them: (the view, the guard row)"""
    import torch

    n = shape[-1]
    rows = int(np.prod(shape[:-1]))
    buf = torch.full((rows + 1, max(n, 4)), SENTINEL[wb], dtype=torch.int32 if wb == 4 else torch.int64, device="cuda:0")
    return buf.view(-1)[:rows * n].view(*shape), buf.view(-1)[rows * n:]


def _intact(guard, wb):
    return bool((guard == SENTINEL[wb]).all())


def _specs(logn, wb):
    """(kind, param, per-row exponents) of the CPU sweep"""
    n, V = 1 << logn, 16 // wb
    specs = [(M.MONOMIAL, e, False) for e in (0, 1, V - 1, V, n - 1, n, n + 1, 2 * n - 1, 2 * n, 2**32 - 1)] + [(M.MONOMIAL, 0, True)]
    return specs + [(M.AUTOMORPHISM, g, False) for g in (1, 3, 5, n + 1, 2 * n - 1) if g < 2 * n]


def _operand(wb, p, polys, batch, n, seed):
    dt = np.uint32 if wb == 4 else np.uint64
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, 2**63, size=(polys, batch, n), dtype=np.uint64) % np.uint64(p)).astype(dt)
    M.edge_rows(a, p)
    return a, rng.integers(0, 2**32, size=batch, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("logn", [1, 2, 6, 10, 13])
@pytest.mark.parametrize("wb,p", MODULI)
def test_map_and_decomposition_bit_exact(eng, wb, p, logn):
    import torch

    pl = eng.NTTPlan(logn, p, wb, 0)  # no table: the maps and the digits need p alone
    n, top, tpolys = 1 << logn, max(BATCHES), max(POLYS)
    a_all, e_all = _operand(wb, p, tpolys, top, n, seed=100 * logn + wb)
    for flags in (False, True):
        for kind, param, perrow in _specs(logn, wb):
            want = M.mapped(a_all, p, kind, param, e_all if perrow else None, flags)
            want_d = [G.decompose(want, p, *dig) for dig in DIGITS[p]]
            for batch in BATCHES:
                d_e = eng.to_device(e_all[:batch], "cuda:0") if perrow else None
                for polys in POLYS:
                    a = np.ascontiguousarray(a_all[:polys, :batch])
                    d_a = eng.to_device(a, "cuda:0")
                    what = (logn, flags, kind, param, perrow, batch, polys)
                    out, guard = _guarded((polys, batch, n), wb)
                    assert pl.negacyclic_map(d_a, kind, param, d_e, flags, out=out) is out
                    assert np.array_equal(eng.to_host(out), want[:polys, :batch]), what
                    assert _intact(guard, wb), what
                    for dig, wd in zip(DIGITS[p], want_d):
                        w, K, l = dig
                        dg, guard = _guarded((polys, K, batch, n), wb)
                        pl.gadget_decompose_map(d_a, kind, param, d_e, flags, log_base=w, levels=K, low_bits=l, out=dg)
                        assert np.array_equal(eng.to_host(dg), wd[:polys, :, :batch]), (what, dig)
                        assert _intact(guard, wb), (what, dig)
                        assert torch.equal(dg, pl.gadget_decompose(out, w, K, l)), (what, dig)  # the composition, on the device
                    assert np.array_equal(eng.to_host(d_a), a), "a was written"
                if perrow:
                    assert np.array_equal(eng.to_host(d_e).view(np.uint32), e_all[:batch]), "the exponents were written"


def _plan(eng, oracle, wb, p, g, logn):
    pl = eng.NTTPlan(logn, p, wb, 0)
    pl.generate_twiddles(2, g)
    T = oracle.make_table(2, 1 << logn, p, g, wb)
    assert np.array_equal(pl.get_twiddles(), T)
    return pl, T


class _Ref:
    """one mapped operand at the largest batch and polynomial count; per (output, term, operand shape) the term's product from the oracle
    pipeline on the reference digits, computed once and never changed (tests/test_gpu_product_gadget.py: _Ref)"""

    def __init__(self, oracle, mapped, b, T, p, dig, rows):
        self.oracle, self.p, self.K, self.T = oracle, p, dig[1], T
        self.b = np.ascontiguousarray(b[:, :, rows])
        self.d = np.ascontiguousarray(G.decompose(mapped, p, *dig)[:, :, rows])
        self._c, self._s = {}, {}

    def _term(self, j, t, bcast):
        if (j, t, bcast) not in self._c:
            self._c[(j, t, bcast)] = R.want(self.oracle, self.d.reshape(-1, *self.d.shape[2:])[t:t + 1], self.b[j, t:t + 1], self.T, self.p, bcast)
        return self._c[(j, t, bcast)]

    def want(self, polys, outs, bcast):
        res = []
        for j in range(outs):
            if (polys, j, bcast) not in self._s:  # the sum over the terms of `polys` polynomials, once per output
                acc = None
                for t in range(polys * self.K):
                    acc = self._term(j, t, bcast) if acc is None else R.addmod(acc, self._term(j, t, bcast), self.p)
                self._s[(polys, j, bcast)] = acc
            res.append(self._s[(polys, j, bcast)])
        return np.stack(res)


# (word bytes, p, g, logn, ntt_plan_info 15)
PRODUCT_SHAPES = [
    (8, GOLD, 7, 6, 0), (8, GOLD, 7, 8, 0), (8, GOLD, 7, 13, 0),
    (8, M64, 3, 6, 0), (8, M64, 3, 8, 1), (8, M64, 3, 13, 0),  # 2^8: polymul_gadget_pre takes its digit kernels, the fused call never does
    (4, 998244353, 3, 5, 0), (4, 998244353, 3, 8, 0), (4, 998244353, 3, 13, 0),
]


@pytest.mark.parametrize("wb,p,g,logn,fused", PRODUCT_SHAPES)
def test_product_bit_exact_against_the_reference_and_the_composition(eng, oracle, wb, p, g, logn, fused):
    import torch

    from ntt_aie_amd import _lib

    pl, T = _plan(eng, oracle, wb, p, g, logn)
    assert _lib.lib().ntt_plan_info(pl._h, 15) == fused
    n, top, tpolys, touts = 1 << logn, max(BATCHES), max(POLYS), max(OUTS)
    dig = DIGITS[p][0]
    w, K, l = dig
    a_all, e_all = _operand(wb, p, tpolys, top, n, seed=7000 + 10 * logn + wb)
    _, b, T2, bhat = R.operands(oracle, wb, p, g, logn, top, touts * tpolys * K, seed=logn + 50)
    assert np.array_equal(T2, T)
    b, bhat = b.reshape(touts, tpolys * K, top, n), bhat.reshape(touts, tpolys * K, top, n)
    add_all, _ = _operand(wb, p, touts, top, n, seed=9000 + logn)
    # the rows held against the oracle's pipeline: all of them, and at the two-pass size -- where that pipeline costs seconds per mapped
    # operand -- row 0 (the edge words, the broadcast row) and the last row of every batch; EVERY row is compared with the composition
    rows = list(range(top)) if logn < 13 else sorted({0} | {bt - 1 for bt in BATCHES})
    for kind, param, perrow in ((M.MONOMIAL, 0, True), (M.AUTOMORPHISM, 5 if logn > 1 else 3, False)):
        for flags in (False, True):
            ref = _Ref(oracle, M.mapped(a_all, p, kind, param, e_all if perrow else None, flags), b, T, p, dig, rows)
            for batch in BATCHES:
                d_e = eng.to_device(e_all[:batch], "cuda:0") if perrow else None
                for polys in POLYS:
                    a = np.ascontiguousarray(a_all[:polys, :batch])
                    d_a = eng.to_device(a, "cuda:0")
                    d_map = pl.negacyclic_map(d_a, kind, param, d_e, flags)
                    for outs in OUTS:
                        d_add = eng.to_device(np.ascontiguousarray(add_all[:outs, :batch]), "cuda:0")
                        for bcast, bh in ((False, bhat[:outs, :polys * K, :batch]), (True, bhat[:outs, :polys * K, 0])):
                            d_bh = eng.to_device(np.ascontiguousarray(bh), "cuda:0")
                            sel = [r for r in rows if r < batch]
                            plain = ref.want(polys, outs, bcast)[:, :len(sel)]
                            comp = pl.polymul_gadget_pre(d_map, w, K, l, d_bh)  # the composition's product, on the device
                            addends = [(None, None), (d_add, add_all[:outs, :batch])] + ([(d_a, a)] if outs == polys else [])
                            for d_ad, ad in addends:
                                what = (logn, kind, flags, batch, polys, outs, bcast, ad is not None, d_ad is d_a)
                                out, guard = _guarded((outs, batch, n), wb)
                                work, wguard = _guarded((polys * K, batch, n), wb)
                                got = pl.polymul_gadget_map_pre(d_a, kind, param, d_e, flags, log_base=w, levels=K, low_bits=l, bhat=d_bh, addend=d_ad, work=work, out=out)
                                assert got is out
                                host = eng.to_host(out)
                                assert np.array_equal(host[:, sel], plain if ad is None else R.addmod(plain, np.ascontiguousarray(ad[:, sel]), p)), what
                                assert _intact(guard, wb) and _intact(wguard, wb), what
                                if ad is None:  # the composition, on the device, every row
                                    assert torch.equal(out, comp), what
                                elif len(sel) < batch:  # ... plus the addend, added on the host with the carry kept
                                    assert np.array_equal(host, R.addmod(eng.to_host(comp), np.ascontiguousarray(ad), p)), what
                            assert np.array_equal(eng.to_host(d_bh), np.ascontiguousarray(bh)), "b^ was written"
                        assert np.array_equal(eng.to_host(d_add), add_all[:outs, :batch]), "the addend was written"
                    assert np.array_equal(eng.to_host(d_a), a), "a was written"
                if perrow:
                    assert np.array_equal(eng.to_host(d_e).view(np.uint32), e_all[:batch]), "the exponents were written"


@pytest.mark.parametrize("wb,p,g", [(8, GOLD, 7), (4, 2013265921, 31)])
def test_ring_level_identities(eng, oracle, wb, p, g):
    """at 2^8, through the library's own product: X^e . a is polymul_negacyclic(a, X^e), and sigma_g is a ring homomorphism"""
    import torch

    logn, batch = 8, 5
    n = 1 << logn
    pl, _ = _plan(eng, oracle, wb, p, g, logn)
    a, _ = _operand(wb, p, 1, batch, n, seed=21)
    b, _ = _operand(wb, p, 1, batch, n, seed=22)
    d_a, d_b = eng.to_device(a, "cuda:0"), eng.to_device(b, "cuda:0")
    for e in (0, 1, 3, n - 1, n, n + 1, 2 * n - 1):
        mono = np.zeros((batch, n), dtype=a.dtype)
        mono[:, e % n] = 1 if e < n else p - 1  # X^e, with X^N = -1
        prod = pl.polymul_negacyclic(d_a[0].clone(), eng.to_device(mono, "cuda:0"))
        assert torch.equal(pl.negacyclic_map(d_a, M.MONOMIAL, e)[0], prod), e
    ab = pl.polymul_negacyclic(d_a[0].clone(), d_b[0].clone())
    for gg in (3, 5, n + 1, 2 * n - 1):
        sa, sb = pl.negacyclic_map(d_a, M.AUTOMORPHISM, gg), pl.negacyclic_map(d_b, M.AUTOMORPHISM, gg)
        lhs = pl.negacyclic_map(ab.view(1, batch, n), M.AUTOMORPHISM, gg)[0]
        assert torch.equal(lhs, pl.polymul_negacyclic(sa[0].clone(), sb[0].clone())), gg
    assert np.array_equal(eng.to_host(d_a), a) and np.array_equal(eng.to_host(d_b), b)


def test_c_abi_errors_write_nothing(eng, oracle):
    import torch

    from ntt_aie_amd import _lib

    L = _lib.lib()
    pl, _ = _plan(eng, oracle, 8, GOLD, 7, 7)
    n, row, S = 128, 128 * 8, SENTINEL[8]
    a = torch.zeros((2, 5, n), dtype=torch.int64, device="cuda:0")
    bh = torch.zeros((2, 6, 5, n), dtype=torch.int64, device="cuda:0")
    ex = torch.zeros((8,), dtype=torch.int32, device="cuda:0")
    mo = torch.full((2, 5, n), S, dtype=torch.int64, device="cuda:0")    # ntt_negacyclic_map's output
    dg = torch.full((6, 5, n), S, dtype=torch.int64, device="cuda:0")    # the digits / the work buffer
    out = torch.full((2, 5, n), S, dtype=torch.int64, device="cuda:0")   # the product's output
    ad = torch.zeros((2, 5, n), dtype=torch.int64, device="cuda:0")
    A, B, E, MO, DG, O, AD = (t.data_ptr() for t in (a, bh, ex, mo, dg, out, ad))
    ARG = _lib.NTT_E_ARG

    def nm(a_=A, o_=MO, polys=2, batch=5, kind=0, param=1, e_=None, flags=0, plan=pl):
        return L.ntt_negacyclic_map(plan._h, a_, o_, polys, batch, kind, param, e_, flags, None)

    def dm(a_=A, d_=DG, polys=2, batch=5, kind=0, param=1, e_=None, flags=0, dig=(8, 3, 40), plan=pl):
        return L.ntt_gadget_decompose_map(plan._h, a_, polys, batch, kind, param, e_, flags, *dig, d_, None)

    def pm(a_=A, polys=2, kind=0, param=1, e_=None, flags=0, dig=(8, 3, 40), w_=DG, b_=B, rows=5, outs=2, ad_=None, o_=O, batch=5, plan=pl):
        return L.ntt_polymul_gadget_map_pre(plan._h, a_, polys, kind, param, e_, flags, *dig, w_, b_, rows, outs, ad_, o_, batch, None)

    # the shared map rules, through all three entry points
    for f in (nm, dm, pm):
        assert f(kind=2) == ARG and f(kind=-1) == ARG                          # an unknown kind
        assert f(flags=2) == ARG and f(flags=3) == ARG and f(flags=-2) == ARG   # an unknown flag bit
        assert f(kind=1, param=2) == ARG and f(kind=1, param=0) == ARG         # an even g
        assert f(kind=1, param=2 * n) == ARG and f(kind=1, param=2 * n + 1) == ARG  # g >= 2N
        assert f(kind=1, param=3, e_=E) == ARG                                 # exponents with the automorphism
        assert f(e_=E + 2) == ARG                                              # exponents not 4-byte aligned
        assert f(a_=None) == ARG and f(a_=A + 8) == ARG                        # null and misaligned data pointers
        assert f(polys=0) == ARG
    assert nm(o_=None) == ARG and nm(o_=MO + 8) == ARG and dm(d_=None) == ARG and dm(d_=DG + 8) == ARG
    for name, ptr in (("w_", DG), ("b_", B), ("o_", O)):
        assert pm(**{name: None}) == ARG and pm(**{name: ptr + 8}) == ARG
    assert pm(ad_=AD + 8) == ARG
    # the row limits
    assert nm(polys=(1 << 31) // 5 + 1) == ARG and dm(polys=(1 << 31) // 15 + 1) == ARG and pm(polys=(1 << 31) // 15 + 1) == ARG
    assert pm(outs=(1 << 31) // 5 + 1) == ARG and pm(outs=0) == ARG and pm(rows=2) == ARG
    assert dm(dig=(8, 3, 48)) == ARG and pm(dig=(0, 3, 0)) == ARG              # the decomposition's rules
    # overlaps: out of place only, and the exponents apart from everything written
    assert nm(o_=A) == ARG and nm(o_=A + 9 * row) == ARG and nm(a_=MO + 9 * row) == ARG
    assert dm(d_=A + 9 * row) == ARG and dm(a_=DG + 29 * row) == ARG
    assert nm(e_=MO) == ARG and nm(e_=MO + 10 * row - 4) == ARG and nm(e_=MO + 10 * row - 20) == ARG  # the last exponent in the first output word ... the first in the last
    assert dm(e_=DG + 30 * row - 4) == ARG
    assert pm(e_=DG + 4) == ARG and pm(e_=O + 10 * row - 4) == ARG
    assert pm(w_=A + 9 * row) == ARG and pm(o_=A + 9 * row) == ARG and pm(b_=A + 9 * row) == ARG and pm(o_=DG + 29 * row) == ARG
    assert pm(o_=B + 59 * row) == ARG and pm(w_=B + 59 * row) == ARG
    assert pm(ad_=DG + 29 * row) == ARG and pm(ad_=O + 9 * row) == ARG and pm(ad_=O) == ARG  # the addend against work and out
    torch.cuda.synchronize()
    for t in (mo, dg, out):
        assert bool((t == S).all()), "an argument error wrote something"
    assert bool((a == 0).all()) and bool((ex == 0).all())
    # ... and the legal neighbours of those errors
    assert nm() == 0 and nm(e_=E) == 0 and nm(kind=1, param=2 * n - 1) == 0 and nm(flags=1) == 0 and nm(param=0xFFFFFFFF) == 0
    assert nm(e_=A) == 0                                                       # exponents inside what is only read
    assert dm() == 0 and dm(e_=E, flags=1) == 0
    assert pm() == 0 and pm(e_=E, flags=1, ad_=A) == 0 and pm(ad_=AD, rows=1) == 0 and pm(ad_=B) == 0  # the addend is only read: a, or b^, will do
    bare = eng.NTTPlan(7, GOLD, 8, 0)  # no tables: the map and the digits need none, the product does
    assert nm(plan=bare) == 0 and dm(plan=bare) == 0 and pm(plan=bare) == _lib.NTT_E_NOTABLE
    assert nm(a_=None, o_=None, batch=0, kind=7) == 0 and dm(a_=None, d_=None, batch=0) == 0  # batch == 0
    assert L.ntt_polymul_gadget_map_pre(pl._h, None, 0, 0, 0, None, 0, 0, 0, 0, None, None, 3, 0, None, None, 0, None) == 0
    assert L.ntt_negacyclic_map(None, A, MO, 2, 5, 0, 1, None, 0, None) == ARG
    torch.cuda.synchronize()
    # the NTTPlan wrappers
    with pytest.raises(ValueError):
        pl.negacyclic_map(a[0], 0, 1)
    with pytest.raises(ValueError):
        pl.negacyclic_map(a, 0, 1, out=dg)
    with pytest.raises(ValueError):
        pl.negacyclic_map(a, 0, exps=ex)  # 8 exponents for 5 rows
    with pytest.raises(ValueError):
        pl.negacyclic_map(a, 0, exps=ex[:5].to(torch.int64))
    with pytest.raises(ValueError):
        pl.gadget_decompose_map(a, 0, 1, log_base=8, levels=0, low_bits=40)
    with pytest.raises(ValueError):
        pl.polymul_gadget_map_pre(a, 0, 1, log_base=8, levels=3, low_bits=40, bhat=bh, addend=ad[:1])
    with pytest.raises(_lib.NTTError):
        pl.negacyclic_map(a, 1, 2)  # the library's NTT_E_ARG, raised by the wrapper
    assert torch.equal(pl.negacyclic_map(a, 0, -1), pl.negacyclic_map(a, 0, 2 * n - 1))
