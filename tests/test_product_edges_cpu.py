"""The transform-domain edge grids of the product entry points (tests/product_edge_ref.py) without a GPU: the builder's own claims --
InvU(a) is the chosen residue word for word, every ordered pair of edge residues occurs, the expected words are the schoolbook
product mod (x^N + 1, p) -- ; the three host index models (emu_polymul_fused, emu_polymul_pre, emu_polymul_dot) on exactly the cases
tests/test_gpu_product_edges.py runs, so its expectations are executed here first; and the coverage claim of that file: read from its
parametrize marks and mapped to kernels with the library's own launch lists, the cases reach every (family, field or 4-byte stream,
unit) the library can launch -- nothing typed in, so the matrix cannot drift."""
import ctypes as C

import numpy as np
import pytest

import emu_lib
import emu_product_dot_lib
import emu_product_pre_lib
import product_dot_ref
import product_edge_ref as R
import test_gpu_product_edges as TE

GOLD = 0xFFFFFFFF00000001
PRODUCT, ROW_SUM = 2, 3  # families of a step in the sequence dumps
TARGET_WGS = 8192


def _params(fn):
    """the (cls, logn) values of a test function of the GPU file, read from its pytest.mark.parametrize"""
    out = []
    for mark in fn.pytestmark:
        if mark.name == "parametrize":
            assert [s.strip() for s in mark.args[0].split(",")] == ["cls", "logn"]
            out += [tuple(getattr(i, "values", i)) for i in mark.args[1]]
    assert out and len(set(out)) == len(out), fn.__name__
    return out


UNITS = _params(TE.test_every_product_kernel_on_the_edge_grids)
BEHIND = _params(TE.test_unit_behind_column_passes)
LONG = _params(TE.test_a_long_sum_at_the_word_boundary)


# ---- the builder -----------------------------------------------------------------------------------------------------------------
def _ints(x):
    return x.astype(object)


@pytest.mark.parametrize("cls", sorted(R.CLASSES))
def test_edge_lists(cls):
    wb, p, g = R.CLASSES[cls]
    E = R.edges(cls)
    assert len(set(E)) == 13 and {0, 1, 2, p - 1, p - 2} <= set(E) and {(p - v) % p for v in E} == set(E)
    if wb == 8:
        assert {2**32 - 1, 2**32, (2**63 - 1) % p, 2**63 % p, p - 2**32} <= set(E)
    else:
        assert {2**30 % p, (2**31 - 1) % p, 2**31 % p, (p - 1) // 2, (p + 1) // 2} <= set(E)
    assert pow(g, (p - 1) // 2, p) == p - 1  # a kind-2 table needs a generator's 2N-th root


def test_batch_rule():
    assert [R.batch_for(l) for l in (6, 7, 8, 13)] == [7, 3, 3, 3]


@pytest.mark.parametrize("cls", sorted(R.CLASSES))
@pytest.mark.parametrize("larger", [False, True])
def test_builder_invariants(oracle, cls, larger):
    wb, p, g = R.CLASSES[cls]
    logn = (7 if wb == 8 else 6) + (0 if not larger else 1 if cls == "kyber" else 3)
    n, batch = 1 << logn, R.batch_for(logn)
    E = R.edges(cls)
    pairs = {(x, y) for x in E for y in E}
    for bcast in (False, True):
        c = R.case(cls, logn, batch, broadcast=bcast)
        T, ea, eb, a, b = c["T"], c["ea"], c["eb"], c["a"], c["b"]
        assert a.shape == ea.shape == (batch, n) and eb.shape == ((1, n) if bcast else (batch, n)) and c["bhat"] is c["eb"]
        assert int(a.max()) < p and int(b.max()) < p
        # the transform-domain control: the unscaled inverse of the operand is the target, word for word
        assert np.array_equal(_ints(oracle.intt(a, T, p)) * n % p, _ints(ea))
        ebr = np.repeat(eb, batch, axis=0) if bcast else eb
        assert b.shape == (batch, n) and np.array_equal(_ints(oracle.intt(b, T, p)) * n % p, _ints(ebr))
        assert set(zip(ea.ravel().tolist(), ebr.ravel().tolist())) == pairs
        for k in range(3):  # every term of the sum is a full grid of its own
            bk = c["bhat_dot"][k]
            inv_k = _ints(oracle.intt(c["a_dot"][k], T, p)) * n % p
            assert set(zip(inv_k.ravel().tolist(), (np.repeat(bk, batch, axis=0) if bcast else bk).ravel().tolist())) == pairs
        if logn <= 7:  # the expectation against the operation's definition, not the network
            ninv = pow(n, -1, p)
            bs = np.stack([oracle.ntt((_ints(np.repeat(x, batch, axis=0) if bcast else x) * ninv % p).astype(a.dtype), T, p) for x in c["bhat_dot"]])
            for r in (0, batch - 1):
                assert np.array_equal(c["want_mul"][r], oracle.negacyclic_schoolbook(a[r], b[r], p).astype(a.dtype))
                assert np.array_equal(c["want_dot"][r], product_dot_ref.schoolbook(oracle, c["a_dot"], bs, p, r))
        if not bcast:  # the transform is linear: the additive expectations are a + b and a - b
            assert np.array_equal(_ints(c["want_plus"]), (_ints(a) + _ints(b)) % p)
            assert np.array_equal(_ints(c["want_minus"]), (_ints(a) - _ints(b)) % p)
            assert int(c["ones"].min()) == int(c["ones"].max()) == 1 and int(c["minus_ones"].min()) == int(c["minus_ones"].max()) == p - 1


@pytest.mark.parametrize("cls,logn", LONG)
def test_long_sum_expectation_is_the_sum_of_its_terms(oracle, cls, logn):
    p = R.CLASSES[cls][1]
    c = R.long_sum(cls, logn, TE.LONG_BATCH, TE.LONG_TERMS)
    assert c["a"].shape == (17, 3, 1 << logn) and p > 2**(8 * R.CLASSES[cls][0] - 1)  # a canonical sum can wrap the word
    assert np.array_equal(_ints(c["want"]), _ints(c["a"]).sum(axis=0) % p)
    sums = (_ints(oracle.intt(c["a"].reshape(-1, 1 << logn), c["T"], p)) * (1 << logn) % p).reshape(c["a"].shape)
    assert set(sums.ravel().tolist()) == set(R.edges(cls))


# ---- the host models on the GPU file's cases -------------------------------------------------------------------------------------
def _fused(c, alias):
    wb = c["a"].dtype.itemsize
    logn = c["a"].shape[1].bit_length() - 1
    sa, sb = c["a"].copy(), c["b"].copy()
    out = sa if alias else np.full_like(sa, 0xFFFFFFFF)
    assert emu_lib.lib().emu_polymul_fused(wb, logn, c["p"], c["T"].ctypes.data, sa.ctypes.data, sb.ctypes.data, out.ctypes.data, sa.shape[0], 8) == 0
    assert np.array_equal(out, c["want_mul"]), ("two operands", alias)


def _pre(c):
    wb = c["a"].dtype.itemsize
    batch, n = c["a"].shape
    sa, bh = c["a"].copy(), c["bhat"].copy()
    rc = emu_product_pre_lib.lib().emu_polymul_pre(wb, n.bit_length() - 1, c["p"], c["T"].ctypes.data, sa.ctypes.data, bh.ctypes.data, bh.shape[0], sa.ctypes.data,
                                                   batch, 8, -1)
    assert rc == 0 and np.array_equal(sa, c["want_mul"]), ("prepared", bh.shape)
    assert np.array_equal(bh, c["bhat"]), "b^ was written"


def _dot(p, T, a, bhat, want, what):
    terms, batch, n = a.shape
    sa, bh, out = a.copy(), np.ascontiguousarray(bhat).copy(), np.full_like(a[0], 0xFFFFFFFF)
    rc = emu_product_dot_lib.lib().emu_polymul_dot(a.dtype.itemsize, n.bit_length() - 1, p, T.ctypes.data, sa.ctypes.data, bh.ctypes.data, bh.shape[1], terms,
                                                   out.ctypes.data, batch, 8, -1)
    assert rc == 0 and np.array_equal(out, want), ("summed", what)
    assert np.array_equal(bh, bhat), "b^ was written"


@pytest.mark.parametrize("cls,logn", UNITS)
def test_host_models_on_the_edge_grids(oracle, cls, logn):
    """what test_every_product_kernel_on_the_edge_grids runs on the GPU, case for case, in the host index models"""
    batch = R.batch_for(logn)
    rows, bc = R.case(cls, logn, batch), R.case(cls, logn, batch, broadcast=True)
    p, T = rows["p"], rows["T"]
    _fused(rows, alias=False)
    _fused(rows, alias=True)
    _pre(rows)
    _pre(bc)
    prep = np.zeros_like(rows["b"])  # ntt_polymul_prepare is the unscaled inverse
    assert emu_lib.lib().emu_transform(rows["b"].dtype.itemsize, logn, p, T.ctypes.data, rows["b"].ctypes.data, prep.ctypes.data, batch, 1, 0, 0, 8, 0) == 0
    assert np.array_equal(prep, rows["eb"])
    _dot(p, T, rows["a_dot"], rows["bhat_dot"], rows["want_dot"], "three terms per row")
    _dot(p, T, bc["a_dot"], bc["bhat_dot"], bc["want_dot"], "three terms broadcast")
    two = np.stack([rows["a"], rows["b"]])
    _dot(p, T, two, np.stack([rows["ones"], rows["ones"]]), rows["want_plus"], "ea + eb")
    _dot(p, T, two, np.stack([rows["ones"], rows["minus_ones"]]), rows["want_minus"], "ea + (p - 1) eb")


@pytest.mark.parametrize("cls,logn", BEHIND)
def test_host_models_behind_column_passes(oracle, cls, logn):
    c = R.case(cls, logn, 3)
    _fused(c, alias=False)
    _pre(c)
    _dot(c["p"], c["T"], c["a_dot"], c["bhat_dot"], c["want_dot"], "three terms per row")


@pytest.mark.parametrize("cls,logn", LONG)
def test_host_model_on_the_long_sum(oracle, cls, logn):
    c = R.long_sum(cls, logn, TE.LONG_BATCH, TE.LONG_TERMS)
    _dot(c["p"], c["T"], c["a"], c["ones"], c["want"], "17 terms")


# ---- the matrix cannot drift -----------------------------------------------------------------------------------------------------
def field_key(wb, p):
    """what selects the kernel family besides the unit: the field kind, and for 4-byte words the instruction stream chosen per launch from
    the modulus (below 2^30, in [2^30, 2^31), from 2^31 on)"""
    if wb == 8:
        return "gl" if p == GOLD else "m64"
    return "m32/stream%d" % (0 if p < 2**30 else 1 if p < 2**31 else 2)


def field_of(cls):
    return field_key(*R.CLASSES[cls][:2])


def _product_units(n, buf, width):
    return [buf[width * i + 3] for i in range(n) if buf[width * i] == PRODUCT]


def kernels_at(wb, p, logn, batch, terms=3, alt=-1):
    """{(family, field, unit)} a call of each entry point launches at this shape, from the library's own launch lists (nothing runs):
    families two / pre / dot, and dot_fallback for a size whose prepared product is fused while the summed one takes the unfused
    sequence with its row sum"""
    key, out = field_key(wb, p), set()
    buf = (C.c_int * (20 * 16))()
    n = emu_lib.lib().emu_sequence(8, wb, logn, p, batch, alt, 0, 0, 0, buf, 16)  # -1: ntt_polymul_negacyclic is not fused here
    out |= {("two", key, u) for u in _product_units(max(n, 0), buf, 16)}
    n = emu_product_pre_lib.lib().emu_polymul_pre_sequence(wb, logn, p, batch, batch, alt, TARGET_WGS, buf, 16)
    assert n > 0
    pre_units = _product_units(n, buf, 16)
    out |= {("pre", key, u) for u in pre_units}
    n = emu_product_dot_lib.lib().emu_polymul_dot_sequence(wb, logn, p, batch, batch, terms, alt, TARGET_WGS, buf, 16)
    assert n > 0
    out |= {("dot", key, u) for u in _product_units(n, buf, 20)}
    if any(buf[20 * i] == ROW_SUM for i in range(n)):
        out |= {("dot_fallback", key, u) for u in pre_units}
    return out


def kernels_of(cls, logn, batch):
    return kernels_at(*R.CLASSES[cls][:2], logn, batch)


def launchable():
    """every (family, field, unit) the library can launch: the host model's own answer to `is this size fused` over logn 5 .. 14, per class"""
    full = set()
    for cls, (wb, p, _) in R.CLASSES.items():
        for logn in range(5, 15):
            pre = emu_product_pre_lib.lib().emu_polymul_pre_fused(wb, logn, p, 3, TARGET_WGS, -1)
            dot = emu_product_dot_lib.lib().emu_polymul_dot_fused(wb, logn, p, 3, TARGET_WGS, -1)
            assert pre in (0, 1) and dot in (0, 1) and dot <= pre
            got = kernels_of(cls, logn, 3)
            fams = {f for f, _, _ in got}
            assert fams == ({"two", "pre", "dot"} if dot else {"two", "pre", "dot_fallback"} if pre else set()), (cls, logn, got)
            full |= got
    return full


def test_every_launchable_product_kernel_has_a_gpu_case():
    full = launchable()
    covered = set()
    for cls, logn in UNITS:
        got = kernels_of(cls, logn, R.batch_for(logn))
        assert {u for _, _, u in got} == {logn}, "a case of the unit list does not run the unit it names"
        covered |= got
    assert covered == full, (sorted(full - covered), sorted(covered - full))
    fields = {field_of(c) for c in R.CLASSES}
    assert fields == {"gl", "m64", "m32/stream0", "m32/stream1", "m32/stream2"} == {f for _, f, _ in full}
    # the two units without a summed kernel are cases too: they run the unfused sequence on the GPU, their prepared and two-operand kernels the fused one
    fallback = {(f, u) for fam, f, u in full if fam == "dot_fallback"}
    assert fallback == {("m64", 10)} | {("m32/stream%d" % s, 13) for s in range(3)}
    for f, u in fallback:
        assert ("dot", f, u) not in full and {("pre", f, u), ("two", f, u)} <= covered
    # the two-operand product shares the prepared one's unit set
    assert {(f, u) for fam, f, u in full if fam == "two"} == {(f, u) for fam, f, u in full if fam == "pre"}
    assert {c for c, _ in UNITS} == set(R.CLASSES)


def test_every_field_and_stream_has_its_unit_behind_column_passes():
    assert {c for c, _ in BEHIND} == set(R.CLASSES) - {"kyber"}
    seen = set()
    for cls, logn in BEHIND:
        got = kernels_of(cls, logn, 3)
        assert {fam for fam, _, _ in got} == {"two", "pre", "dot"} and len({u for _, _, u in got}) == 1 and all(u < logn for _, _, u in got), (cls, logn, got)
        seen |= {f for _, f, _ in got}
    assert seen == {field_of(c) for c in R.CLASSES}
