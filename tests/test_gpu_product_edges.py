"""Every product kernel on a real MI355X at transform-domain edge residues (tests/product_edge_ref.py): ntt_polymul_negacyclic,
ntt_polymul_prepare, ntt_polymul_negacyclic_pre and ntt_polymul_dot_pre through NTTPlan, with operands built so that the words leaving
the inverse rounds of the fused middle pass are 0, 1, 2, p - 1, p - 2, the word-boundary residues of the class and their negatives --
every ordered pair of them meeting in the middle's product, in the accumulator's add and under the N^-1 scaling.  Bit-exact: all
arithmetic is integer and every word canonical.

The parameter lists name every unit size that has a kernel, in every field and every 4-byte instruction stream, as a single-pass size
equal to the unit, so each case runs the kernel it is named for (asserted through ntt_plan_info).  tests/test_product_edges_cpu.py
reads these lists: it runs the same expectations through the host index model first, and it fails when a kernel the library can
launch has no case here."""
import os

import numpy as np
import pytest

import product_edge_ref as R

pytestmark = pytest.mark.gpu

# (class, logn): single-pass sizes equal to the unit.  8-byte words have units 2^7 .. 2^12, 4-byte words 2^6 .. 2^13 in each of the three
# streams (m32 / kyber 0, bb31 / kb31 1, top32 / c32 2); kyber's kind-2 table stops at 2^7; the 62-bit prime and 3221225473 run the same
# kernels as m64 and top32 and get two units each
UNITS = ([(c, l) for c in ("gl", "m64") for l in range(7, 13)] + [(c, l) for c in ("m32", "bb31", "kb31", "top32") for l in range(6, 14)] +
         [("kyber", 6), ("kyber", 7), ("m62", 8), ("m62", 11), ("c32", 8), ("c32", 13)])
# one two-pass size per class (kyber has none): the unit as the first pass of a larger transform
BEHIND_COLUMNS = [(c, 13 if R.CLASSES[c][0] == 8 else 14) for c in sorted(R.CLASSES) if c != "kyber"]
# the two classes whose canonical sums wrap the word
LONG_SUMS = [("m64", 8), ("top32", 10)]
LONG_BATCH, LONG_TERMS = 3, 17


@pytest.fixture(scope="module")
def eng():
    import torch

    import ntt_aie_amd as E

    assert torch.cuda.is_available()
    assert os.path.exists(E.LIB_PATH), "native library missing: the GPU tests must not pass without it"
    torch.cuda.set_device(0)
    return E


def _plan(eng, oracle, cls, logn):
    """the plan with the kind-2 table generated on the device, and [stages of every pass of the default decomposition]"""
    from ntt_aie_amd import _lib

    wb, p, g = R.CLASSES[cls]
    pl = eng.NTTPlan(logn, p, wb, 0)
    pl.generate_twiddles(2, g)
    assert np.array_equal(pl.get_twiddles(), oracle.make_table(2, 1 << logn, p, g, wb))
    L = _lib.lib()
    return pl, [int(L.ntt_plan_info(pl._h, 32 + i)) for i in range(int(L.ntt_plan_info(pl._h, 3)))]


def _dev(eng, x):
    return eng.to_device(np.ascontiguousarray(x), "cuda:0")


def _two_operand(eng, pl, c, alias):
    d_a, d_b = _dev(eng, c["a"]), _dev(eng, c["b"])
    if alias:
        got = pl.polymul_negacyclic(d_a, d_b)
        assert got is d_a
    else:
        out = _dev(eng, np.zeros_like(c["a"]))
        got = pl.polymul_negacyclic(d_a, d_b, out)
        assert got is out
    assert np.array_equal(eng.to_host(got), c["want_mul"]), "two operands, %s" % ("result aliasing a" if alias else "out of place")


def _prepared(eng, pl, c, what):
    d_bh = _dev(eng, c["bhat"])
    got = pl.polymul_negacyclic_pre(_dev(eng, c["a"]), d_bh)
    assert np.array_equal(eng.to_host(got), c["want_mul"]), "prepared, " + what
    assert np.array_equal(eng.to_host(d_bh), c["bhat"]), "b^ was written"


def _summed(eng, pl, a, bhat, want, what):
    d_bh = _dev(eng, bhat)
    out = _dev(eng, np.zeros_like(a[0]))
    got = pl.polymul_dot_pre(_dev(eng, a), d_bh, out)
    assert got is out
    assert np.array_equal(eng.to_host(out), want), "summed, " + what
    assert np.array_equal(eng.to_host(d_bh), bhat), "b^ was written"


@pytest.mark.parametrize("cls,logn", UNITS)
def test_every_product_kernel_on_the_edge_grids(eng, oracle, cls, logn):
    batch = R.batch_for(logn)
    pl, stages = _plan(eng, oracle, cls, logn)
    assert stages == [logn], "not one pass of logn stages: the case would not run the kernel it is named for"
    rows, bc = R.case(cls, logn, batch), R.case(cls, logn, batch, broadcast=True)
    _two_operand(eng, pl, rows, alias=False)
    _two_operand(eng, pl, rows, alias=True)
    _prepared(eng, pl, rows, "per row")
    _prepared(eng, pl, bc, "broadcast")
    # the transform-domain targets, out of the library's own unscaled inverse
    d_b = _dev(eng, rows["b"])
    assert np.array_equal(eng.to_host(pl.polymul_prepare(d_b)), rows["eb"])
    assert np.array_equal(eng.to_host(d_b), rows["b"])
    _summed(eng, pl, rows["a_dot"], rows["bhat_dot"], rows["want_dot"], "three terms per row")
    _summed(eng, pl, bc["a_dot"], bc["bhat_dot"], bc["want_dot"], "three terms broadcast")
    two = np.stack([rows["a"], rows["b"]])
    _summed(eng, pl, two, np.stack([rows["ones"], rows["ones"]]), rows["want_plus"], "ea + eb")
    _summed(eng, pl, two, np.stack([rows["ones"], rows["minus_ones"]]), rows["want_minus"], "ea + (p - 1) eb")


@pytest.mark.parametrize("cls,logn", BEHIND_COLUMNS)
def test_unit_behind_column_passes(eng, oracle, cls, logn):
    """the middle as the first pass of a two-pass transform, in every field and stream: the multiplicative grid through all three
    entry points, the summed one with three terms"""
    pl, stages = _plan(eng, oracle, cls, logn)
    assert len(stages) == 2 and sum(stages) == logn
    c = R.case(cls, logn, 3)
    _two_operand(eng, pl, c, alias=False)
    _prepared(eng, pl, c, "per row")
    _summed(eng, pl, c["a_dot"], c["bhat_dot"], c["want_dot"], "three terms per row")


@pytest.mark.parametrize("cls,logn", LONG_SUMS)
def test_a_long_sum_at_the_word_boundary(eng, oracle, cls, logn):
    """17 terms of the additive grid where a canonical sum can wrap the word: the accumulator's reduction at every step"""
    pl, stages = _plan(eng, oracle, cls, logn)
    assert stages == [logn]
    c = R.long_sum(cls, logn, LONG_BATCH, LONG_TERMS)
    _summed(eng, pl, c["a"], c["ones"], c["want"], "17 terms")
