"""The three 4-byte classes that take the coset and column kernels through instruction streams 1 and 2 (STREAM_CLASSES of
tests/test_gpu_columns.py), without a GPU: the expected words the GPU files compare with -- _case, _lde_case, _cinv_case, through the
oracle -- against a Python-integer network written from include/ntt_hip.h, and the coverage claim itself: the 4-byte moduli of the class
tables reach all three streams, and every GPU test that is parametrised over the tables has every class among its parameters."""
import numpy as np
import pytest

import test_gpu_columns as TC
import test_gpu_columns_large as TG
import test_gpu_coset_inverse as TI
import test_gpu_lde as TR
import test_gpu_lde_columns as TL
from test_gpu_columns import ALL_CLASSES, CLASSES, STREAM_CLASSES

LOGN, WIDTH, COUNT, BETA = 5, 3, 2, 2


def _bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2) if bits else 0


def _network(a, T, p):
    """include/ntt_hip.h: stage s = 0.., stride 2^s, (x, y) -> (x + y, (x - y) * T[n / 2^(s+1) + block])"""
    a, n = list(a), len(a)
    t = 1
    while t < n:
        h = n // (2 * t)
        for i in range(h):
            for j in range(2 * i * t, 2 * i * t + t):
                x, y = a[j], a[j + t]
                a[j], a[j + t] = (x + y) % p, (x - y) * T[h + i] % p
        t *= 2
    return a


def _inverse_network(a, T, p):
    """stages logn-1 .. 0, (u, v) -> (u + v / T, u - v / T), unscaled"""
    a, n = list(a), len(a)
    t = n // 2
    while t >= 1:
        h = n // (2 * t)
        for i in range(h):
            ti = pow(T[h + i], -1, p)
            for j in range(2 * i * t, 2 * i * t + t):
                u, v = a[j], a[j + t] * ti % p
                a[j], a[j + t] = (u + v) % p, (u - v) % p
        t //= 2
    return a


def _columns(x):
    """[count][rows][width] -> {(m, c): column as Python integers}"""
    return {(m, c): [int(v) for v in x[m, :, c]] for m in range(x.shape[0]) for c in range(x.shape[2])}


def _same(want_by_column, got):
    for (m, c), col in want_by_column.items():
        assert [int(v) for v in got[m, :, c]] == col, (m, c)


@pytest.mark.parametrize("cls", sorted(STREAM_CLASSES))
def test_expected_words_are_the_headers_network_in_python_integers(oracle, cls):
    """logn 5, width 3, count 2, blow-up 2, shift g: forward, scaled and unscaled inverse, the LDE and the coset inverse"""
    wb, p, g = STREAM_CLASSES[cls]
    n = 1 << LOGN
    assert wb == 4 and (p - 1) % n == 0 and pow(g, (p - 1) // 2, p) == p - 1
    T = [int(t) for t in TC._table_cached(LOGN, cls)]
    assert T == [int(t) for t in TL._table_cached(LOGN, cls)] and len(T) == n
    n_inv = pow(n, -1, p)
    ref = TC._case(cls, LOGN, WIDTH, COUNT)
    assert ref["x"].shape == (COUNT, n, WIDTH) and ref["x"].dtype == np.uint32 and int(ref["x"].max()) == p - 1
    cols = _columns(ref["x"])
    unscaled = {k: _inverse_network(a, T, p) for k, a in cols.items()}
    _same({k: _network(a, T, p) for k, a in cols.items()}, ref["fwd"])
    _same(unscaled, ref["invu"])
    _same({k: [v * n_inv % p for v in a] for k, a in unscaled.items()}, ref["inv"])
    # ntt_lde_columns: Forward_M(x), x[i << beta] = in[i] * shift^bitrev_logN(i), every other word zero
    x, want = TL._lde_case(cls, LOGN, BETA, WIDTH, COUNT, g)
    small = n >> BETA
    assert x.shape == (COUNT, small, WIDTH) and want.shape == (COUNT, n, WIDTH)
    expanded = {}
    for k, a in _columns(x).items():
        e = [0] * n
        for i in range(small):
            e[i << BETA] = a[i] * pow(g, _bitrev(i, LOGN - BETA), p) % p
        expanded[k] = _network(e, T, p)
    _same(expanded, want)
    # ntt_coset_inverse_columns: InvScaled_M(in)[r] * shift^(-bitrev_logM(r))
    x, want = TL._cinv_case(cls, LOGN, WIDTH, COUNT, g)
    assert x.shape == (COUNT, n, WIDTH)
    _same({k: [v * n_inv * pow(g, -_bitrev(r, LOGN), p) % p for r, v in enumerate(_inverse_network(a, T, p))]
           for k, a in _columns(x).items()}, want)
    # the row files' comparators at the same size: one column as one row
    a = np.ascontiguousarray(x[0].T[:2])
    Tn = TR._table(oracle, LOGN, wb, p, g)
    assert [int(t) for t in Tn] == T
    want_rows = [[v * n_inv * pow(g, -_bitrev(r, LOGN), p) % p for r, v in enumerate(_inverse_network([int(v) for v in row], T, p))] for row in a]
    assert TI._expected(oracle, a, Tn, p, g).tolist() == want_rows
    c = np.ascontiguousarray(a[:, :small])
    want_rows = []
    for row in c:
        e = [0] * n
        for i in range(small):
            e[i << BETA] = int(row[i]) * pow(g, _bitrev(i, LOGN - BETA), p) % p
        want_rows.append(_network(e, T, p))
    assert TR._expected(oracle, c, Tn, p, BETA, g).tolist() == want_rows


def test_the_class_tables_reach_all_three_streams():
    """pass_kernel.inc picks the stream from the modulus: below 2^30, in [2^30, 2^31), from 2^31 on"""
    assert sorted(CLASSES) == ["gl", "kyber", "m32", "m64"] and not set(CLASSES) & set(STREAM_CLASSES)
    assert ALL_CLASSES == {**CLASSES, **STREAM_CLASSES}
    four = [p for wb, p, g in ALL_CLASSES.values() if wb == 4]
    for lo, hi in ((3, 1 << 30), (1 << 30, 1 << 31), (1 << 31, 1 << 32)):
        assert any(lo <= p < hi for p in four), (lo, hi)
    # the GPU files share the one definition
    for mod in (TR, TI, TL, TG):
        assert mod.CLASSES is CLASSES and mod.STREAM_CLASSES is STREAM_CLASSES and mod.ALL_CLASSES is ALL_CLASSES


def _classes_of(fn):
    """the values of the `cls` argument over every pytest.mark.parametrize of the test function, read from its marks"""
    found = set()
    for mark in getattr(fn, "pytestmark", []):
        if mark.name != "parametrize":
            continue
        names = [s.strip() for s in mark.args[0].split(",")] if isinstance(mark.args[0], str) else list(mark.args[0])
        if "cls" not in names:
            continue
        k = names.index("cls")
        for item in mark.args[1]:
            values = item.values if hasattr(item, "values") else item if len(names) > 1 else (item,)  # pytest.param(...) or plain
            found.add(values[k])
    return found


UNION_TESTS = [TR.test_lde_sweep, TI.test_coset_inverse_sweep, TC.test_columns_against_the_oracle_with_guard_words,
               TL.test_lde_columns_against_the_oracle_with_guard_words, TL.test_coset_inverse_columns_against_the_oracle_with_guard_words,
               TG.test_three_passes_against_the_oracle, TG.test_three_pass_lde_columns_against_the_oracle,
               TG.test_three_pass_coset_inverse_columns_against_the_oracle, TG.test_columns_of_edge_residues]


@pytest.mark.parametrize("fn", UNION_TESTS, ids=lambda f: f.__name__)
def test_union_parametrised_gpu_tests_name_every_class(fn):
    assert _classes_of(fn) == set(ALL_CLASSES), fn.__name__


def test_named_cases_of_the_other_streams():
    """the tests that name their classes: the cases the other two streams were given"""
    def params(fn):
        out = set()
        for mark in fn.pytestmark:
            if mark.name == "parametrize":
                out |= {tuple(getattr(i, "values", i if isinstance(i, tuple) else (i,))) for i in mark.args[1]}
        return out

    assert {("bb31", 12), ("kb31", 14), ("top32", 5), ("top32", 10)} <= params(TR.test_lde_stays_inside_the_callers_buffers)
    assert {(12, "bb31"), (13, "bb31"), (12, "top32"), (13, "top32")} <= params(TI.test_coset_inverse_stays_inside_the_callers_buffers)
    assert {("bb31", 8, 4), ("top32", 9, 2)} <= params(TI.test_round_trip_with_lde)
    assert {(3221225473, 5), (2013265921, 31)} == params(TR.test_lde_three_pass_plan) == params(TI.test_coset_inverse_three_pass_plan)
    assert ("bb31",) in params(TC.test_wrapper_round_trip_on_a_strided_view)
    assert {("bb31",), ("top32",)} <= params(TL.test_round_trip_and_sampled_evaluations)
    # the three-pass column tests give the new classes the logn-17 shapes, all of them, and nothing larger
    for fn, shapes in ((TG.test_three_passes_against_the_oracle, TG.THREE_PASS_SHAPES), (TG.test_three_pass_lde_columns_against_the_oracle, TG.THREE_PASS_LDE_SHAPES),
                       (TG.test_three_pass_coset_inverse_columns_against_the_oracle, TG.THREE_PASS_SHAPES)):
        got = params(fn)
        for cls in STREAM_CLASSES:
            assert {s for c, s in got if c == cls} == {s for s in shapes if s[0] == 17}, (fn.__name__, cls)
        for cls in CLASSES:
            assert {s for c, s in got if c == cls} == set(shapes), (fn.__name__, cls)
