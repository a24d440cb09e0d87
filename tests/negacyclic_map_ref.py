"""What the tests of ntt_negacyclic_map / ntt_gadget_decompose_map / ntt_polymul_gadget_map_pre share: the two maps in plain Python
integers FROM THE RING DEFINITION -- multiply by X^e by shifting with wrap-around negation, scatter a[i] to i * g mod 2N with its sign --
and not from the library's gather rule (t -> src, neg), then minus_identity, then gadget_ref.decompose / gadget_ref.want on the mapped
words and product_dot_ref.addmod for the addend."""
import numpy as np

import gadget_ref as G
import product_dot_ref as R

MONOMIAL, AUTOMORPHISM = 0, 1


def ginv(g: int, logn: int) -> int:
    """g^-1 mod 2N by the library's rule: Newton's iteration mod 2^32, masked (csrc/negacyclic_map.h: map_ginv)"""
    x = g
    for _ in range(4):
        x = (x * (2 - g * x)) & 0xFFFFFFFF
    return x & ((2 << logn) - 1)


def monomial_row(row, e: int, p: int):
    """X^e * row mod (X^N + 1, p), a list of Python integers: e is taken mod 2N; one shift by e mod N with the wrapped coefficients
    negated, and the whole row negated once more when e mod 2N >= N (X^N = -1)"""
    n = len(row)
    e %= 2 * n
    s, flip = e % n, e >= n
    y = [0] * n
    for i, x in enumerate(row):
        x = int(x)
        d = i + s
        if d >= n:  # wrapped past X^N
            d, x = d - n, -x
        y[d] = (-x if flip else x) % p
    return y


def automorphism_row(row, g: int, p: int):
    """row(X^g) mod (X^N + 1, p): coefficient i goes to exponent i * g mod 2N; an exponent N + d is -X^d"""
    n = len(row)
    y = [0] * n
    for i, x in enumerate(row):
        d = (i * g) % (2 * n)
        y[d % n] = (-int(x) if d >= n else int(x)) % p
    return y


def mapped_int(a: np.ndarray, p: int, kind: int, param: int = 0, exps=None, minus_identity: bool = False) -> np.ndarray:
    """a [polys, batch, N] -> what ntt_negacyclic_map writes, word by word in Python integers; exps: one exponent per row, shared by the
    polynomials"""
    out = np.empty_like(a)
    for q in range(a.shape[0]):
        for r in range(a.shape[1]):
            row = [int(x) for x in a[q, r]]
            y = monomial_row(row, int(exps[r]) if exps is not None else param, p) if kind == MONOMIAL else automorphism_row(row, param, p)
            if minus_identity:
                y = [(u - v) % p for u, v in zip(y, row)]
            out[q, r] = np.array(y, dtype=object).astype(a.dtype)
    return out


def mapped(a: np.ndarray, p: int, kind: int, param: int = 0, exps=None, minus_identity: bool = False) -> np.ndarray:
    """the same words for the large shapes: the same scatter -- coefficient i of a row to exponent i + e, or i * g, mod 2N, negated when the
    exponent is N or more -- as one numpy assignment per polynomial (the CPU test holds it against mapped_int).  p - x and the wrapping
    difference below are exact in the word's own unsigned type: the true values lie in [0, p)"""
    polys, batch, n = a.shape
    i = np.arange(n, dtype=np.int64)[None, :]
    if kind == MONOMIAL:
        e = (np.asarray(exps, dtype=np.int64) if exps is not None else np.full(batch, int(param), dtype=np.int64)) % (2 * n)
        d = (i + e[:, None]) % (2 * n)
    else:
        d = np.broadcast_to((i * int(param)) % (2 * n), (batch, n))
    rows = np.arange(batch)[:, None]
    pw = a.dtype.type(p)
    out = np.empty_like(a)
    for q in range(polys):
        x = a[q]
        out[q][rows, d % n] = np.where((d >= n) & (x != 0), pw - x, x)
    if minus_identity:
        diff = out - a  # wraps where out < a
        out = np.where(out < a, diff + pw, diff)
    return out


def decompose(a, p, kind, param, exps, minus_identity, w, K, l) -> np.ndarray:
    """what ntt_gadget_decompose_map writes: [polys, K, batch, N]"""
    return G.decompose(mapped(a, p, kind, param, exps, minus_identity), p, w, K, l)


def want(oracle, a, b, T, p, kind, param, exps, minus_identity, w, K, l, broadcast=False, addend=None):
    """block j of ntt_polymul_gadget_map_pre for ONE output: gadget_ref.want of the mapped words, plus the addend"""
    c = G.want(oracle, mapped(a, p, kind, param, exps, minus_identity), b, T, p, w, K, l, broadcast)
    return c if addend is None else R.addmod(c, addend, p)


def edge_rows(a: np.ndarray, p: int) -> None:
    """in place: rows 0 .. 4 (as far as the batch goes) of every polynomial get one of the words 0, 1, (p - 1) / 2, (p + 1) / 2 and p - 1 at
    indices 0 and N - 1 -- the wrap and the negation edges"""
    words = [0, 1 % p, (p - 1) // 2, (p + 1) // 2, p - 1]
    for r in range(a.shape[1]):
        a[:, r, 0] = words[r % 5]
        a[:, r, -1] = words[(r + 2) % 5]
    # ... and with a single row, all five still occur in it where it is long enough
    if a.shape[2] >= 8:
        a[:, 0, 1:6] = np.array(words, dtype=object).astype(a.dtype)
