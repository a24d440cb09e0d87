"""What the tests of ntt_polymul_dot_pre share: operands with the edge words in row 0 of every term, the prepared operand, and the
reference -- the sum mod p over the terms of the oracle's existing pipeline Fwd(Inv(a_k) . Inv(b_k) . N), added with carry-aware numpy."""
import numpy as np


def addmod(x: np.ndarray, y: np.ndarray, p: int) -> np.ndarray:
    """(x + y) mod p for canonical words of either width; the sum may wrap the word (p > half the word range)"""
    s = x + y
    return np.where((s < x) | (s >= x.dtype.type(p)), s - x.dtype.type(p), s)


def operands(oracle, wb, p, g, logn, batch, terms, seed=None, all_max=False):
    """a [terms, batch, N], b [terms, batch, N] (row 0 of every term all p - 1 in both: every carry path), the kind-2 table and
    b^ = InvU(b) of every row"""
    dt = np.uint32 if wb == 4 else np.uint64
    n = 1 << logn
    T = oracle.make_table(2, n, p, g, wb)
    rng = np.random.default_rng(logn if seed is None else seed)
    a = (rng.integers(0, 2**63, size=(terms, batch, n), dtype=np.uint64) % np.uint64(p)).astype(dt)
    b = (rng.integers(0, 2**63, size=(terms, batch, n), dtype=np.uint64) % np.uint64(p)).astype(dt)
    if all_max:
        a[:] = p - 1
        b[:] = p - 1
    a[:, 0, :] = p - 1
    b[:, 0, :] = p - 1
    B = oracle.intt(b.reshape(terms * batch, n), T, p, nthreads=4)
    bhat = oracle.pointwise(B, np.ones_like(B), p, n % p).reshape(terms, batch, n)  # the UNSCALED inverse
    return a, b, T, bhat


def want(oracle, a, b, T, p, broadcast=False):
    """sum_k Fwd(Inv(a_k) . Inv(b_k) . N) mod p; broadcast: row 0 of b_k multiplies every row of a_k"""
    terms, batch, n = a.shape
    acc = None
    for k in range(terms):
        bk = np.repeat(b[k, :1], batch, axis=0) if broadcast else b[k]
        A, B = oracle.intt(np.ascontiguousarray(a[k]), T, p, nthreads=4), oracle.intt(np.ascontiguousarray(bk), T, p, nthreads=4)
        c = oracle.ntt(oracle.pointwise(A, B, p, n % p), T, p, nthreads=4)
        acc = c if acc is None else addmod(acc, c, p)
    return acc


def schoolbook(oracle, a, b, p, row, broadcast=False):
    """sum_k negacyclic_schoolbook(a_k[row], b_k[row | 0]) mod p: one row of the result, in the dtype of a"""
    acc = None
    for k in range(a.shape[0]):
        c = oracle.negacyclic_schoolbook(a[k, row], b[k, 0 if broadcast else row], p)
        acc = c if acc is None else addmod(acc, c, p)
    return acc.astype(a.dtype)
