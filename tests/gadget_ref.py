"""What the tests of ntt_gadget_decompose / ntt_polymul_gadget_pre share: the balanced gadget decomposition of include/ntt_hip.h in plain
Python integers (parts_int: object arrays, nothing can wrap), the same steps in exact uint64 numpy for the large shapes (digits; the
CPU test holds the two against each other), the argument rule, the edge words of row 0, and the reference of the product:
product_dot_ref.want applied to the reference digits."""
import numpy as np

import product_dot_ref as R


def params_ok(p: int, w: int, K: int, l: int) -> bool:
    """the argument rule of the header: anything else is NTT_E_ARG"""
    if not (1 <= w <= 31 and K >= 1 and l >= 0 and l + (K - 1) * w <= 63):
        return False
    h = (1 << (l - 1)) if l > 0 else 0
    u_max = (((p - 1) // 2) + h) >> l
    return (1 << (w - 1)) < p and (u_max >> ((K - 1) * w)) + 1 < p


def parts_int(a, p: int, w: int, K: int, l: int):
    """s, m, u and the K signed digits e_k of every word of `a`, all object arrays of Python integers"""
    a = np.asarray(a).astype(object)
    neg = a > (p - 1) // 2
    s = np.where(neg, -1, 1).astype(object)
    m = np.where(neg, p - a, a).astype(object)
    h = (1 << (l - 1)) if l > 0 else 0
    u = (m + h) >> l
    B = 1 << w
    v = u + sum(1 << (k * w + w - 1) for k in range(K - 1))
    e = [((v >> (k * w)) & (B - 1)) - B // 2 for k in range(K - 1)] + [v >> ((K - 1) * w)]
    return s, m, u, e


def digits_int(a, p: int, w: int, K: int, l: int) -> np.ndarray:
    """[K, *a.shape] canonical words, from the integers"""
    s, _, _, e = parts_int(a, p, w, K, l)
    return np.stack([((s * ek) % p).astype(np.asarray(a).dtype) for ek in e])


def digits(a: np.ndarray, p: int, w: int, K: int, l: int) -> np.ndarray:
    """the same words in uint64 steps, none of which wraps under params_ok (v < 2^64)"""
    u64 = np.uint64
    x = a.astype(u64)
    neg = x > u64((p - 1) // 2)
    m = np.where(neg, u64(p) - x, x)
    v = ((m + u64((1 << (l - 1)) if l > 0 else 0)) >> u64(l)) + u64(sum(1 << (k * w + w - 1) for k in range(K - 1)))
    out = []
    for k in range(K):
        f = v >> u64(k * w)
        if k < K - 1:
            d = f & u64((1 << w) - 1)
            eneg = d < u64(1 << (w - 1))
            mag = np.where(eneg, u64(1 << (w - 1)) - d, d - u64(1 << (w - 1)))
        else:
            eneg, mag = np.zeros(x.shape, dtype=bool), f
        out.append(np.where((mag != 0) & (neg != eneg), u64(p) - mag, mag).astype(a.dtype))
    return np.stack(out)


def decompose(a: np.ndarray, p: int, w: int, K: int, l: int) -> np.ndarray:
    """a [polys, batch, N] -> [polys, K, batch, N]: what ntt_gadget_decompose writes"""
    return np.ascontiguousarray(np.moveaxis(digits(a, p, w, K, l), 0, 1))


def edge_words(p: int, w: int, K: int, l: int):
    """0, 1, the two words around p / 2, p - 1, the words around the rounding point 2^(l-1), and -- with both signs -- the words whose u
    has every lower digit at B/2 - 1 (the largest digit without a carry) and at B/2 (a carry out of every level)"""
    half, B = (p - 1) // 2, 1 << w
    ws = [0, 1 % p, half, half + 1, p - 1]
    if l > 0:
        ws += [x for x in ((1 << (l - 1)) - 1, 1 << (l - 1), (1 << (l - 1)) + 1) if x < p]
    for d in (B // 2 - 1, B // 2):
        u = sum(d << (k * w) for k in range(K - 1))
        for top in (0, 1):
            m = (u + (top << ((K - 1) * w))) << l
            if 0 < m <= half:
                ws += [m, p - m]
    return ws


def operand(wb: int, p: int, w: int, K: int, l: int, polys: int, batch: int, n: int, seed: int) -> np.ndarray:
    """a [polys, batch, N] canonical words: row 0 of every polynomial cycles through the edge words, the rest is random"""
    dt = np.uint32 if wb == 4 else np.uint64
    rng = np.random.default_rng(seed)
    a = (rng.integers(0, 2**63, size=(polys, batch, n), dtype=np.uint64) % np.uint64(p)).astype(dt)
    e = edge_words(p, w, K, l)
    a[:, 0, :] = np.array([e[i % len(e)] for i in range(n)], dtype=dt)
    return a


def want(oracle, a, b, T, p, w, K, l, broadcast=False):
    """the product: product_dot_ref.want of the reference digits [polys * K, batch, N] and b [polys * K, batch, N] (not prepared)"""
    polys, batch, n = a.shape
    return R.want(oracle, decompose(a, p, w, K, l).reshape(polys * K, batch, n), b, T, p, broadcast)
