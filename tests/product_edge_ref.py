"""What tests/test_product_edges_cpu.py and tests/test_gpu_product_edges.py share: operands of the product entry points whose
TRANSFORM-DOMAIN words are edge residues, and the words every entry point must answer with.

Fwd o Inv = id, so a = Fwd(e . N^-1) has InvU(a) = e word for word: the word that leaves the inverse rounds of the fused middle pass
(pass.h: run_product_pass / run_product_dot_pass) and meets b^, the accumulator and the N^-1 scaling is the chosen residue e[r][i].  The
prepared operand b^ is handed in as it is.  Only the RESIDUE of that word is controlled; which lazy representative carries it (a word
in [0, 2p), an unreduced sum) is the kernel's own business, and the inputs a themselves are ordinary-looking canonical words.

The edge list E(class) has 13 residues, every ordered pair of E x E (169 pairs) occurs as (ea[r][i], eb[r][i]) -- asserted here --, and
the pair list is stepped through with a stride coprime to 169, so that pairs do not line up with lane or register positions.  Every
expected word comes from Python integers per pair (169 of them), spread with numpy indexing, then oracle.ntt: neither the oracle's
pointwise product nor any arithmetic of the library is part of the reference."""
import functools

import numpy as np

from test_gpu_columns import ALL_CLASSES

# the seven classes of the coset / column files as they are (m64 is 0xFFFFFFFC00000001: canonical sums wrap the word), and the two
# moduli the older product tests use: the 62-bit prime and a 4-byte prime of stream 2
CLASSES = {**ALL_CLASSES, "m62": (8, 0x3FFFFFEE00000001, 3), "c32": (4, 3221225473, 5)}
NE, NPAIRS, STRIDE = 13, 169, 70  # gcd(70, 169) = 1; 70 = 5 * 13 + 5 moves both members of the pair by 5 per position


def edges(cls):
    """E(class): the closure under v -> (p - v) mod p of the seeds, duplicates removed, in a fixed order"""
    wb, p, _ = CLASSES[cls]
    seeds = [0, 1, 2, p - 1, p - 2]
    seeds += [2**32 - 1, 2**32, 2**63 - 1, 2**63, p - 2**32] if wb == 8 else [2**30, 2**31 - 1, 2**31, (p - 1) // 2, (p + 1) // 2]
    out = []
    for v in seeds:
        for w in (v % p, (p - v) % p):
            if w not in out:
                out.append(w)
    assert len(out) == NE and all(0 <= v < p for v in out), (cls, out)
    return tuple(out)


def batch_for(logn):
    """the smallest odd batch >= 3 with batch * N >= 2 * 169: every pair at least twice, and an odd batch leaves the last polynomial
    group of a many-polynomial workgroup ragged"""
    b = 3
    while (b << logn) < 2 * NPAIRS:
        b += 2
    return b


def table(cls, logn):
    import oracle_py

    wb, p, g = CLASSES[cls]
    T = oracle_py.make_table(2, 1 << logn, p, g, wb)
    T.setflags(write=False)
    return T


class Grid:
    """Which pair sits where.  q[r][i] is the index of the pair at word i of row r (pair q = (E[q // 13], E[q % 13])), and adv(q, k) the
    pair index of the same word in term k of a sum.  per row: q = (r * N + i) * STRIDE mod 169, term k is the grid advanced by k
    positions.  broadcast: b^ is ONE row cycling through E (term k: shifted by k), and ea steps through E by i // 13 and by row so that
    all pairs still occur over the batch (term k: shifted by 2k)."""

    def __init__(self, logn, batch, broadcast):
        n = 1 << logn
        i, r = np.arange(n, dtype=np.int64)[None, :], np.arange(batch, dtype=np.int64)[:, None]
        self.broadcast = broadcast
        if broadcast:
            self.q = ((i // NE + r * (n // NE)) % NE) * NE + i % NE
        else:
            self.q = ((r * n + i) * STRIDE) % NPAIRS
        assert self.q.shape == (batch, n) and len(np.unique(self.q)) == NPAIRS, "a pair of E x E is missing"

    def adv(self, q, k):
        if self.broadcast:
            return ((q // NE + 2 * k) % NE) * NE + (q % NE + k) % NE
        return (q + k * STRIDE) % NPAIRS


class _Builder:
    def __init__(self, cls, logn, batch, broadcast):
        self.wb, self.p, _ = CLASSES[cls]
        self.dt = np.uint32 if self.wb == 4 else np.uint64
        self.n = 1 << logn
        self.E = edges(cls)
        self.T = table(cls, logn)
        self.ninv = pow(self.n, -1, self.p)
        self.grid = Grid(logn, batch, broadcast)

    def spread(self, fn):
        """fn(q) in Python integers for each of the 169 pairs, then at every word the value of its pair"""
        tab = [fn(q) % self.p for q in range(NPAIRS)]
        return np.array(tab, dtype=np.uint64).astype(self.dt)[self.grid.q]

    def fwd(self, w):
        import oracle_py

        return oracle_py.ntt(w, self.T, self.p, nthreads=4)

    def left(self, q):
        return self.E[q // NE]

    def right(self, q):
        return self.E[q % NE]


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def case(cls, logn, batch, broadcast=False, terms=3):
    """One shape.  Read-only arrays, computed once:
         ea, eb [batch][N]         the transform-domain targets (broadcast: eb is [1][N])
         a, b                      Fwd(ea . N^-1), Fwd(eb . N^-1): InvU(a) == ea, InvU(b) == eb
         bhat = eb                 the prepared operand, handed in directly
         want_mul                  Fwd(ea . eb . N^-1): the two-operand and the prepared product
         a_dot, bhat_dot           [terms][batch][N] / [terms][batch or 1][N]: term k is the grid advanced by k
         want_dot                  Fwd(N^-1 . sum_k ea_k . eb_k), the sum in Python integers
       and, per row only, the additive grid of the summed kernel -- two terms a and b with b^_0 all ones:
         ones, minus_ones          b^_1 = all ones / all p - 1
         want_plus, want_minus     Fwd((ea + eb) . N^-1), Fwd((ea + (p - 1) . eb) . N^-1): every pair of edge residues through the
                                   accumulator's add, among them sums equal to p, sums that wrap the word, and 0 + 0"""
    B = _Builder(cls, logn, batch, broadcast)
    p, E, g = B.p, B.E, B.grid
    ea, eb = B.spread(B.left), B.spread(B.right)
    res = {"T": B.T, "p": p, "ea": ea, "a": B.fwd(B.spread(lambda q: B.left(q) * B.ninv)), "b": B.fwd(B.spread(lambda q: B.right(q) * B.ninv)),
           "want_mul": B.fwd(B.spread(lambda q: B.left(q) * B.right(q) * B.ninv))}
    a_dot, bhat_dot = [res["a"]], [eb]
    for k in range(1, terms):
        a_dot.append(B.fwd(B.spread(lambda q: B.left(g.adv(q, k)) * B.ninv)))
        bhat_dot.append(B.spread(lambda q: B.right(g.adv(q, k))))
    res["want_dot"] = B.fwd(B.spread(lambda q: sum(B.left(g.adv(q, k)) * B.right(g.adv(q, k)) for k in range(terms)) * B.ninv))
    if broadcast:  # one row of b^ for every row of a: the grid makes every row of eb the same
        assert all(np.array_equal(x, np.repeat(x[:1], batch, axis=0)) for x in bhat_dot)
        bhat_dot = [x[:1] for x in bhat_dot]
        eb = eb[:1]
        assert sorted(int(v) for v in set(eb[0].tolist())) == sorted(E)
    else:
        res["ones"], res["minus_ones"] = np.ones_like(ea), np.full_like(ea, p - 1)
        res["want_plus"] = B.fwd(B.spread(lambda q: (B.left(q) + B.right(q)) * B.ninv))
        res["want_minus"] = B.fwd(B.spread(lambda q: (B.left(q) + (p - 1) * B.right(q)) * B.ninv))
    res["eb"] = res["bhat"] = np.ascontiguousarray(eb)
    res["a_dot"], res["bhat_dot"] = np.ascontiguousarray(np.stack(a_dot)), np.ascontiguousarray(np.stack(bhat_dot))
    return _freeze(res)


@functools.lru_cache(maxsize=None)
def long_sum(cls, logn, batch, terms=17):
    """The additive grid drawn out: term 2j is the left member and term 2j + 1 the right member of the grid advanced by j, every b^
    all ones.  a [terms][batch][N], ones of the same shape, and Fwd(N^-1 . sum) with the sum in Python integers."""
    B = _Builder(cls, logn, batch, False)
    g = B.grid
    pick = lambda q, k: B.left(g.adv(q, k // 2)) if k % 2 == 0 else B.right(g.adv(q, k // 2))  # noqa: E731
    a = np.ascontiguousarray(np.stack([B.fwd(B.spread(lambda q: pick(q, k) * B.ninv)) for k in range(terms)]))
    return _freeze({"T": B.T, "p": B.p, "a": a, "ones": np.ones_like(a), "want": B.fwd(B.spread(lambda q: sum(pick(q, k) for k in range(terms)) * B.ninv))})
