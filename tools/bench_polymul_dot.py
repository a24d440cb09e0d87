#!/usr/bin/env python3
"""A/B of the negacyclic inner product with prepared operands, one process on one MI355X, the product library (kind-2 tables made on the
device), TERMS = 4 terms:

  D   ntt_polymul_dot_pre, one prepared row per term and row of a
  D1  the same with ONE prepared row per term for the whole batch (the broadcast: a key switch)
  P   TERMS calls of ntt_polymul_negacyclic_pre on the same operands, into TERMS output blocks.  The TERMS - 1 modular sums a caller
      would also pay are NOT in this leg (the library has no modular add): it is a lower bound on the hand-composed path, and the
      comparison is conservative.

Every leg overwrites its TERMS blocks of a: each is timed WITH the device-to-device copy of a, the copy is timed alone in the same rounds,
and the table gives both the raw figure and the one with the copy subtracted.  Before any time is printed, sampled rows of D are compared
word for word with the sum mod p of P's TERMS results (added on the host), and D1 with the same sum on a broadcast operand.  The legs run
interleaved: ROUNDS rounds, in each one burst of K launches per leg between two events; the table gives the median per launch and
min .. max over the bursts.
usage: python tools/bench_polymul_dot.py [--out profiles/polymul_dot_ab.txt] [--rounds 7] [--k 3]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ntt_aie_amd import _lib  # noqa: E402
from ntt_aie_amd.plan import NTTPlan  # noqa: E402

GOLD = 0xFFFFFFFF00000001
TERMS = 4
SHAPES = [("BASELINE config 4: Goldilocks 2^20, batch 512", 20, GOLD, 7, 8, 512),
          ("Goldilocks 2^16, batch 4096", 16, GOLD, 7, 8, 4096)]


def burst(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def host_words(t, wb):
    return t.cpu().numpy().view(np.uint32 if wb == 4 else np.uint64)


def addmod(x, y, p):
    s = x + y
    return np.where((s < x) | (s >= x.dtype.type(p)), s - x.dtype.type(p), s)


def run_shape(name, logn, p, g, wb, batch, rounds, k, lines):
    n = 1 << logn
    pl = NTTPlan(logn, p, wb, 0)
    pl.generate_twiddles(2, g)
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    tdt = torch.int32 if wb == 4 else torch.int64

    def rnd(*shape):
        return torch.randint(0, min(p, 1 << 62), shape, dtype=torch.int64, device="cuda:0", generator=gen).to(tdt)

    x = rnd(TERMS, batch, n)
    bhat = rnd(TERMS, batch, n)
    for t in range(TERMS):
        pl.polymul_prepare(bhat[t], bhat[t])
    bhat1 = bhat[:, :1].clone()
    wa, out, outs = torch.empty_like(x), torch.empty_like(x[0]), torch.empty_like(x)

    def leg_d():
        wa.copy_(x)
        pl.polymul_dot_pre(wa, bhat, out)

    def leg_d1():
        wa.copy_(x)
        pl.polymul_dot_pre(wa, bhat1, out)

    def leg_p():
        wa.copy_(x)
        for t in range(TERMS):
            pl.polymul_negacyclic_pre(wa[t], bhat[t], outs[t])

    def copy():
        wa.copy_(x)

    # the words, before any time is taken: sampled rows of D against the host sum of P's results, D1 against the same on a broadcast
    rows = sorted({0, batch // 2, batch - 1})
    leg_p()
    want = None
    for t in range(TERMS):
        c = host_words(outs[t, rows], wb)
        want = c if want is None else addmod(want, c, p)
    leg_d()
    assert np.array_equal(host_words(out[rows], wb), want), "D differs from the sum of P's results"
    wa.copy_(x)
    want = None
    for t in range(TERMS):
        pl.polymul_negacyclic_pre(wa[t], bhat1[t], outs[t])
        c = host_words(outs[t, rows], wb)
        want = c if want is None else addmod(want, c, p)
    leg_d1()
    assert np.array_equal(host_words(out[rows], wb), want), "D1 differs from the sum of the broadcast products"
    del want
    legs = [("D  dot_pre, per row", leg_d), ("D1 dot_pre, broadcast", leg_d1), ("P  %d x polymul_negacyclic_pre" % TERMS, leg_p)]
    for _, fn in legs:
        fn()
    torch.cuda.synchronize()
    ms = {nm: [] for nm, _ in legs}
    cp = []
    for _ in range(rounds):
        for nm, fn in legs:
            ms[nm].append(burst(fn, k))
        cp.append(burst(copy, k))
    passes = [st for _, _, st in pl.passes_for(batch)]
    lines.append("")
    lines.append("%s, %d terms   passes %s" % (name, TERMS, passes))
    c_med = statistics.median(cp)
    lines.append("  copy of the %d blocks of a alone: %.4f ms (median)" % (TERMS, c_med))
    net = {}
    for nm, _ in legs:
        v = ms[nm]
        net[nm] = [t - c_med for t in v]
        lines.append("  %-34s raw %9.4f ms (min %9.4f .. max %9.4f)   less copy %9.4f ms (min %9.4f .. max %9.4f)"
                     % (nm, statistics.median(v), min(v), max(v), statistics.median(net[nm]), min(net[nm]), max(net[nm])))
    d, d1, pp = (net[nm] for nm, _ in legs)
    lines.append("  D / P = %.3f   D1 / P = %.3f   (medians, copy subtracted; P omits the %d modular sums of a caller.  Derived, not measured: "
                 "traffic (4K+3)/(7K) = %.3f, butterflies (K+1)/(2K) = %.3f%s)"
                 % (statistics.median(d) / statistics.median(pp), statistics.median(d1) / statistics.median(pp), TERMS - 1, (4 * TERMS + 3) / (7 * TERMS),
                    (TERMS + 1) / (2 * TERMS), "" if len(passes) == 2 else "; the traffic figure is the two-pass one"))
    lines.append("  D faster than P in every burst: %s   D1 faster than P in every burst: %s" % (max(d) < min(pp), max(d1) < min(pp)))
    pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="*", help="indices into SHAPES (default: all)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["negacyclic inner product with prepared operands, A/B  (tools/bench_polymul_dot.py; library %s)" % os.path.basename(_lib.LIB_PATH),
             "GPU: %s   kernel-source hash: %s" % (torch.cuda.get_device_name(0), _lib.kernel_source_hash()),
             "%d interleaved rounds, one burst of %d launches per leg and round, median per launch; the legs' words agree on sampled rows (checked)" % (a.rounds, a.k)]
    for i, shape in enumerate(SHAPES):
        if a.shapes is None or i in a.shapes:
            run_shape(*shape, a.rounds, a.k, lines)
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
