#!/usr/bin/env python3
"""A/B of the negacyclic product with a prepared operand, one process on one MI355X, the product library (kind-2 tables made on the device):

  A   ntt_polymul_negacyclic_pre, one prepared row per row of a
  A1  the same with ONE prepared row for the whole batch (the broadcast)
  B   ntt_polymul_negacyclic on fresh copies of both operands (the call overwrites them)
  C   the hand composition a caller can write without the new entry point: ntt_inverse (unscaled) + ntt_pointwise_mul (* N^-1) +
      ntt_forward

A and A1 overwrite a, B overwrites a and b: each leg is timed WITH its device-to-device operand copies (one for A / A1, two for B, none
for C, whose inverse runs out of place), the copies are timed alone in the same rounds, and the table gives both the raw figure and
the one with the copies subtracted.  Every variant's product is compared word for word with A's (A1 against a B run on a broadcast
operand) before any time is printed.  The legs run interleaved: ROUNDS rounds, in each one burst of K launches per leg between two
events; the table gives the median per launch and min .. max over the bursts.
usage: python tools/bench_polymul_pre.py [--out profiles/polymul_pre_ab.txt] [--rounds 7] [--k 3]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ntt_aie_amd import _lib  # noqa: E402
from ntt_aie_amd.plan import NTTPlan  # noqa: E402

GOLD = 0xFFFFFFFF00000001
SHAPES = [("BASELINE config 4: Goldilocks 2^20, batch 512", 20, GOLD, 7, 8, 512),
          ("Goldilocks 2^16, batch 4096", 16, GOLD, 7, 8, 4096),
          ("Goldilocks 2^12, batch 4096 (single pass: the product is ONE launch)", 12, GOLD, 7, 8, 4096),
          ("p = 2013265921 (31 bit) 2^12, batch 8192", 12, 2013265921, 31, 4, 8192)]


def burst(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def run_shape(name, logn, p, g, wb, batch, rounds, k, lines):
    n = 1 << logn
    pl = NTTPlan(logn, p, wb, 0)
    pl.generate_twiddles(2, g)
    ninv = pow(n, p - 2, p)
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    tdt = torch.int32 if wb == 4 else torch.int64

    def rnd(rows):
        return torch.randint(0, min(p, 1 << 62), (rows, n), dtype=torch.int64, device="cuda:0", generator=gen).to(tdt)

    x, y = rnd(batch), rnd(batch)
    wa, wy, out = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    bhat = pl.polymul_prepare(y)
    bhat1 = bhat[:1].clone()

    def leg_a():
        wa.copy_(x)
        pl.polymul_negacyclic_pre(wa, bhat, out)

    def leg_a1():
        wa.copy_(x)
        pl.polymul_negacyclic_pre(wa, bhat1, out)

    def leg_b():
        wa.copy_(x)
        wy.copy_(y)
        pl.polymul_negacyclic(wa, wy, out)

    def leg_c():
        pl.inverse(x, wa, scale=False)
        pl.pointwise_mul(wa, bhat, wa, scale=ninv)
        pl.forward(wa, out)

    def copy1():
        wa.copy_(x)

    def copy2():
        wa.copy_(x)
        wy.copy_(y)

    # every variant's words, before any time is taken
    leg_a()
    ref = out.clone()
    leg_b()
    assert torch.equal(out, ref), "B differs from A"
    leg_c()
    assert torch.equal(out, ref), "C differs from A"
    leg_a1()
    got1 = out.clone()
    wa.copy_(x)
    wy.copy_(y[:1].expand(batch, n))
    pl.polymul_negacyclic(wa, wy, out)
    assert torch.equal(out, got1), "A1 differs from the product with a broadcast operand"
    del ref, got1
    legs = [("A  pre, per row", leg_a, 1), ("A1 pre, broadcast", leg_a1, 1), ("B  polymul_negacyclic", leg_b, 2), ("C  inverse + pointwise + forward", leg_c, 0)]
    for _, fn, _ in legs:
        fn()
    torch.cuda.synchronize()
    ms = {nm: [] for nm, _, _ in legs}
    cp = {1: [], 2: []}
    for _ in range(rounds):
        for nm, fn, _ in legs:
            ms[nm].append(burst(fn, k))
        cp[1].append(burst(copy1, k))
        cp[2].append(burst(copy2, k))
    fused = len(pl.passes_for(batch))
    lines.append("")
    lines.append("%s   passes %s" % (name, [st for _, _, st in pl.passes_for(batch)]))
    c_med = {0: 0.0, 1: statistics.median(cp[1]), 2: statistics.median(cp[2])}
    lines.append("  operand copies alone: one %.4f ms, two %.4f ms (median)" % (c_med[1], c_med[2]))
    net = {}
    for nm, _, ncopies in legs:
        v = ms[nm]
        net[nm] = [t - c_med[ncopies] for t in v]
        lines.append("  %-34s raw %9.4f ms (min %9.4f .. max %9.4f)   less copies %9.4f ms (min %9.4f .. max %9.4f)"
                     % (nm, statistics.median(v), min(v), max(v), statistics.median(net[nm]), min(net[nm]), max(net[nm])))
    a, a1, b, c = (net[nm] for nm, _, _ in legs)
    lines.append("  A / B = %.3f   A / C = %.3f   A1 / B = %.3f   (medians, copies subtracted; traffic arithmetic 7/9 = 0.778, butterflies 2/3 = 0.667%s)"
                 % (statistics.median(a) / statistics.median(b), statistics.median(a) / statistics.median(c), statistics.median(a1) / statistics.median(b),
                    "" if fused == 2 else "; those figures are the two-pass ones"))
    lines.append("  A faster than B in every burst: %s   A faster than C in every burst: %s" % (max(a) < min(b), max(a) < min(c)))
    pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="*", help="indices into SHAPES (default: all)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    lines = ["negacyclic product with a prepared operand, A/B  (tools/bench_polymul_pre.py; library %s)" % os.path.basename(_lib.LIB_PATH),
             "GPU: %s   kernel-source hash: %s" % (torch.cuda.get_device_name(0), _lib.kernel_source_hash()),
             "%d interleaved rounds, one burst of %d launches per leg and round, median per launch; all legs produce the same words (checked)" % (a.rounds, a.k)]
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
