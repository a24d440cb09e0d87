#!/usr/bin/env python3
"""A/B/C of the row-major matrix transforms, one process on one MI355X (the product library):

  a  forward_columns / inverse_columns on the matrix [N][width] where it lies
  b  what a caller had to do before: transpose -> contiguous, plan.forward / plan.inverse on [width][N], transpose -> contiguous back
  c  plan.forward / plan.inverse on a [width][N] buffer of the same size: a yardstick only, it holds different data

Shapes: Goldilocks N = 2^16 x width 4096 (the headline's bytes), a 31-bit prime N = 2^15 x width 8192, and one narrow case (width 16,
pitch 16: half of a 4-byte tile's lanes are dead) to show what dead lanes cost.  Outputs are compared before any time is printed:
a == b word for word, and c on the transposed input == a transposed.  Each leg: warm-up, then REPEATS timed bursts of BURST launches
between two events; the table gives the median per launch and the min .. max over the bursts.
Condition (from traffic: b moves the batch through HBM at least twice more than a, same butterflies): a's burst maximum is below b's
burst minimum at both wide shapes, both directions.  How a stands against c is reported, not required.
usage: python tools/bench_columns.py [--out profiles/columns_ab.txt] [--repeats 7] [--burst 3] [--only-a]"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ntt_aie_amd import NTTPlan, _lib  # noqa: E402

SHAPES = [("Goldilocks N = 2^16 x width 4096", 16, 0xFFFFFFFF00000001, 7, 8, 4096, True),
          ("p = 2013265921 (31 bit) N = 2^15 x width 8192", 15, 2013265921, 31, 4, 8192, True),
          ("Goldilocks N = 2^16 x width 16, pitch 16 (narrow: dead lanes)", 16, 0xFFFFFFFF00000001, 7, 8, 16, False),
          ("p = 2013265921 (31 bit) N = 2^15 x width 16, pitch 16 (narrow: half of every tile is dead)", 15, 2013265921, 31, 4, 16, False)]


def timed(fn, repeats, burst, warmup=2):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(burst):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / burst)
    return statistics.median(ms), min(ms), max(ms)


def run_shape(name, logn, p, g, wb, width, required, repeats, burst, only_a, lines, verdict):
    n = 1 << logn
    pl = NTTPlan(logn, p, wb, 0)
    pl.generate_twiddles(1, g)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    mat = torch.randint(0, min(p, 2**62), (n, width), dtype=torch.int32 if wb == 4 else torch.int64, device="cuda:0", generator=gen)
    if wb == 4 and p >= 2**31:
        raise SystemExit("shape needs p < 2^31 for torch.randint on int32")
    out_a, out_b = torch.empty_like(mat), torch.empty_like(mat)
    rows = torch.empty((width, n), dtype=mat.dtype, device="cuda:0")
    lines.append("")
    lines.append("%s   column passes %s   (c: plan passes %s)" % (name, [m for _, m in pl.column_passes], [st for _, _, st in pl.passes_for(width)]))
    for direction, cols_fn, rows_fn in (("forward", pl.forward_columns, pl.forward), ("scaled inverse", pl.inverse_columns, pl.inverse)):
        res = {}

        def leg_a():
            cols_fn(mat, out_a)

        def leg_b():
            t = mat.t().contiguous()
            rows_fn(t, t)
            out_b.copy_(t.t())

        def leg_c():
            rows_fn(mat_t, rows)

        res["a columns in place of the matrix"] = timed(leg_a, repeats, burst)
        if not only_a:
            res["b transpose, rows, transpose back"] = timed(leg_b, repeats, burst)
            assert torch.equal(out_a, out_b), "a differs from b"
            mat_t = mat.t().contiguous()
            res["c rows on [width][N] (yardstick)"] = timed(leg_c, repeats, burst)
            assert torch.equal(rows.t(), out_a), "c on the transposed input differs from a"
            del mat_t
        lines.append("  %s" % direction)
        for k, (med, lo, hi) in res.items():
            lines.append("    %-36s %9.4f ms   (min %9.4f .. max %9.4f)" % (k, med, lo, hi))
        if not only_a:
            a, b, c = (res[k] for k in res)
            ok = a[2] < b[1]
            lines.append("    a / b = %.3f   a / c = %.3f   a's burst maximum below b's burst minimum: %s%s" % (a[0] / b[0], a[0] / c[0], ok, "" if required else "   (reported, not required)"))
            if required:
                verdict.append((name, direction, ok))
    pl.close()
    del mat, out_a, out_b, rows
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--burst", type=int, default=3)
    ap.add_argument("--only-a", action="store_true", help="leg a alone (a kernel trace of the matrix passes)")
    a = ap.parse_args()
    lines = ["row-major matrix transforms A/B/C  (tools/bench_columns.py; product library, ntt_version %d)" % _lib.lib().ntt_version(),
             "GPU: %s   kernel-source hash: %s" % (torch.cuda.get_device_name(0), _lib.kernel_source_hash()),
             "%d bursts of %d launches per leg, median per launch; a == b and c == a transposed, word for word (checked before timing is printed)" % (a.repeats, a.burst)]
    verdict = []
    for shape in SHAPES:
        run_shape(*shape, a.repeats, a.burst, a.only_a, lines, verdict)
    lines.append("")
    for name, direction, ok in verdict:
        lines.append("condition, %s, %s: a faster than b in every burst: %s" % (name, direction, ok))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
