#!/usr/bin/env python3
"""Coset LDE and coset interpolation on the columns of a row-major trace, one process on one MI355X (the product library):

  lde      A   lde_columns: [N][width] -> [M][width], the expansion fused into the first column pass
           B   what a caller could write before: rows scaled by s (pointwise_mul with a row-constant [N][width] matrix), scattered
               with torch into a zeroed [M][pitch], forward_columns on that
           C   transpose -> lde on [width][N] rows -> transpose back
           D   forward_columns of size M on the output-sized matrix: a yardstick only, it holds different data
  inverse  A'  coset_inverse_columns in place of the [M][width] matrix
           B'  transpose -> coset_inverse on [width][M] rows -> transpose back
           D'  inverse_columns(scale = 1): the yardstick

Shapes: Goldilocks 2^13 -> 2^16 at width 4096 (pitch 4096), a 31-bit prime 2^12 -> 2^15 at width 8192.  Outputs are compared before
any time is printed: A == B == C and A' == B', word for word.  Each leg: warm-up, then REPEATS timed bursts of BURST launches
between two events; the table gives the median per launch and the min .. max over the bursts.
Conditions (from traffic): A's burst maximum is below the burst minimum of B and of C; A is no slower than D by more than D's own
burst spread (its first pass reads 1 / 2^beta of the bytes); the same for A' against B' and D'.
usage: python tools/bench_lde_columns.py [--out profiles/lde_columns_ab.txt] [--repeats 7] [--burst 3]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_columns import timed  # noqa: E402
from ntt_aie_amd import NTTPlan, _lib  # noqa: E402

SHAPES = [("Goldilocks 2^13 -> 2^16 x width 4096", 16, 3, 0xFFFFFFFF00000001, 7, 8, 4096),
          ("p = 2013265921 (31 bit) 2^12 -> 2^15 x width 8192", 15, 3, 2013265921, 31, 4, 8192)]


def _bitrev(i, bits):
    return int(format(i, "0%db" % bits)[::-1], 2)


def run_shape(name, logm, beta, p, g, wb, width, repeats, burst, lines, verdict):
    m, n = 1 << logm, (1 << logm) >> beta
    tdt, ndt = (torch.int32, np.uint32) if wb == 4 else (torch.int64, np.uint64)
    big = NTTPlan(logm, p, wb, 0)
    big.generate_twiddles(1, g)
    big.set_coset(beta, g)
    big.set_coset_inverse(g)
    small = NTTPlan(logm - beta, p, wb, 0)  # leg B's row scaling (pointwise_mul takes [batch][N] words)
    small.generate_twiddles(1, g)
    gen = torch.Generator(device="cuda:0").manual_seed(1)
    mat = torch.randint(0, min(p, 2**62), (n, width), dtype=tdt, device="cuda:0", generator=gen)
    s_rows = np.array([pow(g, _bitrev(i, logm - beta), p) for i in range(n)], dtype=ndt)
    s_mat = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(s_rows[:, None], (n, width))).view(np.int32 if wb == 4 else np.int64)).to("cuda:0")
    out_a, out_b = torch.empty((m, width), dtype=tdt, device="cuda:0"), torch.empty((m, width), dtype=tdt, device="cuda:0")
    scaled = torch.empty_like(mat)
    rows_out = torch.empty((width, m), dtype=tdt, device="cuda:0")
    out_c = torch.empty_like(out_a)
    lines.append("")
    lines.append("%s   blow-up 2^%d   column passes %s" % (name, beta, [k for _, k in big.column_passes]))

    def leg_a():
        big.lde_columns(mat, out_a)

    def leg_b():
        small.pointwise_mul(mat.view(width, n), s_mat.view(width, n), scaled.view(width, n))
        out_b.zero_()
        out_b[:: 1 << beta] = scaled
        big.forward_columns(out_b, out_b)

    def leg_c():
        t = mat.t().contiguous()
        big.lde(t, rows_out)
        out_c.copy_(rows_out.t())

    def leg_d():
        big.forward_columns(out_c, out_b)

    res = {"A  lde_columns": timed(leg_a, repeats, burst), "B  scale, zero-fill, scatter, forward_columns": timed(leg_b, repeats, burst),
           "C  transpose, lde on rows, transpose back": timed(leg_c, repeats, burst)}
    assert torch.equal(out_a, out_b), "A differs from B"
    assert torch.equal(out_a, out_c), "A differs from C"
    res["D  forward_columns of size M (yardstick)"] = timed(leg_d, repeats, burst)
    lines.append("  lde")
    for k, (med, lo, hi) in res.items():
        lines.append("    %-48s %9.4f ms   (min %9.4f .. max %9.4f)" % (k, med, lo, hi))
    a, b, c, d = (res[k] for k in res)
    ok_b, ok_c, ok_d = a[2] < b[1], a[2] < c[1], a[0] <= d[0] + (d[2] - d[1])
    lines.append("    A / B = %.3f   A / C = %.3f   A / D = %.3f   A's burst maximum below B's minimum: %s, below C's minimum: %s; A within D's burst spread of D: %s"
                 % (a[0] / b[0], a[0] / c[0], a[0] / d[0], ok_b, ok_c, ok_d))
    verdict.append((name, "lde", ok_b and ok_c, ok_d))

    vals = out_a.clone()  # values on the coset: the interpolation's input
    work = torch.empty_like(vals)

    def leg_a2():
        big.coset_inverse_columns(vals, work)

    def leg_b2():
        t = vals.t().contiguous()
        big.coset_inverse(t, t)
        out_b.copy_(t.t())

    def leg_d2():
        big.inverse_columns(vals, out_c)

    res = {"A' coset_inverse_columns": timed(leg_a2, repeats, burst), "B' transpose, coset_inverse on rows, transpose back": timed(leg_b2, repeats, burst)}
    assert torch.equal(work, out_b), "A' differs from B'"
    assert torch.equal(work[:: 1 << beta], mat) and not bool(work.view(n, 1 << beta, width)[:, 1:].any()), "A'(A(x)) is not x on every 2^beta-th row"
    res["D' inverse_columns, scaled (yardstick)"] = timed(leg_d2, repeats, burst)
    lines.append("  coset inverse")
    for k, (med, lo, hi) in res.items():
        lines.append("    %-48s %9.4f ms   (min %9.4f .. max %9.4f)" % (k, med, lo, hi))
    a, b, d = (res[k] for k in res)
    ok_b, ok_d = a[2] < b[1], a[0] <= d[0] + (d[2] - d[1])
    lines.append("    A' / B' = %.3f   A' / D' = %.3f   A' burst maximum below B' minimum: %s; A' within D' burst spread of D': %s" % (a[0] / b[0], a[0] / d[0], ok_b, ok_d))
    verdict.append((name, "coset inverse", ok_b, ok_d))
    big.close()
    small.close()
    del mat, s_mat, out_a, out_b, out_c, scaled, rows_out, vals, work
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--burst", type=int, default=3)
    a = ap.parse_args()
    lines = ["coset LDE / coset interpolation on matrix columns  (tools/bench_lde_columns.py; product library, ntt_version %d)" % _lib.lib().ntt_version(),
             "GPU: %s   kernel-source hash: %s" % (torch.cuda.get_device_name(0), _lib.kernel_source_hash()),
             "%d bursts of %d launches per leg, median per launch; A == B == C and A' == B', word for word (checked before timing is printed)" % (a.repeats, a.burst)]
    verdict = []
    for shape in SHAPES:
        run_shape(*shape, a.repeats, a.burst, lines, verdict)
    lines.append("")
    for name, what, faster, within in verdict:
        lines.append("condition, %s, %s: fused faster than every alternative in every burst: %s; within the yardstick's burst spread: %s" % (name, what, faster, within))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
