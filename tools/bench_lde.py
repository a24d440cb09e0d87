#!/usr/bin/env python3
"""A/B of the coset low-degree extension, one process on one MI355X (the experiment build, tools/_explib.py):

  A  the composition a caller can write against the API WITHOUT ntt_lde: pre-built [batch][N] scale rows (outside the timed
     region), pointwise_mul, zero-fill of [batch][M], strided copy, forward in place.  Uses only entry points the library had
     before ntt_lde, so the tool also runs on a checkout without it -- A (and D) are then that checkout's numbers, B / C are absent.
  B  ntt_lde with the separate expansion kernel forced (NTT_LDE_UNFUSED=1, an experiment-build knob read at plan creation)
  C  ntt_lde, expansion fused into the first pass
  D  plain forward at size M, same batch (in place)
and the first pass alone of C and of D (NTT_ONLY_PASS=0 plans: only that launch runs).

Shapes: Goldilocks N = 2^16 -> 2^19 at batch 512; a 31-bit prime N = 2^12 -> 2^15 at batch 8192.  Each leg: warm-up, then REPEATS
timed bursts of BURST launches between two events; the table gives the median per launch and the min .. max over the bursts, and
`spread` = (max - min) / median of the noisiest leg is the run-to-run spread a difference has to exceed.
usage: python tools/bench_lde.py [--out profiles/lde_ab.txt] [--repeats 9] [--burst 5]"""
import argparse
import os
import re
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _explib  # noqa: E402

LIBNAME = _explib.select()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ntt_aie_amd import _lib  # noqa: E402
from ntt_aie_amd.plan import NTTPlan, to_device  # noqa: E402

SHAPES = [("Goldilocks 2^16 -> 2^19, batch 512", 16, 3, 0xFFFFFFFF00000001, 7, 8, 512),
          ("p = 2013265921 (31 bit) 2^12 -> 2^15, batch 8192", 12, 3, 2013265921, 31, 4, 8192)]


def plan_with_env(logn, p, wb, g, **env):
    """a plan made while the experiment build's knobs say `env` (they are read at ntt_plan_create)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        pl = NTTPlan(logn, p, wb, 0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    pl.generate_twiddles(1, g)
    return pl


def timed(fn, repeats, burst, warmup=3):
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


def bitrev(i, bits):
    r = 0
    for k in range(bits):
        r |= ((i >> k) & 1) << (bits - 1 - k)
    return r


def clocks():
    try:
        out = subprocess.run(["rocm-smi", "-d", "0", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        s = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
        m = re.search(r"mclk clock level: \d+: \((\d+)Mhz\)", out)
        return "sclk %s MHz, mclk %s MHz (read after the timed legs)" % (s.group(1) if s else "?", m.group(1) if m else "?")
    except Exception as e:  # no rocm-smi on this box
        return "clocks not readable (%s)" % type(e).__name__


def run_shape(name, logn, beta, p, g, wb, batch, repeats, burst, lines):
    n, m = 1 << logn, 1 << (logn + beta)
    dt = np.uint32 if wb == 4 else np.uint64
    have_lde = hasattr(_lib.lib(), "ntt_lde")
    rng = np.random.default_rng(1)
    coeffs = to_device((rng.integers(0, 2**63, size=(batch, n), dtype=np.uint64) % np.uint64(p)).astype(dt), "cuda:0")
    out = torch.empty((batch, m), dtype=coeffs.dtype, device="cuda:0")
    small = plan_with_env(logn, p, wb, g)   # A's pointwise_mul runs on [batch][N] rows
    big = plan_with_env(logn + beta, p, wb, g)
    shift = g
    srow = np.array([pow(shift, bitrev(i, logn), p) for i in range(n)], dtype=dt)
    scale_rows = to_device(np.broadcast_to(srow, (batch, n)).copy(), "cuda:0")  # pre-built, outside the timed region
    prod = torch.empty_like(coeffs)

    def leg_a():
        small.pointwise_mul(coeffs, scale_rows, prod)
        out.zero_()
        out.view(batch, n, 1 << beta)[:, :, 0].copy_(prod)
        big.forward(out, out)

    res = {}
    res["A composed (parent API)"] = timed(leg_a, repeats, burst)
    ref = out.clone() if have_lde else None
    if have_lde:
        big.set_coset(beta, shift)
        unf = plan_with_env(logn + beta, p, wb, g, NTT_LDE_UNFUSED=1)
        unf.set_coset(beta, shift)
        assert big.lde_fused and not unf.lde_fused
        res["B lde, separate expansion"] = timed(lambda: unf.lde(coeffs, out), repeats, burst)
        assert torch.equal(out, ref), "B differs from A"
        res["C lde, fused first pass"] = timed(lambda: big.lde(coeffs, out), repeats, burst)
        assert torch.equal(out, ref), "C differs from A"
    res["D forward at size M"] = timed(lambda: big.forward(out, out), repeats, burst)
    first = plan_with_env(logn + beta, p, wb, g, NTT_ONLY_PASS=0)
    if have_lde:
        first.set_coset(beta, shift)
        res["C first pass alone"] = timed(lambda: first.lde(coeffs, out), repeats, burst)
    res["D first pass alone"] = timed(lambda: first.forward(out, out), repeats, burst)
    lines.append("")
    lines.append("%s   passes %s" % (name, [st for _, _, st in big.passes_for(batch)]))
    spread = 0.0
    for k, (med, lo, hi) in res.items():
        lines.append("  %-30s %9.4f ms   (min %9.4f .. max %9.4f, %+5.1f %%)" % (k, med, lo, hi, 100 * (hi - lo) / med))
        spread = max(spread, (hi - lo) / med)
    lines.append("  run-to-run spread (noisiest leg): %.1f %%" % (100 * spread))
    if have_lde:
        a, b, c = res["A composed (parent API)"][0], res["B lde, separate expansion"][0], res["C lde, fused first pass"][0]
        c1, d1 = res["C first pass alone"][0], res["D first pass alone"][0]
        lines.append("  C / A = %.3f   C / B = %.3f   C first pass / D first pass = %.3f  (bar: <= 1.03)" % (c / a, c / b, c1 / d1))
        lines.append("  C < A beyond the spread: %s   C < B beyond the spread: %s   first pass within the bar: %s"
                     % (c < a * (1 - spread), c < b * (1 - spread), c1 <= 1.03 * d1))
    for pl in (small, big, first):
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--burst", type=int, default=5)
    a = ap.parse_args()
    lines = ["coset LDE A/B  (tools/bench_lde.py; library %s; ntt_lde %s)" % (LIBNAME, "present" if hasattr(_lib.lib(), "ntt_lde") else "ABSENT: legs A and D only"),
             "GPU: %s   kernel-source hash: %s" % (torch.cuda.get_device_name(0), _lib.kernel_source_hash()),
             "%d bursts of %d launches per leg, median per launch; all legs produce the same words (checked)" % (a.repeats, a.burst)]
    for shape in SHAPES:
        run_shape(*shape, a.repeats, a.burst, lines)
    lines.insert(2, clocks())
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
