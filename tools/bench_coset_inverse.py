#!/usr/bin/env python3
"""A/B/C of the coset interpolation, one process on one MI355X (the experiment build, tools/_explib.py):

  A  ntt_coset_inverse, the vector sweep fused into the inverse's last pass
  B  the same through the separate row-scaling kernel (NTT_COSET_INV_UNFUSED=1, an experiment-build knob read at plan creation)
  C  plain ntt_inverse(scale = 1) of that shape: on THIS build, and -- with --parent-lib PATH, a libntt_hip.so built from the
     parent commit -- on the parent's library as well (opened beside this one; the pass kernels of both are the same code)

Shapes: Goldilocks 2^19 at batch 512, Goldilocks 2^16 at batch 4096, a 31-bit prime 2^15 at batch 8192.  Each leg: warm-up, then
REPEATS timed bursts of BURST launches between two events; the table gives the median per launch and the min .. max over the bursts.
Decision rule per word class: the fused path ships only if A's burst maximum is below B's burst minimum at every shape of the class.
usage: python tools/bench_coset_inverse.py [--out profiles/coset_inverse_ab.txt] [--repeats 9] [--burst 5] [--parent-lib PATH]"""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _explib  # noqa: E402

LIBNAME = _explib.select()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_lde import clocks, plan_with_env, timed  # noqa: E402
from ntt_aie_amd import _lib  # noqa: E402
from ntt_aie_amd.plan import to_device  # noqa: E402

SHAPES = [("Goldilocks 2^19, batch 512", "8-byte words", 19, 0xFFFFFFFF00000001, 7, 8, 512),
          ("Goldilocks 2^16, batch 4096", "8-byte words", 16, 0xFFFFFFFF00000001, 7, 8, 4096),
          ("p = 2013265921 (31 bit) 2^15, batch 8192", "4-byte words", 15, 2013265921, 31, 4, 8192)]


class ParentPlan:
    """ntt_inverse of another build of the C-ABI (the parent commit's), through its own handle"""

    def __init__(self, path, logn, p, wb, g):
        self.L = _lib.open_library(path)
        self.h = C.c_void_p()
        assert self.L.ntt_plan_create(C.byref(self.h), logn, p, wb, 0) == 0
        assert self.L.ntt_plan_generate_twiddles(self.h, 1, g) == 0

    def inverse(self, x, out):
        rc = self.L.ntt_inverse(self.h, x.data_ptr(), out.data_ptr(), x.shape[0], 0, 1, torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc

    def close(self):
        self.L.ntt_plan_destroy(self.h)


def run_shape(name, cls, logm, p, g, wb, batch, repeats, burst, parent_lib, lines, verdict):
    m = 1 << logm
    dt = np.uint32 if wb == 4 else np.uint64
    rng = np.random.default_rng(1)
    evals = to_device((rng.integers(0, 2**63, size=(batch, m), dtype=np.uint64) % np.uint64(p)).astype(dt), "cuda:0")
    out = torch.empty_like(evals)
    fused = plan_with_env(logm, p, wb, g)
    unf = plan_with_env(logm, p, wb, g, NTT_COSET_INV_UNFUSED=1)
    for pl in (fused, unf):
        pl.set_coset_inverse(g)
    assert fused.coset_inverse_fused and not unf.coset_inverse_fused
    res = {}
    res["A coset_inverse, fused last pass"] = timed(lambda: fused.coset_inverse(evals, out), repeats, burst)
    ref = out.clone()
    res["B coset_inverse, separate scaling"] = timed(lambda: unf.coset_inverse(evals, out), repeats, burst)
    assert torch.equal(out, ref), "B differs from A"
    res["C inverse(scale=1), this build"] = timed(lambda: fused.inverse(evals, out), repeats, burst)
    if parent_lib:
        par = ParentPlan(parent_lib, logm, p, wb, g)
        inv_here = out.clone()
        res["C inverse(scale=1), parent build"] = timed(lambda: par.inverse(evals, out), repeats, burst)
        assert torch.equal(out, inv_here), "the parent's inverse differs"
        par.close()
    lines.append("")
    lines.append("%s   passes %s" % (name, [st for _, _, st in fused.passes_for(batch)]))
    for k, (med, lo, hi) in res.items():
        lines.append("  %-36s %9.4f ms   (min %9.4f .. max %9.4f, %+5.1f %%)" % (k, med, lo, hi, 100 * (hi - lo) / med))
    a, b = res["A coset_inverse, fused last pass"], res["B coset_inverse, separate scaling"]
    c = res.get("C inverse(scale=1), parent build", res["C inverse(scale=1), this build"])
    lines.append("  A / B = %.3f   A / C = %.3f   B / C = %.3f   C's own burst spread %.1f %%" % (a[0] / b[0], a[0] / c[0], b[0] / c[0], 100 * (c[2] - c[1]) / c[0]))
    ok = a[2] < b[1]
    lines.append("  A's burst maximum below B's burst minimum: %s   A exceeds C by more than C's spread: %s" % (ok, a[0] - c[0] > c[2] - c[1]))
    verdict[cls] = verdict.get(cls, True) and ok
    for pl in (fused, unf):
        pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--burst", type=int, default=5)
    ap.add_argument("--parent-lib")
    a = ap.parse_args()
    lines = ["coset interpolation A/B/C  (tools/bench_coset_inverse.py; library %s; parent library %s)" % (LIBNAME, "given" if a.parent_lib else "not given"),
             "GPU: %s   kernel-source hash: %s" % (torch.cuda.get_device_name(0), _lib.kernel_source_hash()),
             "%d bursts of %d launches per leg, median per launch; A and B produce the same words (checked)" % (a.repeats, a.burst)]
    verdict = {}
    for shape in SHAPES:
        run_shape(*shape, a.repeats, a.burst, a.parent_lib, lines, verdict)
    lines.append("")
    for cls, ok in verdict.items():
        lines.append("decision, %s: the fused path %s (A max < B min at every shape of the class: %s)" % (cls, "ships" if ok else "does NOT clear the rule", ok))
    lines.insert(2, clocks())
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
