#!/usr/bin/env python3
"""A/B of the prepared products with the balanced gadget decomposition fused in, one process on one MI355X, kind-2 tables made on the
device, 2 polynomials, 3 levels and 2 outputs (a TFHE external product), per row and broadcast:

  A   ntt_polymul_gadget_pre of this tree: where the plan has digit kernels (ntt_plan_info 15) the middle launches alone, reading a
      and decomposing in registers.  Where the product library does not use them for the class (launch.h: product_gadget_unit) the leg
      runs on the experiment build, which keeps them, and the table says so
  B   ntt_gadget_decompose + ntt_polymul_matvec_pre in the same library: the decomposition kernel writes polys * levels * batch * N words,
      the product reads them back
  C   ntt_polymul_matvec_pre alone on pre-made digits, on the PARENT commit's library (--parent-lib): shows that the existing path did
      not move, and is a lower bound for B.  It overwrites its operand, so it is timed WITH one device-to-device copy of the digits; the
      copy is timed alone in the same rounds and the table gives the raw figure and the one with the copy subtracted

Before any time is printed, sampled rows of every output of legs A and B are compared word for word with leg C's.  The legs run
interleaved: ROUNDS rounds, in each one burst of K launches per leg between two events; the table gives the median per launch and
min .. max over the bursts.
The rule the table serves (per word class): the product library uses the digit kernels for a class only if the
burst maximum of leg A is below the burst minimum of leg B at every shape of the class.
usage: python tools/bench_polymul_gadget.py --parent-lib PATH [--out profiles/polymul_gadget_ab.txt] [--rounds 7] [--k 3] [--shapes i ...]"""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from ntt_aie_amd import _lib  # noqa: E402

GOLD = 0xFFFFFFFF00000001
M64 = 0x3FFFFFEE00000001
POLYS, OUTS = 2, 2
# (name, logn, p, g, word bytes, batch, (log_base, levels, low_bits))
SHAPES = ([("Goldilocks 2^%d, batch 4096" % n, n, GOLD, 7, 8, 4096, (8, 3, 40)) for n in (10, 11, 12)] +
          [("31-bit prime 2013265921, 2^%d, batch 8192" % n, n, 2013265921, 31, 4, 8192, (8, 3, 6)) for n in (10, 11, 12)] +
          [("general 64-bit modulus 0x3FFFFFEE00000001, 2^%d, batch 4096" % n, n, M64, 3, 8, 4096, (10, 3, 32)) for n in (11, 12)])


def burst(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def make_plan(L, logn, p, wb, g):
    h = C.c_void_p()
    assert L.ntt_plan_create(C.byref(h), logn, p, wb, 0) == 0
    assert L.ntt_plan_generate_twiddles(h, 2, g) == 0
    return h


def run_shape(libs, name, logn, p, g, wb, batch, dig, bcast, rounds, k, lines):
    n = 1 << logn
    w, K, l = dig
    terms = POLYS * K
    L_tree, L_exp, L_parent = libs
    h_tree, h_c = make_plan(L_tree, logn, p, wb, g), make_plan(L_parent, logn, p, wb, g)
    shipped = L_tree.ntt_plan_info(h_tree, 15) == 1
    L_a, h_a = (L_tree, h_tree) if shipped else (L_exp, make_plan(L_exp, logn, p, wb, g))
    assert L_a.ntt_plan_info(h_a, 15) == 1, "no digit kernel for this shape in either build"
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    tdt = torch.int32 if wb == 4 else torch.int64

    def rnd(*shape):  # canonical words: any are a valid operand
        return torch.randint(0, min(p, 1 << 62), shape, dtype=torch.int64, device="cuda:0", generator=gen).to(tdt)

    rows = 1 if bcast else batch
    x = rnd(POLYS, batch, n)
    bhat = rnd(OUTS, terms, rows, n)
    work, digits = torch.empty((terms, batch, n), dtype=tdt, device="cuda:0"), torch.empty((terms, batch, n), dtype=tdt, device="cuda:0")
    out = torch.empty((OUTS, batch, n), dtype=tdt, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    assert L_tree.ntt_gadget_decompose(h_tree, x.data_ptr(), POLYS, batch, w, K, l, digits.data_ptr(), st) == 0  # leg C's pre-made digits

    def leg_a():
        assert L_a.ntt_polymul_gadget_pre(h_a, x.data_ptr(), POLYS, w, K, l, work.data_ptr(), bhat.data_ptr(), rows, OUTS, out.data_ptr(), batch, st) == 0

    def leg_b():
        assert L_tree.ntt_gadget_decompose(h_tree, x.data_ptr(), POLYS, batch, w, K, l, work.data_ptr(), st) == 0
        assert L_tree.ntt_polymul_matvec_pre(h_tree, work.data_ptr(), bhat.data_ptr(), rows, terms, OUTS, out.data_ptr(), batch, st) == 0

    def leg_c():
        work.copy_(digits)
        assert L_parent.ntt_polymul_matvec_pre(h_c, work.data_ptr(), bhat.data_ptr(), rows, terms, OUTS, out.data_ptr(), batch, st) == 0

    def copy():
        work.copy_(digits)

    legs = [("A  gadget_pre" + ("" if shipped else " (EXPERIMENT build: not shipped for this class)"), leg_a, 0),
            ("B  gadget_decompose + matvec_pre", leg_b, 0), ("C  matvec_pre on pre-made digits, parent library", leg_c, 1)]
    # the words, before any time is taken: sampled rows of every output of legs A and B against leg C's
    sample = sorted({0, batch // 2, batch - 1})
    keep = x.clone()
    leg_c()
    want = out[:, sample].clone()
    for nm, fn, _ in legs[:2]:
        out.zero_()
        fn()
        assert torch.equal(out[:, sample], want), nm + " differs from the matrix-vector product of the digits on the parent library"
    assert torch.equal(x, keep), "a was written"
    for _, fn, _ in legs:
        fn()
    torch.cuda.synchronize()
    ms = {nm: [] for nm, _, _ in legs}
    cp = []
    for _ in range(rounds):
        for nm, fn, _ in legs:
            ms[nm].append(burst(fn, k))
        cp.append(burst(copy, k))
    lines.append("")
    lines.append("%s, %s, %d polynomials, digits (log_base %d, levels %d, low_bits %d), %d outputs"
                 % (name, "broadcast (one prepared row per output and term)" if bcast else "per row", POLYS, w, K, l, OUTS))
    c_med = statistics.median(cp)
    lines.append("  copy of the %d blocks of digits alone: %.4f ms (median)" % (terms, c_med))
    for nm, _, copies in legs:
        v = ms[nm]
        net = [t - copies * c_med for t in v]
        lines.append("  %-62s raw %9.4f ms (min %9.4f .. max %9.4f)%s"
                     % (nm, statistics.median(v), min(v), max(v),
                        "   less the copy %9.4f ms (min %9.4f .. max %9.4f)" % (statistics.median(net), min(net), max(net)) if copies else ""))
    a, b, c = (ms[nm] for nm, _, _ in legs)
    ok = max(a) < min(b)
    words = lambda f: f * n * batch * wb / 1e6  # noqa: E731
    lines.append("  A max < B min: %s   A / B = %.3f (medians).  Derived, not measured, broadcast b^: (P + J) N = %d N words against (P + 2 P K + J) N = %d N per row "
                 "(%.0f MB against %.0f MB), ratio %.3f%s"
                 % (ok, statistics.median(a) / statistics.median(b), POLYS + OUTS, POLYS + 2 * terms + OUTS, words(POLYS + OUTS), words(POLYS + 2 * terms + OUTS),
                    (POLYS + OUTS) / (POLYS + 2 * terms + OUTS), "" if bcast else "; per row b^ adds J P K N words to both"))
    for L, h in ((L_tree, h_tree), (L_parent, h_c)) + (() if shipped else ((L_exp, h_a),)):
        L.ntt_plan_destroy(h)
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True, help="libntt_hip.so built from the parent commit")
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="*", help="indices into SHAPES (default: all)")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    tree = os.path.join(ROOT, "ntt_aie_amd", "libntt_hip.so")
    libs = (_lib.open_library(tree), _lib.open_library(os.path.join(ROOT, "ntt_aie_amd", "libntt_hip_exp.so")), _lib.open_library(os.path.abspath(a.parent_lib)))
    assert not hasattr(libs[2], "ntt_polymul_gadget_pre"), "--parent-lib has the new entry point: not the parent commit's library"
    lines = ["prepared products with the gadget decomposition fused in, A/B  (tools/bench_polymul_gadget.py)",
             "GPU: %s   kernel-source hash: %s" % (torch.cuda.get_device_name(0), _lib.kernel_source_hash()),
             "%d interleaved rounds, one burst of %d launches per leg and round, median per launch; the legs' words agree on sampled rows of every output (checked)"
             % (a.rounds, a.k)]
    verdict = {}
    for i, (name, logn, p, g, wb, batch, dig) in enumerate(SHAPES):
        if a.shapes is None or i in a.shapes:
            for bcast in (True, False):
                ok = run_shape(libs, name, logn, p, g, wb, batch, dig, bcast, a.rounds, a.k, lines)
                cls = "Goldilocks" if p == GOLD else "4-byte words" if wb == 4 else "general 64-bit modulus"
                verdict[cls] = verdict.get(cls, True) and ok
                torch.cuda.empty_cache()
    lines.append("")
    for cls, ok in verdict.items():
        lines.append("%s: leg A below leg B's burst minimum in every burst at every shape run: %s" % (cls, ok))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
