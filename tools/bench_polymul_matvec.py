#!/usr/bin/env python3
"""A/B of several prepared inner products of one operand, one process on one MI355X, kind-2 tables made on the device, K = 4 terms and
J = 2 outputs (an RLWE key switch):

  A   ntt_polymul_matvec_pre, the product library of this tree
  Ax  the same call on the experiment build of this tree (the library leg C needs: shows what the build itself costs)
  C   the same call on the experiment build with the two-output kernel switched off (NTT_MATVEC_SINGLE=1, read at plan creation): shared
      column passes, then one summed middle launch per output
  B   J calls of ntt_polymul_dot_pre on the PARENT commit's library (--parent-lib), each on a fresh copy of a: what a caller did before

Legs A, Ax and C overwrite a and are timed WITH one device-to-device copy of a; leg B needs J copies.  The copy is timed alone in the same
rounds, and the table gives the raw figure and the one with the leg's copies subtracted.  Before any time is printed, sampled rows of every
output of every leg are compared word for word with leg B's.  The legs run interleaved: ROUNDS rounds, in each one burst of K launches
per leg between two events; the table gives the median per launch and min .. max over the bursts.
The rule the table serves (per word class): the two-output kernel is used only where the burst maximum of EVERY leg
that runs it (A and Ax) is below C's burst minimum at every shape of the class.  Where the product library does not use the two-output
kernel for a class (launch.h: product_mv_unit; asked of the plan, ntt_plan_info 14), leg A runs leg C's sequence on the product library: the
table says so, A is then what the library ships, and the rule is judged on Ax alone.
usage: python tools/bench_polymul_matvec.py --parent-lib PATH [--out profiles/polymul_matvec_ab.txt] [--rounds 7] [--k 3] [--shapes i ...]"""
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
TERMS, OUTS = 4, 2
SHAPES = [("Goldilocks 2^20, batch 512", 20, GOLD, 7, 8, 512),
          ("Goldilocks 2^16, batch 4096", 16, GOLD, 7, 8, 4096),
          ("Goldilocks 2^12, batch 4096", 12, GOLD, 7, 8, 4096),
          ("31-bit prime 2013265921, 2^12, batch 8192", 12, 2013265921, 31, 4, 8192),
          ("general 64-bit modulus 0x3FFFFFEE00000001, 2^12, batch 4096", 12, 0x3FFFFFEE00000001, 3, 8, 4096)]


def burst(fn, k):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(k):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / k


def make_plan(L, logn, p, wb, g, env=None):
    for key, val in (env or {}).items():
        os.environ[key] = val
    h = C.c_void_p()
    assert L.ntt_plan_create(C.byref(h), logn, p, wb, 0) == 0
    for key in (env or {}):
        del os.environ[key]
    assert L.ntt_plan_generate_twiddles(h, 2, g) == 0
    return h


def run_shape(libs, name, logn, p, g, wb, batch, bcast, rounds, k, lines):
    n = 1 << logn
    L_tree, L_exp, L_parent = libs
    h_a, h_ax, h_b = make_plan(L_tree, logn, p, wb, g), make_plan(L_exp, logn, p, wb, g), make_plan(L_parent, logn, p, wb, g)
    h_c = make_plan(L_exp, logn, p, wb, g, {"NTT_MATVEC_SINGLE": "1"})
    gen = torch.Generator(device="cuda:0").manual_seed(3)
    tdt = torch.int32 if wb == 4 else torch.int64

    def rnd(*shape):  # canonical words: any are a valid prepared operand
        return torch.randint(0, min(p, 1 << 62), shape, dtype=torch.int64, device="cuda:0", generator=gen).to(tdt)

    rows = 1 if bcast else batch
    x = rnd(TERMS, batch, n)
    bhat = torch.stack([rnd(TERMS, rows, n) for _ in range(OUTS)])
    wa, out = torch.empty_like(x), torch.empty((OUTS, batch, n), dtype=tdt, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream

    def matvec(L, h):
        def leg():
            wa.copy_(x)
            assert L.ntt_polymul_matvec_pre(h, wa.data_ptr(), bhat.data_ptr(), rows, TERMS, OUTS, out.data_ptr(), batch, st) == 0
        return leg

    def leg_b():
        for j in range(OUTS):
            wa.copy_(x)
            assert L_parent.ntt_polymul_dot_pre(h_b, wa.data_ptr(), bhat[j].data_ptr(), rows, TERMS, out[j].data_ptr(), batch, st) == 0

    def copy():
        wa.copy_(x)

    legs = [("A  matvec_pre", matvec(L_tree, h_a), 1), ("Ax matvec_pre, experiment build", matvec(L_exp, h_ax), 1),
            ("C  matvec_pre, one summed launch per output", matvec(L_exp, h_c), 1), ("B  %d x dot_pre, parent library" % OUTS, leg_b, OUTS)]
    # the words, before any time is taken: sampled rows of every output of every leg against leg B's
    sample = sorted({0, batch // 2, batch - 1})
    leg_b()
    want = out[:, sample].clone()
    for nm, fn, _ in legs[:3]:
        out.zero_()
        fn()
        assert torch.equal(out[:, sample], want), nm + " differs from the inner products of the parent library"
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
    lines.append("%s, %s, %d terms, %d outputs" % (name, "broadcast (one prepared row per output and term)" if bcast else "per row", TERMS, OUTS))
    c_med = statistics.median(cp)
    lines.append("  copy of the %d blocks of a alone: %.4f ms (median)" % (TERMS, c_med))
    net = {}
    for nm, _, copies in legs:
        v = ms[nm]
        net[nm] = [t - copies * c_med for t in v]
        lines.append("  %-46s raw %9.4f ms (min %9.4f .. max %9.4f)   less %d cop%s %9.4f ms (min %9.4f .. max %9.4f)"
                     % (nm, statistics.median(v), min(v), max(v), copies, "y  " if copies == 1 else "ies", statistics.median(net[nm]), min(net[nm]), max(net[nm])))
    a, ax, c, b = (ms[nm] for nm, _, _ in legs)
    na, _, _, nb = (net[nm] for nm, _, _ in legs)
    a_pairs, ax_pairs = L_tree.ntt_plan_info(h_a, 14) == 1, L_exp.ntt_plan_info(h_ax, 14) == 1
    assert ax_pairs and L_exp.ntt_plan_info(h_c, 14) == 0, "the experiment build must pair in leg Ax and must not in leg C"
    ok = max(ax) < min(c) and (not a_pairs or max(a) < min(c))
    lines.append("  two-output kernel in leg A (product library): %s   A max < C min: %s   Ax max < C min: %s   the rule at this shape: %s   A / C = %.3f  Ax / C = %.3f (medians, raw)"
                 % ("yes" if a_pairs else "NO, A runs C's sequence", max(a) < min(c), max(ax) < min(c), ok, statistics.median(a) / statistics.median(c),
                    statistics.median(ax) / statistics.median(c)))
    lines.append("  A / B = %.3f with the copies, %.3f with the copies subtracted (medians).  Derived, not measured: traffic 26/38 = %.3f (26/46 = %.3f with "
                 "B's one extra copy), half-transforms 12/20 = %.3f%s" % (statistics.median(a) / statistics.median(b), statistics.median(na) / statistics.median(nb), 26 / 38, 26 / 46, 12 / 20,
                                                                          "" if 13 <= logn <= 20 and wb == 8 else "; those are the figures of a two-pass size"))
    for L, h in ((L_tree, h_a), (L_exp, h_ax), (L_exp, h_c), (L_parent, h_b)):
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
    assert not hasattr(libs[2], "ntt_polymul_matvec_pre"), "--parent-lib has the new entry point: not the parent commit's library"
    lines = ["several prepared inner products of one operand, A/B  (tools/bench_polymul_matvec.py)",
             "GPU: %s   kernel-source hash: %s" % (torch.cuda.get_device_name(0), _lib.kernel_source_hash()),
             "%d interleaved rounds, one burst of %d launches per leg and round, median per launch; the legs' words agree on sampled rows of every output (checked)"
             % (a.rounds, a.k)]
    verdict = {}
    for i, (name, logn, p, g, wb, batch) in enumerate(SHAPES):
        if a.shapes is None or i in a.shapes:
            for bcast in (False, True):
                ok = run_shape(libs, name, logn, p, g, wb, batch, bcast, a.rounds, a.k, lines)
                cls = "Goldilocks" if p == GOLD else "4-byte words" if wb == 4 else "general 64-bit modulus"
                verdict[cls] = verdict.get(cls, True) and ok
                torch.cuda.empty_cache()
    lines.append("")
    for cls, ok in verdict.items():
        lines.append("%s: every leg with the two-output kernel below C's burst minimum in every burst at every shape run: %s" % (cls, ok))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
