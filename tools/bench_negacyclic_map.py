#!/usr/bin/env python3
"""A/B of the blind-rotation step -- X^e_r . ACC - ACC, its gadget digits, the products with a broadcast b^ and ACC added back -- one
process on one MI355X, kind-2 tables made on the device, 2 polynomials, 3 levels, 2 outputs, the monomial with one device exponent per
row and NTT_MAP_MINUS_IDENTITY, addend = a:

  A   ntt_polymul_gadget_map_pre: the map and the digits in one launch a -> work, the matrix-vector product of work, the accumulate
  B   ntt_negacyclic_map a -> mapped, then ntt_polymul_gadget_pre of mapped, both in the same library, then the accumulate through the
      same kernel as leg A's (the experiment build exports that launch alone, ntt_add_rows_exp: the same source).  Where the plan has
      digit kernels (ntt_plan_info 15: the general 64-bit modulus) B's product decomposes inside its middle launch and may win

Before any time is printed every word of leg A's output is compared with leg B's, and a with its copy.  The legs run interleaved:
ROUNDS rounds, in each one burst of K launches per leg between two events; the table gives the median per launch and min .. max over
the bursts.  No routing decision depends on the outcome, and no ratio is fixed in advance.
usage: python tools/bench_negacyclic_map.py [--out profiles/negacyclic_map_ab.txt] [--rounds 7] [--k 3] [--shapes i ...]"""
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
SHAPES = [("Goldilocks 2^12, batch 4096", 12, GOLD, 7, 8, 4096, (8, 3, 40)),
          ("general 64-bit modulus 0x3FFFFFEE00000001, 2^12, batch 4096", 12, M64, 3, 8, 4096, (10, 3, 32)),
          ("31-bit prime 2013265921, 2^12, batch 8192", 12, 2013265921, 31, 4, 8192, (8, 3, 6))]


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


def run_shape(L, L_exp, name, logn, p, g, wb, batch, dig, rounds, k, lines):
    n = 1 << logn
    w, K, l = dig
    terms = POLYS * K
    h, h_exp = make_plan(L, logn, p, wb, g), make_plan(L_exp, logn, p, wb, g)
    gen = torch.Generator(device="cuda:0").manual_seed(5)
    tdt = torch.int32 if wb == 4 else torch.int64

    def rnd(*shape):  # canonical words: any are a valid operand
        return torch.randint(0, min(p, 1 << 62), shape, dtype=torch.int64, device="cuda:0", generator=gen).to(tdt)

    a = rnd(POLYS, batch, n)
    bhat = rnd(OUTS, terms, 1, n)
    exps = torch.randint(0, 2 * n, (batch,), dtype=torch.int64, device="cuda:0", generator=gen).to(torch.int32)  # one exponent per row, as from an LWE mask
    work = torch.empty((terms, batch, n), dtype=tdt, device="cuda:0")
    mapped = torch.empty((POLYS, batch, n), dtype=tdt, device="cuda:0")
    out_a, out_b = torch.empty((OUTS, batch, n), dtype=tdt, device="cuda:0"), torch.empty((OUTS, batch, n), dtype=tdt, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    MONO, MI = _lib.NTT_MAP_MONOMIAL, _lib.NTT_MAP_MINUS_IDENTITY

    def leg_a():
        assert L.ntt_polymul_gadget_map_pre(h, a.data_ptr(), POLYS, MONO, 0, exps.data_ptr(), MI, w, K, l, work.data_ptr(), bhat.data_ptr(), 1, OUTS, a.data_ptr(),
                                            out_a.data_ptr(), batch, st) == 0

    def leg_b():
        assert L.ntt_negacyclic_map(h, a.data_ptr(), mapped.data_ptr(), POLYS, batch, MONO, 0, exps.data_ptr(), MI, st) == 0
        assert L.ntt_polymul_gadget_pre(h, mapped.data_ptr(), POLYS, w, K, l, work.data_ptr(), bhat.data_ptr(), 1, OUTS, out_b.data_ptr(), batch, st) == 0
        assert L_exp.ntt_add_rows_exp(h_exp, out_b.data_ptr(), a.data_ptr(), OUTS * batch, st) == 0

    fused = L.ntt_plan_info(h, 15) == 1
    legs = [("A  gadget_map_pre (map + digits in one launch, addend)", leg_a),
            ("B  negacyclic_map + gadget_pre%s + the same add kernel" % (" (digits inside its middle launch)" if fused else ""), leg_b)]
    # the words, before any time is taken
    keep = a.clone()
    out_a.zero_()
    out_b.fill_(1)
    leg_a()
    leg_b()
    torch.cuda.synchronize()
    assert torch.equal(out_a, out_b), "the fused call and the separate calls differ"
    assert torch.equal(a, keep), "a was written"
    del keep
    ms = {nm: [] for nm, _ in legs}
    for _ in range(rounds):
        for nm, fn in legs:
            ms[nm].append(burst(fn, k))
    lines.append("")
    lines.append("%s, broadcast b^, %d polynomials, digits (log_base %d, levels %d, low_bits %d), %d outputs, per-row exponents, minus identity, addend = a"
                 % (name, POLYS, w, K, l, OUTS))
    for nm, _ in legs:
        v = ms[nm]
        lines.append("  %-78s %9.4f ms (min %9.4f .. max %9.4f)" % (nm, statistics.median(v), min(v), max(v)))
    va, vb = (ms[nm] for nm, _ in legs)
    lines.append("  A / B = %.3f (medians); A max < B min: %s; B max < A min: %s.  Derived, not measured: where B runs the decomposition kernel A saves 2 P N = %d N "
                 "words per row (%.0f MB) and one launch" % (statistics.median(va) / statistics.median(vb), max(va) < min(vb), max(vb) < min(va), 2 * POLYS,
                                                            2 * POLYS * n * batch * wb / 1e6))
    L.ntt_plan_destroy(h)
    L_exp.ntt_plan_destroy(h_exp)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--shapes", type=int, nargs="*", help="indices into SHAPES (default: all)")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.open_library(os.path.join(ROOT, "ntt_aie_amd", "libntt_hip.so"))
    L_exp = _lib.open_library(os.path.join(ROOT, "ntt_aie_amd", "libntt_hip_exp.so"))
    L_exp.ntt_add_rows_exp.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    lines = ["blind-rotation step: the fused map + digits against the separate map, A/B  (tools/bench_negacyclic_map.py)",
             "GPU: %s   kernel-source hash: %s" % (torch.cuda.get_device_name(0), _lib.kernel_source_hash()),
             "%d interleaved rounds, one burst of %d launches per leg and round, median per launch; every word of the two legs' outputs agrees (checked)"
             % (args.rounds, args.k)]
    for i, (name, logn, p, g, wb, batch, dig) in enumerate(SHAPES):
        if args.shapes is None or i in args.shapes:
            run_shape(L, L_exp, name, logn, p, g, wb, batch, dig, args.rounds, args.k, lines)
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
