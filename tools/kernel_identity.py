#!/usr/bin/env python3
"""Are the kernels of one build the kernels of another?  Reads the gfx950 assembly hipcc leaves beside the objects
(`make -C ntt_aie_amd/csrc EXTRA=-save-temps=obj`: build/<unit>-hip-amdgcn-amd-amdhsa-gfx950.s) of two trees and, per translation
unit, matches the kernels of the first in the second by (sha256 of the instruction text, instruction lines, VGPRs, SGPRs).  The
instruction text is the function body without comments and directives, block labels renumbered -- so a kernel whose mangled name
changed (a template that gained a defaulted parameter) still matches when its code did not.
usage: python tools/kernel_identity.py <parent build dir> <branch build dir> [--list]"""
import collections
import glob
import hashlib
import os
import re
import sys


def kernels(d):
    out = {}
    for f in sorted(glob.glob(os.path.join(d, "*-hip-amdgcn-amd-amdhsa-gfx950.s"))):
        unit = os.path.basename(f).split("-hip")[0]
        name, body, cur = None, [], None
        for line in open(f):
            m = re.match(r"^(_Z\w+):", line)
            if m:
                name, body = m.group(1), []
                continue
            if name and line.startswith(".Lfunc_end"):
                out[(unit, name)] = [hashlib.sha256("\n".join(body).encode()).hexdigest()[:16], sum(1 for b in body if not b.startswith(".LBB")), None, None]
                name = None
                continue
            if name:
                code = re.sub(r"\.LBB\d+_", ".LBB_", line.split(";")[0].rstrip())
                if code.strip() and (not code.strip().startswith(".") or code.strip().startswith(".LBB")):
                    body.append(code)
                continue
            m = re.match(r"\s+\.name:\s+(_Z\w+)", line)
            if m:
                cur = m.group(1)
            for key, slot in ((".vgpr_count", 2), (".sgpr_count", 3)):
                m = re.match(r"\s+\%s:\s+(\d+)" % key, line)
                if m and (unit, cur) in out:
                    out[(unit, cur)][slot] = int(m.group(1))
    return out


def main():
    P, B = kernels(sys.argv[1]), kernels(sys.argv[2])
    print("unit                   parent  branch  identical  new   sha256 over the parent's (hash, lines, VGPRs, SGPRs) / the same found in the branch")
    for u in sorted({u for u, _ in P}):
        pb = collections.Counter(tuple(v) for (uu, _), v in P.items() if uu == u)
        bb = collections.Counter(tuple(v) for (uu, _), v in B.items() if uu == u)
        found = pb & bb
        dig = [hashlib.sha256(repr(sorted(c.items())).encode()).hexdigest()[:16] for c in (pb, found)]
        print("%-22s %6d  %6d  %9d  %3d   %s / %s" % (u, sum(pb.values()), sum(bb.values()), sum(found.values()), sum((bb - pb).values()), dig[0], dig[1]))
    if "--list" in sys.argv:
        for tag, K in (("parent", P), ("branch", B)):
            for (u, n), v in sorted(K.items()):
                print("%s %s %s lines=%d vgpr=%s sgpr=%s %s" % (tag, u, v[0], v[1], v[2], v[3], n))


if __name__ == "__main__":
    main()
