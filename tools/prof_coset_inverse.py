#!/usr/bin/env python3
"""Driver for a per-kernel profile of the coset interpolation (profiles/coset_inverse_kernel_stats.csv): 20 fused ntt_coset_inverse
and 20 plain scaled ntt_inverse calls at Goldilocks 2^16 x 4096 and at a 31-bit prime 2^15 x 8192, so that the twin kernel
(PassCfg<..., true>) stands beside the scaled kernel it replaces in one table.  Run it under the profiler, in a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o coset_inverse -- python tools/prof_coset_inverse.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _explib  # noqa: E402

_explib.select()

import numpy as np  # noqa: E402
import torch  # noqa: E402

from ntt_aie_amd.plan import NTTPlan, to_device  # noqa: E402

SHAPES = [(16, 0xFFFFFFFF00000001, 7, 8, 4096), (15, 2013265921, 31, 4, 8192)]


def main():
    for logm, p, g, wb, batch in SHAPES:
        pl = NTTPlan(logm, p, wb, 0)
        pl.generate_twiddles(1, g)
        pl.set_coset_inverse(g)
        dt = np.uint32 if wb == 4 else np.uint64
        x = to_device((np.random.default_rng(1).integers(0, 2**63, size=(batch, 1 << logm), dtype=np.uint64) % np.uint64(p)).astype(dt), "cuda:0")
        out = torch.empty_like(x)
        for _ in range(20):
            pl.coset_inverse(x, out)
            pl.inverse(x, out)
        torch.cuda.synchronize()
        pl.close()


if __name__ == "__main__":
    main()
