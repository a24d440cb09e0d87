"""Row-major matrix batches without a GPU: the virtual-polynomial claim the header makes (a Python-integer model, no library), the
matrix twin of the column pass in the host index model against the oracle on the transposed columns, the planner's decomposition,
the launcher's refusals, and the part of the error contract that is reported before any launch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

GOLD = 0xFFFFFFFF00000001
CLASSES = {"gl": (8, GOLD, 7), "m64": (8, 0xFFFFFFFC00000001, 10), "m32": (4, 998244353, 3)}


def _network(a, T, p):
    """include/ntt_hip.h: stage s = 0.., stride 2^s, (x, y) -> (x + y, (x - y) * T[n / 2^(s+1) + block])"""
    a, n = list(a), len(a)
    t = 1
    while t < n:
        h = n // (2 * t)
        for i in range(h):
            for j in range(2 * i * t, 2 * i * t + t):
                x, y = a[j], a[j + t]
                a[j], a[j + t] = (x + y) % p, (x - y) * T[h + i] % p
        t *= 2
    return a


def _virtual_stages(a, logn, w, T, p):
    """stages w .. w + logn - 1 of the size-2^(logn + w) network on `a`, every twiddle taken from the size-2^logn table T at the
    index the column pass forms: T[2^(logn - s - 1) + (j >> (w + s + 1))] for stage w + s"""
    a = list(a)
    big = 1 << (logn + w)
    assert len(a) == big
    for s in range(logn):
        t = 1 << (w + s)
        blocks = big // (2 * t)
        assert blocks == 1 << (logn - s - 1)
        for i in range(blocks):
            for j in range(2 * i * t, 2 * i * t + t):
                assert j >> (w + s + 1) == i
                x, y = a[j], a[j + t]
                a[j], a[j + t] = (x + y) % p, (x - y) * T[blocks + i] % p
    return a


@pytest.mark.parametrize("p,g", [(3329, 3), (998244353, 3), (GOLD, 7)])
def test_a_padded_matrix_is_one_virtual_polynomial(p, g):
    """the claim of include/ntt_hip.h: on the matrix [N][2^w] read as one polynomial of 2^(logn + w) words, stages w .. w + logn - 1
    with the size-N table are the per-column networks; logn 1..5, w 0..3, any table (random words, not even roots)"""
    rng = np.random.default_rng(21)
    for logn in range(1, 6):
        n = 1 << logn
        T = [int(v) % p for v in rng.integers(0, 2**62, size=n)]
        for w in range(4):
            cols = 1 << w
            mat = [[int(v) % p for v in rng.integers(0, 2**62, size=cols)] for _ in range(n)]
            mat[0][0], mat[-1][-1] = p - 1, 0
            flat = [mat[r][c] for r in range(n) for c in range(cols)]
            got = _virtual_stages(flat, logn, w, T, p)
            for c in range(cols):
                want = _network([mat[r][c] for r in range(n)], T, p)
                assert [got[r * cols + c] for r in range(n)] == want, (logn, w, c)


def test_plan_column_passes():
    """plan.h: plan_column_passes for logn 4..24: every pass has 4..8 stages, the stages are contiguous and sum to logn, the pass
    count is ceil(logn / 8), the split is even with the longer passes first; nothing below four stages"""
    import emu_columns_lib as E

    for logn in range(0, 4):
        assert E.column_passes(logn) == []
    for logn in range(4, 25):
        passes = E.column_passes(logn)
        assert len(passes) == -(-logn // 8), logn
        s = 0
        for s0, m in passes:
            assert s0 == s and 4 <= m <= 8, (logn, passes)
            s += m
        assert s == logn
        sizes = [m for _, m in passes]
        assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True), (logn, passes)
    assert [m for _, m in E.column_passes(16)] == [8, 8]
    assert [m for _, m in E.column_passes(12)] == [6, 6]
    assert [m for _, m in E.column_passes(10)] == [5, 5]
    assert [m for _, m in E.column_passes(17)] == [6, 6, 5]
    assert [m for _, m in E.column_passes(9)] == [5, 4]


def test_the_launcher_refuses_what_it_should():
    """launch.h: fill_pass_args refuses a MAT twin without its three arguments and the arguments on any other configuration (plain
    column, CONTIG), width > pitch, a scaled launch outside the pass that holds stage 0, a matrix beyond 2^28 words; it accepts the
    matching pair; and pass_dispatch -- an ordinary launch's rule -- never names a MAT kernel"""
    import emu_columns_lib as E

    assert E.lib().emu_columns_refusals() == 63


def test_the_launcher_takes_the_size_limit_at_equality():
    """launch.h: fill_pass_args accepts a matrix of exactly 2^28 words and a virtual polynomial of exactly 2^28 words (logn 20: pitch
    256; 129 columns) and refuses one step beyond either (pitch 257; 257 columns): both sides of the boundary on one shape"""
    import emu_columns_lib as E

    assert E.lib().emu_columns_limit() == 15


def _sweep_cases():
    for logn in (4, 5, 8, 9, 10, 12):
        for width in (1, 3, 16, 17, 33):
            p2 = 1 << (width - 1).bit_length()
            for pitch in (width, width + 1, p2 + 16):
                for count in (1, 3):
                    yield logn, width, pitch, count, (0, 1, 2)


def _three_pass_cases():
    """(logn, width, pitch, count, modes): logn 17 = 6 + 6 + 5 -- the middle pass is the only launch with several hi blocks, a first
    stage above mat_w and a row stride above 1 at once, and the only one that neither reads the caller's input nor holds stage 0 --
    and one forward case of logn 18 = 6 + 6 + 6"""
    for width in (1, 17):
        for pitch in (width, width + 1):
            yield 17, width, pitch, 1, (0, 1, 2)
    yield 18, 1, 1, 1, (0,)


@pytest.mark.parametrize("cls", sorted(CLASSES))
def test_columns_in_the_host_model(oracle, cls):
    """pass.h's PassCfg::MAT kernels stepped on the host (tests/emu/emu_columns.cpp, LDS hazard tracker on) through mat_dispatch /
    pass_geometry_of / fill_pass_args over plan_column_passes: forward, scaled and unscaled inverse x logn {4, 5, 8, 9, 10, 12} x
    width {1, 3, 16, 17, 33} x pitch {width, width + 1, next power of two + 16} x count {1, 3}, then the three-pass shapes of
    _three_pass_cases; in place and out of place, ppw 1 and > 1; buffers of exactly (count * N - 1) * pitch + width words; every live
    word is the oracle's transform of its column, every padding word keeps its sentinel (>= p: junk on the input side)"""
    import emu_columns_lib as E

    L = E.lib()
    wb, p, g = CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    sent = np.iinfo(dt).max - 10
    assert sent >= p
    rng = np.random.default_rng(31)
    tables, case = {}, 0
    for logn, width, pitch, count, modes in list(_sweep_cases()) + list(_three_pass_cases()):
        n = 1 << logn
        if logn not in tables:
            tables[logn] = oracle.make_table(1, n, p, g, wb)
        T = tables[logn]
        assert len(E.column_passes(logn)) == (3 if logn >= 17 else 2 if logn >= 9 else 1)
        words = (count * n - 1) * pitch + width
        x = (rng.integers(0, 2**63, size=(count, n, width), dtype=np.uint64) % np.uint64(p)).astype(dt)
        x[0, 0, 0], x[-1, -1, -1] = p - 1, 0
        cols = np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(count * width, n)
        fwd = oracle.ntt(cols, T, p)
        inv = oracle.intt(cols, T, p) if modes != (0,) else None
        unscaled = oracle.pointwise(inv, np.full_like(inv, n % p), p) if modes != (0,) else None
        live = np.zeros(count * n * pitch, dtype=bool).reshape(count * n, pitch)
        live[:, :width] = True
        live = live.reshape(-1)[:words]
        for mode, want_cols in ((0, fwd), (1, inv), (2, unscaled)):
            if mode not in modes:
                continue
            want = np.ascontiguousarray(want_cols.reshape(count, width, n).transpose(0, 2, 1))
            in_place = bool(case & 1)
            target = 2 if case & 2 else 16384
            case += 1
            a = np.full(words, sent, dtype=dt)
            a[live] = x.reshape(-1)
            a0 = a.copy()
            out = a if in_place else np.full(words, sent - 1, dtype=dt)
            rc = L.emu_columns(wb, logn, p, T.ctypes.data, a.ctypes.data, out.ctypes.data, width, pitch, count, int(mode != 0), int(mode == 1), target)
            key = (cls, logn, width, pitch, count, mode, in_place, target)
            assert rc == 0, key
            assert np.array_equal(out[live], want.reshape(-1)), key
            assert np.all(out[~live] == (sent if in_place else sent - 1)), key  # padding of the output keeps its contents
            if not in_place:
                assert np.array_equal(a, a0), key  # the input is read only
    assert case == 6 * 5 * 3 * 2 * 3 + 2 * 2 * 3 + 1
    # 16 matrices per workgroup (logn 4), several groups per workgroup, a ragged last group
    n, width, pitch, count = 16, 5, 7, 3 * 16 + 1
    T = oracle.make_table(1, n, p, g, wb)
    x = (rng.integers(0, 2**63, size=(count, n, width), dtype=np.uint64) % np.uint64(p)).astype(dt)
    want = oracle.ntt(np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, n), T, p).reshape(count, width, n).transpose(0, 2, 1)
    buf = np.full((count * n, pitch), sent, dtype=dt)
    buf[:, :width] = x.reshape(count * n, width)
    flat = buf.reshape(-1)[: (count * n - 1) * pitch + width].copy()
    assert L.emu_columns(wb, 4, p, T.ctypes.data, flat.ctypes.data, flat.ctypes.data, width, pitch, count, 0, 0, 2) == 0
    got = np.concatenate([flat, np.full(pitch - width, sent, dtype=dt)]).reshape(count * n, pitch)
    assert np.array_equal(got[:, :width].reshape(count, n, width), want) and np.all(got[:, width:] == sent)


def test_error_contract_without_a_device():
    """every NTT_E_* case of the two entry points that is reported before a launch and needs no plan on a device; the binding, the
    header and the info codes agree"""
    from ntt_aie_amd import _lib

    L = _lib.lib()
    assert {"ntt_forward_columns", "ntt_inverse_columns"} <= set(_lib.EXPORTS)
    assert len(L.ntt_forward_columns.argtypes) == 7 and len(L.ntt_inverse_columns.argtypes) == 8
    assert L.ntt_forward_columns(None, None, None, 1, 1, 1, None) == _lib.NTT_E_ARG
    assert L.ntt_inverse_columns(None, None, None, 1, 1, 1, 1, None) == _lib.NTT_E_ARG
    assert L.ntt_forward_columns(None, None, None, 0, 0, 0, None) == _lib.NTT_E_ARG  # no plan: not even an empty batch
    assert L.ntt_version() >= 500
    assert L.ntt_error_string(-11) == b"unknown error"  # existing codes only
    hdr = open(os.path.join(ROOT, "include", "ntt_hip.h")).read()
    assert re.search(r"int ntt_forward_columns\(ntt_plan_t plan, const void \*d_in, void \*d_out, size_t width, size_t pitch, size_t count, void \*stream\);", hdr)
    assert re.search(r"int ntt_inverse_columns\(ntt_plan_t plan, const void \*d_in, void \*d_out, size_t width, size_t pitch, size_t count, int scale,\s+void \*stream\);", hdr)
    for text in (r"\(count \* N - 1\) \* pitch \+ width words is sufficient", r"13 number of passes of the columns decomposition", r"96 \+ i: stages in pass i",
                 r"128 \+ i: first stage of pass i", r"N \* pitch <= 2\^NTT_MAX_LOGN words and logn \+ w <= NTT_MAX_LOGN", r"multiple of 128 bytes"):
        assert re.search(text, hdr), text
    import ntt_aie_amd as eng

    for name in ("forward_columns", "inverse_columns", "column_passes"):
        assert hasattr(eng.NTTPlan, name)


def _library_column_target():
    """the workgroup count the library sizes its column launches for: the initialiser of target_wgs_col in the plan facts (sequence.h)"""
    src = open(os.path.join(ROOT, "ntt_aie_amd", "csrc", "sequence.h")).read()
    m = re.search(r"^\s*uint32_t\s+target_wgs_col\s*=\s*([0-9][0-9\s*]*);", src, re.M)
    assert m, "the initialiser of target_wgs_col was not found in sequence.h"
    target = 1
    for f in m.group(1).split("*"):
        target *= int(f)
    return target


def test_gpu_loop_shapes_do_loop():
    """tests/test_gpu_columns_large.py's LOOP_SHAPES exist to run the batch loop of the matrix kernels on hardware.  With launch.h's own
    mat_dispatch / pass_geometry_of (emu_columns_geometry) at the library's own column target, every pass of every such shape, in
    every word class and direction, streams two groups or more per workgroup (ppw >= 2), is tapered over at least two levels, and its
    count fills neither the last workgroup (a multiple of 2^log_up; where a workgroup holds several matrices at all) nor the last row
    of the batch loop (a multiple of ppw << log_up): a change of the target or of the tile shapes cannot quietly take the GPU test
    back to ppw == 1"""
    import emu_columns_lib as E
    from test_gpu_columns_large import LOOP_SHAPES

    target = _library_column_target()
    assert target >= 2
    assert len(LOOP_SHAPES) >= 2 and {len(E.column_passes(s[0])) for s in LOOP_SHAPES} >= {1, 2}
    several_per_workgroup = False
    for logn, width, pitch, count in LOOP_SHAPES:
        for cls, (wb, p, g) in dict(CLASSES, kyber=(4, 3329, 3)).items():
            for k in range(len(E.column_passes(logn))):
                for inverse in (False, True):
                    geo = E.geometry(wb, p, logn, width, pitch, count, target, k, inverse)
                    key = (logn, width, pitch, count, cls, k, inverse, geo)
                    assert geo["ppw"] >= 2, key
                    assert sum(1 for r in geo["taper"] if r) >= 2 and sum(geo["taper"]) == geo["grid_y"], key
                    assert count % (geo["ppw"] << geo["log_up"]) != 0, key
                    if geo["log_up"] > 0:  # (a matrix of two passes never shares its workgroup: every count is a multiple of 2^0)
                        assert count % (1 << geo["log_up"]) != 0, key
                        several_per_workgroup = True
                    assert geo["grid_y"] <= 65535, key  # one launch: the slicing path is not what these shapes are about
    assert several_per_workgroup
