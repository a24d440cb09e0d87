"""The column entry points (ntt_forward_columns / ntt_inverse_columns / ntt_lde_columns / ntt_coset_inverse_columns) where the other GPU
files do not take them: three column passes (logn 17 = 6 + 6 + 5, logn 20 = 7 + 7 + 6: the only launches with a plain in-place pass in
the middle), a matrix of exactly N * pitch = 2^28 words, launches large enough for the batch loop and the taper at the library's own
workgroup target, columns of edge residues, and the plan plumbing (clone, graph capture, pinned policy, a plan shared by threads).

Every result is compared word for word with the ORACLE on the transposed columns, with the helpers of tests/test_gpu_columns.py and
tests/test_gpu_lde_columns.py: guards on both sides of every buffer, non-canonical junk in the input's padding, another sentinel in
the output's, the input read only in out-of-place calls."""
import numpy as np
import pytest

import test_gpu_columns as TC
import test_gpu_lde_columns as TL
from test_gpu_columns import ALL_CLASSES, CLASSES, GOLD, STREAM_CLASSES

pytestmark = pytest.mark.gpu

# ---- B1: three passes.  (logn, width, pitch, count); 6 + 6 + 5 with two matrices, and with w = 6 at a padded pitch; 7 + 7 + 6
THREE_PASS_SHAPES = [(17, 3, 3, 2), (17, 33, 48, 1), (20, 2, 5, 1)]
# (logm, beta, width, in_pitch, out_pitch, count): in_pitch != out_pitch, one of them odd
THREE_PASS_LDE_SHAPES = [(17, 1, 3, 3, 4, 2), (17, 4, 33, 40, 33, 1), (20, 3, 2, 5, 4, 1)]
_PLAIN_ID, _LDE_ID = (lambda s: "n%d_w%d_p%d_c%d" % s), (lambda s: "m%d_b%d_w%d_ip%d_op%d_c%d" % s)


def _three_pass_params(shapes, ident):
    """every shape for the four classes of CLASSES (ids as two stacked parametrisations give them); for the three 4-byte classes of the
    other two instruction streams the logn-17 shapes only: there the plain in-place pass in the middle runs in streams 1 and 2"""
    return ([pytest.param(cls, s, id="%s-%s" % (ident(s), cls)) for cls in sorted(CLASSES) for s in shapes]
            + [pytest.param(cls, s, id="%s-%s" % (ident(s), cls)) for cls in sorted(STREAM_CLASSES) for s in shapes if s[0] == 17])


# ---- B2: the size limit at equality: N * pitch == 2^28 words
LIMIT_LOGN, LIMIT_PITCH = 20, 256
# ---- B3: (logn, width, pitch, count) with so many matrices that, at the library's own column target, every pass streams two groups
# or more per workgroup (PassArgs::ppw >= 2: the `it * pg_stride` term of the matrix address), tapered, with a ragged count.
# tests/test_columns_cpu.py::test_gpu_loop_shapes_do_loop holds these shapes to that with the launcher's own geometry code.
#   logn 9: two passes of 2 workgroups per matrix: 2 * ceil(count / 2) >= 16384 workgroups from count 16384 on
#   logn 4: 16 matrices per workgroup: 32768 groups and one matrix more in a group of its own; the live data of the 8-byte classes
#           stays near 200 MB per buffer only with a narrow matrix, hence 2 columns at pitch 3
LOOP_SHAPES = [(9, 3, 3, 16411), (4, 2, 3, 32768 * 16 + 1)]
LOOP_LDE = {9: (1, 4, 3), 4: (3, 2, 3)}  # logn: (beta, in_pitch, out_pitch)
# ---- B4 / B5
EDGE_SHAPE = (9, 33, 40, 1)
PLUMBING_SHAPE = (13, 33, 48)


def _tdt(wb):
    import torch

    return torch.int32 if wb == 4 else torch.int64


def _fill(g, x):
    """the matrices x [count][rows][width] into the live words of the guarded buffer g"""
    import torch

    import ntt_aie_amd as eng

    g.live.copy_(eng.to_device(x, "cuda:0"))
    torch.cuda.synchronize()


def _plain_calls(pl, width, pitch, count):
    from ntt_aie_amd import _lib

    L = _lib.lib()
    return {"fwd": lambda a, b: L.ntt_forward_columns(pl._h, a, b, width, pitch, count, None),
            "inv": lambda a, b: L.ntt_inverse_columns(pl._h, a, b, width, pitch, count, 1, None),
            "invu": lambda a, b: L.ntt_inverse_columns(pl._h, a, b, width, pitch, count, 0, None)}


def _check_plain(cls, shape, ref, pl, names, out_of_place=True, in_place=True):
    """ntt_forward_columns / ntt_inverse_columns on guarded buffers against ref[name]"""
    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    logn, width, pitch, count = shape
    gin, gout = TL._Guarded(1 << logn, pitch, width, count, -3, _tdt(wb)), None
    calls = _plain_calls(pl, width, pitch, count)
    for name in names:
        if out_of_place:
            gout = gout or TL._Guarded(1 << logn, pitch, width, count, -5, _tdt(wb))
            _fill(gin, ref["x"])
            gout.live.fill_(-7)
            assert calls[name](gin.view.data_ptr(), gout.view.data_ptr()) == 0
            assert gin.intact() and gout.intact(), (cls, shape, name)
            assert np.array_equal(eng.to_host(gout.live), ref[name]), (cls, shape, name, "out of place")
            assert np.array_equal(eng.to_host(gin.live), ref["x"]), (cls, shape, name, "input is read only")
        if in_place:
            _fill(gin, ref["x"])
            assert calls[name](gin.view.data_ptr(), gin.view.data_ptr()) == 0
            assert gin.intact(), (cls, shape, name, "in place")
            assert np.array_equal(eng.to_host(gin.live), ref[name]), (cls, shape, name, "in place")


def _check_lde(cls, shape, x, want, pl):
    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    wb, p, g = ALL_CLASSES[cls]
    logm, beta, width, in_pitch, out_pitch, count = shape
    gin = TL._Guarded((1 << logm) >> beta, in_pitch, width, count, -3, _tdt(wb))
    gout = TL._Guarded(1 << logm, out_pitch, width, count, -5, _tdt(wb))
    _fill(gin, x)
    gout.live.fill_(-7)
    assert _lib.lib().ntt_lde_columns(pl._h, gin.view.data_ptr(), in_pitch, gout.view.data_ptr(), out_pitch, width, count, None) == 0
    assert gin.intact() and gout.intact(), (cls, shape)
    assert np.array_equal(eng.to_host(gin.live), x), (cls, shape, "input is read only")
    assert np.array_equal(eng.to_host(gout.live), want), (cls, shape)


def _check_cinv(cls, shape, x, want, pl, out_of_place=True, in_place=True):
    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    wb, p, g = ALL_CLASSES[cls]
    logn, width, pitch, count = shape
    call = lambda a, b: _lib.lib().ntt_coset_inverse_columns(pl._h, a, b, width, pitch, count, None)
    gin = TL._Guarded(1 << logn, pitch, width, count, -3, _tdt(wb))
    _fill(gin, x)
    if out_of_place:
        gout = TL._Guarded(1 << logn, pitch, width, count, -5, _tdt(wb))
        gout.live.fill_(-7)
        assert call(gin.view.data_ptr(), gout.view.data_ptr()) == 0
        assert gin.intact() and gout.intact(), (cls, shape)
        assert np.array_equal(eng.to_host(gin.live), x), (cls, shape, "input is read only")
        assert np.array_equal(eng.to_host(gout.live), want), (cls, shape, "out of place")
    if in_place:
        assert call(gin.view.data_ptr(), gin.view.data_ptr()) == 0
        assert gin.intact(), (cls, shape, "in place")
        assert np.array_equal(eng.to_host(gin.live), want), (cls, shape, "in place")


def _three(pl, shape):
    assert len(pl.column_passes) == 3, (shape, pl.column_passes)  # a planner change must not turn this into a two-pass test


# ---- B1 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls,shape", _three_pass_params(THREE_PASS_SHAPES, _PLAIN_ID))
def test_three_passes_against_the_oracle(oracle, cls, shape):
    """forward, scaled and unscaled inverse, out of place and in place: the middle pass has several hi blocks, a first stage above
    mat_w and a row stride above 1 at once, and neither reads the caller's input nor holds stage 0"""
    pl = TC._plan(shape[0], cls)
    _three(pl, shape)
    _check_plain(cls, shape, TC._case(cls, shape[0], shape[1], shape[3]), pl, ("fwd", "inv", "invu"))
    pl.close()


@pytest.mark.parametrize("cls,shape", _three_pass_params(THREE_PASS_LDE_SHAPES, _LDE_ID))
def test_three_pass_lde_columns_against_the_oracle(oracle, cls, shape):
    """the fused first pass (compact source in), then two plain in-place passes"""
    logm, beta, width, in_pitch, out_pitch, count = shape
    shift = TL._shift(cls, THREE_PASS_LDE_SHAPES.index(shape) + 2)  # p - 1, 1, g
    x, want = TL._lde_case(cls, logm, beta, width, count, shift)
    pl = TL._plan(logm, cls)
    _three(pl, shape)
    pl.set_coset(beta, shift)
    _check_lde(cls, shape, x, want, pl)
    pl.close()


@pytest.mark.parametrize("cls,shape", _three_pass_params(THREE_PASS_SHAPES, _PLAIN_ID))
def test_three_pass_coset_inverse_columns_against_the_oracle(oracle, cls, shape):
    """two plain passes, then the fused last pass (row r times u[r]); out of place and in place"""
    logn, width, pitch, count = shape
    shift = TL._shift(cls, THREE_PASS_SHAPES.index(shape) + 1)  # g, p - 1, 1
    x, want = TL._cinv_case(cls, logn, width, count, shift)
    pl = TL._plan(logn, cls)
    _three(pl, shape)
    pl.set_coset_inverse(shift)
    _check_cinv(cls, shape, x, want, pl)
    pl.close()


# ---- B2 ---------------------------------------------------------------------------------------------------------------------
class _AtTheLimit:
    """one matrix [rows][pitch] of which exactly (rows - 1) * pitch + width words are the caller's, inside one allocation with `guard`
    sentinel words before it and the rest of the last row plus `guard` words after it; everything is checked on the device"""

    def __init__(self, rows, pitch, width, sentinel, tdt, guard=4096):
        import torch

        self.rows, self.pitch, self.width, self.s, self.guard = rows, pitch, width, sentinel, guard
        self.big = torch.full((guard + rows * pitch + guard,), sentinel, dtype=tdt, device="cuda:0")
        self.view = self.big[guard: guard + rows * pitch].view(rows, pitch)
        self.live = self.view[:, :width]
        assert self.view.data_ptr() % 16 == 0

    def refill(self, sentinel):
        self.s = sentinel
        self.big.fill_(sentinel)

    def intact(self):
        import torch

        torch.cuda.synchronize()
        end = self.guard + self.rows * self.pitch
        return bool((self.big[:self.guard] == self.s).all()) and bool((self.big[end:] == self.s).all()) and bool((self.view[:, self.width:] == self.s).all())


@pytest.mark.parametrize("cls", ["gl", "m32"])
def test_a_matrix_of_exactly_2_to_the_28_words(oracle, cls):
    """logn 20, pitch 256: N * pitch == 2^28 words, the most the header accepts; byte offsets of 8-byte words reach 2^31 - 8.  Forward,
    scaled inverse and coset inverse in place, then the LDE from a compact [2^19][256] source into the same 2^28-word buffer; two live
    columns, every live word the oracle's; and one step beyond (pitch 257; width 257 at pitch 512) is refused on the same plan"""
    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    wb, p, g = ALL_CLASSES[cls]
    logn, pitch, width = LIMIT_LOGN, LIMIT_PITCH, 2
    n = 1 << logn
    assert n * pitch == 1 << 28
    L, E = _lib.lib(), _lib
    pl = TC._plan(logn, cls)
    _three(pl, (logn, width, pitch, 1))
    buf = _AtTheLimit(n, pitch, width, -3, _tdt(wb))
    a = buf.view.data_ptr()
    ref = TC._case(cls, logn, width, 1)
    calls = _plain_calls(pl, width, pitch, 1)
    for name in ("fwd", "inv"):
        buf.live.copy_(eng.to_device(ref["x"][0], "cuda:0"))
        assert calls[name](a, a) == 0
        assert buf.intact(), (cls, name)
        assert np.array_equal(eng.to_host(buf.live), ref[name][0]), (cls, name)
    shift = TL._shift(cls, 3)  # the shift of the three-pass test of this shape: one oracle run for both
    x, want = TL._cinv_case(cls, logn, width, 1, shift)
    pl.set_coset_inverse(shift)
    buf.live.copy_(eng.to_device(x[0], "cuda:0"))
    assert L.ntt_coset_inverse_columns(pl._h, a, a, width, pitch, 1, None) == 0
    assert buf.intact(), (cls, "coset inverse")
    assert np.array_equal(eng.to_host(buf.live), want[0]), (cls, "coset inverse")
    # the LDE: N_in * in_pitch = 2^27 words in, 2^28 out
    shift = g
    x, want = TL._lde_case(cls, logn, 1, width, 1, shift)
    pl.set_coset(1, shift)
    src = _AtTheLimit(n >> 1, pitch, width, -3, _tdt(wb))
    src.live.copy_(eng.to_device(x[0], "cuda:0"))
    buf.refill(-5)
    buf.live.fill_(-7)
    assert L.ntt_lde_columns(pl._h, src.view.data_ptr(), pitch, a, pitch, width, 1, None) == 0
    assert src.intact() and buf.intact(), (cls, "lde")
    assert np.array_equal(eng.to_host(src.live), x[0]), (cls, "lde", "input is read only")
    assert np.array_equal(eng.to_host(buf.live), want[0]), (cls, "lde")
    # one step beyond, on the same plan and buffer
    assert L.ntt_forward_columns(pl._h, a, a, width, pitch + 1, 1, None) == E.NTT_E_ARG
    assert L.ntt_inverse_columns(pl._h, a, a, width, pitch + 1, 1, 1, None) == E.NTT_E_ARG
    assert L.ntt_forward_columns(pl._h, a, a, 257, 512, 1, None) == E.NTT_E_ARG
    assert L.ntt_coset_inverse_columns(pl._h, a, a, width, pitch + 1, 1, None) == E.NTT_E_ARG
    assert L.ntt_lde_columns(pl._h, src.view.data_ptr(), pitch, a, pitch + 1, width, 1, None) == E.NTT_E_ARG
    torch.cuda.synchronize()
    assert buf.intact() and src.intact()
    pl.close()


def test_the_limit_with_129_live_columns(oracle):
    """Goldilocks, logn 20, width 129 (w = 8: logn + w == 28 as well), pitch 256, forward in place.  Eight random base columns; column
    c is k_c * base[c % 8] with distinct non-zero k_c, so -- the network being linear -- its transform is k_c * oracle(base[c % 8])
    (oracle.pointwise), every column differs from every other, and the oracle runs 8 transforms.  Every live word is compared, on the
    device"""
    import torch

    import ntt_aie_amd as eng
    from ntt_aie_amd import _lib

    cls, width = "gl", 129
    wb, p, g = ALL_CLASSES[cls]
    logn, pitch = LIMIT_LOGN, LIMIT_PITCH
    n = 1 << logn
    T = TC._table_cached(logn, cls)
    rng = np.random.default_rng(129)
    base = rng.integers(0, 2**63, size=(8, n), dtype=np.uint64) % np.uint64(p)
    base[0, 0], base[7, -1] = p - 1, 0
    k = set()
    while len(k) < width:
        k.add(int(rng.integers(1, 2**63)) % p or 1)
    k = sorted(k)
    rng.shuffle(k)
    fwd8 = oracle.ntt(base, T, p, nthreads=8)
    ones = np.ones(n, dtype=np.uint64)
    cols, want = np.empty((width, n), dtype=np.uint64), np.empty((width, n), dtype=np.uint64)
    for c in range(width):
        cols[c] = oracle.pointwise(base[c % 8], ones, p, int(k[c]))
        want[c] = oracle.pointwise(fwd8[c % 8], ones, p, int(k[c]))
    assert len({int(v) for v in cols[:, 1]}) == width  # distinct columns
    pl = TC._plan(logn, cls)
    _three(pl, (logn, width, pitch, 1))
    buf = _AtTheLimit(n, pitch, width, -3, _tdt(wb))
    buf.live.copy_(eng.to_device(cols, "cuda:0").t())
    dwant = eng.to_device(want, "cuda:0")
    a = buf.view.data_ptr()
    assert _lib.lib().ntt_forward_columns(pl._h, a, a, width, pitch, 1, None) == 0
    assert buf.intact()
    assert torch.equal(buf.live, dwant.t())
    assert _lib.lib().ntt_forward_columns(pl._h, a, a, 257, 512, 1, None) == _lib.NTT_E_ARG
    pl.close()


# ---- B3 ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", sorted(CLASSES))
@pytest.mark.parametrize("shape", LOOP_SHAPES, ids=lambda s: "n%d_w%d_p%d_c%d" % s)
def test_batch_loop_and_taper(oracle, cls, shape):
    """forward and scaled inverse in place, the LDE, the coset inverse out of place, on so many matrices that every workgroup of
    every pass streams several groups (and the last rows fewer: the taper).  The oracle's arrays are not kept (200 MB each)"""
    logn, width, pitch, count = shape
    pl = TC._plan(logn, cls)
    _check_plain(cls, shape, TC._case.__wrapped__(cls, logn, width, count), pl, ("fwd", "inv"), out_of_place=False)
    beta, in_pitch, out_pitch = LOOP_LDE[logn]
    shift = TL._shift(cls, LOOP_SHAPES.index(shape) + 1)
    x, want = TL._lde_case.__wrapped__(cls, logn, beta, width, count, shift)
    pl.set_coset(beta, shift)
    _check_lde(cls, (logn, beta, width, in_pitch, out_pitch, count), x, want, pl)
    x, want = TL._cinv_case.__wrapped__(cls, logn, width, count, shift)
    pl.set_coset_inverse(shift)
    _check_cinv(cls, shape, x, want, pl, in_place=False)
    pl.close()


# ---- B4 ---------------------------------------------------------------------------------------------------------------------
def _edge_matrix(cls, rows, width, seed):
    """[1][rows][width]: columns of all p - 1, all 0, all 1, alternating 0 / p - 1, p - 1 in row 0 only, p - 1 in the last row only;
    for 8-byte words also columns of 2^32 - 1, 2^32, 2^63 and p - 2^32 (mod p); for 4-byte words columns of 2^30, 2^31 - 1, 2^31,
    (p - 1) / 2 and (p + 1) / 2 (mod p) -- where a sum first reaches 2^31 and 2^32: the `small` stream's v_min corrections and the `any`
    stream's carry selects change arm there; the other columns are random"""
    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    x = (np.random.default_rng(seed).integers(0, 2**63, size=(1, rows, width), dtype=np.uint64) % np.uint64(p)).astype(dt)
    m = x[0]
    m[:, 0], m[:, 1], m[:, 2] = p - 1, 0, 1
    m[0::2, 3], m[1::2, 3] = 0, p - 1
    m[:, 4], m[0, 4] = 0, p - 1
    m[:, 5], m[-1, 5] = 0, p - 1
    fills = [v % p for v in ((2**32 - 1, 2**32, 2**63, p - 2**32) if wb == 8 else (2**30, 2**31 - 1, 2**31, (p - 1) // 2, (p + 1) // 2))]
    for i, v in enumerate(fills):
        m[:, 6 + i] = v
    assert 6 + len(fills) < width
    return x


@pytest.mark.parametrize("cls", sorted(ALL_CLASSES))
def test_columns_of_edge_residues(oracle, cls):
    """forward, scaled inverse, the LDE (beta 1) and the coset inverse with the shifts p - 1 and g, on a matrix whose first columns
    are the residues at which the arithmetic can go wrong: the multiplications by s[row >> beta] in the fused LDE load and by u[row]
    before the fused coset-inverse store see them as well as the butterflies"""
    wb, p, g = ALL_CLASSES[cls]
    dt = np.uint32 if wb == 4 else np.uint64
    logn, width, pitch, count = EDGE_SHAPE
    n, beta = 1 << logn, 1
    T = TC._table_cached(logn, cls)
    t = lambda m: np.ascontiguousarray(m.transpose(0, 2, 1)).reshape(count * width, -1)
    back = lambda c: np.ascontiguousarray(c.reshape(count, width, -1).transpose(0, 2, 1))
    x = _edge_matrix(cls, n, width, 7)
    pl = TC._plan(logn, cls)
    inv = oracle.intt(t(x), T, p)
    _check_plain(cls, EDGE_SHAPE, {"x": x, "fwd": back(oracle.ntt(t(x), T, p)), "inv": back(inv)}, pl, ("fwd", "inv"))
    xs = _edge_matrix(cls, n >> beta, width, 8)
    for shift in (p - 1, g):
        s = TL._powers(shift, TL._bitrev_array(logn - beta), p, dt)
        cols = np.zeros((count * width, n), dtype=dt)
        cols[:, :: 1 << beta] = oracle.pointwise(t(xs), np.broadcast_to(s, (count * width, n >> beta)).copy(), p)
        pl.set_coset(beta, shift)
        _check_lde(cls, (logn, beta, width, pitch + 1, pitch, count), xs, back(oracle.ntt(cols, T, p)), pl)
        u = TL._powers(pow(shift, p - 2, p), TL._bitrev_array(logn), p, dt)
        pl.set_coset_inverse(shift)
        _check_cinv(cls, EDGE_SHAPE, x, back(oracle.pointwise(inv, np.broadcast_to(u, inv.shape).copy(), p)), pl)
    pl.close()


# ---- B5 ---------------------------------------------------------------------------------------------------------------------
def _plumbing(cls):
    """plan with twiddles, coset (beta 3, shift g) and coset-inverse (shift g) set; inputs and the oracle's words of all four entry
    points at PLUMBING_SHAPE"""
    wb, p, g = ALL_CLASSES[cls]
    logn, width, pitch = PLUMBING_SHAPE
    pl = TL._plan(logn, cls)
    pl.set_coset(3, g)
    pl.set_coset_inverse(g)
    ref = TC._case(cls, logn, width, 1)
    xl, want_lde = TL._lde_case(cls, logn, 3, width, 1, g)
    xc, want_cinv = TL._cinv_case(cls, logn, width, 1, g)
    return pl, {"x": ref["x"][0], "fwd": ref["fwd"][0], "inv": ref["inv"][0], "xl": xl[0], "lde": want_lde[0], "xc": xc[0], "cinv": want_cinv[0]}


def _padded(x, pitch, tdt, sentinel=-3):
    """x [rows][width] as the live part of a [rows][pitch] tensor"""
    import torch

    import ntt_aie_amd as eng

    big = torch.full((x.shape[0], pitch), sentinel, dtype=tdt, device="cuda:0")
    view = big[:, :x.shape[1]]
    view.copy_(eng.to_device(x, "cuda:0"))
    return big, view


def _all_four(pl, r, pitch, tdt, key):
    """the four entry points through the wrappers on padded views against the oracle's words in r"""
    import torch

    import ntt_aie_amd as eng

    width = r["x"].shape[1]
    for name, src, call in (("fwd", "x", pl.forward_columns), ("inv", "x", pl.inverse_columns), ("cinv", "xc", pl.coset_inverse_columns)):
        big, view = _padded(r[src], pitch, tdt)
        obig = torch.full_like(big, -5)
        assert np.array_equal(eng.to_host(call(view, out=obig[:, :width])), r[name]), (key, name)
        assert bool((obig[:, width:] == -5).all()) and bool((big[:, width:] == -3).all()) and np.array_equal(eng.to_host(view), r[src]), (key, name)
        assert call(view, out=view) is view and np.array_equal(eng.to_host(view), r[name]), (key, name, "in place")
        assert bool((big[:, width:] == -3).all()), (key, name, "in place")
    big, view = _padded(r["xl"], pitch - 1, tdt)
    obig = torch.full((r["lde"].shape[0], pitch), -5, dtype=tdt, device="cuda:0")
    assert np.array_equal(eng.to_host(pl.lde_columns(view, out=obig[:, :width])), r["lde"]), (key, "lde")
    assert bool((obig[:, width:] == -5).all()) and bool((big[:, width:] == -3).all()) and np.array_equal(eng.to_host(view), r["xl"]), (key, "lde")


@pytest.mark.parametrize("cls", ["gl", "m32"])
def test_clone_carries_the_column_configuration(oracle, cls):
    """the clone owns its coset and coset-inverse vectors: changing both on the source does not reach lde_columns /
    coset_inverse_columns of the clone, and forward_columns / inverse_columns give the oracle's words there too"""
    wb, p, g = ALL_CLASSES[cls]
    pl, r = _plumbing(cls)
    cl = pl.clone()
    assert cl.column_passes == pl.column_passes and cl.log_blowup == 3 and cl.coset_inverse_set
    pl.set_coset(1, 1)
    pl.set_coset_inverse(p - 1)
    _all_four(cl, r, PLUMBING_SHAPE[2], _tdt(wb), (cls, "clone"))
    pl.close()
    cl.close()


@pytest.mark.parametrize("cls", ["gl", "m32"])
def test_graph_capture_of_the_column_entry_points(oracle, cls):
    """forward_columns, lde_columns and coset_inverse_columns warmed up on a side stream, then captured one after the other on ONE
    stream (no parallel branches) into one graph; two replays into zeroed outputs give the oracle's words"""
    import torch

    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    logn, width, pitch = PLUMBING_SHAPE
    tdt = _tdt(wb)
    pl, r = _plumbing(cls)
    ins = {k: _padded(r[k], pitch, tdt) for k in ("x", "xl", "xc")}
    outs = {k: torch.full((1 << logn, pitch), -5, dtype=tdt, device="cuda:0") for k in ("fwd", "lde", "cinv")}

    def work():
        pl.forward_columns(ins["x"][1], out=outs["fwd"][:, :width])
        pl.lde_columns(ins["xl"][1], out=outs["lde"][:, :width])
        pl.coset_inverse_columns(ins["xc"][1], out=outs["cinv"][:, :width])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        work()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        work()
    for _ in range(2):
        for o in outs.values():
            o[:, :width].zero_()
        gr.replay()
        torch.cuda.synchronize()
        for k, o in outs.items():
            assert np.array_equal(eng.to_host(o[:, :width]), r[k]), (cls, k)
            assert bool((o[:, width:] == -5).all()), (cls, k)
    for k, (big, view) in ins.items():
        assert np.array_equal(eng.to_host(view), r[k]) and bool((big[:, width:] == -3).all()), (cls, k)
    del gr
    pl.close()


@pytest.mark.parametrize("cls", ["gl", "m32"])
def test_a_pinned_policy_leaves_the_columns_alone(oracle, cls):
    """include/ntt_hip.h: the columns decomposition is fixed by logn.  Under every pinned alternative of the plan column_passes is
    unchanged and all four entry points give the oracle's words"""
    wb, p, g = ALL_CLASSES[cls]
    pl, r = _plumbing(cls)
    passes = pl.column_passes
    alts = pl.alternatives
    assert passes == [(0, 7), (7, 6)] and len(alts) >= 1
    try:
        for k in range(len(alts)):
            pl.set_policy(k)
            assert pl.column_passes == passes, (cls, k)
            _all_four(pl, r, PLUMBING_SHAPE[2], _tdt(wb), (cls, "policy", k))
    finally:
        pl.set_policy(-1)
    assert pl.column_passes == passes
    _all_four(pl, r, PLUMBING_SHAPE[2], _tdt(wb), (cls, "policy", -1))
    pl.close()


@pytest.mark.parametrize("cls", ["gl", "m32"])
def test_columns_of_a_shared_plan_from_two_host_threads(oracle, cls):
    """two host threads share one configured plan, each on its own stream and its own buffers: forward_columns, then inverse_columns
    of the result; both forwards equal the oracle's, both round trips the input"""
    import threading

    import torch

    import ntt_aie_amd as eng

    wb, p, g = ALL_CLASSES[cls]
    logn, width, pitch = PLUMBING_SHAPE
    pl, r = _plumbing(cls)
    dt = np.uint32 if wb == 4 else np.uint64
    T = TC._table_cached(logn, cls)
    data = [r["x"], (np.random.default_rng(77).integers(0, 2**63, size=r["x"].shape, dtype=np.uint64) % np.uint64(p)).astype(dt)]
    want = [r["fwd"], np.ascontiguousarray(oracle.ntt(np.ascontiguousarray(data[1].T), T, p).T)]
    fwd, back, errors = [None, None], [None, None], []

    def worker(i):
        try:
            torch.cuda.set_device(0)
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                big, view = _padded(data[i], pitch, _tdt(wb))
                fbig, bbig = torch.full_like(big, -5), torch.full_like(big, -7)
                for _ in range(10):
                    f = pl.forward_columns(view, out=fbig[:, :width], stream=s)
                    b = pl.inverse_columns(f, out=bbig[:, :width], stream=s)
                    s.synchronize()
                fwd[i], back[i] = eng.to_host(f), eng.to_host(b)
                assert bool((big[:, width:] == -3).all()) and bool((fbig[:, width:] == -5).all()) and bool((bbig[:, width:] == -7).all())
        except Exception as e:  # surfaced in the main thread
            errors.append(repr(e))

    ts = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    for i in range(2):
        assert np.array_equal(fwd[i], want[i]), (cls, i)
        assert np.array_equal(back[i], data[i]), (cls, i)
    pl.close()
