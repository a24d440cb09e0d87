"""Python host of the MI355X NTT engine.

Mirrors the reference host procedure (src/test.cpp:115-190): make the twiddle
table with the reference's rule, hand over (input, root, output) buffers, launch,
wait.  torch is used only for device memory and streams; every transform goes
through the C-ABI in libntt_hip.so (ntt_aie_amd/_lib.py).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib
from ._lib import LAYOUT_AIE_BLOCK16, LAYOUT_NATURAL, check

GOLDILOCKS = 0xFFFFFFFF00000001


def _np_dtype(word_bytes: int):
    return np.uint32 if word_bytes == 4 else np.uint64


def _torch_dtype(word_bytes: int):
    # torch tensors are plain device memory here: signed types carry the same bits
    return torch.int32 if word_bytes == 4 else torch.int64


def to_device(a: np.ndarray, device) -> torch.Tensor:
    """Host words -> device buffer with the same bit pattern."""
    a = np.ascontiguousarray(a)
    signed = a.view(np.int32 if a.dtype.itemsize == 4 else np.int64)
    return torch.from_numpy(signed).to(device)


def to_host(t: torch.Tensor) -> np.ndarray:
    a = t.detach().cpu().contiguous().numpy()
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


class NTTPlan:
    """One (logn, p, word size) transform plan on one GPU.

    The plan owns the device copies of the twiddle table ("root" buffer,
    src/test.cpp:119-120) and of its inverse; data buffers stay caller-owned.
    """

    def __init__(self, logn: int, p: int, word_bytes: int | None = None, device: int | None = None):
        if word_bytes is None:
            word_bytes = 8 if p >= (1 << 32) else 4
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        self.logn, self.n, self.p, self.word_bytes, self.device = logn, 1 << logn, p, word_bytes, device
        self._h = C.c_void_p()
        check(_lib.lib().ntt_plan_create(C.byref(self._h), logn, p, word_bytes, device), "ntt_plan_create")
        self.table: np.ndarray | None = None

    def close(self) -> None:
        if self._h:
            _lib.lib().ntt_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- tables (host side, like the reference's make_roots) -----------------
    def make_roots(self, g: int) -> np.ndarray:
        """src/test.cpp:27-32 + :138: T[0]=1, T[i]=T[i-1]*g^((p-1)/N) mod p."""
        return self.make_table(0, g)

    def make_table(self, kind: int, g: int) -> np.ndarray:
        T = np.empty(self.n, dtype=_np_dtype(self.word_bytes))
        check(_lib.lib().ntt_make_table(self._h, kind, g, T.ctypes.data), "ntt_make_table")
        return T

    def set_twiddles(self, T: np.ndarray) -> None:
        T = np.ascontiguousarray(T, dtype=_np_dtype(self.word_bytes))
        if T.shape != (self.n,):
            raise ValueError("twiddle table must have N = %d words" % self.n)
        check(_lib.lib().ntt_plan_set_twiddles(self._h, T.ctypes.data), "ntt_plan_set_twiddles")
        self.table = T

    def generate_twiddles(self, kind: int, g: int) -> None:
        """Make the table (and its inverse) on the device: no host table, no upload."""
        check(_lib.lib().ntt_plan_generate_twiddles(self._h, kind, g), "ntt_plan_generate_twiddles")
        self.table = None

    def get_twiddles(self, inverse: bool = False) -> np.ndarray:
        T = np.empty(self.n, dtype=_np_dtype(self.word_bytes))
        check(_lib.lib().ntt_plan_get_twiddles(self._h, int(inverse), T.ctypes.data), "ntt_plan_get_twiddles")
        return T

    @property
    def hbm_passes(self) -> int:
        return int(_lib.lib().ntt_plan_info(self._h, 3))

    @property
    def passes(self) -> list[tuple[str, int, int]]:
        """[(kind, first stage, stages)] of one forward transform; kind is 'contig' for pass 0, 'col' after."""
        L = _lib.lib()
        return [("contig" if i == 0 else "col", int(L.ntt_plan_info(self._h, 64 + i)), int(L.ntt_plan_info(self._h, 32 + i)))
                for i in range(self.hbm_passes)]

    def passes_for(self, batch: int) -> list[tuple[str, int, int]]:
        """The decomposition ntt_forward / ntt_inverse run for THIS batch (the plan keeps alternatives and the launcher picks
        by batch size and modulus class; `passes` is the default one)."""
        L = _lib.lib()
        alt = int(L.ntt_plan_select(self._h, batch))
        k = int(L.ntt_plan_info(self._h, 256 + 16 * alt))
        return [("contig" if i == 0 else "col", int(L.ntt_plan_info(self._h, 256 + 16 * alt + 8 + i)),
                 int(L.ntt_plan_info(self._h, 256 + 16 * alt + 1 + i))) for i in range(k)]

    @property
    def alternatives(self) -> list[tuple[list[int], int]]:
        """[(stages per pass, smallest batch it is chosen for)] of every launch-time decomposition of this plan."""
        L = _lib.lib()
        out = []
        for a in range(int(L.ntt_plan_info(self._h, 6))):
            k = int(L.ntt_plan_info(self._h, 256 + 16 * a))
            out.append(([int(L.ntt_plan_info(self._h, 256 + 16 * a + 1 + i)) for i in range(k)],
                        int(L.ntt_plan_info(self._h, 256 + 16 * a + 15))))
        return out

    @property
    def alternative_variants(self) -> list[list[int]]:
        """[kernel variant per pass] of every alternative (ntt_plan_info 512+: 0 = the default kernel of the pass shape)."""
        L = _lib.lib()
        return [[int(L.ntt_plan_info(self._h, 512 + 16 * a + i)) for i in range(len(stages))]
                for a, (stages, _) in enumerate(self.alternatives)]

    def set_policy(self, alternative: int) -> None:
        """-1 (default): the launcher picks the decomposition by batch; k >= 0: always alternative k (ntt_plan_set_policy)."""
        check(_lib.lib().ntt_plan_set_policy(self._h, alternative), "ntt_plan_set_policy")

    def clone(self, device: int | None = None) -> "NTTPlan":
        """A copy of this plan on `device` (default: the same one): tables travel device-to-device (ntt_plan_clone)."""
        device = self.device if device is None else device
        new = object.__new__(NTTPlan)
        new.logn, new.n, new.p, new.word_bytes, new.device = self.logn, self.n, self.p, self.word_bytes, device
        new._h = C.c_void_p()
        new.table = self.table
        check(_lib.lib().ntt_plan_clone(self._h, device, C.byref(new._h)), "ntt_plan_clone")
        return new

    # ---- coset low-degree extension (this plan is the size-M one) ------------------
    def set_coset(self, log_blowup: int, shift: int) -> None:
        """Configure lde(): N = M >> log_blowup coefficients in, values on shift * <w_M> out (ntt_plan_set_coset).  The plan builds
        its N-word vector shift^bitrev(i) on the device.  Configuration: call before the plan is shared between threads."""
        check(_lib.lib().ntt_plan_set_coset(self._h, log_blowup, shift), "ntt_plan_set_coset")

    @property
    def log_blowup(self) -> int:
        """log2 of the blow-up set by set_coset(); 0 = not set."""
        return int(_lib.lib().ntt_plan_info(self._h, 9))

    @property
    def lde_fused(self) -> bool:
        """Does lde() expand inside the first pass (True from logn = 5 on) or through the separate expansion kernel."""
        return bool(_lib.lib().ntt_plan_info(self._h, 10))

    # ---- coset interpolation: values on shift * <w_M> back to coefficients ------------
    def set_coset_inverse(self, shift: int) -> None:
        """Configure coset_inverse() (ntt_plan_set_coset_inverse): the plan builds its M-word vector shift^-bitrev(i) * M^-1 on the
        device.  Independent of set_coset().  Configuration: call before the plan is shared between threads."""
        check(_lib.lib().ntt_plan_set_coset_inverse(self._h, shift), "ntt_plan_set_coset_inverse")

    @property
    def coset_inverse_set(self) -> bool:
        return bool(_lib.lib().ntt_plan_info(self._h, 11))

    @property
    def coset_inverse_fused(self) -> bool:
        """Does coset_inverse() scale inside the inverse's last pass (True from logn = 5 on) or through the separate row-scaling kernel."""
        return bool(_lib.lib().ntt_plan_info(self._h, 12))

    @property
    def column_passes(self) -> list[tuple[int, int]]:
        """[(first stage, stages)] of the column passes forward_columns() / inverse_columns() run (ntt_plan_info 13 / 128+ / 96+);
        empty when logn < 4, where no column kernel shape exists."""
        L = _lib.lib()
        return [(int(L.ntt_plan_info(self._h, 128 + i)), int(L.ntt_plan_info(self._h, 96 + i))) for i in range(int(L.ntt_plan_info(self._h, 13)))]

    @property
    def has_inverse(self) -> bool:
        return bool(_lib.lib().ntt_plan_info(self._h, 4))

    # ---- buffers ---------------------------------------------------------------
    def empty(self, batch: int) -> torch.Tensor:
        return torch.empty((batch, self.n), dtype=_torch_dtype(self.word_bytes),
                           device=torch.device("cuda", self.device))

    def _batch(self, *ts: torch.Tensor) -> int:
        for t in ts:
            if not t.is_cuda or t.device.index != self.device:
                raise ValueError("buffer is not on cuda:%d" % self.device)
            if not t.is_contiguous() or t.element_size() != self.word_bytes:
                raise ValueError("buffer must be contiguous with %d-byte words" % self.word_bytes)
            if t.numel() % self.n or t.numel() != ts[0].numel():
                raise ValueError("buffer sizes must be equal multiples of N")
        return ts[0].numel() // self.n

    @staticmethod
    def _stream(stream) -> int:
        if stream is None:
            stream = torch.cuda.current_stream()
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)

    def _out_like(self, inp: torch.Tensor, stream) -> torch.Tensor:
        """Output buffer for a launch on `stream`: allocated UNDER that stream, so that torch's caching allocator
        ties the block's reuse to the stream the kernels run on (allocating on the current stream and launching on
        another would let the allocator recycle the block while the transform is still writing it)."""
        if stream is None:
            return torch.empty_like(inp)
        if not hasattr(stream, "cuda_stream"):  # a raw hipStream_t handle
            stream = torch.cuda.ExternalStream(int(stream), device=inp.device)
        with torch.cuda.stream(stream):
            return torch.empty_like(inp)

    # ---- transforms ------------------------------------------------------------
    def forward(self, inp: torch.Tensor, out: torch.Tensor | None = None, layout: int = LAYOUT_NATURAL,
                stream=None) -> torch.Tensor:
        """The reference network (src/test.cpp:34-60) on every polynomial of `inp`."""
        out = self._out_like(inp, stream) if out is None else out
        b = self._batch(inp, out)
        check(_lib.lib().ntt_forward(self._h, inp.data_ptr(), out.data_ptr(), b, layout,
                                     self._stream(stream)), "ntt_forward")
        return out

    def lde(self, inp: torch.Tensor, out: torch.Tensor | None = None, layout: int = LAYOUT_NATURAL, stream=None) -> torch.Tensor:
        """Low-degree extension (ntt_lde): `inp` is [batch][N] words, N = M >> log_blowup, in the order inverse() of the size-N
        plan returns them; the result is [batch][M].  `out` must not overlap `inp`."""
        beta = self.log_blowup
        if beta == 0:
            raise ValueError("set_coset() first")
        n_small = self.n >> beta
        if not inp.is_cuda or inp.device.index != self.device:
            raise ValueError("buffer is not on cuda:%d" % self.device)
        if not inp.is_contiguous() or inp.element_size() != self.word_bytes or inp.numel() % n_small:
            raise ValueError("input must be contiguous [batch][%d] %d-byte words" % (n_small, self.word_bytes))
        b = inp.numel() // n_small
        if out is None:
            if stream is None:
                out = torch.empty((b, self.n), dtype=inp.dtype, device=inp.device)
            else:  # allocated under the launch stream, as _out_like does
                st = stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(stream), device=inp.device)
                with torch.cuda.stream(st):
                    out = torch.empty((b, self.n), dtype=inp.dtype, device=inp.device)
        if self._batch(out) != b:
            raise ValueError("output must be [batch][%d] words for %d input rows" % (self.n, b))
        check(_lib.lib().ntt_lde(self._h, inp.data_ptr(), out.data_ptr(), b, layout, self._stream(stream)), "ntt_lde")
        return out

    def forward_profile(self, inp: torch.Tensor, out: torch.Tensor | None = None,
                        layout: int = LAYOUT_NATURAL, stream=None) -> list[float]:
        """forward() with a hipEvent pair around every HBM pass; returns ms per pass (blocking)."""
        out = self._out_like(inp, stream) if out is None else out
        b = self._batch(inp, out)
        ms = (C.c_float * 8)()
        k = C.c_int(0)
        check(_lib.lib().ntt_forward_profile(self._h, inp.data_ptr(), out.data_ptr(), b, layout,
                                             self._stream(stream), ms, 8, C.byref(k)), "ntt_forward_profile")
        return [float(ms[i]) for i in range(k.value)]

    def inverse(self, inp: torch.Tensor, out: torch.Tensor | None = None, layout: int = LAYOUT_NATURAL,
                scale: bool = True, stream=None) -> torch.Tensor:
        out = self._out_like(inp, stream) if out is None else out
        b = self._batch(inp, out)
        check(_lib.lib().ntt_inverse(self._h, inp.data_ptr(), out.data_ptr(), b, layout, int(scale),
                                     self._stream(stream)), "ntt_inverse")
        return out

    # ---- row-major matrices: every column of [N][width] is a polynomial -------------
    def _matrix(self, t: torch.Tensor, what: str, rows: int | None = None) -> tuple[int, int, int]:
        """(width, pitch, count) of a matrix view the C-ABI can address: [N][width] or [count][N][width], last stride 1, row stride =
        pitch >= width, matrix stride = N * pitch.  `rows`: the row count where it is not the plan's N (the compact input of
        lde_columns())."""
        rows = self.n if rows is None else rows
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError("%s is not on cuda:%d" % (what, self.device))
        if t.element_size() != self.word_bytes:
            raise ValueError("%s must hold %d-byte words" % (what, self.word_bytes))
        if t.dim() not in (2, 3) or t.shape[-2] != rows:
            raise ValueError("%s must be [N][width] or [count][N][width] with N = %d rows" % (what, rows))
        width, count = int(t.shape[-1]), (int(t.shape[0]) if t.dim() == 3 else 1)
        if width == 0 or count == 0:
            return width, width, count
        pitch = int(t.stride(-2))
        if width > 1 and t.stride(-1) != 1:
            raise ValueError("%s: the last stride must be 1 (columns of a row are adjacent words)" % what)
        if pitch < width:
            raise ValueError("%s: the row stride (pitch) must be >= width" % what)
        if t.dim() == 3 and count > 1 and t.stride(0) != rows * pitch:
            raise ValueError("%s: the matrix stride must be N * pitch = %d words" % (what, rows * pitch))
        return width, pitch, count

    def _columns(self, fn, name: str, mat: torch.Tensor, out: torch.Tensor | None, stream, *extra) -> torch.Tensor:
        width, pitch, count = self._matrix(mat, "mat")
        if out is None:
            if stream is None:
                out = torch.empty(mat.shape, dtype=mat.dtype, device=mat.device)
            else:  # allocated under the launch stream, as _out_like does
                st = stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(stream), device=mat.device)
                with torch.cuda.stream(st):
                    out = torch.empty(mat.shape, dtype=mat.dtype, device=mat.device)
        if out is not mat:
            if tuple(out.shape) != tuple(mat.shape):
                raise ValueError("out must have the shape of mat")
            w2, p2, c2 = self._matrix(out, "out")
            if width and count and p2 != pitch:
                raise ValueError("out must have the pitch of mat (%d words), or be allocated by the call" % pitch)
        check(fn(self._h, mat.data_ptr(), out.data_ptr(), width, pitch, count, *extra, self._stream(stream)), name)
        return out

    def forward_columns(self, mat: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """forward() on every COLUMN of the row-major matrix (or matrices) `mat`, where it lies (ntt_forward_columns): [N][width] or
        [count][N][width], natural order; a strided view such as big[:, :, :width] is taken as it is, and words outside it are neither
        read nor written.  `out=mat` transforms in place, and `out=` a tensor of mat's shape and pitch is written by the first pass: neither
        costs a copy.  `out=None` allocates a contiguous result; for a contiguous `mat` that is free as well, but for a STRIDED view it
        first copies the live words into the result (one extra trip of the matrix through HBM, what this entry point exists to avoid:
        the C-ABI takes one pitch for both buffers) and transforms them there.  Pass `out=mat`, or an `out` of mat's pitch, to avoid it."""
        if out is None and not mat.is_contiguous():
            return self._columns_to_contiguous(_lib.lib().ntt_forward_columns, "ntt_forward_columns", mat, stream)
        return self._columns(_lib.lib().ntt_forward_columns, "ntt_forward_columns", mat, out, stream)

    def inverse_columns(self, mat: torch.Tensor, out: torch.Tensor | None = None, scale: bool = True, stream=None) -> torch.Tensor:
        """inverse(scale=...) on every column of `mat` (ntt_inverse_columns); buffers as for forward_columns(), the extra copy of a strided
        `mat` with `out=None` included."""
        if out is None and not mat.is_contiguous():
            return self._columns_to_contiguous(_lib.lib().ntt_inverse_columns, "ntt_inverse_columns", mat, stream, int(scale))
        return self._columns(_lib.lib().ntt_inverse_columns, "ntt_inverse_columns", mat, out, stream, int(scale))

    def _columns_to_contiguous(self, fn, name: str, mat: torch.Tensor, stream, *extra) -> torch.Tensor:
        """A strided view in, a fresh contiguous result out: the C-ABI takes ONE pitch for both buffers, so the live words are copied
        into the result under the launch stream and transformed in place there."""
        self._matrix(mat, "mat")
        st = None if stream is None else (stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(stream), device=mat.device))
        if st is None:
            out = mat.contiguous()
        else:
            with torch.cuda.stream(st):
                out = mat.contiguous()
        return self._columns(fn, name, out, out, stream, *extra)

    def lde_columns(self, mat: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """lde() on every COLUMN of the row-major matrix (or matrices) `mat` (ntt_lde_columns): [N][width] or [count][N][width] in,
        N = M >> log_blowup rows in the order inverse_columns() of the size-N plan leaves them, strided views taken as they are;
        [M][width] (or [count][M][width]) out.  `out=None` allocates a contiguous [count][M][width] (or [M][width]) result; an `out`
        view may have any pitch of its own, and must not overlap `mat`.  Nothing of the big size is read or written before the first
        pass's own store."""
        beta = self.log_blowup
        if beta == 0:
            raise ValueError("set_coset() first")
        n_small = self.n >> beta
        width, in_pitch, count = self._matrix(mat, "mat", n_small)
        shape = tuple(mat.shape[:-2]) + (self.n, width)
        if out is None:
            if stream is None:
                out = torch.empty(shape, dtype=mat.dtype, device=mat.device)
            else:  # allocated under the launch stream, as _out_like does
                st = stream if hasattr(stream, "cuda_stream") else torch.cuda.ExternalStream(int(stream), device=mat.device)
                with torch.cuda.stream(st):
                    out = torch.empty(shape, dtype=mat.dtype, device=mat.device)
        if tuple(out.shape) != shape:
            raise ValueError("out must be %s for this mat" % (shape,))
        _, out_pitch, _ = self._matrix(out, "out")
        check(_lib.lib().ntt_lde_columns(self._h, mat.data_ptr(), in_pitch, out.data_ptr(), out_pitch, width, count, self._stream(stream)),
              "ntt_lde_columns")
        return out

    def coset_inverse_columns(self, mat: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """coset_inverse() on every column of `mat` (ntt_coset_inverse_columns): [M][width] or [count][M][width]; buffers as for
        inverse_columns(), the extra copy of a strided `mat` with `out=None` included.  With kind-1 tables and rows holding the values
        at shift * w_M^k in, row j of the result holds coefficient bitrev_M(j) of every column: the order lde_columns() consumes."""
        if not self.coset_inverse_set:
            raise ValueError("set_coset_inverse() first")
        if out is None and not mat.is_contiguous():
            return self._columns_to_contiguous(_lib.lib().ntt_coset_inverse_columns, "ntt_coset_inverse_columns", mat, stream)
        return self._columns(_lib.lib().ntt_coset_inverse_columns, "ntt_coset_inverse_columns", mat, out, stream)

    def coset_inverse(self, inp: torch.Tensor, out: torch.Tensor | None = None, layout: int = LAYOUT_NATURAL, stream=None) -> torch.Tensor:
        """Coset interpolation (ntt_coset_inverse): the scaled inverse of every row of `inp` (given in `layout`), word i times
        shift^-bitrev(i).  With kind-1 tables and values on shift * <w_M> in, the coefficients come out in the bit-reversed order
        lde() consumes.  `out` may be `inp`."""
        out = self._out_like(inp, stream) if out is None else out
        b = self._batch(inp, out)
        check(_lib.lib().ntt_coset_inverse(self._h, inp.data_ptr(), out.data_ptr(), b, layout, self._stream(stream)), "ntt_coset_inverse")
        return out

    def pointwise_mul(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None,
                      scale: int = 1, stream=None) -> torch.Tensor:
        out = self._out_like(a, stream) if out is None else out
        n = self._batch(a, b, out)
        check(_lib.lib().ntt_pointwise_mul(self._h, a.data_ptr(), b.data_ptr(), out.data_ptr(), n, scale,
                                           self._stream(stream)), "ntt_pointwise_mul")
        return out

    def polymul_negacyclic(self, a: torch.Tensor, b: torch.Tensor, out: torch.Tensor | None = None,
                           stream=None) -> torch.Tensor:
        """c = a*b mod (x^N + 1, p); needs a kind-2 table.  a and b are overwritten."""
        out = a if out is None else out
        n = self._batch(a, b, out)
        check(_lib.lib().ntt_polymul_negacyclic(self._h, a.data_ptr(), b.data_ptr(), out.data_ptr(), n,
                                                self._stream(stream)), "ntt_polymul_negacyclic")
        return out

    def polymul_prepare(self, b: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """The transform-domain form polymul_negacyclic_pre() takes as its fixed operand (ntt_polymul_prepare): exactly
        inverse(b, scale=False) -- [rows][N] canonical words in natural order, valid for every clone of the plan and every batch.
        `out` may be `b`."""
        out = self._out_like(b, stream) if out is None else out
        rows = self._batch(b, out)
        check(_lib.lib().ntt_polymul_prepare(self._h, b.data_ptr(), out.data_ptr(), rows, self._stream(stream)), "ntt_polymul_prepare")
        return out

    def polymul_negacyclic_pre(self, a: torch.Tensor, bhat: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """c = a*b mod (x^N + 1, p) with b given prepared, bhat = polymul_prepare(b) (ntt_polymul_negacyclic_pre); needs a kind-2
        table.  bhat of shape [N] or [1, N] multiplies EVERY row of a (the broadcast); [batch, N] is one operand per row.  a is
        overwritten (scratch; `out` defaults to it), bhat is only read and must not overlap a or out."""
        out = a if out is None else out
        n = self._batch(a, out)
        if not bhat.is_cuda or bhat.device.index != self.device:
            raise ValueError("buffer is not on cuda:%d" % self.device)
        if not bhat.is_contiguous() or bhat.element_size() != self.word_bytes:
            raise ValueError("buffer must be contiguous with %d-byte words" % self.word_bytes)
        if bhat.numel() == self.n and bhat.dim() in (1, 2):
            rows = 1
        elif bhat.numel() == a.numel() and bhat.dim() >= 2:
            rows = n
        else:
            raise ValueError("bhat must be [N] or [1, N] (broadcast) or have one row of N words per row of a")
        check(_lib.lib().ntt_polymul_negacyclic_pre(self._h, a.data_ptr(), bhat.data_ptr(), rows, out.data_ptr(), n,
                                                    self._stream(stream)), "ntt_polymul_negacyclic_pre")
        return out

    def polymul_dot_pre(self, a: torch.Tensor, bhat: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """sum_k a[k]*b[k] mod (x^N + 1, p) with every b[k] given prepared (ntt_polymul_dot_pre); needs a kind-2 table.  a is
        [K, batch, N]; bhat is [K, batch, N], one prepared operand per term and row, or [K, N] / [K, 1, N]: one per term that
        multiplies every row (the key-switching case).  The sum runs inside the middle pass and ONE forward transform follows.
        a is overwritten (scratch); `out`, [batch, N], defaults to a[0]; bhat is only read and must not overlap a or out."""
        if a.dim() != 3 or a.shape[2] != self.n:
            raise ValueError("a must be [terms, batch, N]")
        terms, rows_a = int(a.shape[0]), int(a.shape[1])
        if bhat.dim() == 3 and tuple(bhat.shape) == (terms, rows_a, self.n):
            rows = rows_a
        elif tuple(bhat.shape) in ((terms, self.n), (terms, 1, self.n)):
            rows = 1
        else:
            raise ValueError("bhat must be [terms, batch, N], or [terms, N] / [terms, 1, N] (broadcast)")
        if terms == 0:
            raise ValueError("a has no terms")
        out = a[0] if out is None else out
        if out.dim() != 2 or tuple(out.shape) != (rows_a, self.n):
            raise ValueError("out must be [batch, N]")
        self._batch(a)
        self._batch(out)
        if not bhat.is_cuda or bhat.device.index != self.device:
            raise ValueError("buffer is not on cuda:%d" % self.device)
        if not bhat.is_contiguous() or bhat.element_size() != self.word_bytes:
            raise ValueError("buffer must be contiguous with %d-byte words" % self.word_bytes)
        check(_lib.lib().ntt_polymul_dot_pre(self._h, a.data_ptr(), bhat.data_ptr(), rows, terms, out.data_ptr(), rows_a,
                                             self._stream(stream)), "ntt_polymul_dot_pre")
        return out

    def polymul_matvec_pre(self, a: torch.Tensor, bhat: torch.Tensor, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """out[j] = sum_k a[k]*b[j][k] mod (x^N + 1, p) for every j, all b[j][k] given prepared (ntt_polymul_matvec_pre); needs a kind-2
        table.  a is [K, batch, N]; bhat is [J, K, batch, N], one prepared operand per output, term and row, or [J, K, N] / [J, K, 1, N]:
        one per output and term that multiplies every row (the key-switching case).  a is transformed once for all J outputs.  a is
        overwritten (scratch); `out`, [J, batch, N], is allocated when not given and must not overlap a (unlike polymul_dot_pre's);
        bhat is only read and must not overlap a or out."""
        if a.dim() != 3 or a.shape[2] != self.n:
            raise ValueError("a must be [terms, batch, N]")
        terms, rows_a = int(a.shape[0]), int(a.shape[1])
        if bhat.dim() == 4 and tuple(bhat.shape[1:]) == (terms, rows_a, self.n):
            rows = rows_a
        elif (bhat.dim() == 3 and tuple(bhat.shape[1:]) == (terms, self.n)) or (bhat.dim() == 4 and tuple(bhat.shape[1:]) == (terms, 1, self.n)):
            rows = 1
        else:
            raise ValueError("bhat must be [outs, terms, batch, N], or [outs, terms, N] / [outs, terms, 1, N] (broadcast)")
        outs = int(bhat.shape[0])
        if terms == 0 or outs == 0:
            raise ValueError("a has no terms" if terms == 0 else "bhat has no outputs")
        if out is None:
            out = torch.empty((outs, rows_a, self.n), dtype=a.dtype, device=a.device)
        if out.dim() != 3 or tuple(out.shape) != (outs, rows_a, self.n):
            raise ValueError("out must be [outs, batch, N]")
        self._batch(a)
        self._batch(out)
        if not bhat.is_cuda or bhat.device.index != self.device:
            raise ValueError("buffer is not on cuda:%d" % self.device)
        if not bhat.is_contiguous() or bhat.element_size() != self.word_bytes:
            raise ValueError("buffer must be contiguous with %d-byte words" % self.word_bytes)
        check(_lib.lib().ntt_polymul_matvec_pre(self._h, a.data_ptr(), bhat.data_ptr(), rows, terms, outs, out.data_ptr(), rows_a,
                                                self._stream(stream)), "ntt_polymul_matvec_pre")
        return out

    def _operand(self, t: torch.Tensor) -> None:
        if not t.is_cuda or t.device.index != self.device:
            raise ValueError("buffer is not on cuda:%d" % self.device)
        if not t.is_contiguous() or t.element_size() != self.word_bytes:
            raise ValueError("buffer must be contiguous with %d-byte words" % self.word_bytes)

    def gadget_decompose(self, a: torch.Tensor, log_base: int, levels: int, low_bits: int = 0, out: torch.Tensor | None = None,
                         stream=None) -> torch.Tensor:
        """The balanced gadget digits of a (ntt_gadget_decompose; include/ntt_hip.h has the definition): a is [polys, batch, N] canonical
        words and is only read; the result, [polys, levels, batch, N], viewed as [polys * levels, batch, N] is an operand of
        polymul_dot_pre / polymul_matvec_pre.  Needs no table."""
        if a.dim() != 3 or a.shape[2] != self.n:
            raise ValueError("a must be [polys, batch, N]")
        polys, rows = int(a.shape[0]), int(a.shape[1])
        if polys == 0 or levels < 1:
            raise ValueError("a has no polynomials" if polys == 0 else "levels must be at least 1")
        if out is None:
            out = torch.empty((polys, levels, rows, self.n), dtype=a.dtype, device=a.device)
        if tuple(out.shape) != (polys, levels, rows, self.n):
            raise ValueError("out must be [polys, levels, batch, N]")
        self._operand(a)
        self._operand(out)
        check(_lib.lib().ntt_gadget_decompose(self._h, a.data_ptr(), polys, rows, log_base, levels, low_bits, out.data_ptr(), self._stream(stream)),
              "ntt_gadget_decompose")
        return out

    def polymul_gadget_pre(self, a: torch.Tensor, log_base: int, levels: int, low_bits: int, bhat: torch.Tensor, work: torch.Tensor | None = None,
                           out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """out[j] = sum_t digit_{t mod levels}(a[t div levels]) * b[j][t] mod (x^N + 1, p), all b[j][t] given prepared
        (ntt_polymul_gadget_pre): polymul_matvec_pre of gadget_decompose(a), bit for bit, with the decomposition inside the middle launch
        where the plan has such a kernel.  a is [polys, batch, N] and is NOT written; bhat is [J, polys * levels, batch, N], or
        [J, polys * levels, N] / [J, polys * levels, 1, N] (broadcast); `work`, scratch of polys * levels * batch * N words, and `out`,
        [J, batch, N], are allocated when not given.  The four buffers must not overlap."""
        if a.dim() != 3 or a.shape[2] != self.n:
            raise ValueError("a must be [polys, batch, N]")
        polys, rows_a = int(a.shape[0]), int(a.shape[1])
        if polys == 0 or levels < 1:
            raise ValueError("a has no polynomials" if polys == 0 else "levels must be at least 1")
        terms = polys * levels
        if bhat.dim() == 4 and tuple(bhat.shape[1:]) == (terms, rows_a, self.n):
            rows = rows_a
        elif (bhat.dim() == 3 and tuple(bhat.shape[1:]) == (terms, self.n)) or (bhat.dim() == 4 and tuple(bhat.shape[1:]) == (terms, 1, self.n)):
            rows = 1
        else:
            raise ValueError("bhat must be [outs, polys * levels, batch, N], or [outs, polys * levels, N] / [outs, polys * levels, 1, N] (broadcast)")
        outs = int(bhat.shape[0])
        if outs == 0:
            raise ValueError("bhat has no outputs")
        if work is None:
            work = torch.empty((terms, rows_a, self.n), dtype=a.dtype, device=a.device)
        if work.numel() != terms * rows_a * self.n:
            raise ValueError("work must hold polys * levels * batch * N words")
        if out is None:
            out = torch.empty((outs, rows_a, self.n), dtype=a.dtype, device=a.device)
        if out.dim() != 3 or tuple(out.shape) != (outs, rows_a, self.n):
            raise ValueError("out must be [outs, batch, N]")
        for t in (a, work, bhat, out):
            self._operand(t)
        check(_lib.lib().ntt_polymul_gadget_pre(self._h, a.data_ptr(), polys, log_base, levels, low_bits, work.data_ptr(), bhat.data_ptr(), rows, outs,
                                                out.data_ptr(), rows_a, self._stream(stream)), "ntt_polymul_gadget_pre")
        return out

    def _map_args(self, a: torch.Tensor, kind: int, param: int, exps: torch.Tensor | None, minus_identity: bool) -> tuple[int, int, int, int, int]:
        """(polys, batch, param word, exps pointer or None, flags) of the three *_map calls; the library checks kind, g and the flag"""
        if a.dim() != 3 or a.shape[2] != self.n:
            raise ValueError("a must be [polys, batch, N]")
        polys, rows = int(a.shape[0]), int(a.shape[1])
        if polys == 0:
            raise ValueError("a has no polynomials")
        ptr = None
        if exps is not None:
            if not exps.is_cuda or exps.device.index != self.device:
                raise ValueError("exps is not on cuda:%d" % self.device)
            if exps.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or not exps.is_contiguous() or exps.numel() != rows:
                raise ValueError("exps must be a contiguous uint32 / int32 tensor of batch elements")
            ptr = exps.data_ptr()
        return polys, rows, int(param) & 0xFFFFFFFF, ptr, _lib.NTT_MAP_MINUS_IDENTITY if minus_identity else 0

    def negacyclic_map(self, a: torch.Tensor, kind: int, param: int = 0, exps: torch.Tensor | None = None, minus_identity: bool = False,
                       out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """The signed coefficient permutation of every row of a (ntt_negacyclic_map; include/ntt_hip.h has the definition): kind
        NTT_MAP_MONOMIAL gives X^e * a mod (x^N + 1) with e = exps[r] for row r of every polynomial (a device tensor of batch words, read on
        the device) or, without exps, e = param for every row -- any integer, taken mod 2N --; kind NTT_MAP_AUTOMORPHISM gives a(X^g) with
        g = param odd and below 2N.  minus_identity subtracts a itself.  a is [polys, batch, N] canonical words and is only read; `out`, of
        the same shape, must not overlap it.  Needs no table."""
        polys, rows, word, ptr, flags = self._map_args(a, kind, param, exps, minus_identity)
        if out is None:
            out = self._out_like(a, stream)
        if tuple(out.shape) != tuple(a.shape):
            raise ValueError("out must be [polys, batch, N]")
        self._operand(a)
        self._operand(out)
        check(_lib.lib().ntt_negacyclic_map(self._h, a.data_ptr(), out.data_ptr(), polys, rows, kind, word, ptr, flags, self._stream(stream)), "ntt_negacyclic_map")
        return out

    def gadget_decompose_map(self, a: torch.Tensor, kind: int, param: int = 0, exps: torch.Tensor | None = None, minus_identity: bool = False, *,
                             log_base: int, levels: int, low_bits: int = 0, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """gadget_decompose(negacyclic_map(a, ...)), bit for bit, in one launch (ntt_gadget_decompose_map): [polys, levels, batch, N]."""
        polys, rows, word, ptr, flags = self._map_args(a, kind, param, exps, minus_identity)
        if levels < 1:
            raise ValueError("levels must be at least 1")
        if out is None:
            out = torch.empty((polys, levels, rows, self.n), dtype=a.dtype, device=a.device)
        if tuple(out.shape) != (polys, levels, rows, self.n):
            raise ValueError("out must be [polys, levels, batch, N]")
        self._operand(a)
        self._operand(out)
        check(_lib.lib().ntt_gadget_decompose_map(self._h, a.data_ptr(), polys, rows, kind, word, ptr, flags, log_base, levels, low_bits, out.data_ptr(),
                                                  self._stream(stream)), "ntt_gadget_decompose_map")
        return out

    def polymul_gadget_map_pre(self, a: torch.Tensor, kind: int, param: int = 0, exps: torch.Tensor | None = None, minus_identity: bool = False, *,
                               log_base: int, levels: int, low_bits: int, bhat: torch.Tensor, addend: torch.Tensor | None = None,
                               work: torch.Tensor | None = None, out: torch.Tensor | None = None, stream=None) -> torch.Tensor:
        """polymul_gadget_pre(negacyclic_map(a, ...), ...) + addend, bit for bit (ntt_polymul_gadget_map_pre): the map and the digits in one
        launch a -> work, the matrix-vector product of work, and with `addend`, [J, batch, N] canonical words, out[j] += addend[j] mod p.
        addend may be a itself (J == polys: the blind-rotation step) or any buffer apart from work and out.  The other arguments are
        polymul_gadget_pre's; a is NOT written."""
        polys, rows_a, word, ptr, flags = self._map_args(a, kind, param, exps, minus_identity)
        if levels < 1:
            raise ValueError("levels must be at least 1")
        terms = polys * levels
        if bhat.dim() == 4 and tuple(bhat.shape[1:]) == (terms, rows_a, self.n):
            rows = rows_a
        elif (bhat.dim() == 3 and tuple(bhat.shape[1:]) == (terms, self.n)) or (bhat.dim() == 4 and tuple(bhat.shape[1:]) == (terms, 1, self.n)):
            rows = 1
        else:
            raise ValueError("bhat must be [outs, polys * levels, batch, N], or [outs, polys * levels, N] / [outs, polys * levels, 1, N] (broadcast)")
        outs = int(bhat.shape[0])
        if outs == 0:
            raise ValueError("bhat has no outputs")
        if work is None:
            work = torch.empty((terms, rows_a, self.n), dtype=a.dtype, device=a.device)
        if work.numel() != terms * rows_a * self.n:
            raise ValueError("work must hold polys * levels * batch * N words")
        if out is None:
            out = torch.empty((outs, rows_a, self.n), dtype=a.dtype, device=a.device)
        if out.dim() != 3 or tuple(out.shape) != (outs, rows_a, self.n):
            raise ValueError("out must be [outs, batch, N]")
        if addend is not None and tuple(addend.shape) != (outs, rows_a, self.n):
            raise ValueError("addend must be [outs, batch, N]")
        for t in (a, work, bhat, out) + (() if addend is None else (addend,)):
            self._operand(t)
        check(_lib.lib().ntt_polymul_gadget_map_pre(self._h, a.data_ptr(), polys, kind, word, ptr, flags, log_base, levels, low_bits, work.data_ptr(), bhat.data_ptr(),
                                                    rows, outs, None if addend is None else addend.data_ptr(), out.data_ptr(), rows_a, self._stream(stream)),
              "ntt_polymul_gadget_map_pre")
        return out

    def count_noncanonical(self, buf: torch.Tensor) -> int:
        """How many words of `buf` are >= p (the transforms require canonical residues)."""
        b = self._batch(buf)
        n = C.c_uint64(0)
        check(_lib.lib().ntt_count_noncanonical(self._h, buf.data_ptr(), b, C.byref(n)), "ntt_count_noncanonical")
        return int(n.value)

    def forward_stages(self, inp: torch.Tensor, stage: int, out: torch.Tensor | None = None,
                       stream=None) -> torch.Tensor:
        """Stages 0..stage only (the reference's test_stage hook, src/test.cpp:55-58, 67)."""
        out = self._out_like(inp, stream) if out is None else out
        b = self._batch(inp, out)
        check(_lib.lib().ntt_forward_stages(self._h, inp.data_ptr(), out.data_ptr(), b, stage,
                                            self._stream(stream)), "ntt_forward_stages")
        return out


def lde_from_evals(small_plan: NTTPlan, big_plan: NTTPlan, evals: torch.Tensor, out: torch.Tensor | None = None,
                   layout: int = LAYOUT_NATURAL, stream=None, coeffs: torch.Tensor | None = None) -> torch.Tensor:
    """Values of each row's polynomial on the coset big_plan was configured for (set_coset), from its values on <w_N>.
    small_plan (size N) and big_plan (size M = N << log_blowup) hold kind-1 tables from the same generator.  Two steps: the scaled
    inverse at size N (coefficients, in the bit-reversed order the network returns) and big_plan.lde(); `coeffs` is an optional
    [batch][N] scratch buffer for the coefficients (default: allocated; pass `evals` itself to transform in place)."""
    if small_plan.logn + big_plan.log_blowup != big_plan.logn or small_plan.p != big_plan.p or small_plan.word_bytes != big_plan.word_bytes:
        raise ValueError("plans do not match: need logn_small + log_blowup == logn_big, same modulus and word size")
    c = small_plan.inverse(evals, coeffs, scale=True, stream=stream)
    return big_plan.lde(c, out, layout=layout, stream=stream)
