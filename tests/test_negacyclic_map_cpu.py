"""The signed negacyclic maps on the CPU: the loops of negacyclic_map_kernel (csrc/negacyclic_map.h: negacyclic_map_thread, the chunk loop
and the word tail, the one body the device kernel runs) in a stand-alone program under AddressSanitizer and UBSan
(tests/emu/emu_negacyclic_map.cpp, its own main, exact-size malloc() buffers for a, the output and the exponents; nothing is loaded into
Python), compared inside the program with a scatter from the ring definition and here -- through its `dump` mode -- with
negacyclic_map_ref, the reference the GPU tests use; and the host's Newton inverse of g against pow(g, -1, 2N)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import negacyclic_map_ref as M

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "emu", "emu_negacyclic_map.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=98", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
# 4 moduli x 5 sizes x 3 batches x 2 polynomial counts x 2 flag values x (11 exponent cases + the g below 2N: 2 at N = 2, 4 at N = 4, else 5)
# x (no digits, 3 levels, 1 level) = 11376 when this was written
FLOOR = 11376
GOLD, M64 = 0xFFFFFFFF00000001, 0x3FFFFFEE00000001


def _sanitizers_available(tmp):
    if shutil.which("g++") is None:
        return False
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SAN, src, "-o", os.path.join(tmp, "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([os.path.join(tmp, "probe")]).returncode == 0


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("negacyclic_map_asan"))
    if not _sanitizers_available(tmp):
        pytest.skip("no g++ with the ASan / UBSan runtimes")
    out = os.path.join(tmp, "emu_negacyclic_map")
    r = subprocess.run(["g++", "-O1", "-g1", "-std=c++17", *SAN, SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_kernel_loops_are_clean_and_match_the_ring_definition(exe):
    r = subprocess.run([exe], capture_output=True, text=True, env=ENV, timeout=600)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-4000:]}"
    last = r.stdout.strip().splitlines()[-1]
    assert last.endswith("cases clean"), last
    assert int(last.split(":")[1].split()[0]) >= FLOOR  # the sweep did not silently shrink


# (word bytes, p, logn, batch, polys, kind, param, per-row exponents, flags, (w, K, l))
DUMPS = [
    (4, 3329, 1, 5, 2, 0, 1, False, 1, (4, 3, 0)),           # N = 2 of 4-byte words, an odd batch: the word tail alone
    (4, 3329, 1, 2, 1, 0, 3, False, 0, (6, 1, 0)),           # ... an even batch: whole chunks of rows shorter than a chunk
    (4, 3221225473, 3, 5, 2, 0, 0, True, 1, (8, 3, 8)),      # p above 2^31, device exponents
    (4, 3221225473, 6, 33, 1, 1, 65, False, 1, (12, 1, 4)),  # g = N + 1
    (8, GOLD, 2, 5, 2, 0, 0xFFFFFFFF, False, 1, (8, 3, 40)),  # e = -1 as an unsigned word
    (8, GOLD, 6, 33, 2, 0, 0, True, 0, (16, 1, 0)),
    (8, M64, 3, 5, 1, 1, 15, False, 0, (10, 3, 32)),         # g = 2N - 1
    (8, M64, 10, 5, 2, 1, 5, False, 1, (16, 1, 0)),
]


@pytest.mark.parametrize("wb,p,logn,batch,polys,kind,param,perrow,flags,dig", DUMPS)
def test_program_output_equals_the_python_reference(exe, tmp_path, wb, p, logn, batch, polys, kind, param, perrow, flags, dig):
    w, K, l = dig
    path = str(tmp_path / "case.bin")
    r = subprocess.run([exe, "dump", str(wb), str(p), str(logn), str(batch), str(polys), str(kind), str(param), str(int(perrow)), str(flags), str(w), str(K), str(l),
                        str(1000 + logn), path], capture_output=True, text=True, env=ENV, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    dt, n = (np.uint32 if wb == 4 else np.uint64), 1 << logn
    raw = open(path, "rb").read()
    words = polys * batch * n
    a = np.frombuffer(raw, dtype=dt, count=words).reshape(polys, batch, n)
    exps = np.frombuffer(raw, dtype=np.uint32, count=batch, offset=words * wb)
    got = np.frombuffer(raw, dtype=dt, count=words, offset=words * wb + 4 * batch).reshape(polys, batch, n)
    digits = np.frombuffer(raw, dtype=dt, count=words * K, offset=2 * words * wb + 4 * batch).reshape(polys, K, batch, n)
    assert len(raw) == (2 + K) * words * wb + 4 * batch
    e = exps if perrow else None
    assert np.array_equal(got, M.mapped_int(a, p, kind, param, e, bool(flags)))
    assert np.array_equal(got, M.mapped(a, p, kind, param, e, bool(flags)))  # the numpy form of the same scatter, used at the large shapes
    assert np.array_equal(digits, M.decompose(a, p, kind, param, e, bool(flags), w, K, l))
    assert int(a.max()) < p


def test_reference_identities():
    """the reference itself, on the hand-checked cases of the definition: e = 1 gives y[0] = -a[N - 1] and y[1] = a[0]; e = N gives -a; X^e after
    X^f is X^(e + f); sigma_g after sigma_h is sigma_(g h); g = 1 and e = 0 are the identity"""
    p, n = 3329, 8
    a = [(7 * i + 3) % p for i in range(n)]
    y = M.monomial_row(a, 1, p)
    assert y[0] == (-a[n - 1]) % p and y[1] == a[0]
    assert M.monomial_row(a, n, p) == [(-x) % p for x in a]
    assert M.monomial_row(a, 2 * n, p) == a and M.monomial_row(a, 0, p) == a and M.automorphism_row(a, 1, p) == a
    assert M.monomial_row(a, -1 & 0xFFFFFFFF, p) == M.monomial_row(a, 2 * n - 1, p)
    for e in range(2 * n):
        for f in (1, 5, n + 2):
            assert M.monomial_row(M.monomial_row(a, e, p), f, p) == M.monomial_row(a, e + f, p)
    for g in range(1, 2 * n, 2):
        for h in (3, 2 * n - 1):
            assert M.automorphism_row(M.automorphism_row(a, g, p), h, p) == M.automorphism_row(a, (g * h) % (2 * n), p)
        # sigma_g(X . a) = X^g . sigma_g(a)
        assert M.automorphism_row(M.monomial_row(a, 1, p), g, p) == M.monomial_row(M.automorphism_row(a, g, p), g, p)


def test_newton_inverse_of_g():
    for logn in range(1, 9):
        for g in range(1, 2 << logn, 2):
            assert M.ginv(g, logn) == pow(g, -1, 2 << logn), (g, logn)
    for logn in (16, 28):  # the largest size: the 32-bit iteration still has every bit it needs
        for g in (1, 3, 5, (1 << logn) + 1, (2 << logn) - 1, 0x0ABCDEF1 & ((2 << logn) - 1) | 1):
            assert M.ginv(g, logn) == pow(g, -1, 2 << logn), (g, logn)
