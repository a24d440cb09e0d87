"""ntt_polymul_matvec_pre in the host index model under AddressSanitizer and UBSan (tests/emu/emu_product_mv.cpp -DEMU_PRODUCT_MV_MAIN),
the way test_product_dot_emu_asan.py runs the inner product: a stand-alone program on exact-size malloc() buffers -- terms * batch * N
words of a, outs * terms * bhat_rows * N words of b^, outs * batch * N words of out -- for three word classes x every fused unit size, a
two-pass and a three-pass size x ragged batches (1, 3, 5, 9, 17, 33) x 2, 3 and 4 outputs x 1, 2, 3 and 5 terms x per-row and broadcast x
every plan alternative, each case also compared with the oracle.  Nothing is loaded into Python.  The SECOND output's last term of a
BROADCAST with a ragged last polynomial group is the point: the lanes of polynomials that do not exist must not reach past that term's
single row, where the allocation of b^ ends exactly, and the address rule the sweep steps (pass.h: pre_addr, per output and term) is
the one the GPU runs."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emu", "emu_product_mv.cpp")
ORACLE_C = os.path.join(ROOT, "oracle", "ntt_oracle.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
FIELDS = {"gl": 1, "m64": 2, "m32": 4}  # EMU_PRODUCT_MV_FIELDS bit of each executable
FLOOR = 309  # cases of the three programs together (gl 97 + m64 97 + m32 115 when this was written)


def _sanitizers_available(tmp):
    if shutil.which("g++") is None:
        return False
    src = os.path.join(tmp, "probe.cpp")
    with open(src, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", *SAN, src, "-o", os.path.join(tmp, "probe")], capture_output=True, text=True)
    return r.returncode == 0 and subprocess.run([os.path.join(tmp, "probe")]).returncode == 0


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("product_mv_asan"))
    if not _sanitizers_available(tmp):
        pytest.skip("no g++ with the ASan / UBSan runtimes")
    obj = os.path.join(tmp, "oracle.o")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-c", ORACLE_C, "-o", obj])

    def one(item):
        name, bit = item
        exe = os.path.join(tmp, "product_mv_" + name)
        r = subprocess.run(["g++", "-O1", "-g1", "-std=c++17", *SAN, "-DEMU_PRODUCT_MV_MAIN", f"-DEMU_PRODUCT_MV_FIELDS={bit}", SRC, obj, "-fopenmp", "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{name}: {r.stderr[-2000:]}"
        return name, exe

    with ThreadPoolExecutor(max_workers=3) as ex:
        return dict(ex.map(one, FIELDS.items()))


def test_product_mv_sweep_is_clean(exes):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=98", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               OMP_NUM_THREADS="1")
    with ThreadPoolExecutor(max_workers=3) as ex:
        results = list(ex.map(lambda kv: (kv[0], subprocess.run([kv[1], kv[0]], capture_output=True, text=True, env=env, timeout=1500)), exes.items()))
    total = 0
    for name, r in results:
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-4000:]}"
        assert "cases clean" in r.stdout
        total += int(r.stdout.strip().splitlines()[-1].split(":")[1].split()[0])
        # THE case -- a ragged broadcast through the two-output kernel -- occurred: the program itself fails when a size that pairs has
        # none; here, that the classes the library pairs for have any at all (Goldilocks runs summed launches: launch.h, product_mv_unit)
        point = [int(l.split(":")[1].split()[0]) for l in r.stdout.splitlines() if l.endswith("paired ragged broadcast cases")]
        assert len(point) == 1 and (point[0] > 0) == (name != "gl"), (name, point)
    assert total >= FLOOR  # the sweep did not silently shrink
