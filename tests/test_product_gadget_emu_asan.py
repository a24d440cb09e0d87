"""ntt_polymul_gadget_pre in the host index model under AddressSanitizer and UBSan (tests/emu/emu_product_gadget.cpp
-DEMU_PRODUCT_GADGET_MAIN), the way test_product_mv_emu_asan.py runs the matrix-vector product: a stand-alone program on exact-size
malloc() buffers -- polys * batch * N words of a, polys * levels * batch * N words of work, outs * polys * levels * bhat_rows * N words of
b^, outs * batch * N words of out -- for three word classes x the size below the smallest unit, every fused unit size and a two-pass size x
ragged batches (1, 5, 33) x 1 and 2 polynomials x four digit parameter sets x 1, 2 and 3 outputs x per-row and broadcast x every plan
alternative, each case compared with the oracle on digits computed from the definition in 128-bit integers, and a compared with its copy.
Nothing is loaded into Python.  The digit launches read a directly, so the last polynomial's last unit of a ends exactly where its
allocation ends; a BROADCAST on a ragged batch through the two-output digit kernel ends the allocation of b^ the same way."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emu", "emu_product_gadget.cpp")
ORACLE_C = os.path.join(ROOT, "oracle", "ntt_oracle.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
FIELDS = {"gl": 1, "m64": 2, "m32": 4}  # EMU_PRODUCT_GADGET_FIELDS bit of each executable
FLOOR = 134  # cases of the three programs together (gl 42 + m64 42 + m32 50 when this was written)


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
    tmp = str(tmp_path_factory.mktemp("product_gadget_asan"))
    if not _sanitizers_available(tmp):
        pytest.skip("no g++ with the ASan / UBSan runtimes")
    obj = os.path.join(tmp, "oracle.o")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-c", ORACLE_C, "-o", obj])

    def one(item):
        name, bit = item
        exe = os.path.join(tmp, "product_gadget_" + name)
        r = subprocess.run(["g++", "-O1", "-g1", "-std=c++17", *SAN, "-DEMU_PRODUCT_GADGET_MAIN", "-DNTT_EXPERIMENT", f"-DEMU_PRODUCT_GADGET_FIELDS={bit}", SRC, obj, "-fopenmp", "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{name}: {r.stderr[-2000:]}"
        return name, exe

    with ThreadPoolExecutor(max_workers=3) as ex:
        return dict(ex.map(one, FIELDS.items()))


def test_product_gadget_sweep_is_clean(exes):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=98", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               OMP_NUM_THREADS="1")
    with ThreadPoolExecutor(max_workers=3) as ex:
        results = list(ex.map(lambda kv: (kv[0], subprocess.run([kv[1], kv[0]], capture_output=True, text=True, env=env, timeout=600)), exes.items()))
    total = 0
    for name, r in results:
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-4000:]}"
        assert "cases clean" in r.stdout
        total += int(r.stdout.strip().splitlines()[-1].split(":")[1].split()[0])
        # the programs are the model of the EXPERIMENT build (-DNTT_EXPERIMENT), which keeps the digit kernels of every word class and
        # pairs outputs for every class (launch.h: product_gadget_unit, product_mv_unit).  The digit launches ran, and THE case -- a ragged
        # broadcast through the two-output digit kernel -- occurred: the program itself fails when a size that pairs has none
        fused = [int(l.split(":")[1].split()[0]) for l in r.stdout.splitlines() if l.endswith("cases with digit launches")]
        assert len(fused) == 1 and fused[0] > 0, (name, fused)
        point = [int(l.split(":")[1].split()[0]) for l in r.stdout.splitlines() if l.endswith("paired ragged broadcast cases")]
        assert len(point) == 1 and point[0] > 0, (name, point)
    assert total >= FLOOR  # the sweep did not silently shrink
