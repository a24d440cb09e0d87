"""ntt_polymul_negacyclic_pre in the host index model under AddressSanitizer and UBSan (tests/emu/emu_product_pre.cpp
-DEMU_PRODUCT_PRE_MAIN), the way test_lde_emu_asan.py runs the fused expansion: a stand-alone program on exact-size malloc() buffers --
batch * N words of a and of out, bhat_rows * N words of b^ -- for three word classes x every fused unit size, a two-pass and a
three-pass size x ragged batches x per-row and broadcast x every plan alternative, each case also compared with the oracle.  The
ragged last polynomial group of a BROADCAST is the point: the lanes of polynomials that do not exist must not reach past the one row
of b^, and the address rule the sweep steps (pass.h: pre_addr) is the one the GPU runs."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emu", "emu_product_pre.cpp")
ORACLE_C = os.path.join(ROOT, "oracle", "ntt_oracle.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
FIELDS = {"gl": 1, "m64": 2, "m32": 4}  # EMU_PRODUCT_PRE_FIELDS bit of each executable
FLOOR = 450  # cases of the three programs together (gl 146 + m64 146 + m32 172 when this was written)


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
    tmp = str(tmp_path_factory.mktemp("product_pre_asan"))
    if not _sanitizers_available(tmp):
        pytest.skip("no g++ with the ASan / UBSan runtimes")
    obj = os.path.join(tmp, "oracle.o")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-c", ORACLE_C, "-o", obj])

    def one(item):
        name, bit = item
        exe = os.path.join(tmp, "product_pre_" + name)
        r = subprocess.run(["g++", "-O1", "-g1", "-std=c++17", *SAN, "-DEMU_PRODUCT_PRE_MAIN", f"-DEMU_PRODUCT_PRE_FIELDS={bit}", SRC, obj, "-fopenmp", "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{name}: {r.stderr[-2000:]}"
        return name, exe

    with ThreadPoolExecutor(max_workers=3) as ex:
        return dict(ex.map(one, FIELDS.items()))


def test_product_pre_sweep_is_clean(exes):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=98", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               OMP_NUM_THREADS="1")
    with ThreadPoolExecutor(max_workers=3) as ex:
        results = list(ex.map(lambda kv: (kv[0], subprocess.run([kv[1], kv[0]], capture_output=True, text=True, env=env, timeout=1500)), exes.items()))
    total = 0
    for name, r in results:
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-4000:]}"
        assert "cases clean" in r.stdout
        total += int(r.stdout.strip().splitlines()[-1].split(":")[1].split()[0])
    assert total >= FLOOR  # the sweep did not silently shrink
