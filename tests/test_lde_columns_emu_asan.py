"""The coset twins of the matrix column pass in the host index model under AddressSanitizer and UBSan (tests/emu/emu_lde_columns.cpp
-DEMU_LDE_COLUMNS_MAIN), built exactly as test_columns_emu_asan.py builds its own: a stand-alone executable run as a subprocess,
nothing loaded into Python.  malloc() buffers of EXACTLY (count * rows - 1) * pitch + width words, input and output separately --
the footprints include/ntt_hip.h promises are sufficient -- for three word classes x {lde, coset inverse} x logn {4, 5, 8, 9, 12} x
every legal blow-up x width {1, 3, 16, 17, 33} x pitch {width, width + 1, next power of two + 16} (input and output pitch differ
for the lde) x count {1, 3}, the coset inverse in place and out of place, ppw 1 and > 1, plus 49 matrices of 16 rows (ragged last
group).  Padding columns hold a sentinel >= p before and after; every live word is the oracle's network on the expanded / scaled
column."""
import os
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "emu", "emu_lde_columns.cpp")
ORACLE_C = os.path.join(ROOT, "oracle", "ntt_oracle.c")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
FIELDS = {"gl": 1, "m64": 2, "m32": 4}  # EMU_LDE_COLUMNS_FIELDS bit of each executable


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
    tmp = str(tmp_path_factory.mktemp("lde_columns_asan"))
    if not _sanitizers_available(tmp):
        pytest.skip("no g++ with the ASan / UBSan runtimes")
    obj = os.path.join(tmp, "oracle.o")
    subprocess.check_call(["gcc", "-O2", "-fopenmp", "-c", ORACLE_C, "-o", obj])

    def one(item):
        name, bit = item
        exe = os.path.join(tmp, "lde_columns_" + name)
        r = subprocess.run(["g++", "-O1", "-g1", "-std=c++17", *SAN, "-DEMU_LDE_COLUMNS_MAIN", f"-DEMU_LDE_COLUMNS_FIELDS={bit}", SRC, obj, "-fopenmp", "-o", exe],
                           capture_output=True, text=True)
        assert r.returncode == 0, f"{name}: {r.stderr[-2000:]}"
        return name, exe

    with ThreadPoolExecutor(max_workers=3) as ex:
        return dict(ex.map(one, FIELDS.items()))


def test_lde_columns_sweep_is_clean(exes):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=98", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1",
               OMP_NUM_THREADS="1")
    with ThreadPoolExecutor(max_workers=3) as ex:
        results = list(ex.map(lambda kv: (kv[0], subprocess.run([kv[1], kv[0]], capture_output=True, text=True, env=env, timeout=1500)), exes.items()))
    total = 0
    for name, r in results:
        assert r.returncode == 0, f"{name}: exit {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-4000:]}"
        assert "cases clean" in r.stdout
        total += int(r.stdout.strip().splitlines()[-1].split(":")[1].split()[0])
    assert total >= 2400  # 3 x 815: the sweep did not silently shrink
