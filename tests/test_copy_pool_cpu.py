"""The staging copy of csrc/copy_pool.hpp on its own, on the CPU: tests/native/copy_pool_test.cpp
built twice, with -fsanitize=address,undefined and with -fsanitize=thread, and run as an ordinary
program (no GPU, nothing loaded into this interpreter, no preloaded runtime).

The program compares every copy with its source byte for byte, into a poisoned destination between
two guards, for KZGMI_COPY_THREADS of 1 to 33, lengths around the 2 MiB threshold, every remainder
of 64 * parts, the 16 MiB ring size and the three lengths whose tail the earlier part arithmetic
(per = (len / parts + 63) & ~63) never copied; and four host threads sharing one pool.  It prints
one line per failing case; a sanitizer report fails the run as well."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "kzg-batch-verification-scheme_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "native", "copy_pool_test.cpp")
COMPILERS = ["g++", "clang++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]
KINDS = {
    "asan_ubsan": ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
    "tsan": ["-fsanitize=thread"],
}
# a report of any sanitizer ends the run with a status of its own
ENV = {"ASAN_OPTIONS": "exitcode=97:detect_leaks=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1",
       "TSAN_OPTIONS": "exitcode=98:halt_on_error=1"}


def _flags(kind):
    return ["-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-pthread"] + KINDS[kind]


def _compiler_for(kind, tmp):
    """The first compiler that builds and runs an empty program of this kind (it has the runtime)."""
    probe = os.path.join(tmp, "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    for cxx in COMPILERS:
        exe = shutil.which(cxx)
        if not exe:
            continue
        out = os.path.join(tmp, "probe_" + kind)
        r = subprocess.run([exe] + _flags(kind) + [probe, "-o", out], capture_output=True, text=True, timeout=120)
        if r.returncode == 0 and subprocess.run([out], capture_output=True, timeout=60, env=_run_env()).returncode == 0:
            return exe
    return None


def _run_env():
    env = dict(os.environ)
    env.update(ENV)
    return env


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("copy_pool"))
    exes = {}
    for kind in KINDS:
        cxx = _compiler_for(kind, tmp)
        if cxx is None:
            continue
        exe = os.path.join(tmp, "copy_pool_test_" + kind)
        r = subprocess.run([cxx] + _flags(kind) + ["-I", CSRC, SRC, "-o", exe], capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        exes[kind] = exe
    return exes


@pytest.mark.parametrize("kind", list(KINDS))
def test_copy_pool_under_sanitizer(built, kind):
    if kind not in built:
        pytest.skip("no compiler here builds and runs a %s program" % KINDS[kind][0])
    r = subprocess.run([built[kind]], capture_output=True, text=True, timeout=600, env=_run_env())
    tail = (r.stdout[-3000:] + "\n" + r.stderr[-3000:]).strip()
    assert r.returncode == 0, tail
    assert r.stdout.strip().splitlines()[-1] == "ok: 0 failing cases", tail
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, tail


def test_copy_pool_header_is_plain_cpp():
    """csrc/copy_pool.hpp includes no HIP header and reads no environment variable: api.hip's
    copy_pool() passes KZGMI_COPY_THREADS in, and this program passes its thread counts."""
    with open(os.path.join(CSRC, "copy_pool.hpp")) as f:
        text = f.read()
    includes = re.findall(r'#\s*include\s*[<"]([^>"]+)[>"]', text)
    assert includes and not [i for i in includes if "hip" in i.lower() or i.endswith(".hpp")], includes
    assert "getenv" not in text
    with open(os.path.join(CSRC, "api.hip")) as f:
        api = f.read()
    assert '#include "copy_pool.hpp"' in api and 'getenv("KZGMI_COPY_THREADS")' in api
    assert "class CopyPool" not in api
