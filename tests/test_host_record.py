"""csrc/slrecord.h's put_record_at -- the packer of the mesh writers' 13-byte face and 51-byte coloured vertex records
-- over record counts around one, a quarter and a whole workgroup, in ascending and in descending record order,
against the byte-wise concatenation of the records and a canary after them, in a stand-alone program
(tests/host/record_pack_check.cpp) built by the host C++ compiler with the address and undefined-behaviour sanitizers
and run here, on the CPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "host", "record_pack_check.cpp")
INCLUDES = [os.path.join(REPO, "structured_light_for_3d_model_replication_amd", "csrc")]


def test_put_record_at_in_both_orders(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "c++")) or shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "record_pack_check")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           *[f"-I{d}" for d in INCLUDES], SRC, "-o", exe]
    # the sanitizers' runtimes inside the program where the compiler has them as archives (GCC links them shared by
    # default, and a shared one insists on being the first library a process loads)
    built = subprocess.run(cmd + ["-static-libasan", "-static-libubsan"], capture_output=True, text=True)
    if built.returncode != 0:
        built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr
    ran = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert ran.returncode == 0, ran.stdout[-4000:] + ran.stderr[-4000:]
    assert ran.stdout.strip().endswith("put_record_at: 0 failed checks"), ran.stdout[-2000:]
