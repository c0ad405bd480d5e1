"""CPU: the workspace arena (csrc/arena.h) and its two-pass plan on host memory. tests/arena_check.cpp is a stand-alone
program (its own main, arena.h its only project header) built here with the host C++ compiler under AddressSanitizer and
UBSan: a counting pass and a real pass give the same offsets and total, every buffer is 256-byte aligned, the capacity is
the counted total to the byte (the last byte is written, one byte less refuses the last get), a larger plan grows the
arena and a smaller one leaves it alone, and a layout that differs between its passes is SVC_ERR_STATE."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compiler():
    """the host C++ compiler: $CXX, g++ / c++ / clang++, or hipcc compiling plain C++"""
    for cxx in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        if cxx and shutil.which(cxx):
            return [shutil.which(cxx)]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "no host C++ compiler found"
    return [hipcc, "-x", "c++"]


def test_arena_plan_on_host_memory(tmp_path):
    exe = str(tmp_path / "arena_check")
    cmd = _compiler() + ["-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                         "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "svc_inference_pipeline_amd", "csrc"),
                         os.path.join(REPO, "tests", "arena_check.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "arena_check: ok" in r.stdout
