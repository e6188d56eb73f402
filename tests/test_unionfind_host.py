"""
The union-find of ``csrc/unionfind.hip.h`` under host threads (CPU tier): ``tests/unionfind_host.cpp`` includes the header through
the host side of its atomic shim -- the same text the join kernels compile -- and 16 threads unite the edges of a clique, of three
long paths and of a random sparse graph, then flatten.  The program itself checks every ``parent[i]`` against a sequential DFS and
``parent[i] <= i`` after every operation; this test compiles it as a stand-alone program under the thread sanitizer (without it
where the compiler has no runtime for it) and runs the binary.
"""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "unionfind_host.cpp")
INCLUDE = os.path.join(ROOT, "iscc_search_amd", "csrc")


def compile_program(out, sanitize):
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-pthread", "-I", INCLUDE, "-o", out, SOURCE]
    if sanitize:
        cmd.insert(1, "-fsanitize=thread")
    return subprocess.run(cmd, capture_output=True, text=True)


def test_unionfind_under_threads(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to compile tests/unionfind_host.cpp")
    binary = str(tmp_path / "unionfind_host")
    built = compile_program(binary, sanitize=True)
    sanitized = built.returncode == 0
    if not sanitized:
        # no thread-sanitizer runtime for this compiler: the program's own checks still run
        print("compiling without -fsanitize=thread:", built.stderr[-400:])
        built = compile_program(binary, sanitize=False)
    assert built.returncode == 0, built.stderr
    run = subprocess.run([binary], capture_output=True, text=True)
    if sanitized and "FATAL: ThreadSanitizer" in run.stderr:
        # the runtime is there but cannot start on this machine (its address-space layout, not a finding about the program:
        # those are WARNINGs): as without the runtime
        print("running without -fsanitize=thread:", run.stderr[-400:])
        built = compile_program(binary, sanitize=False)
        assert built.returncode == 0, built.stderr
        run = subprocess.run([binary], capture_output=True, text=True)
    print(run.stdout)
    print(run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ThreadSanitizer" not in run.stderr
    lines = run.stdout.strip().splitlines()
    assert lines[-1] == "ok" and len(lines) == 6
    for name in ("clique", "path, ascending labels", "path, descending labels", "path, permuted labels", "random sparse"):
        assert any(line.startswith(name) and ": 0 entries above their index, 0 not the component minimum" in line for line in lines), name
