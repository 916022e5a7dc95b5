"""The pair cache's table (csrc/yrwi_pair_cache.h: key, LRU, pins, generations,
byte budget, block allocation), checked on the CPU: tests/pair_cache_main.cpp is
compiled as a stand-alone program with the address and undefined-behaviour
sanitizers and run."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_cache_table_program(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = tmp_path / "pair_cache"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "pair_cache_main.cpp"), "-o", str(exe)],
                   check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pair_cache: OK" in r.stdout
