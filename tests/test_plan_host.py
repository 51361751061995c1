"""The host planning of promp_amd/csrc/promp_plan.h -- network shapes and padding, the Gram / fit kernel dispatch of sample
processing, the step tables, k_gram_tiled's wave map -- run on the host alone: tests/host/plan_check.cpp includes the header and
nothing else of the project, is built with AddressSanitizer and UBSan, and says what does not hold.  No GPU, no emulator."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'plan_check.cpp')
HEADER = os.path.join(ROOT, 'promp_amd', 'csrc', 'promp_plan.h')


def test_plan_header_compiles_alone():
    """plain g++ -std=c++17, no HIP header, no emulator define, no kernel header"""
    gxx = shutil.which('g++')
    assert gxx, 'g++ is required'
    r = subprocess.run([gxx, '-std=c++17', '-fsyntax-only', '-Wall', '-Wextra', '-Werror', '-x', 'c++', '-include', HEADER, os.devnull],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_plan_check(tmp_path):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is required'
    exe = str(tmp_path / 'plan_check')
    r = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall', '-Wextra',
                        SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, 'plan_check failed:\n' + r.stdout + r.stderr
    assert 'all expectations hold' in r.stdout
