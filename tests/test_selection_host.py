"""The selections of promp_amd/csrc/promp_plan.h (subsampled constraint products: the count rule, the validation of a selection,
the compact slab's offsets and tables) run on the host alone: tests/host/selection_check.cpp includes the header and nothing
else of the project, is built with AddressSanitizer and UBSan, and says what does not hold.  No GPU, no emulator."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'selection_check.cpp')


def test_selection_check(tmp_path):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is required'
    exe = str(tmp_path / 'selection_check')
    r = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall', '-Wextra',
                        SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, 'selection_check failed:\n' + r.stdout + r.stderr
    assert 'all expectations hold' in r.stdout


def test_python_count_rule_is_the_headers():
    """the optimizer's own count (it draws the subsample) against exact integer arithmetic, at the same values"""
    from promp_amd.optimizers.conjugate_gradient_optimizer import subsample_counts
    for pct in (10, 20, 25, 29, 30, 50, 70, 100):
        paths = [1, 3, 5, 10, 20, 100]
        assert subsample_counts(pct / 100.0, paths) == [max(1, pct * p // 100) for p in paths], pct
    assert subsample_counts(np.float32(0.5), [4, 4, 4]) == [2, 2, 2]
