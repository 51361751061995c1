"""The partitions of promp_amd/csrc/promp_plan.h (minibatched Adam epochs: every minibatch's compact slab laid out as an upload of
its paths alone, the copy launch's table, the refusals) run on the host alone: tests/host/partition_check.cpp includes the header
and nothing else of the project, is built with AddressSanitizer and UBSan, and says what does not hold.  And the rule that deals
a task's paths to the minibatches (optimizers.maml_first_order_optimizer.minibatch_assignment).  No GPU, no emulator."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host', 'partition_check.cpp')


def test_partition_check(tmp_path):
    gxx = shutil.which('g++')
    assert gxx, 'g++ is required'
    exe = str(tmp_path / 'partition_check')
    r = subprocess.run([gxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall', '-Wextra',
                        SRC, '-o', exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, 'partition_check failed:\n' + r.stdout + r.stderr
    assert 'all expectations hold' in r.stdout


@pytest.mark.parametrize('B', [1, 2, 3, 4, 7])
def test_minibatch_assignment(B):
    from promp_amd.optimizers.maml_first_order_optimizer import minibatch_assignment
    counts = [1 * B, B + 1, 2 * B - 1, 20, 100]
    counts = [P for P in counts if P >= B]
    np.random.seed(11)
    a = minibatch_assignment(counts, B)
    assert a.dtype == np.int32 and a.shape == (sum(counts),)
    at = 0
    for P in counts:
        share = a[at:at + P]
        at += P
        # every path in exactly one share of [0, B), every share non-empty, sizes within one of each other
        assert share.min() >= 0 and share.max() < B
        sizes = np.bincount(share, minlength=B)
        assert sizes.sum() == P and sizes.min() >= 1 and sizes.max() - sizes.min() <= 1, (P, sizes)
        assert sorted(sizes) == sorted(np.bincount((np.arange(P) * B) // P, minlength=B))
    # the same seed gives the same draw, another seed another one; an explicit generator is honoured
    np.random.seed(11)
    assert np.array_equal(minibatch_assignment(counts, B), a)
    if B > 1:
        np.random.seed(12)
        assert not np.array_equal(minibatch_assignment(counts, B), a)
        r1, r2 = np.random.RandomState(5), np.random.RandomState(5)
        state = np.random.get_state()[1].copy()
        assert np.array_equal(minibatch_assignment(counts, B, rng=r1), minibatch_assignment(counts, B, rng=r2))
        assert np.array_equal(np.random.get_state()[1], state)
    else:
        assert not a.any()


def test_minibatch_assignment_refuses_too_few_paths():
    from promp_amd.optimizers.maml_first_order_optimizer import minibatch_assignment
    for counts, B in (([4, 2, 4], 3), ([1], 2), ([20, 100, 6], 7)):
        with pytest.raises(ValueError, match='exceeds the %d paths of task %d' % (min(counts), counts.index(min(counts)))):
            minibatch_assignment(counts, B)
    with pytest.raises(ValueError, match='>= 1'):
        minibatch_assignment([4, 4], 0)
    from promp_amd.optimizers.maml_first_order_optimizer import MAMLFirstOrderOptimizer
    with pytest.raises(ValueError, match='>= 1'):
        MAMLFirstOrderOptimizer(num_minibatches=0)
    assert MAMLFirstOrderOptimizer(num_minibatches=4)._num_minibatches == 4
