"""Environments that live on the device (tests/device_env_checks.py) on the real MI355X, product library: a partial wave (M = 3,
B = 5), the second 64-lane chunk of k_collect_tables and the second block of k_policy_step (M = 2, B = 70), a fused and a
layer-by-layer policy shape, the refusal of pageable host memory, and a torch environment on a stream of its own."""
import subprocess
import sys

import pytest

from promp_amd import _lib, session
from tests import device_env_checks as dc, devlib

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.fixture()
def product_library():
    _lib.set_library_for_testing(None)      # default: promp_amd/libpromp_hip.so
    yield
    session._current = None


@pytest.mark.parametrize('hidden', [(32, 32), (16, 16, 16)], ids=['fused', 'layered'])
@pytest.mark.parametrize('M,B', [(3, 5), (2, 70)])
def test_host_loop_against_device_path(lib, M, B, hidden):
    dc.check_host_against_device(lib, M, B, 6, hidden, step=1 if B == 70 else 0, clip_infos=B != 70)


def test_fixed_horizon(lib):
    dc.check_fixed_horizon(lib)


def test_upload_step_dev(lib):
    dc.check_upload_step_dev(lib)


def test_stop_and_progress(lib):
    dc.check_stop_and_progress(lib, M=3, B=5, T=6)


def test_refusals(lib):
    dc.check_refusals(lib, emulated=False)


def test_sampler(lib, product_library):
    dc.check_sampler(lib, M=3, B=5, T=6, rollouts=7, poll_every=3)


_TORCH_CHILD = """
import sys
try:
    import torch
except ImportError:
    print('SKIP: torch is not installed')
    sys.exit(0)
if not torch.cuda.is_available():
    print('SKIP: torch sees no GPU')
    sys.exit(0)
from tests import device_env_checks as dc
dc.check_torch()
print('TORCH-ENV-OK')
"""


def test_torch_environment_on_its_own_stream():
    """In a child process of its own, where torch is imported BEFORE the library is loaded: a torch wheel brings its own HIP runtime,
    and whichever of the two is loaded first serves both (in this process the library's came first, with the tests above).  The only
    test here that may skip: when torch cannot be imported or sees no GPU."""
    done = subprocess.run([sys.executable, '-c', _TORCH_CHILD], cwd=dc.helpers.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          universal_newlines=True, timeout=600)
    out = done.stdout
    assert done.returncode == 0, out[-4000:]
    skip = [line for line in out.splitlines() if line.startswith('SKIP: ')]
    if skip:
        pytest.skip(skip[0][6:])
    assert 'TORCH-ENV-OK' in out, out[-4000:]
