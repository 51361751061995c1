"""The sampler-level scenarios of tests/point_family_sampler_checks.py on the real MI355X (product library, no emulator)."""
import pytest

from promp_amd import _lib, session
from tests import point_family_checks as fc, point_family_sampler_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def product_library():
    _lib.set_library_for_testing(None)      # default: promp_amd/libpromp_hip.so
    yield
    session._current = None


@pytest.mark.parametrize('kind', fc.KINDS)
def test_device_sampler_paths_are_the_numpy_environment(kind):
    sc.run_sampler_scenario(kind, M=4, B=20, T=30)


@pytest.mark.parametrize('kind', fc.KINDS)
def test_trainer_with_device_rollouts(kind):
    sc.run_trainer_scenario(kind)
