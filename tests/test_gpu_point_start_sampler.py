"""DevicePointEnvSampler with start states drawn on the device, on the MI355X (tests/point_start_sampler_checks.py): all five
point-mass classes, the running normalisation against the table path, and the resident slabs through the stack."""
import pytest

from promp_amd import _lib, session
from tests import devlib, point_start_sampler_checks as pss

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu():
    lib = devlib.gpu_library()
    _lib.set_library_for_testing(lib)
    yield lib
    _lib.set_library_for_testing(None)
    session._current = None


@pytest.mark.parametrize('name', pss.CLASSES)
def test_sampler_starts_are_the_restated_draw(gpu, name):
    pss.run_sampler_scenario(name)


@pytest.mark.parametrize('name', ['origin', 'momentum'])
def test_normalisation_state_is_the_table_path(gpu, name):
    pss.run_normalised_scenario(name)


def test_collected_slabs_feed_the_stack(gpu):
    pss.check_feeds_the_stack(gpu, 3, 5, 8, (64, 64))
