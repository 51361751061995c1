"""DevicePointEnvSampler on MetaPointEnv and MetaPointEnvV2 on the MI355X (tests/point_collect_checks.py:run_sampler_scenario)."""
import pytest

from promp_amd import _lib, session
from tests import devlib, point_collect_checks as pc

pytestmark = pytest.mark.gpu


@pytest.fixture
def gpu():
    lib = devlib.gpu_library()
    _lib.set_library_for_testing(lib)
    yield lib
    _lib.set_library_for_testing(None)
    session._current = None


def test_sampler_on_the_goal_class(gpu):
    pc.run_sampler_scenario('goal', wrapped=True)


def test_sampler_on_the_origin_class_bare(gpu):
    pc.run_sampler_scenario('origin', wrapped=False)


def test_sampler_with_device_noise(gpu):
    pc.run_sampler_scenario('goal', wrapped=False, device_noise=True)
