"""DevicePointEnvSampler with start states drawn on the device, on the kernel emulator at the tiniest shapes
(tests/point_start_sampler_checks.py; tests/test_gpu_point_start_sampler.py runs every class on the MI355X)."""
import pytest

from promp_amd import _lib, session
from tests import devlib, point_start_sampler_checks as pss


@pytest.fixture
def emu(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')
    lib = devlib.emu_library()
    _lib.set_library_for_testing(lib)
    yield lib
    _lib.set_library_for_testing(None)
    session._current = None


@pytest.mark.parametrize('name', ['goal', 'momentum'])
def test_sampler_starts_are_the_restated_draw(emu, name):
    pss.run_sampler_scenario(name, M=2, B=2, R=3, T=4)


def test_normalisation_state_is_the_table_path(emu):
    pss.run_normalised_scenario('origin', M=2, B=2, R=3, T=3)


def test_collected_slabs_feed_the_stack(emu):
    pss.check_feeds_the_stack(emu, 2, 3, 6, (32, 32), data_seed=11)
