"""DevicePointEnvSampler under running observation / reward normalisation on the kernel emulator, at the tiniest cases
(tests/point_norm_checks.py:run_sampler_scenario; tests/test_gpu_point_norm_sampler.py runs the rest on the MI355X)."""
import pytest

from promp_amd import _lib, session
from tests import devlib, point_norm_checks as pn


@pytest.fixture
def emu(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')
    lib = devlib.emu_library()
    _lib.set_library_for_testing(lib)
    yield lib
    _lib.set_library_for_testing(None)
    session._current = None


def test_sampler_on_the_goal_class(emu):
    pn.run_sampler_scenario('goal', M=2, B=2, R=3, T=4)


def test_sampler_on_the_momentum_class(emu):
    pn.run_sampler_scenario('momentum', M=2, B=None, R=2, T=3)
