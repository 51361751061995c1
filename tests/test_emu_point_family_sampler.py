"""DevicePointEnvSampler and three Trainer iterations on the walls and the momentum environment, on the kernel emulator at tiny
shapes (tests/point_family_sampler_checks.py).  The same scenarios run on the GPU in test_gpu_point_family_sampler.py."""
import pytest

from promp_amd import _lib, session
from tests import devlib, point_family_checks as fc, point_family_sampler_checks as sc


@pytest.fixture(autouse=True)
def _two_emulated_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


@pytest.fixture()
def emu():
    lib = devlib.emu_library()
    _lib.set_library_for_testing(lib)
    yield lib
    _lib.set_library_for_testing(None)
    session._current = None


@pytest.mark.parametrize('kind', fc.KINDS)
def test_device_sampler_paths_are_the_numpy_environment(emu, kind):
    sc.run_sampler_scenario(kind)


@pytest.mark.parametrize('kind', fc.KINDS)
def test_trainer_with_device_rollouts(emu, kind):
    sc.run_trainer_scenario(kind)


def test_sampler_refuses_other_environments_and_dimensions(emu):
    from promp_amd.envs.point_env import MetaPointEnvMomentum
    from promp_amd.policies.meta_gaussian_mlp_policy import MetaGaussianMLPPolicy
    from promp_amd.samplers.device_point_sampler import DevicePointEnvSampler
    policy = MetaGaussianMLPPolicy(name='p', obs_dim=2, action_dim=2, meta_batch_size=2, hidden_sizes=(32, 32))
    with pytest.raises(AssertionError, match='obs_dim 4'):
        DevicePointEnvSampler(env=MetaPointEnvMomentum(), policy=policy, rollouts_per_meta_task=2, meta_batch_size=2, max_path_length=3)

    class Other(object):
        sample_tasks = set_task = None
    with pytest.raises(AssertionError, match='MetaPointEnvWalls'):
        DevicePointEnvSampler(env=Other(), policy=policy, rollouts_per_meta_task=2, meta_batch_size=2, max_path_length=3)
