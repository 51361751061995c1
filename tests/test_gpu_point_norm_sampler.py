"""DevicePointEnvSampler under normalize(env, normalize_obs=True, normalize_reward=True, obs_alpha=0.1, reward_alpha=0.2) on the
MI355X (tests/point_norm_checks.py:run_sampler_scenario): MetaPointEnvV2, whose episodes end early, and MetaPointEnvMomentum, a
fixed-horizon class routed through the collection call.  Obtain_samples twice with a process_samples between, the moments against
the replay, the paths as MetaSampler hands them out, the state across a re-created context and through get / set."""
import pytest

from promp_amd import session
from tests import point_norm_checks as pn

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def fresh_session():
    yield
    session._current = None


def test_sampler_on_the_goal_class():
    pn.run_sampler_scenario('goal', M=3, B=3, R=4, T=10, hidden=(32, 32))


def test_sampler_on_the_momentum_class():
    pn.run_sampler_scenario('momentum', M=2, B=None, R=5, T=8, hidden=(64, 64))
