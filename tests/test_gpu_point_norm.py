"""promp_collect_point_family_norm on the MI355X (tests/point_norm_checks.py): collections under the normalize wrapper's running
observation / reward normalisation -- raw states, tables and moments by induction from what the device stored, the slab against the
replay's normalised values --, two consecutive calls per case from a non-default state, the plain call bit for bit with both flags
off, and the refusals.  A handful of sub-millisecond launches per case.  test_point_norm_host.py checks on the CPU that every case
meets the events, margins and variances it is built for.

Moments on the MI355X: bitwise equal to the NumPy replay in every case and both calls (the deviation printed by check_call is 0)."""
import pytest

from tests import devlib, point_norm_checks as pn

# kind, M, B, max_path_length, hidden, normalization_scale, noise, step, seed, clip_infos, (normalize_obs, normalize_reward), more
CASES = [
    ('goal', 3, 65, 6, (32, 32), 10, 'host', 0, 0, True, (1, 1), dict(data_seed=0)),                       # a second loop trip
    ('goal', 2, 129, 5, (64, 64), 5, 'device', 1, pn.SEED64, False, (1, 0), dict(data_seed=0)),           # a third
    ('momentum', 2, 5, 12, (128, 128), 10, 'host', 0, 0, True, (1, 1), dict(reward_type='dense_squared')),   # O = 4, max_steps = T
    ('walls', 2, 3, 8, (32, 16, 24), 0, 'device', 1, pn.SEED31, False, (1, 0), dict(rollouts=6)),         # layer by layer; two episodes
    # a fixed-horizon kind that stops early: 9 staged steps where total_samples needs 6; O = 4 on the layered kernel
    ('momentum', 2, 3, 6, (32, 16, 24), 10, 'device', 0, pn.SEED64, True, (1, 1), dict(S=9, reward_type='dense_squared')),
    ('corner', 3, 1, 16, (64, 64), 10, 'host', 0, 0, False, (0, 1), dict(rollouts=2, reward_type='dense_squared', data_seed=11)),   # B = 1
]
ids = ['-'.join(str(v) for v in c[:5]).replace(' ', '') for c in CASES]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.mark.parametrize('case', CASES, ids=ids)
def test_normalised_collection(lib, case):
    pn.check_norm_collect(lib, *case[:-1], **case[-1])


@pytest.mark.parametrize('kind,dims,noise,step,seed', [('goal', (3, 65, 6, (32, 32)), 'host', 0, 0),
                                                       ('momentum', (2, 5, 12, (128, 128)), 'device', 1, pn.SEED64),
                                                       ('goal', (2, 3, 8, (32, 16, 24)), 'device', 0, pn.SEED31)])
def test_flags_off_is_the_plain_call(lib, kind, dims, noise, step, seed):
    pn.check_flags_off_is_the_plain_call(lib, kind, *dims, noise=noise, step=step, seed=seed)


def test_refusals_leave_the_state(lib):
    pn.check_refusals(lib)
