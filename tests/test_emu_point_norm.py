"""promp_collect_point_family_norm on the kernel emulator (tests/point_norm_checks.py): indexing and host sequencing of
k_point_norm_collect / k_gen_point_norm_collect, the staged moments and k_point_norm_commit, at sizes one OS thread per lane affords.

Left to tests/test_gpu_point_norm.py (-m gpu): B = 129, horizons beyond a few steps, walls and corner."""
import pytest

from tests import devlib, point_norm_checks as pn

# kind, M, B, max_path_length, hidden, normalization_scale, noise, step, seed, clip_infos, (normalize_obs, normalize_reward), more
CASES = [
    ('goal', 2, 65, 2, (32, 32), 10, 'host', 0, 0, True, (1, 1), dict(S=3, rollouts=40)),                 # a second loop trip; max_steps 3
    ('goal', 2, 2, 3, (100, 100), 10, 'device', 1, pn.SEED31, True, (1, 0), dict(data_seed=34)),          # zero-padded
    ('goal', 2, 2, 4, (32, 16, 24), 5, 'host', 0, 0, False, (0, 1), dict(rollouts=3)),                    # layer by layer
    ('momentum', 2, 3, 2, (32, 32), 10, 'host', 1, 0, True, (1, 1), dict(reward_type='dense_squared')),   # O = 4
]


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c[:5]).replace(' ', ''))
def test_two_consecutive_normalised_collections(lib, case):
    pn.check_norm_collect(lib, *case[:-1], **case[-1])


def test_flags_off_is_the_plain_call(lib):
    pn.check_flags_off_is_the_plain_call(lib, 'goal', 2, 3, 4, (32, 32), noise='host', step=0, seed=0)


def test_refusals_leave_the_state(lib):
    pn.check_refusals(lib)
