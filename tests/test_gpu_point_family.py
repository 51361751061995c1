"""promp_rollout_point_family on the MI355X (tests/point_family_checks.py): the walls environment by induction on the slab, the
momentum environment against a free-running float64 oracle, the corner environment bit for bit against promp_rollout_point_env, and
a momentum slab through the passes -- a few sub-millisecond launches per case."""
import pytest

from tests import devlib, point_family_checks as fc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


# (M, B, T, hidden), reward_type, normalization_scale, noise, step, seed, clip_infos, start radii, data_seed
WALLS = [
    ((3, 65, 12, (32, 32)), 'dense', 10, 'host', 0, 0, True, (0.93, 1.93), 0),                     # a second loop trip
    ((2, 129, 8, (64, 64)), 'sparse', 0, 'device', 1, fc.SEED64, False, (0.93, 1.93), 0),          # a third
    ((2, 5, 20, (100, 100)), 'dense_squared', 10, 'device', 0, fc.SEED31, True, (0.93,), 0),       # zero-padded to (128, 128)
    ((2, 3, 12, (32, 16, 24)), 'dense', 0, 'host', 1, 0, False, (1.93,), 0),                       # layer by layer
    ((2, 4, 1, (32, 32)), 'dense', 10, 'device', 1, fc.SEED64, True, (0.93,), 1),                  # T = 1
]
# (M, B, T, hidden), reward_type, normalization_scale, noise, step, seed, clip_infos, data_seed
MOMENTUM = [
    ((3, 65, 12, (32, 32)), 'sparse', 10, 'host', 0, 0, True, 0),
    ((2, 129, 8, (64, 64)), 'dense', 0, 'device', 1, fc.SEED64, False, 0),
    ((2, 5, 20, (128, 128)), 'dense_squared', 10, 'device', 0, fc.SEED31, True, 1),
    ((2, 3, 12, (32, 16, 24)), 'sparse', 0, 'device', 1, fc.SEED64, True, 0),                      # layer by layer
    ((3, 1, 16, (64, 64)), 'dense', 10, 'host', 0, 0, False, 0),                                   # B = 1
]
ids = lambda cases: ['-'.join(str(v) for v in c).replace(' ', '') for c in cases]


def test_cases_cover_rewards_scales_noise_steps_seeds_and_clip_modes():
    for cases in (WALLS, MOMENTUM):
        assert {c[1] for c in cases} == {'dense', 'dense_squared', 'sparse'} and {c[2] for c in cases} == {0, 10}
        assert {c[3] for c in cases} == {'host', 'device'} and {c[4] for c in cases} == {0, 1} and {c[6] for c in cases} == {True, False}
        assert {c[5] for c in cases if c[3] == 'device'} == {fc.SEED64, fc.SEED31}
        assert any(len(c[0][3]) == 3 for c in cases) and any(c[0][1] > 128 for c in cases)
    assert {r for c in WALLS for r in c[7]} == {0.93, 1.93}


@pytest.mark.parametrize('dims,reward_type,scale,noise,step,seed,clip_infos,radii,data_seed', WALLS, ids=ids(WALLS))
def test_walls_rollout(lib, dims, reward_type, scale, noise, step, seed, clip_infos, radii, data_seed):
    fc.check_walls_rollout(lib, *dims, reward_type=reward_type, normalization_scale=scale, noise=noise, step=step, seed=seed,
                           radii=radii, clip_infos=clip_infos, data_seed=data_seed)


@pytest.mark.parametrize('dims,reward_type,scale,noise,step,seed,clip_infos,data_seed', MOMENTUM, ids=ids(MOMENTUM))
def test_momentum_rollout(lib, dims, reward_type, scale, noise, step, seed, clip_infos, data_seed):
    """Measured on one MI355X (replay deviation -> bound; device):
        (3,65,12,(32,32)) sparse 10 host          obs 2.38e-7 -> 2.00e-6; 2.38e-7   act 2.55e-6 -> 1.02e-5; 2.55e-6   rew 1.40e-7 -> 2.00e-6; 1.40e-7
        (2,129,8,(64,64)) dense 0 device          obs 9.54e-7 -> 3.81e-6; 1.19e-6   act 2.81e-6 -> 1.12e-5; 5.02e-6   rew 1.28e-6 -> 5.13e-6; 1.76e-6
        (2,5,20,(128,128)) dense_squared 10 dev.  obs 4.77e-7 -> 2.00e-6; 4.77e-7   act 1.51e-6 -> 6.03e-6; 4.15e-6   rew 4.98e-6 -> 1.99e-5; 4.98e-6
        (2,3,12,(32,16,24)) sparse 0 device       obs 1.19e-6 -> 4.77e-6; 4.77e-7   act 1.52e-6 -> 6.06e-6; 2.59e-6   rew 8.19e-7 -> 5.00e-6; 3.54e-7
        (3,1,16,(64,64)) dense 10 host            obs 1.19e-7 -> 2.00e-6; 5.96e-8   act 1.24e-6 -> 4.96e-6; 1.24e-6   rew 3.77e-7 -> 2.00e-6; 3.77e-7
    (means: device 2.8e-7 .. 4.9e-7 under bounds of 2.0e-6 .. 2.2e-6.)

    With fast_tanh in the mean network the second case missed its bound: observations 4.02e-6 against 3.81e-6, rewards 5.23e-6
    against 5.13e-6.  It is the bare environment (scale 0) with exploration of std 0.55 .. 1: an action inside the +-0.1 box
    enters the velocity at gain 1 and the position with weights T, T - 1, ..., so the few 1e-7 of fast_tanh's absolute error in
    the mean (3.5e-7 at the worst environment, the environment arithmetic itself exact on the downloaded slab) came out as 4e-6
    after 8 steps.  The kernels of walls and momentum evaluate tanhf instead (promp_kernels_rollout.h); the figures above are
    with it."""
    fc.check_momentum_rollout(lib, *dims, reward_type=reward_type, normalization_scale=scale, noise=noise, step=step, seed=seed,
                              clip_infos=clip_infos, data_seed=data_seed)


def test_corner_through_the_family_entry_point_is_bitwise_the_old_one(lib):
    fc.check_corner_bitwise(lib, 3, 65, 12, (32, 32), 'sparse', 10, 'host', step=0, seed=0, clip_infos=True)
    fc.check_corner_bitwise(lib, 3, 65, 12, (32, 32), 'dense', 0, 'device', step=1, seed=fc.SEED64, clip_infos=False)


def test_momentum_slab_feeds_the_passes(lib):
    fc.check_momentum_feeds_the_passes(lib, 2, 5, 6, (64, 64), step=1, seed=fc.SEED64, clip_infos=True)


def test_argument_errors_are_refused_by_name(lib):
    fc.check_refusals(lib)
