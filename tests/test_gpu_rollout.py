"""The rollout kernels on the MI355X (tests/rollout_checks.py): per-task parameters, more than one block and loop trip, every
two-layer family and the zero-padded widths, the layer-by-layer kernels, both slab layouts, 64-bit seeds and stream 1, clip_infos
on and off, hand-written path tables -- against the float64 oracle, a handful of sub-millisecond launches per case."""
import pytest

from tests import devlib, rollout_checks as rc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


# (M, B, T, O, A, hidden), layout, step, seed, clip_infos
FAST_STEP = [
    ((3, 65, 3, 4, 3, (32, 32)), 'fixed', 0, rc.SEED64, True),        # a second block holding one thread
    ((3, 65, 3, 4, 3, (32, 32)), 'staged', 1, rc.SEED31, False),
    ((2, 64, 2, 20, 6, (64, 64)), 'staged', 0, rc.SEED64, True),      # exactly one full block
    ((2, 130, 2, 20, 8, (64, 64)), 'fixed', 1, rc.SEED64, False),     # three blocks, A = 8
    ((3, 5, 4, 7, 1, (32, 32)), 'staged', 1, rc.SEED64, True),        # A = 1: the second normal of the pair is dropped
    ((2, 5, 3, 111, 8, (128, 128)), 'fixed', 1, rc.SEED31, True),
    ((2, 5, 3, 111, 8, (128, 128)), 'staged', 0, rc.SEED64, False),
    ((2, 5, 3, 50, 4, (100, 100)), 'fixed', 0, rc.SEED64, False),     # zero-padded to (128, 128)
    ((2, 5, 3, 40, 3, (48, 20)), 'staged', 1, rc.SEED31, True),       # zero-padded to (64, 64)
    ((2, 5, 3, 20, 6, (32, 64)), 'fixed', 1, rc.SEED64, True),
    ((2, 5, 3, 100, 6, (64, 64)), 'staged', 0, rc.SEED31, False),
]
# (M, B, T, O, A, hidden), hidden_act, output_act, layout, step, seed, clip_infos
LAYERED_STEP = [
    ((2, 3, 3, 376, 17, (64, 64)), 'tanh', None, 'staged', 0, rc.SEED64, True),
    ((2, 3, 3, 30, 6, (256, 256)), 'relu', None, 'fixed', 1, rc.SEED31, False),
    ((2, 2, 3, 9, 11, (48, 40, 24)), 'tanh', None, 'fixed', 0, rc.SEED64, False),
    ((2, 2, 3, 5, 3, (32, 32)), 'tanh', 'tanh', 'staged', 1, rc.SEED64, True),
    ((2, 2, 2, 12, 64, (64, 64)), 'tanh', None, 'staged', 1, rc.SEED31, False),      # act_dim at its maximum
    ((2, 2, 2, 6, 1, (16,)), 'tanh', None, 'fixed', 0, rc.SEED64, True),
]
# (M, B, T, hidden), reward_type, normalization_scale, noise, step, seed, clip_infos, hidden_act, data_seed
POINT = [
    ((3, 65, 12, (32, 32)), 'sparse', 10, 'host', 0, 0, True, 'tanh', 0),
    ((2, 129, 8, (64, 64)), 'dense', 0, 'device', 1, rc.SEED64, False, 'tanh', 0),
    ((2, 5, 40, (128, 128)), 'dense_squared', 10, 'device', 0, rc.SEED31, True, 'tanh', 0),
    ((2, 5, 20, (100, 100)), 'sparse', 0, 'host', 1, 0, False, 'tanh', 0),
    ((2, 4, 1, (32, 32)), 'dense', 10, 'device', 1, rc.SEED64, True, 'tanh', 0),               # T = 1
    ((3, 1, 16, (64, 64)), 'dense', 10, 'host', 0, 0, False, 'tanh', 0),                       # B = 1
    ((2, 3, 12, (32, 16, 24)), 'sparse', 10, 'device', 1, rc.SEED64, True, 'tanh', 0),         # layer by layer
    ((2, 3, 10, (24, 24)), 'dense_squared', 0, 'host', 0, 0, False, 'identity', 0),            # linear hidden units
]
ids = lambda cases: ['-'.join(str(v) for v in c).replace(' ', '') for c in cases]


def test_cases_cover_both_layouts_steps_seeds_and_clip_modes():
    steps = FAST_STEP + [(c[0],) + c[3:] for c in LAYERED_STEP]
    for layout in ('fixed', 'staged'):
        assert any(c[0][1] == 65 and c[1] == layout for c in steps) and any(c[0][5] == (128, 128) and c[1] == layout for c in steps)
    assert {c[2] for c in steps} == {0, 1} and {c[4] for c in steps} == {True, False}
    assert rc.SEED64 >> 32 and rc.SEED64 & 0xFFFFFFFF and rc.SEED31 < 2 ** 31 and {c[3] for c in steps} == {rc.SEED64, rc.SEED31}
    assert {c[1] for c in POINT} == {'dense', 'dense_squared', 'sparse'} and {c[2] for c in POINT} == {0, 10}
    assert {c[3] for c in POINT} == {'host', 'device'} and {c[4] for c in POINT} == {0, 1}


@pytest.mark.parametrize('dims,layout,step,seed,clip_infos', FAST_STEP, ids=ids(FAST_STEP))
def test_policy_step_fast_path(lib, dims, layout, step, seed, clip_infos):
    rc.check_policy_step(lib, *dims, layout=layout, step=step, seed=seed, clip_infos=clip_infos)


@pytest.mark.parametrize('dims,hidden_act,output_act,layout,step,seed,clip_infos', LAYERED_STEP, ids=ids(LAYERED_STEP))
def test_policy_step_layer_by_layer(lib, dims, hidden_act, output_act, layout, step, seed, clip_infos):
    rc.check_policy_step(lib, *dims, layout=layout, step=step, seed=seed, clip_infos=clip_infos, hidden_act=hidden_act,
                         output_act=output_act)


@pytest.mark.parametrize('dims,reward_type,scale,noise,step,seed,clip_infos,hidden_act,data_seed', POINT, ids=ids(POINT))
def test_point_rollout(lib, dims, reward_type, scale, noise, step, seed, clip_infos, hidden_act, data_seed):
    rc.check_point_rollout(lib, *dims, reward_type=reward_type, normalization_scale=scale, noise=noise, step=step, seed=seed,
                           clip_infos=clip_infos, hidden_act=hidden_act, data_seed=data_seed)


def test_gather_hand_written_path_table(lib):
    rc.check_gather(lib)
    rc.check_gather(lib, step=1, seed=rc.SEED31, clip_infos=True, hidden=(64, 64, 64))      # staging rows of k_gen_policy_step


@pytest.mark.parametrize('batch', [1, 256, 257, 513])
@pytest.mark.parametrize('hidden', [(64, 64), (64, 64, 64)])
def test_policy_forward_row_loop(lib, hidden, batch):
    rc.check_policy_forward(lib, 3, batch, 20, 6, hidden)


@pytest.mark.parametrize('O,A,hidden', [(111, 8, (128, 128)), (50, 4, (100, 100))])
def test_policy_forward_wide(lib, O, A, hidden):
    rc.check_policy_forward(lib, 2, 257, O, A, hidden)


def test_rollout_feeds_the_passes(lib):
    rc.check_rollout_feeds_the_passes(lib, 2, 5, 6, 20, 6, (64, 64), step=1, seed=rc.SEED64, clip_infos=True)
    rc.check_rollout_feeds_the_passes(lib, 2, 3, 6, 9, 11, (48, 40, 24), step=0, seed=rc.SEED31, clip_infos=False)
