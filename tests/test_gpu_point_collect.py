"""promp_collect_point_family on the MI355X (tests/point_collect_checks.py): collections of the goal kind whose episodes end early --
tables against the free-running oracle, the slab by induction per listed path --, the fixed-horizon kinds through the new entry point
bit for bit against promp_rollout_point_family, collected slabs through the stack, the table kernels on a hand-made end_len, and
the refusals.  A handful of sub-millisecond launches per case.  test_point_collect_host.py checks on the CPU that every case meets
the events and margins it is built for."""
import pytest

from tests import devlib, point_collect_checks as pc

ALL = pc.EVENTS
# (M, B, T, hidden), normalization_scale, noise, step, seed, clip_infos, events, data_seed, rollouts_per_meta_task (None: B), origin
GOAL = [
    ((3, 65, 12, (32, 32)), 10, 'host', 0, 0, True, ALL, 2, None, False),                          # a second loop trip
    ((2, 129, 8, (64, 64)), 0, 'device', 1, pc.SEED64, False, ALL, 1, None, False),                # a third; the bare environment
    ((2, 5, 20, (100, 100)), 10, 'device', 0, pc.SEED31, True,
     ('done', 'dropped_tail', 'horizon', 'length_1', 'rows_exceed', 'stop_beyond_T', 'unequal_counts'), 2, None, False),   # zero-padded
    ((2, 3, 12, (32, 16, 24)), 0, 'host', 1, 0, False, ALL, 2, None, False),                       # layer by layer
    ((3, 1, 16, (64, 64)), 10, 'host', 0, 0, False,
     ('done', 'dropped_tail', 'horizon', 'rows_exceed', 'stop_beyond_T', 'unequal_counts'), 10, None, False),              # B = 1
    ((2, 4, 1, (32, 32)), 10, 'device', 1, pc.SEED64, True, ('horizon', 'length_1'), 0, None, False),   # T = 1: every step ends an episode
    ((2, 3, 10, (32, 32)), 10, 'host', 0, 0, True, ALL, 3, 6, True),       # envs_per_task 3 < rollouts_per_meta_task 6; goal (0, 0)
]
# kind, (M, B, T, hidden), reward_type, normalization_scale, step, clip_infos
FIXED = [
    ('corner', (3, 65, 12, (32, 32)), 'sparse', 10, 0, True),
    ('momentum', (2, 5, 8, (64, 64)), 'dense', 0, 1, False),
    ('corner', (2, 3, 6, (32, 16, 24)), 'dense', 0, 1, False),                                     # layer by layer
]
ids = lambda cases: ['-'.join(str(v) for v in c[:4]).replace(' ', '') for c in cases]

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.mark.parametrize('dims,scale,noise,step,seed,clip_infos,wanted,data_seed,rollouts,origin', GOAL, ids=ids(GOAL))
def test_goal_collection(lib, dims, scale, noise, step, seed, clip_infos, wanted, data_seed, rollouts, origin):
    pc.check_goal_collect(lib, *dims, normalization_scale=scale, noise=noise, step=step, seed=seed, clip_infos=clip_infos,
                          wanted=wanted, data_seed=data_seed, rollouts=rollouts, origin=origin)


@pytest.mark.parametrize('kind,dims,reward_type,scale,step,clip_infos', FIXED, ids=ids(FIXED))
def test_fixed_kinds_are_bitwise_the_family_rollout(lib, kind, dims, reward_type, scale, step, clip_infos):
    pc.check_fixed_kind_bitwise(lib, kind, *dims, reward_type=reward_type, normalization_scale=scale, step=step, clip_infos=clip_infos)


def test_table_kernels_on_a_hand_made_end_len(lib):
    pc.check_hand_tables(lib)


def test_collected_slabs_feed_the_stack(lib):
    pc.check_feeds_the_stack(lib, 3, 5, 10, (64, 64), seed=pc.SEED64, data_seed=2)


def test_refusals_by_name(lib):
    pc.check_refusals(lib)
