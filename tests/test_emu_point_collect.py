"""promp_collect_point_family on the kernel emulator (tests/point_collect_checks.py): indexing and host sequencing of k_point_collect /
k_gen_point_collect, k_collect_stop, k_collect_tables and the gather with staged rewards, at sizes one OS thread per lane affords.

Left to tests/test_gpu_point_collect.py (-m gpu): B = 129, horizons beyond a few steps, the full event set."""
import pytest

from tests import devlib, point_collect_checks as pc


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


def test_table_kernels_on_a_hand_made_end_len(lib):
    pc.check_hand_tables(lib)


def test_goal_second_trip_host_noise(lib):
    pc.check_goal_collect(lib, 2, 65, 3, (32, 32), 10, 'host', step=0, seed=0, clip_infos=True,
                          wanted=('done', 'horizon', 'length_1', 'rows_exceed', 'dropped_tail', 'unequal_counts'))


def test_goal_device_noise_bare(lib):
    pc.check_goal_collect(lib, 2, 3, 4, (32, 32), 0, 'device', step=1, seed=pc.SEED64, clip_infos=False, wanted=('done', 'horizon'),
                          data_seed=EMU_SEEDS['bare'])


def test_goal_zero_padded_and_layer_by_layer(lib):
    pc.check_goal_collect(lib, 2, 2, 3, (100, 100), 10, 'device', step=0, seed=pc.SEED31, clip_infos=True, wanted=('horizon',),
                          data_seed=EMU_SEEDS['padded'])
    pc.check_goal_collect(lib, 2, 2, 4, (32, 16, 24), 10, 'host', step=1, seed=0, clip_infos=False, wanted=('done', 'horizon'),
                          data_seed=EMU_SEEDS['layered'], rollouts=3)


def test_fixed_kinds_are_bitwise_the_family_rollout(lib):
    pc.check_fixed_kind_bitwise(lib, 'corner', 2, 3, 2, (32, 32), 'dense', 10, step=0, clip_infos=True)
    pc.check_fixed_kind_bitwise(lib, 'momentum', 2, 3, 2, (32, 32), 'dense_squared', 0, step=1, clip_infos=False)


def test_collected_slabs_feed_the_stack(lib):
    pc.check_feeds_the_stack(lib, 2, 3, 6, (32, 32), seed=pc.SEED64, data_seed=11)


def test_refusals_by_name(lib):
    pc.check_refusals(lib)


EMU_SEEDS = dict(bare=3, padded=0, layered=4)          # (chosen on the CPU so that the events asked for occur)
