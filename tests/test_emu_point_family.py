"""promp_rollout_point_family on the kernel emulator (tests/point_family_checks.py): indexing and host sequencing of
k_point_family_rollout / k_gen_point_family_rollout for the walls and the momentum environment, at sizes one OS thread per lane
affords: B = 65 (a second loop trip) at (32,32), the zero-padded widths and the layer-by-layer kernel at B = T = 2.

Left to tests/test_gpu_point_family.py (-m gpu): B = 129, horizons beyond 2, three reward types per environment."""
import pytest

from tests import devlib, point_family_checks as fc


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


def test_walls_second_trip_host_noise(lib):
    fc.check_walls_rollout(lib, 2, 65, 2, (32, 32), 'dense', 10, 'host', step=0, seed=0, radii=(0.93, 1.93), clip_infos=True)


def test_walls_second_trip_device_noise(lib):
    fc.check_walls_rollout(lib, 2, 65, 2, (32, 32), 'sparse', 0, 'device', step=1, seed=fc.SEED64, radii=(0.93, 1.93), clip_infos=False)


def test_walls_zero_padded_and_layer_by_layer(lib):
    fc.check_walls_rollout(lib, 2, 2, 2, (100, 100), 'dense_squared', 0, 'host', step=0, seed=0, radii=(0.93,), clip_infos=False)
    fc.check_walls_rollout(lib, 2, 2, 2, (32, 16, 24), 'dense', 0, 'device', step=1, seed=fc.SEED31, radii=(1.93,), clip_infos=True)


def test_momentum_second_trip_host_noise(lib):
    fc.check_momentum_rollout(lib, 2, 65, 2, (32, 32), 'dense_squared', 10, 'host', step=0, seed=0, clip_infos=True)


def test_momentum_second_trip_device_noise(lib):
    fc.check_momentum_rollout(lib, 2, 65, 2, (32, 32), 'dense', 0, 'device', step=1, seed=fc.SEED64, clip_infos=False)


def test_momentum_zero_padded_and_layer_by_layer(lib):
    fc.check_momentum_rollout(lib, 2, 2, 2, (100, 100), 'dense_squared', 10, 'host', step=0, seed=0, clip_infos=False, data_seed=2)
    fc.check_momentum_rollout(lib, 2, 2, 2, (32, 16, 24), 'dense', 0, 'device', step=1, seed=fc.SEED31, clip_infos=True)


def test_corner_through_the_family_entry_point_is_bitwise_the_old_one(lib):
    fc.check_corner_bitwise(lib, 2, 3, 2, (32, 32), 'dense', 10, 'host', step=0, seed=0, clip_infos=True)
    fc.check_corner_bitwise(lib, 2, 3, 2, (32, 32), 'dense_squared', 0, 'device', step=1, seed=fc.SEED64, clip_infos=False)


def test_momentum_slab_feeds_the_passes(lib):
    fc.check_momentum_feeds_the_passes(lib, 2, 3, 2, (32, 32), step=1, seed=fc.SEED64, clip_infos=True)


def test_argument_errors_are_refused_by_name(lib):
    fc.check_refusals(lib)
