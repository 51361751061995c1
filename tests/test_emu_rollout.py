"""The rollout kernels on the kernel emulator (tests/rollout_checks.py): indexing and host sequencing of k_policy_step /
k_gen_policy_step, k_point_rollout / k_gen_point_rollout, k_gather_paths and k_policy_forward / k_gen_policy_forward under per-task
parameters, at sizes one OS thread per lane affords.  k_policy_step and k_point_rollout run 64-thread blocks over tiny networks,
so B = 65 (a second block / a second loop trip) is affordable at (32,32); the layer-by-layer kernels run one 256-thread workgroup
per environment and stay at B <= 3, T <= 2.

Left to tests/test_gpu_rollout.py (-m gpu): three blocks (B = 130) and B = 129, horizons beyond 2, and the row loop of
k_policy_forward beyond its second trip (batch 513)."""
import pytest

from tests import devlib, rollout_checks as rc


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')      # dozens of launches per case: fewer host threads per emulated launch


# ---- k_policy_step ---------------------------------------------------------------------------------------------------------------

def test_policy_step_second_block_fixed_layout(lib):
    rc.check_policy_step(lib, 2, 65, 2, 4, 3, (32, 32), 'fixed', step=1, seed=rc.SEED64, clip_infos=True)


def test_policy_step_second_block_staged_layout(lib):
    rc.check_policy_step(lib, 2, 65, 2, 4, 3, (32, 32), 'staged', step=0, seed=rc.SEED31, clip_infos=False)


def test_policy_step_one_action_and_eight(lib):
    rc.check_policy_step(lib, 3, 3, 2, 7, 1, (32, 32), 'staged', step=1, seed=rc.SEED64, clip_infos=False)
    rc.check_policy_step(lib, 2, 3, 2, 20, 8, (64, 64), 'fixed', step=0, seed=rc.SEED64, clip_infos=True)


def test_policy_step_128_wide_and_zero_padded(lib):
    rc.check_policy_step(lib, 2, 2, 2, 111, 8, (128, 128), 'fixed', step=1, seed=rc.SEED64, clip_infos=False)
    rc.check_policy_step(lib, 2, 2, 2, 50, 4, (100, 100), 'staged', step=0, seed=rc.SEED64, clip_infos=True)
    rc.check_policy_step(lib, 2, 2, 2, 40, 3, (48, 20), 'fixed', step=0, seed=rc.SEED31, clip_infos=True)


def test_policy_step_unequal_widths_and_wide_observations(lib):
    rc.check_policy_step(lib, 2, 2, 2, 20, 6, (32, 64), 'staged', step=1, seed=rc.SEED64, clip_infos=True)
    rc.check_policy_step(lib, 2, 2, 2, 100, 6, (64, 64), 'fixed', step=0, seed=rc.SEED31, clip_infos=False)


# ---- k_gen_policy_step -----------------------------------------------------------------------------------------------------------

def test_policy_step_layer_by_layer(lib):
    rc.check_policy_step(lib, 2, 3, 2, 9, 11, (48, 40, 24), 'fixed', step=1, seed=rc.SEED64, clip_infos=False)
    rc.check_policy_step(lib, 2, 2, 2, 5, 3, (32, 32), 'staged', step=0, seed=rc.SEED64, clip_infos=True, output_act='tanh')
    rc.check_policy_step(lib, 2, 2, 2, 6, 1, (16,), 'fixed', step=0, seed=rc.SEED31, clip_infos=True)


def test_policy_step_layer_by_layer_humanoid_inputs_and_relu(lib):
    rc.check_policy_step(lib, 2, 2, 2, 376, 17, (64, 64), 'staged', step=1, seed=rc.SEED64, clip_infos=True)
    rc.check_policy_step(lib, 2, 2, 2, 30, 6, (256, 256), 'staged', step=0, seed=rc.SEED31, clip_infos=False, hidden_act='relu')


def test_policy_step_layer_by_layer_act_dim_at_its_maximum(lib):
    rc.check_policy_step(lib, 2, 2, 2, 12, 64, (64, 64), 'fixed', step=1, seed=rc.SEED31, clip_infos=False)


# ---- k_point_rollout / k_gen_point_rollout ------------------------------------------------------------------------------------------

def test_point_rollout_second_trip_host_noise(lib):
    rc.check_point_rollout(lib, 2, 65, 2, (32, 32), 'sparse', 10, 'host', step=0, seed=0, clip_infos=True)


def test_point_rollout_second_trip_device_noise(lib):
    rc.check_point_rollout(lib, 2, 65, 2, (32, 32), 'dense', 0, 'device', step=1, seed=rc.SEED64, clip_infos=False)


def test_point_rollout_128_wide_and_zero_padded(lib):
    rc.check_point_rollout(lib, 2, 2, 2, (128, 128), 'dense_squared', 10, 'device', step=0, seed=rc.SEED31, clip_infos=True, data_seed=1)
    rc.check_point_rollout(lib, 2, 2, 2, (100, 100), 'dense', 0, 'host', step=1, seed=0, clip_infos=False)


def test_point_rollout_layer_by_layer(lib):
    rc.check_point_rollout(lib, 2, 3, 2, (32, 16, 24), 'dense', 10, 'device', step=1, seed=rc.SEED64, clip_infos=True, data_seed=1)
    rc.check_point_rollout(lib, 2, 2, 2, (24, 24), 'dense_squared', 0, 'host', step=0, seed=0, clip_infos=False, hidden_act='identity')


# ---- k_gather_paths, k_policy_forward, the passes behind a rollout -------------------------------------------------------------------

def test_gather_hand_written_path_table(lib):
    rc.check_gather(lib)


def test_policy_forward_second_trip(lib):
    rc.check_policy_forward(lib, 2, 257, 5, 3, (32, 32))
    rc.check_policy_forward(lib, 2, 257, 5, 3, (16, 24, 16))


def test_rollout_feeds_the_passes(lib):
    rc.check_rollout_feeds_the_passes(lib, 2, 3, 2, 4, 3, (32, 32), step=1, seed=rc.SEED64, clip_infos=True)
    rc.check_rollout_feeds_the_passes(lib, 2, 2, 2, 9, 11, (16, 24, 16), step=0, seed=rc.SEED31, clip_infos=False)
