"""Minibatched Adam epochs on the GPU (tests/minibatch_checks.py): a context told the assignment against the by-hand sequence of
contexts that hold one minibatch's paths alone, bit for bit, on every kernel family; B = 1 against optimize(); the statistics;
the float64 trajectory; what the call leaves behind; refusals; ProMP's num_minibatches."""
import pytest

from tests import devlib, minibatch_checks as mc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.mark.parametrize('hidden,O,A,K', [((32, 32), 5, 3, 1), ((64, 64), 20, 6, 2), ((128, 128), 111, 8, 1), ((100, 100), 20, 6, 1),
                                          ((48, 48, 48), 9, 3, 1)])
def test_minibatches_equal_truncated_batches(lib, hidden, O, A, K):
    mc.check_equals_truncated_batch(lib, 41, O, A, hidden, K)


def test_minibatches_equal_truncated_batches_ratio(lib):
    mc.check_equals_truncated_batch(lib, 42, 5, 3, (32, 32), 1, inner='ratio')


def test_minibatches_equal_truncated_batches_compact_log_std(lib):
    mc.check_equals_truncated_batch(lib, 43, 5, 3, (32, 32), 1, compact_log_std=True)


def test_minibatches_equal_truncated_batches_trainable_step_sizes(lib):
    mc.check_equals_truncated_batch(lib, 44, 5, 3, (32, 32), 1, train_sizes=True)


@pytest.mark.parametrize('hidden,O,A', [((32, 32), 5, 3), ((128, 128), 111, 8)])
def test_one_minibatch_is_optimize(lib, hidden, O, A):
    mc.check_one_minibatch_is_optimize(lib, 45, O, A, hidden)
    mc.check_python_path_one_minibatch(lib, 45, O, A, hidden)


def test_statistics_are_whole_batch(lib):
    mc.check_statistics(lib, 46)


@pytest.mark.parametrize('hidden,O,A,K', [((32, 32), 5, 3, 1), ((64, 64), 20, 6, 2)])
def test_trajectory_against_float64(lib, hidden, O, A, K):
    mc.check_against_float64(lib, 47, O, A, hidden, K)


def test_state_left_behind(lib):
    mc.check_state_left_behind(lib, 48)


def test_refusals_move_nothing(lib):
    mc.check_refusals(lib)


def test_plugin_num_minibatches(lib):
    mc.check_plugin(lib, 49)
