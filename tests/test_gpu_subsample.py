"""Subsampled constraint products on the GPU (tests/subsample_checks.py): a context with a selection against a context that
holds the selected paths alone, bit for bit, on every kernel family; the oracle, staleness, refusals and the plugin's
subsample_factor."""
import pytest

from tests import devlib, subsample_checks as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.mark.parametrize('hidden,O,A,K', [((32, 32), 5, 3, 1), ((64, 64), 20, 6, 2), ((128, 128), 111, 8, 1), ((100, 100), 20, 6, 1),
                                          ((48, 48, 48), 9, 3, 1)])
def test_selection_equals_truncated_batch(lib, hidden, O, A, K):
    sc.check_equals_truncated_batch(lib, 21, O, A, hidden, K)


def test_selection_equals_truncated_batch_ratio(lib):
    sc.check_equals_truncated_batch(lib, 22, 5, 3, (32, 32), 1, inner='ratio')


def test_selection_equals_truncated_batch_compact_log_std(lib):
    sc.check_equals_truncated_batch(lib, 23, 5, 3, (32, 32), 1, compact_log_std=True)


@pytest.mark.parametrize('hidden,O,A', [((32, 32), 5, 3), ((128, 128), 111, 8)])
def test_full_selection_is_no_selection(lib, hidden, O, A):
    sc.check_full_selection_is_no_selection(lib, 24, O, A, hidden, 1)


@pytest.mark.parametrize('hidden,O,A,K', [((32, 32), 5, 3, 1), ((64, 64), 20, 6, 2)])
def test_selection_against_oracle(lib, hidden, O, A, K):
    sc.check_oracle(lib, 25, O, A, hidden, K)


def test_selection_staleness_and_refusals(lib):
    sc.check_staleness(lib, 26)


def test_malformed_selections_are_refused(lib):
    sc.check_malformed(lib)


def test_plugin_subsample_factor(lib):
    sc.check_plugin(lib, 27)
