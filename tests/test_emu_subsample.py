"""Subsampled constraint products on the kernel emulator (tests/subsample_checks.py): the selection's gather, its tables and the
sequencing of the evaluations on it, at sizes one OS thread per lane affords -- (32,32), O = 5, A = 3, two tasks with 3 and 2
paths of at most 20 rows, K = 1.  Left to tests/test_gpu_subsample.py (-m gpu): the other kernel families, K = 2, the ragged
three-task batch."""
import pytest

from tests import devlib, subsample_checks as sc


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


EMU = dict(lengths=sc.EMU_LENGTHS, selections=sc.EMU_SELECTIONS)


def test_selection_equals_truncated_batch(lib):
    sc.check_equals_truncated_batch(lib, 11, 5, 3, (32, 32), 1, solves=((2, 2), (0, 1)), **EMU)


def test_full_selection_is_no_selection(lib):
    sc.check_full_selection_is_no_selection(lib, 12, 5, 3, (32, 32), 1, lengths=sc.EMU_LENGTHS, solves=((2, 1),))


def test_selection_against_oracle(lib):
    sc.check_oracle(lib, 13, 5, 3, (32, 32), 1, **EMU)


def test_selection_staleness_and_refusals(lib):
    sc.check_staleness(lib, 14, resize_solves=((2, 1),), **EMU)


def test_malformed_selections_are_refused(lib):
    sc.check_malformed(lib)


def test_plugin_subsample_factor(lib):
    sc.check_plugin(lib, 15, T=6, modes=('exact',))
