"""Minibatched Adam epochs on the kernel emulator (tests/minibatch_checks.py): the copy launch, the tables of the minibatches' slabs,
the observation ranges it leaves and the sequencing of the Adam steps, at sizes one OS thread per lane affords -- (32,32), O = 5,
A = 3, two tasks with 3 and 2 paths of at most 20 rows, K = 1, two compute units.  Left to tests/test_gpu_minibatch.py (-m gpu):
the other kernel families, K = 2, B = 3, two epochs, the ragged three-task batch, the float64 trajectory."""
import pytest

from tests import devlib, minibatch_checks as mc

EMU = dict(lengths=mc.EMU_LENGTHS)


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


def test_minibatches_equal_truncated_batches(lib):
    mc.check_equals_truncated_batch(lib, 31, 5, 3, (32, 32), 1, runs=((2, [mc.EMU_ASSIGN_2]),), **EMU)


def test_statistics_are_whole_batch(lib):
    mc.check_statistics(lib, 32, pattern=mc.EMU_ASSIGN_2, **EMU)


def test_refusals_move_nothing(lib):
    mc.check_refusals(lib, pattern=mc.EMU_ASSIGN_2, **EMU)


def test_plugin_num_minibatches(lib):
    mc.check_plugin(lib, 33, T=6)
