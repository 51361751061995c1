"""DiCE sample processing (promp_process_samples_dice) on the kernel emulator: the small cases of dice_processing_checks.py.
All of them, and one case per Gram / fit family, run on the GPU in tests/test_gpu_dice_processing.py (-m gpu)."""
import pytest

from promp_amd import _lib, session
from tests import devlib, dice_processing_checks as dp


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture()
def emu(lib):
    _lib.set_library_for_testing(lib)
    yield lib
    _lib.set_library_for_testing(None)
    session._current = None


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


@pytest.mark.parametrize('name', dp.GOLDEN_CASES)
def test_reference_outputs(lib, name):
    dp.check_golden(lib, name)


def test_minimum_is_a_padded_zero(lib):
    dp.check_edges(lib, 160, 'zero', 'positive', normalize_adv=True, positive_adv=True, expect_min_padding=True)
    dp.check_edges(lib, 160, 'zero', 'positive', normalize_adv=False, positive_adv=True, expect_min_padding=True)


def test_minimum_is_a_valid_entry(lib):
    dp.check_edges(lib, 160, 'linear_feature', 'normal', normalize_adv=True, positive_adv=True, expect_min_padding=False)


def test_longest_path_unpadded(lib):
    dp.check_edges(lib, 130, 'linear_feature', 'normal', normalize_adv=True, positive_adv=False)


def test_task_without_padding(lib):
    dp.check_unpadded_task(lib)


def test_installed_weights(lib):
    dp.check_installed_weights(lib)


def test_plain_call_unchanged(lib):
    dp.check_plain_call_unchanged(lib)


@pytest.mark.parametrize('vpg', [False, True], ids=['dice_maml', 'vpg_dice_maml'])
def test_plugin_residency(emu, vpg):
    M, O, A, hidden = 2, 4, 2, (32, 32)
    dp.check_plugin_residency(dp.hand_built_batches(M, O, A, hidden, [[6, 9, 4], [9, 3, 8]]), M, O, A, hidden, 10, vpg)


def test_refusals(lib):
    dp.check_refusals(lib)
