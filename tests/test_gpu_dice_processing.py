"""DiCE sample processing (promp_process_samples_dice) on the MI355X: every case of dice_processing_checks.py, one case per
Gram / fit family of sample_plan(), and the run script."""
import csv
import os
import subprocess
import sys

import pytest

from promp_amd import session
from tests import devlib, dice_processing_checks as dp

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.fixture()
def fresh_session():
    yield
    session._current = None


@pytest.mark.parametrize('name', dp.GOLDEN_CASES)
def test_reference_outputs(lib, name):
    dp.check_golden(lib, name)


@pytest.mark.parametrize('T', [130, 160])
@pytest.mark.parametrize('normalize_adv', [False, True])
@pytest.mark.parametrize('positive_adv', [False, True])
def test_scan_and_padding_edges(lib, T, normalize_adv, positive_adv):
    dp.check_edges(lib, T, 'linear_feature', 'normal', normalize_adv, positive_adv,
                   expect_min_padding=False if T == 160 else None)
    dp.check_edges(lib, T, 'zero', 'positive', normalize_adv, positive_adv,
                   expect_min_padding=True if T == 160 else None)


def test_task_without_padding(lib):
    dp.check_unpadded_task(lib)


def test_installed_weights(lib):
    dp.check_installed_weights(lib)


def test_plain_call_unchanged(lib):
    dp.check_plain_call_unchanged(lib)


@pytest.mark.parametrize('vpg', [False, True], ids=['dice_maml', 'vpg_dice_maml'])
def test_plugin_residency(fresh_session, vpg):
    dp.check_plugin_residency(dp.point_env_batches(2, 3, 20), 2, 2, 2, (32, 32), 20, vpg)


def test_refusals(lib):
    dp.check_refusals(lib)


@pytest.mark.parametrize('obs_dim', [20, 40, 111], ids=['k_gram_k_fit_wave', 'k_gram_wide_k_fit_wide', 'k_gram_tiled'])
def test_target_reaches_every_gram_family(lib, obs_dim):
    dp.check_family(lib, obs_dim)


@pytest.mark.parametrize('flags', [[], ['--vpg']], ids=['dice_maml', 'vpg_dice_maml'])
def test_run_script(tmp_path, flags):
    """run_scripts/dice_maml_run_point_mass.py in a fresh child process: two iterations, a finite logged LossBefore"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = os.path.join(root, 'run_scripts', 'dice_maml_run_point_mass.py')
    subprocess.run([sys.executable, script, '--n_itr', '2', '--dump_path', str(tmp_path), '--quiet'] + flags, check=True, timeout=120)
    rows = list(csv.DictReader(open(os.path.join(str(tmp_path), 'progress.csv'))))
    assert len(rows) == 2
    for r in rows:
        v = float(r['LossBefore'])
        assert v == v and abs(v) != float('inf')
