"""The outer optimiser's rule, its arguments and the gradient clip on the kernel emulator (tests/outer_optimizer_checks.py): the
general final-stage kernels -- fused and split, with and without trained step sizes -- at M 2, P 1, T 30 on the chain kernels (the
final stage does not depend on the pass family).  The parity tests proper are tests/test_gpu_outer_optimizer.py (-m gpu)."""
import pytest

from tests import devlib, minibatch_checks as mb, outer_optimizer_checks as oc, step_size_checks as sc


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


@pytest.fixture(scope='module')
def case():
    return sc.PrompCase(701, M=2, P=1, T=30, O=7, A=3, hidden=(32, 32), K=1, ragged=True)


@pytest.mark.parametrize('key', sorted(oc.RULES))
def test_rule_against_its_mirror(lib, case, key):
    oc.check_rule(lib, case, key, clip=False, steps=2)
    oc.check_rule(lib, case, key, clip=True, steps=2)


def test_rule_with_learn_std_false_and_with_trained_step_sizes(lib, case):
    oc.check_rule(lib, case, 'nesterov', clip=True, learn_std=False, steps=2)
    oc.check_rule(lib, case, 'adam', clip=True, sizes=True, steps=2)


def test_forced_general_kernels_equal_the_plain_ones(lib, case, monkeypatch):
    oc.check_generic_equals_plain(lib, case, monkeypatch)


def test_final_stage_grid_edge(lib, monkeypatch):
    """Theta 62, K 2 (outer_optimizer_checks.EDGE_SHAPES): the scalar columns straddle two column blocks, and with trained step
    sizes the reduce grid is exactly full.  These two checks only -- measured at 57 s on the emulator (twelve contexts; the same
    pair on the module's own shape takes 31 s for the first check alone) against 110 to 190 s for the five checks the GPU suite runs
    on each edge shape"""
    case = oc.edge_case('theta62')
    oc.check_generic_equals_plain(lib, case, monkeypatch)
    oc.check_stats_against_exchange(lib, case)


def test_inactive_clip_is_no_clip(lib, case):
    oc.check_inactive_clip(lib, case, epochs=2)
    oc.check_inactive_clip(lib, case, epochs=2, sizes=True)


def test_routes_agree_with_clipping_on(lib, case):
    oc.check_routes_with_clip(lib, case, 'adam', sizes=True)
    oc.check_routes_with_clip(lib, case, 'momentum')


def test_minibatched_sgd_with_clip_equals_truncated_batches(lib):
    oc.check_minibatch_sgd_clip(lib, 703, lengths=mb.EMU_LENGTHS, pattern=mb.EMU_ASSIGN_2)


def test_state(lib, case):
    oc.check_state(lib, case)
    oc.check_session_keeps_settings(lib)


def test_refusals(lib, case):
    oc.check_refusals(lib, case)
