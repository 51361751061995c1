"""The fused and cooperative pass kernels (k_pass / k_chain_hvp, k_wide_*, k_wb_*) on work items of several rounds, tiles and
segments, on an MI355X: tests/fused_checks.py holds the cases, the reasons and the tolerances (parity_checks' own: the float64 oracle,
1e-4).  Every test plans its contexts for one compute unit (two in row cases D and E), so that a work item is a whole task or half of
one; tests/host/plan_check.cpp pins the tables that gives, profiles/fused_rows.txt keeps the worst errors of a run."""
import numpy as np
import pytest

from tests import devlib, fused_checks as fc

pytestmark = pytest.mark.gpu

SHAPES = list(fc.ROW_SHAPES)
CASES = sorted(fc.ROW_CASES)


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.mark.parametrize('what', ['loss_grad', 'hvp'])
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('case', CASES)
def test_row_loops(lib, monkeypatch, case, shape, what):
    # loss_grad: the four objectives (ratio, clip, log-likelihood, mean KL) with and without the log_std clip
    fc.plan(monkeypatch, lib, fc.ROW_CASES[case]['max_cus'], shape)
    fc.check_rows(lib, case, shape, what)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('case', fc.META_CASES)
def test_row_loops_meta(lib, monkeypatch, case, shape):
    # K = 1, one epoch: the forward-only instances (loss_after) and the per-task reduction over several partial rows
    fc.plan(monkeypatch, lib, fc.ROW_CASES[case]['max_cus'], shape)
    fc.check_rows(lib, case, shape, 'meta')


@pytest.mark.parametrize('shape', fc.ONE_PER_FAMILY)
def test_row_loops_meta_two_inner_steps(lib, monkeypatch, shape):
    fc.plan(monkeypatch, lib, fc.ROW_CASES['D']['max_cus'], shape)
    fc.check_rows(lib, 'D', shape, 'meta', tag=' K=2', K=2)


@pytest.mark.parametrize('shape', fc.FAMILY_SHAPES['Chain'])
@pytest.mark.parametrize('case', fc.META_CASES)
def test_primal_cache_blocks_of_later_tiles(lib, monkeypatch, case, shape):
    fc.plan(monkeypatch, lib, fc.ROW_CASES[case]['max_cus'], shape)
    fc.check_cache(lib, case, shape)


@pytest.mark.parametrize('shape', fc.ONE_PER_FAMILY)
def test_row_loops_per_task_old_distribution(lib, monkeypatch, shape):
    # compact_log_std: the old log_std comes from the per-task table, not from the rows
    fc.plan(monkeypatch, lib, 1, shape)
    fc.check_rows(lib, 'B', shape, 'loss_grad', tag=' compact_log_std', compact_log_std=True)


def test_wide_fp32_switch_at_128_wide(lib, monkeypatch):
    # PROMP_WIDE_FP32=1: (128,128) at obs 20 on k_wide_* <128, 2> instead of k_wb_*; the switch is read when a context is created, so it
    # is set in this process around the contexts of the case (monkeypatch restores it)
    shape = 'h128x128_o20_a6_fp32'
    fc.plan(monkeypatch, lib, 1)
    g_default = fc.gradients(lib, 'B', shape)
    fc.plan(monkeypatch, lib, 1, shape)
    g_switched = fc.gradients(lib, 'B', shape)
    assert g_switched.shape == g_default.shape and not np.array_equal(g_switched, g_default), 'the switch changed nothing'
    for what in ('loss_grad', 'hvp', 'meta'):
        fc.check_rows(lib, 'B', shape, what, tag=' PROMP_WIDE_FP32=1')


@pytest.mark.parametrize('shape', sorted(fc.DICE_SHAPES))
def test_dice_row_tangents_over_several_rounds(lib, monkeypatch, shape):
    fc.plan(monkeypatch, lib, 1)
    fc.check_dice(lib, shape)


@pytest.mark.parametrize('shape', sorted(fc.RANGE_SHAPES))
def test_split_range_on_one_compute_unit(lib, monkeypatch, shape):
    fc.plan(monkeypatch, lib, 1)
    fc.check_range(lib, shape)
