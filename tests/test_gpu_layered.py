"""The layer-by-layer kernels on work items of several rounds / chunks / loss blocks and at the edges of their widths, on an MI355X:
tests/layered_checks.py holds the cases, the reasons and the tolerances (parity_checks' own: the float64 oracle, 1e-4).  Every test
plans its contexts for one compute unit (two in row case D), so that a work item is a whole task; profiles/layered_edges.txt keeps
the worst errors of a run."""
import pytest

from tests import devlib, layered_checks as lc

pytestmark = pytest.mark.gpu

SHAPES = sorted(lc.ROW_SHAPES)


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.mark.parametrize('what', ['loss_grad', 'hvp', 'meta'])
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('case', sorted(lc.ROW_CASES))
def test_row_loop_edges(lib, monkeypatch, case, shape, what):
    lc.long_items(monkeypatch, lib, lc.ROW_CASES[case]['max_cus'])
    lc.check_rows(lib, case, shape, what)


@pytest.mark.parametrize('shape', SHAPES)
def test_row_loop_edges_per_task_old_distribution(lib, monkeypatch, shape):
    # compact_log_std: k_gen_loss reads the old log_std from its per-task table, not from the rows
    lc.long_items(monkeypatch, lib, 1)
    lc.check_rows(lib, 'B', shape, 'loss_grad', compact_log_std=True, tag=' compact_log_std')


@pytest.mark.parametrize('what', ['loss_grad', 'hvp', 'meta'])
@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('case', ['B', 'C'])
def test_row_loop_edges_exact_fp32_gemms(lib, monkeypatch, case, shape, what):
    # PROMP_GEN_FP32=1: the same edges in k_gen_linear / k_gen_wgrad's row loops (the switch changes nothing for the three-action
    # shape, which the cooperative kernels take)
    lc.long_items(monkeypatch, lib, lc.ROW_CASES[case]['max_cus'], gen_fp32=True)
    lc.check_rows(lib, case, shape, what, tag=' PROMP_GEN_FP32=1')


def test_dice_row_tangents_over_several_loss_blocks(lib, monkeypatch):
    lc.long_items(monkeypatch, lib, 1)
    lc.check_dice(lib)


@pytest.mark.parametrize('name', sorted(lc.WIDTH_CASES))
def test_width_edges(lib, monkeypatch, name):
    """Held to parity_checks' 1e-4 like everything else: measured (profiles/layered_edges.txt) the contraction over 1024 / 1023
    observations gives 2.3e-5 / 8.7e-6 on the Hessian-vector product and 2.4e-6 / 2.7e-6 on the gradient, four layers of 256 units
    1.9e-6 -- no bound of their own was needed."""
    lc.long_items(monkeypatch, lib, 1)
    lc.check_width(lib, name, 'loss_grad')
    lc.check_width(lib, name, 'hvp')
    if lc.WIDTH_CASES[name].get('meta'):
        lc.check_width(lib, name, 'meta')
