"""Learned inner step sizes on the kernel emulator (tests/step_size_checks.py): the two float64 references against each other
(no device at all), then the chain kernels, the DiCE two-piece reduction and the split / fused final stage at M 2, P 1, T 30.
The parity tests proper are tests/test_gpu_step_sizes.py (-m gpu)."""
import pytest

from tests import devlib, dice_shape_checks as ds, step_size_checks as sc


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')      # dozens of launches per case: fewer host threads per emulated launch


@pytest.fixture(scope='module')
def chain_case():
    return sc.PrompCase(501, M=2, P=1, T=30, O=7, A=3, hidden=(32, 32), K=1, ragged=True)


DICE_CASE = ds.case(506, M=2, P=1, T=30, O=7, A=3, hidden=(32, 32), K=2, ragged=True)


def test_analytic_step_size_gradient_agrees_with_central_differences(chain_case):
    sc.check_references(chain_case)
    sc.check_references(sc.PrompCase(502, M=2, P=2, T=20, O=5, A=2, hidden=(16, 16), K=2, ragged=True))


@pytest.mark.parametrize('outer', ['dice', 'vpg'])
def test_analytic_dice_step_size_gradient_agrees_with_central_differences(outer):
    sc.check_dice_references(DICE_CASE, outer)


def test_step_size_gradient_chain_kernels(lib, chain_case):
    sc.check_alpha_grad(lib, chain_case)


def test_step_size_gradient_dice_inner_objective(lib):
    sc.check_dice_alpha_grad(lib, DICE_CASE)


def test_step_size_split_path_equals_fused(lib, chain_case):
    sc.check_split_equals_fused(lib, chain_case)


def test_host_exchange_route_equals_optimize(lib, chain_case):
    sc.check_host_exchange_route(lib, chain_case)
