"""DiCE objectives outside the register-chained kernels, on the kernel emulator: the row tangents k_wide_hvp / k_wb_hvp /
k_gen_loss hand to k_dice_scan (sign, scale, partial last tiles) and the host sequencing around them, at tiny shapes.
The parity tests proper are tests/test_gpu_dice_shapes.py (-m gpu)."""
import pytest

from tests import devlib, dice_shape_checks as ds


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')      # dozens of launches per case: fewer host threads per emulated launch


def test_general_torch_reference_is_the_oracle_on_tanh():
    ds.check_general_reference_against_oracle(ds.case(301, M=2, P=2, T=8, O=6, A=3, hidden=(16, 16, 16), K=2, alpha=0.05, ragged=True, Tmax=9))


# M = 2 tasks, P = 2 paths, T <= 12; the trims leave task 0 of step 0 with a path of one row
def test_dice_coop_fp32(lib):
    ds.check_dice_shape(lib, ds.case(311, M=2, P=2, T=12, O=40, A=3, hidden=(64, 64), trim=[(0, 0, 1, 1)]))


def test_dice_coop_split(lib):
    ds.check_dice_shape(lib, ds.case(312, M=2, P=2, T=12, O=20, A=6, hidden=(128, 128), ragged=True))


def test_dice_zero_padded_widths(lib):
    ds.check_dice_shape(lib, ds.case(313, M=2, P=2, T=10, O=40, A=3, hidden=(48, 20), trim=[(0, 1, 0, 1)]))


def test_dice_layered(lib):
    ds.check_dice_shape(lib, ds.case(314, M=2, P=2, T=10, O=11, A=3, hidden=(100,), ragged=True))
