"""Start states drawn on the device, on the kernel emulator (tests/point_start_checks.py): k_point_starts and the DEVICE_START
instantiations of the rollout and collection kernels against the table path, bit for bit, at sizes one OS thread per lane affords --
the smallest case of each group.

Left to tests/test_gpu_point_start.py (-m gpu): B = 65 and 129, the bare environment, walls and momentum collections."""
import pytest

from tests import devlib, point_start_checks as ps


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


def test_draw_is_the_restatement(lib):
    ps.check_draw(lib, *ps.DRAW_CASES[0])


@pytest.mark.parametrize('case', ps.EMU_COLLECT_CASES, ids=lambda c: '-'.join(str(v) for v in c[:7]).replace(' ', ''))
def test_collection_is_the_table_path(lib, case):
    ps.check_collect(lib, case)


def test_rollout_is_the_table_path(lib):
    ps.check_rollout(lib, *ps.ROLLOUT_CASES[0])


def test_refusals(lib):
    ps.check_refusals(lib)
