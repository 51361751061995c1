"""Start states drawn on the device, on the MI355X (tests/point_start_checks.py): promp_draw_point_starts against the NumPy
restatement, promp_collect_point_family_dev and promp_rollout_point_family_dev against the table entry points handed the restated
table -- tables, slab and moments bit for bit --, and the refusals.  A handful of sub-millisecond launches per case.
test_point_start_host.py checks on the CPU that every collection case meets the events it is built for."""
import pytest

from tests import devlib, point_start_checks as ps

pytestmark = pytest.mark.gpu
ids = lambda c: '-'.join(str(v) for v in c[:7]).replace(' ', '')


@pytest.fixture(scope='module')
def lib():
    return devlib.gpu_library()


@pytest.mark.parametrize('case', ps.DRAW_CASES, ids=lambda c: '-'.join(str(v) for v in c[:3]))
def test_draw_is_the_restatement(lib, case):
    ps.check_draw(lib, *case)


@pytest.mark.parametrize('case', ps.COLLECT_CASES, ids=ids)
def test_collection_is_the_table_path(lib, case):
    ps.check_collect(lib, case)


@pytest.mark.parametrize('case', ps.ROLLOUT_CASES, ids=ids)
def test_rollout_is_the_table_path(lib, case):
    ps.check_rollout(lib, *case)


def test_refusals(lib):
    ps.check_refusals(lib)
