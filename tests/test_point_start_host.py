"""CPU-only checks of tests/point_start_checks.py: the NumPy restatement of the device's start-state draw (range, moments, the counter
domain beside the action noise's), and that every collection case of the emulator and GPU files meets the events it is built for, on
point_collect_checks.collect_oracle fed the restated table."""
import pytest

from tests import point_start_checks as ps

ids = ['-'.join(str(v) for v in c[:7]).replace(' ', '') for c in ps.COLLECT_CASES]


def test_restatement_range_moments_and_counter_domain():
    ps.check_restatement_on_cpu()


@pytest.mark.parametrize('case', ps.COLLECT_CASES, ids=ids)
def test_collection_case_meets_its_events(case):
    ps.collect_case_is_sound(case)
