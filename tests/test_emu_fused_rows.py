"""tests/fused_checks.py's subset for the emulator (kernel sources on the SIMT interpreter, one OS thread per lane): row case D on the
register-chained (32, 32) kernels -- 300 rows on two workgroups, the middle task split between them at tile 4 -- and a 65-row work
item on the cooperative FP32 (64, 64) kernels, a second and a third round of one row.  The conditions on the inputs of every GPU case
(a dropped row must move the oracle's gradient by ten tolerances; every shape on the family it is meant for) are checked here,
without any kernel."""
import pytest

from tests import devlib, fused_checks as fc


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.mark.parametrize('case,shape', fc.ROW_PAIRS)
def test_inputs_of_the_row_cases_show_a_dropped_row(monkeypatch, case, shape):
    if fc.ALL_SHAPES[shape].get('wide_fp32'):
        monkeypatch.setenv('PROMP_WIDE_FP32', '1')
    else:
        monkeypatch.delenv('PROMP_WIDE_FP32', raising=False)
    fc.shape_kwargs(fc.ROW_CASES[case]['lengths'], **fc.ALL_SHAPES[shape])
    fc.check_inputs_show_a_dropped_row(case, shape)


@pytest.mark.parametrize('what', ['loss_grad', 'hvp'])
@pytest.mark.parametrize('name', sorted(fc.EMU_CASES))
def test_several_rounds_per_work_item(lib, monkeypatch, name, what):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')      # fewer host threads per emulated launch
    fc.plan(monkeypatch, lib, fc.EMU_CASES[name]['max_cus'])
    fc.check_emu(lib, name, what)
