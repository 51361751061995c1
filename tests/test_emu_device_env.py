"""Environments that live on the device (tests/device_env_checks.py) on the kernel emulator: host sequencing, the counters and
refusals, k_file_step's indexing and the sampler's loop, at the smallest shapes (M = 2, B = 3, max_path_length 4; one OS thread per
lane).  The same checks run on the GPU, with a partial wave, a second 64-lane chunk and the layer-by-layer shape, in
test_gpu_device_env.py.  The emulator's pointer check passes every non-NULL pointer (its device is the host's heap), so the
refusal of pageable memory is the GPU file's."""
import pytest

from promp_amd import _lib, session
from tests import device_env_checks as dc, devlib


@pytest.fixture(scope='module')
def lib():
    return devlib.emu_library()


@pytest.fixture(autouse=True)
def two_cus(monkeypatch):
    monkeypatch.setenv('PROMP_EMU_CUS', '2')


@pytest.fixture()
def bound(lib):
    _lib.set_library_for_testing(lib)
    yield lib
    _lib.set_library_for_testing(None)
    session._current = None


def test_host_loop_against_device_path(lib):
    dc.check_host_against_device(lib, 2, 3, 4, (32, 32))


def test_host_loop_against_device_path_layer_by_layer(lib):
    dc.check_host_against_device(lib, 2, 3, 4, (16, 16, 16), step=1, clip_infos=False)


def test_fixed_horizon(lib):
    dc.check_fixed_horizon(lib)


def test_upload_step_dev(lib):
    dc.check_upload_step_dev(lib)


def test_stop_and_progress(lib):
    dc.check_stop_and_progress(lib)


def test_refusals(lib):
    dc.check_refusals(lib, emulated=True)


def test_sampler(bound):
    dc.check_sampler(bound)


def test_pointer_extractor_without_a_library():
    """device_pointer alone: ints, __cuda_array_interface__, data_ptr() objects and what it refuses, by name"""
    import numpy as np

    class Tensor(object):
        def __init__(self, dtype='torch.float32', contiguous=True, cuda=True, n=6):
            self.dtype, self._c, self.is_cuda, self._n, self.device = dtype, contiguous, cuda, n, 'cuda:0' if cuda else 'cpu'
        def data_ptr(self): return 4096
        def is_contiguous(self): return self._c
        def numel(self): return self._n

    class Cai(object):
        def __init__(self, shape=(2, 3), typestr='<f4', strides=None):
            self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(8192, False), version=2, strides=strides)

    ptr = lambda x, dt=np.float32, n=6: _lib.device_pointer(x, dt, n, 'x')
    assert ptr(None) is None and ptr(12345) == 12345 and ptr(Tensor()) == 4096 and ptr(Cai()) == 8192
    assert ptr(Cai(strides=(12, 4))) == 8192 and ptr(Tensor('torch.bool'), np.uint8) == 4096
    for bad, why in ((Tensor('torch.float64'), 'dtype'), (Tensor(contiguous=False), 'not contiguous'), (Tensor(cuda=False), 'not on the GPU'),
                     (Tensor(n=5), '5 elements'), (Cai(typestr='<f8'), 'dtype'), (Cai(strides=(4, 8)), 'not C-contiguous'),
                     (Cai(shape=(7,)), '7 elements'), (np.zeros(6, np.float32), 'ndarray is not device memory'), ([0.0] * 6, 'list is not')):
        with pytest.raises(_lib.PrompError, match=why):
            ptr(bad)
    assert _lib.stream_handle(None) == 0 and _lib.stream_handle(77) == 77
    assert _lib.stream_handle(type('S', (), dict(cuda_stream=99))()) == 99
