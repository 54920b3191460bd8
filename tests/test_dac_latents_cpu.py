"""CPU suite: nc_dac_from_latents[_dev] is exported, bound, refuses a null handle and never computes on the host."""
import ctypes as C

import numpy as np
import pytest

from neuralcodecs_amd import _lib

NAMES = ("nc_dac_from_latents", "nc_dac_from_latents_dev")


def test_both_symbols_are_exported_and_bound():
    L = _lib.lib()
    table = {s[0]: s for s in _lib.SYMBOLS}
    for name in NAMES:
        assert hasattr(L, name), f"{name} is not exported by libnc_mi355x.so"
        _, res, args = table[name]
        fn = getattr(L, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == list(args)
        # (h, latents, B, C_lat, frames, z, projected, codes)
        assert args == [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]


def test_python_method_exists():
    from neuralcodecs_amd import DAC
    assert callable(getattr(DAC, "from_latents", None))


def _call(name, h):
    lat = np.ones((1, 8, 4), np.float32)
    z = np.full((1, 16, 4), 7.0, np.float32); p = np.full((1, 8, 4), 7.0, np.float32); c = np.full((1, 1, 4), 7, np.int64)
    st = getattr(_lib.lib(), name)(h, lat.ctypes.data, 1, 8, 4, z.ctypes.data, p.ctypes.data, c.ctypes.data)
    return st, bool(np.all(z == 7.0) and np.all(p == 7.0) and np.all(c == 7))


@pytest.mark.parametrize("name", NAMES)
def test_null_handle_is_einval_and_writes_nothing(name):
    st, untouched = _call(name, None)
    assert st == _lib.NC_EINVAL and untouched
    assert b"null codec handle" in _lib.lib().nc_last_error()


@pytest.mark.skipif(_lib.lib().nc_device_count() > 0, reason="GPU present: covered by the gpu suite")
def test_no_cpu_fallback():
    """Without a device there is no handle to call it with: creation fails with NC_EDEVICE, and the entry points compute nothing."""
    from neuralcodecs_amd import DAC, DACConfig
    with pytest.raises(_lib.NcDeviceError):
        DAC(DACConfig())
    for name in NAMES:
        st, untouched = _call(name, None)
        assert st != _lib.NC_OK and untouched
