"""CPU: aqz_ds_run_device_volume_tiled and aqz_ds_run_device_volume_chunked are
declared in include/aqz_downsampler.h, exported by the library, bound by the
package, and answer null arguments with AQZ_INVALID_ARGUMENT without touching
a device (a handle cannot be made without one, so the null that can be passed
here is the handle; tests/test_gpu_volume_tiled.py refuses the rest)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("aqz_ds_run_device_volume_tiled", "aqz_ds_run_device_volume_chunked")
AQZ_INVALID_ARGUMENT = 1


def test_declared_and_exported(aqz):
    src = open(os.path.join(ROOT, "include", "aqz_downsampler.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = aqz.lib()
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), f"{n} is not declared"
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in aqz.EXPORTS
    assert hasattr(aqz.Downsampler, "run_device_volume_tiled")
    assert hasattr(aqz.Downsampler, "run_device_volume_chunked")


def test_null_handle(aqz):
    lib = aqz.lib()
    assert lib.aqz_ds_run_device_volume_tiled(None, None, 4, None, None, None, None, None,
                                              None) == AQZ_INVALID_ARGUMENT
    assert lib.aqz_ds_run_device_volume_chunked(None, None, 4, None, None, None,
                                                None) == AQZ_INVALID_ARGUMENT
