"""CPU: aqz_ds_run_device_batch_tiled_base, aqz_ds_run_device_batch_chunked_base
and aqz_ds_tiled_base_flag_slots are declared in include/aqz_downsampler.h,
exported by the library, bound by the package, and answer a null handle
without touching a device (a handle cannot be made without one, so the null
that can be passed here is the handle; tests/test_gpu_tiled_base.py refuses the
rest)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("aqz_ds_run_device_batch_tiled_base", "aqz_ds_run_device_batch_chunked_base")
SLOTS = "aqz_ds_tiled_base_flag_slots"
AQZ_INVALID_ARGUMENT = 1


def test_declared_and_exported(aqz):
    src = open(os.path.join(ROOT, "include", "aqz_downsampler.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = aqz.lib()
    for n in CALLS:
        assert re.search(r"\bint\s+" + n + r"\s*\(", src), f"{n} is not declared"
    assert re.search(r"\buint32_t\s+" + SLOTS + r"\s*\(", src), f"{SLOTS} is not declared"
    for n in CALLS + (SLOTS,):
        assert hasattr(lib, n), f"{n} is not exported"
        assert n in aqz.EXPORTS
    for m in ("run_device_batch_tiled_base", "run_device_batch_chunked_base",
              "tiled_base_flag_slots"):
        assert hasattr(aqz.Downsampler, m), m


def test_the_header_documents_kind_6():
    src = open(os.path.join(ROOT, "include", "aqz_downsampler.h")).read()
    doc = src[: src.index("int aqz_ds_last_batch_kind(")]
    doc = doc[doc.rindex("/*"):]
    assert re.search(r"\b6 = fused 2-D cascade writing chunk tiles, base included", doc)


def test_null_handle(aqz):
    lib = aqz.lib()
    assert lib.aqz_ds_run_device_batch_tiled_base(None, None, 4, None, None, None, None, None,
                                                  None) == AQZ_INVALID_ARGUMENT
    assert lib.aqz_ds_run_device_batch_chunked_base(None, None, 4, None, None, None,
                                                    None) == AQZ_INVALID_ARGUMENT
    assert lib.aqz_ds_tiled_base_flag_slots(None, 64, 64) == 0
