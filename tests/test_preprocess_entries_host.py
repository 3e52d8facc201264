"""CPU: the argument rules the four record entries of csrc/preprocess.hip share -- batch size, output dtype, NULL and overlapping
buffers -- asked of each entry with made-up (never dereferenced) device addresses and real host records.  Every refusal comes
before any device call; what each entry checks of its own records is in its own file."""
import numpy as np
import pytest

from eqxvision_amd import _lib
from eqxvision_amd import preprocess as P

INVALID, UNSUPPORTED = -1, -2
SIZES = [(40, 30), (400, 44)]
X_BYTES = 3 * (40 * 30 + 400 * 44)
X, Y, DEV = 1 << 20, 2 << 20, 5 << 20


def _ragged(lib, B, y, dtype):
    rec, tables, (hout, wout) = P.ragged_plan(SIZES, [(36, 27), (40, 36)], (1, 2, 20, 24))
    return lib.mv_preprocess_u8_ragged_fwd(X, X_BYTES, y, rec.ctypes.data, DEV, DEV, tables.size, DEV, DEV, B, hout, wout, 0, dtype, 0, None)


def _boxes(lib, B, y, dtype):
    rec, (hout, wout) = P.boxes_plan(SIZES, [(1, 2, 20, 24), (0, 4, 300, 40)], [False, True], 32)
    return lib.mv_preprocess_u8_boxes_fwd(X, X_BYTES, y, rec.ctypes.data, DEV, DEV, DEV, B, hout, wout, 0, dtype, 0, None)


def _mix(lib, B, y, dtype):
    rec, (hout, wout) = P.boxes_plan(SIZES, [(1, 2, 20, 24), (0, 4, 300, 40)], [False, True], 32)
    mix = P.mix_plan(2, (hout, wout), partner=[1, 0], lam=[0.5, 0.5])
    return lib.mv_preprocess_u8_mix_fwd(X, X_BYTES, y, rec.ctypes.data, DEV, mix.ctypes.data, DEV, DEV, DEV, None, None, None, 0, 1.0, 0.0,
                                        B, hout, wout, 0, dtype, 0, None)


def _seg(lib, B, y, dtype):
    rec, (hout, wout) = P.seg_plan(SIZES, [(50, 20), (36, 48)], [(18, 0), (4, 8)], [False, True], (32, 40))
    return lib.mv_preprocess_u8_seg_fwd(X, X_BYTES, None, 0, y, None, rec.ctypes.data, DEV, DEV, DEV, B, hout, wout, 0, 255, 0, dtype, 0, None)


@pytest.mark.parametrize("name,entry,max_B", [("preprocess_u8_ragged", _ragged, 65535), ("preprocess_u8_boxes", _boxes, 65535),
                                              ("preprocess_u8_mix", _mix, 32767), ("preprocess_u8_seg", _seg, 65535)])
def test_every_record_entry_refuses_the_common_arguments_before_any_device_call(built_lib, name, entry, max_B):
    def call(B=2, y=Y, dtype=_lib.F32):
        return entry(built_lib, B, y, dtype), built_lib.mv_last_error()

    rc, msg = call(B=0)
    assert rc == INVALID and (name + ": bad sizes").encode() in msg, (rc, msg)
    rc, msg = call(B=max_B + 1)
    assert rc == INVALID and f"{name}: batch {max_B + 1} too large".encode() in msg, (rc, msg)
    rc, msg = call(dtype=7)
    assert rc == INVALID and (name + ": out_dtype must be MV_F32 or MV_BF16").encode() in msg, (rc, msg)
    rc, msg = call(y=None)
    assert rc == UNSUPPORTED and (name + ": null buffer").encode() in msg, (rc, msg)
    for y in (X + 100, X + X_BYTES - 1, X - 1):                # inside x, on its last byte, one byte before it
        rc, msg = call(y=y)
        assert rc == UNSUPPORTED and msg.startswith((name + ": ").encode()) and b"overlap" in msg, (y, rc, msg)
    # no call with sound arguments: where there is a device it would launch on the made-up addresses
