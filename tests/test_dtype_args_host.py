"""CPU: the memory-bound entries refuse a dtype code outside {MV_F32, MV_BF16} before any HIP call -- a negative
MV_E_INVALID and a message naming the entry -- instead of launching nothing and returning MV_OK.  Pointers are dummy
non-null integers and are never dereferenced: the dtype check comes before the launch."""
import pytest

BAD = 7          # not a dtype code (MV_F32 = 0, MV_BF16 = 1)
P, Q, R = 0x1000, 0x2000, 0x3000

# (entry, the name its messages carry, arguments with {i} / {o} for the in / out dtype)
TWO_DTYPES = [
    ("mv_adaptive_avgpool2d_nhwc_fwd", b"avgpool", lambda i, o: (P, Q, 1, 2, 2, 8, 1, 1, i, o, None)),
    ("mv_adaptive_avgpool2d_nhwc_fwd", b"avgpool", lambda i, o: (P, Q, 1, 4, 4, 3, 2, 2, i, o, None)),
    ("mv_layernorm_fwd", b"layernorm", lambda i, o: (P, None, None, Q, 2, 8, 0, 1e-5, i, o, None)),
    ("mv_layernorm_fwd", b"layernorm", lambda i, o: (P, None, None, Q, 2, 5, 0, 1e-5, i, o, None)),
    ("mv_cast", b"cast", lambda i, o: (P, Q, 8, i, o, None)),
    ("mv_nchw_to_nhwc", b"nchw_to_nhwc", lambda i, o: (P, Q, 1, 3, 2, 2, i, o, None)),
]
ONE_DTYPE = [
    ("mv_eltwise_fwd", b"eltwise", lambda d: (P, Q, 8, 1, d, None)),
    ("mv_eltwise_fwd", b"eltwise", lambda d: (P, Q, 5, 1, d, None)),
    ("mv_add_fwd", b"add", lambda d: (P, Q, R, 8, 0, d, None)),
    ("mv_add_fwd", b"add", lambda d: (P, Q, R, 5, 0, d, None)),
]


def _refused(lib, entry, who, args):
    rc = getattr(lib, entry)(*args)
    msg = lib.mv_last_error()
    assert rc == -1, f"{entry}{args} returned {rc}"
    assert who in msg and b"dtype" in msg, msg


@pytest.mark.parametrize("case", range(len(TWO_DTYPES)))
@pytest.mark.parametrize("dtypes", [(BAD, BAD), (BAD, 0), (1, BAD)])
def test_unknown_in_out_dtype_is_refused(built_lib, case, dtypes):
    entry, who, args = TWO_DTYPES[case]
    _refused(built_lib, entry, who, args(*dtypes))


@pytest.mark.parametrize("case", range(len(ONE_DTYPE)))
def test_unknown_dtype_is_refused(built_lib, case):
    entry, who, args = ONE_DTYPE[case]
    _refused(built_lib, entry, who, args(BAD))
