"""Helpers shared by the GPU tests of the concat-free kernels (SqueezeNet, GoogLeNet, DenseNet): raw pointers for `_lib.call`,
sentinel-filled strided destinations with a guard behind them, and the check that a kernel wrote its channel slice and nothing else."""
import torch

SENTINEL = -7.0
GUARD = 64


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _dest(M, ld, dtype=torch.bfloat16):
    """A sentinel-filled destination of M rows of ld bf16 (or `dtype`) with a guard behind it."""
    return torch.full((M * ld + GUARD,), SENTINEL, dtype=dtype, device="cuda")


def _read(buf, M, ld):
    host = buf.float().cpu()
    return host[:M * ld].reshape(M, ld), host[M * ld:]


def _check_slice(y, guard, c, ref, bound, tag, exact=False):
    """Inside [c, c + n) the reference to `bound` (or bit-equal); outside the sentinel; the guard intact; no NaN anywhere."""
    n = ref.shape[1]
    assert not bool(torch.isnan(y).any()) and not bool(torch.isnan(guard).any()), (tag, "NaN")
    assert bool((guard == SENTINEL).all()), tag
    outside = torch.cat([y[:, :c], y[:, c + n:]], 1)
    assert bool((outside == SENTINEL).all()), (tag, "written outside the slice")
    if exact:
        wrong = y[:, c:c + n].double() != ref
        assert not bool(wrong.any()), (tag, int(wrong.sum()), torch.nonzero(wrong)[:8].tolist())
        return 0.0
    err = float((y[:, c:c + n].double() - ref).abs().max())
    assert err <= bound, (tag, err, bound)
    return err
