"""What the strict GPU modules (test_strict_gpu.py, test_strict_mem_gpu.py) share: the module fixture that loads the library and reads the
device status word before and after, device / host conversions, the sentinel-filled output and the flag scope."""
import numpy as np
import pytest
import torch

from eqxvision_amd import _lib

DT = {"bf16": _lib.BF16, "fp32": _lib.F32}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    _lib.load()
    _lib.check_device_status()
    yield
    _lib.check_device_status()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _dev(a, dtype="bf16"):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(torch.bfloat16) if dtype == "bf16" else t).cuda()


def _host(t):
    return t.float().cpu().numpy().astype(np.float64)


def _out(shape, dtype="bf16", fill=-7.0):
    return torch.full(shape, fill, dtype=torch.bfloat16 if dtype == "bf16" else torch.float32, device="cuda")


class _Flags:
    def __init__(self, flags):
        self.flags = [(f.split("=")[0], int(f.split("=")[1]) if "=" in f else 1) for f in flags]

    def __enter__(self):
        for k, v in self.flags:
            _lib.set_flag(k, v)

    def __exit__(self, *a):
        for k, _ in self.flags:
            _lib.set_flag(k, 0)
