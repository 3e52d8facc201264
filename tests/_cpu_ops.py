"""The CPU fake of the host tests: forwards run WITHOUT a GPU because every launch is replaced by a recorder and every device
allocation by a CPU tensor.  The host-side dispatch -- which kernel serves which layer, with which prepared operands -- is pure
Python plus the library's `_supported` entries, which need no device."""
import numpy as np
import torch


def cpu_ops(monkeypatch):
    """Apply the fake; returns the recorder's list of (entry name, argument tuple), filled as launches are made."""
    from eqxvision_amd import _act, _lib, ops
    calls = []
    cpu = lambda: torch.device("cpu")
    zeros = lambda shape, dtype: torch.zeros(shape, dtype=dtype)
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)) or 0)
    monkeypatch.setattr(_act, "device", cpu)
    monkeypatch.setattr(ops, "device", cpu)
    monkeypatch.setattr(ops, "empty", zeros)
    monkeypatch.setattr(_act, "empty", zeros)
    monkeypatch.setattr(ops, "stream_ptr", lambda: 0)
    monkeypatch.setattr(ops, "_dev", lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt))
    monkeypatch.setattr(ops, "_splitk_scratch", lambda *a, **k: None)
    monkeypatch.setattr(ops, "_fc_workspace", lambda nbytes: torch.zeros(1))
    return calls
