"""The host side of the device-tensor route, without a GPU: what counts as device data, what is refused before
anything could be launched, that numpy callers never load torch through the package, and the C-ABI's new names.
(CUDA tensors are stood in for by torch's fake tensors: a device, a dtype and strides, no memory and no GPU.)"""
from __future__ import annotations

import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from libcluster_amd import capi

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ("lc_ctx_set_data_device", "lc_ctx_data_range", "lc_learn_ctx", "lc_ctx_get_qz_rows_device",
               "lc_ctx_get_predictions_device")


def fake_cuda(shape, dtype):
    import torch
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        return torch.empty(shape, device="cuda", dtype=dtype)


def test_numpy_route_never_imports_torch():
    code = ("import sys, numpy as np\n"
            "import libcluster_amd\n"
            "from libcluster_amd import capi\n"
            "X = np.zeros((4, 3))\n"
            "assert capi.is_device_tensor(X) is False\n"
            "assert capi.device_blocks(X) is None and capi.device_blocks([X, X]) is None\n"
            "assert 'torch' not in sys.modules, 'torch was imported'\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cpu_tensor_is_host_data():
    import torch

    t = torch.zeros((4, 3), dtype=torch.float64)
    assert capi.is_device_tensor(t) is False
    assert capi.device_blocks(t) is None and capi.device_blocks([t, np.zeros((2, 3))]) is None
    assert capi.device_blocks(torch.zeros((4, 3), dtype=torch.float32)) is None  # (np.asarray converts it, as ever)


def test_device_tensors_are_recognised_and_checked():
    import torch

    t = fake_cuda((6, 3), torch.float64)
    assert capi.is_device_tensor(t)
    assert len(capi.device_blocks(t)) == 1 and capi.device_blocks(t)[0] is t
    assert len(capi.device_blocks([t, fake_cuda((0, 3), torch.float64)])) == 2
    with pytest.raises(TypeError, match=r"float64.*X\.double\(\)"):
        capi.device_blocks(fake_cuda((6, 3), torch.float32))
    with pytest.raises(TypeError, match="float64"):
        capi.device_blocks([t, fake_cuda((6, 3), torch.int64)])
    with pytest.raises(ValueError, match="mixes"):
        capi.device_blocks([t, np.zeros((6, 3))])
    with pytest.raises(ValueError, match="mixes"):
        capi.device_blocks([torch.zeros((6, 3), dtype=torch.float64), t])
    with pytest.raises(ValueError, match="2-D"):
        capi.device_blocks(fake_cuda((6,), torch.float64))
    with pytest.raises(ValueError, match="inconsistent"):
        capi.device_blocks([t, fake_cuda((6, 4), torch.float64)])


def test_new_entry_points_are_declared(lib):
    names = capi.declared_symbols()
    for n in NEW_SYMBOLS:
        assert n in names and hasattr(lib, n)
