"""hvc_normalize_lut (include/hvc_jpeg.h, Typed output; csrc/hvc_normalize_lut.cpp): the table
((float)v / 255.0f - mean[c]) / std[c] in IEEE single, rounded once to the element type, bit-equal to torch on the CPU --
((v.float() / 255) - mean) / std, then .to(dtype) -- for float32, float16 and bfloat16.  Host only: no GPU, no context."""
import ctypes as C

import numpy as np
import pytest

IMAGENET = ((0.485, 0.456, 0.406), (0.229, 0.224, 0.225))
CONSTANTS = {
    "imagenet": IMAGENET,
    "plain": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
    "negative-mean": ((-0.3, 0.5, 1.25), (0.5, 2.0, 0.1)),
    # beyond the ordinary: results that overflow float16 to infinity, and results in float16's subnormal range
    "tiny-std": ((0.0, 0.5, 0.0), (1e-6, 1e-5, 3e-7)),
    "huge-std": ((0.0, 0.25, 0.0), (1e6, 3e7, 65000.0)),
}


def torch_table(mean, std, dtype):
    import torch
    v = torch.arange(256, dtype=torch.uint8)[None, :].expand(3, 256)
    m = torch.tensor(mean, dtype=torch.float32)[:, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None]
    t = (((v.float() / 255) - m) / s).to(dtype)
    return t.view({4: torch.int32, 2: torch.int16}[t.element_size()]).numpy()


@pytest.mark.parametrize("name", list(CONSTANTS))
@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_bit_equal_to_torch(name, dtype):
    import torch
    import video_coding_amd as hvc
    mean, std = CONSTANTS[name]
    want = torch_table(mean, std, getattr(torch, dtype))
    got = hvc.normalize_lut(mean, std, dtype)
    assert got.shape == (3, 256) and got.dtype.itemsize == want.dtype.itemsize
    assert np.array_equal(got.view(want.dtype), want)
    assert np.array_equal(hvc.normalize_lut(mean, std, getattr(torch, dtype)).view(want.dtype), want)   # a torch dtype names it too


def test_the_numpy_form_is_the_same_table():
    import os
    import sys
    import video_coding_amd as hvc
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import resize_reference as rr
    for mean, std in (IMAGENET, CONSTANTS["negative-mean"]):
        assert np.array_equal(rr.normalize_lut(mean, std, np.float32).view(np.uint32), hvc.normalize_lut(mean, std, "float32").view(np.uint32))
        assert np.array_equal(rr.normalize_lut(mean, std, np.float16).view(np.uint16), hvc.normalize_lut(mean, std, "float16").view(np.uint16))


def test_refusals():
    import video_coding_amd as hvc
    L = hvc.lib()
    out = np.full(3 * 256, 7, dtype=np.float32)
    good = (C.c_float * 3)(0.5, 0.5, 0.5)

    def call(mean, std, elem, lut=out.ctypes.data):
        return L.hvc_normalize_lut(mean, std, elem, lut)

    assert call(good, good, 1) == 0 and out[0] == -1.0 and out[255] == 1.0
    out[:] = 7
    for bad in ((0.5, 0.0, 0.5), (0.5, -0.0, 0.5), (float("nan"), 1, 1), (1, float("inf"), 1), (1, 1, float("-inf"))):
        arr = (C.c_float * 3)(*bad)
        assert call(good, arr, 1) == -1, bad                     # std: zero or non-finite
        if 0.0 not in bad:
            assert call(arr, good, 1) == -1, bad                 # mean: non-finite
    for elem in (0, 4, -1, 16):
        assert call(good, good, elem) == -1                      # an unknown element type
    assert call(None, good, 1) == -1 and call(good, None, 1) == -1 and call(good, good, 1, None) == -1
    assert (out == 7).all()                                      # a refused call writes nothing
    with pytest.raises(hvc.HvcError) as e:
        hvc.normalize_lut((0, 0, 0), (1, 0, 1))
    assert e.value.code == -1
    with pytest.raises(ValueError):
        hvc.normalize_lut(dtype="float64")
