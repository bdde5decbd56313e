"""Keyword paths of the binding's shared tails that no other GPU test takes, on the file set of test_binding_layouts.py
(mini.jpg, its first 100 bytes, Mouse480.jpg): a mixed scaled RGB batch whose layout and buffer are made by the call itself, on
the host and on the device, against the per-file call; and the capacity a caller offers to the restart and optimised GPU
Huffman coder wrappers.  Every comparison is exact equality."""
import numpy as np
import pytest

from conftest import golden_bytes

pytestmark = pytest.mark.gpu

HVC_E_TRUNCATED = -8


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd
    return video_coding_amd


@pytest.fixture()
def ctx(hvc):
    c = hvc.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files():
    mini = golden_bytes("mini.jpg")
    return [mini, mini[:100], golden_bytes("Mouse480.jpg")]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("layout,row_align", [("interleaved", 0), ("planar", 64)])
def test_scaled_rgb_batch_makes_its_own_layout_and_buffer(ctx, files, layout, row_align, device):
    results = ctx.jpeg_decode_batch_mixed_scaled_rgb(files, 2, threads=2, device=device, layout=layout, row_align=row_align)
    assert len(results) == 3
    assert results[1] == (HVC_E_TRUNCATED, None, None)
    for f in (0, 2):
        status, info, image = results[f]
        want_info, want = ctx.jpeg_decode_scaled_rgb(files[f], 2, layout)
        assert status == 0 and (info.width, info.height) == (want_info.width, want_info.height)
        assert hasattr(image, "cpu") == device
        image = image.cpu().numpy() if device else image
        assert image.shape == want.shape and np.array_equal(image, want), f


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_offered_capacity_reaches_the_restart_and_optimised_coders(ctx, hvc, device):
    import torch
    info, rec = hvc.hvc.jpeg_entropy_decode(golden_bytes("mini.jpg"))
    arg = torch.from_numpy(rec).cuda() if device else rec
    n = info.coef_count
    plain, plain_specs = ctx.huffman_encode_frames_optimised(info, arg, n, 1)
    cut, cut_specs = ctx.huffman_encode_frames_optimised(info, arg, n, 1, restart_interval=2)
    marked = ctx.huffman_encode_frames(info, arg, n, 1, restart_interval=2)
    # a capacity of the caller's that holds the segment: the same bytes
    assert ctx.huffman_encode_frames_optimised(info, arg, n, 1, out_cap=len(plain[0])) == (plain, plain_specs)
    assert ctx.huffman_encode_frames_optimised(info, arg, n, 1, out_cap=len(cut[0]), restart_interval=2) == (cut, cut_specs)
    assert ctx.huffman_encode_frames(info, arg, n, 1, out_cap=len(marked[0]), restart_interval=2) == marked
    # and one byte less is refused: the capacity offered is the capacity passed on
    for call in (lambda: ctx.huffman_encode_frames_optimised(info, arg, n, 1, out_cap=len(plain[0]) - 1),
                 lambda: ctx.huffman_encode_frames_optimised(info, arg, n, 1, out_cap=len(cut[0]) - 1, restart_interval=2),
                 lambda: ctx.huffman_encode_frames(info, arg, n, 1, out_cap=len(marked[0]) - 1, restart_interval=2)):
        with pytest.raises(hvc.HvcError):
            call()
