"""bench.py --dump-outputs without a GPU: dump_outputs() on a host tensor laid out as bench.py lays out its batch (the GPU runs of
the flag are in tests/test_gpu_checksum_bench.py)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def batch(n, align):
    import torch
    import video_coding_amd as hvc
    planes = [(6, 4, 0), (3, 2, 1), (3, 2, 1)]
    tspecs, _, tpfs = hvc.hvc.frame_layout(planes)
    specs, _, pfs = hvc.hvc.frame_layout(planes, align=align)
    tight = torch.from_numpy(np.random.Generator(np.random.PCG64(n)).integers(0, 256, size=(n, tpfs), dtype=np.uint8))
    return tight, hvc.hvc.spread_records(tight, tspecs, specs, pfs, "plane_offset"), specs


@pytest.mark.parametrize("n", [1, 3, 40])
def test_whole_records_in_float32_whatever_the_layout(tmp_path, n):
    """first, last and two seeded records, gathered tight: the same file from the aligned and the back-to-back layout"""
    got = []
    for align in (1, 4096):
        tight, recs, specs = batch(n, align)
        d = tmp_path / str(align)
        info = bench.dump_outputs(str(d), "pixels", recs, specs, "plane_offset")
        a = np.load(d / "pixels.npy")
        assert a.dtype == np.float32 and info["file"] == "pixels.npy" and info["positions"] == "all %d" % tight.shape[1]
        assert info["records"][0] == 0 and info["records"][-1] == n - 1 and len(info["records"]) == min(n, 4)
        assert np.array_equal(a, tight[info["records"]].numpy().astype(np.float32))
        got.append(a)
    assert np.array_equal(got[0], got[1])


def test_a_larger_output_is_a_fixed_seeded_sample_within_the_budget(tmp_path):
    tight, recs, specs = batch(40, 4096)
    budget = 4096 + 4 * 4 * 500
    files = []
    for k in range(2):
        info = bench.dump_outputs(str(tmp_path / str(k)), "pixels", recs, specs, "plane_offset", budget=budget)
        assert info["positions"] == "500 of %d, seeded" % tight.shape[1]
        assert os.path.getsize(tmp_path / str(k) / "pixels.npy") <= budget
        files.append(np.load(tmp_path / str(k) / "pixels.npy"))
    assert files[0].shape == (4, 500) and np.array_equal(files[0], files[1])
    rows = tight[info["records"]].numpy()
    assert all(np.isin(files[0][i], rows[i]).all() for i in range(4))   # every value is one of the record's own


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False and bench.parse_args(["--full"]).full is True
    assert bench.parse_args(["--config", "3", "--full"]).full is True


def test_steps_sets_the_timed_steps():
    assert bench.parse_args(["--steps", "7"]).steps == 7 and bench.parse_args(["--dump-outputs", "d"]).dump_outputs == "d"
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
