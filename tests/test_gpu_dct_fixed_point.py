"""hvc_dct_fixed / hvc_dct_reference / hvc_dct_error_search on the MI355X, bit for bit against the restatements of
tests/test_dct_fixed_point.py, and the `dct` command line."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_dct_fixed_point import (SEARCH, blocks, fixed_coefs, reference_np, round_trip_errors, transform,  # noqa: E402
                                  worst)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import torch
    import video_coding_amd as hvc
    c = hvc.Context(0)
    c.set_stream(torch.cuda.current_stream().cuda_stream)  # device-memory calls in order with torch's copies
    yield c
    c.reset_stream()
    c.close()


def fixed_inputs(xmax, inverse):
    """random blocks, all +-xmax, the sign pattern of each output's row pair, impulses at both ends of the range"""
    rng = np.random.default_rng(5 + inverse)
    parts = [rng.integers(-xmax, xmax + 1, size=(64, 8, 8)), np.full((1, 8, 8), xmax), np.full((1, 8, 8), -xmax)]
    for p in (1, 8, 12, 16):
        c = fixed_coefs(p).T if inverse else fixed_coefs(p)
        for r in range(8):
            s = np.sign(np.outer(c[r], c[r]))
            s[s == 0] = 1
            parts += [xmax * s[None], -xmax * s[None]]
    for j in range(64):
        for v in (xmax, -xmax):
            b = np.zeros((1, 64), dtype=np.int64)
            b[0, j] = v
            parts.append(b.reshape(1, 8, 8))
    return np.concatenate(parts).astype(np.int32)


@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_fixed_is_the_model_at_every_precision(ctx, direction):
    import torch
    inv = direction == "inverse"
    x = fixed_inputs(32768 if inv else 2048, inv)
    dx = torch.from_numpy(x).cuda()
    dy = torch.empty_like(dx)
    for p in range(17):
        for tp in range(9):
            want = transform(x, p, tp, inverse=inv)
            assert np.array_equal(ctx.dct_fixed(direction, p, tp, x), want), (direction, p, tp)
            ctx.dct_fixed(direction, p, tp, dx, dy)
            assert np.array_equal(dy.cpu().numpy(), want), ("device", direction, p, tp)


def test_fixed_refuses_out_of_range(ctx):
    import torch
    import video_coding_amd as hvc
    x = np.zeros((2, 8, 8), dtype=np.int32)
    x[1, 3, 3] = 2049
    for args in (("forward", 17, 0), ("forward", 12, 9), ("forward", 12, 2)):
        with pytest.raises(hvc.HvcError) as e:
            ctx.dct_fixed(args[0], args[1], args[2], x)
        assert e.value.code == -5
    dx = torch.from_numpy(x).cuda()
    dy = torch.full_like(dx, 7)
    with pytest.raises(hvc.HvcError) as e:
        ctx.dct_fixed("forward", 12, 2, dx, dy)
    assert e.value.code == -5
    y = dy.cpu().numpy()
    assert np.array_equal(y[0], transform(x[0], 12, 2)) and np.all(y[1] == 7)   # the bad block is left unwritten
    x[1, 3, 3] = 32768
    assert np.array_equal(ctx.dct_fixed("inverse", 12, 2, x), transform(x, 12, 2, inverse=True))


@pytest.mark.parametrize("direction", ["forward", "inverse"])
def test_reference_is_the_ordered_float64_product(ctx, direction):
    import torch
    inv = direction == "inverse"
    x = np.concatenate([blocks(9, 2048, 0, 200), fixed_inputs(2048, inv)[:40]]).astype(np.int32)
    want = reference_np(x, inv)
    got = ctx.dct_reference(direction, x)
    assert got.tobytes() == want.tobytes()
    d = torch.empty(x.shape, dtype=torch.float64, device="cuda")
    ctx.dct_reference(direction, torch.from_numpy(x).cuda(), d)
    assert d.cpu().numpy().tobytes() == want.tobytes()


def test_search_is_the_restatement_over_every_default_tuple(ctx):
    n = 300
    x = blocks(0, 128, 0, n)
    e, w = ctx.dct_error_search([("round_trip",) + t for t in SEARCH], 0, 128, 0, n)
    for k, t in enumerate(SEARCH):
        want = worst(round_trip_errors(x, *t))
        assert (e[k], int(w[k])) == (float(want[0]), want[1]), t


@pytest.mark.parametrize("mode", ["forward", "inverse"])
def test_search_float_errors_are_bit_equal(ctx, mode):
    n, rng = 400, 200 if mode == "forward" else 3000
    inv = mode == "inverse"
    x = blocks(2, rng, 10, n)
    ref = reference_np(x, inv)
    cfgs = [(mode, p, tp, p, tp) for p, tp in ((8, 0), (12, 2), (12, 4), (16, 8), (3, 5))]
    e, w = ctx.dct_error_search(cfgs, 2, rng, 10, n)
    for k, (_, p, tp, _, _) in enumerate(cfgs):
        err = np.abs(transform(x, p, tp, inverse=inv).astype(np.float64) - ref).reshape(n, 64).max(axis=1)
        m, i = worst(err)
        assert e[k].tobytes() == np.float64(m).tobytes() and int(w[k]) == 10 + i, (mode, p, tp)


def test_search_mixed_modes_split_and_whole(ctx):
    cfgs = [("round_trip", 9, 1, 10, 0), ("forward", 12, 2, 0, 0), ("inverse", 0, 0, 11, 3),
            ("round_trip", 16, 5, 8, 5)] * 20
    whole = ctx.dct_error_search(cfgs, 4, 128, 100, 5000)
    a = ctx.dct_error_search(cfgs, 4, 128, 100, 1777)
    b = ctx.dct_error_search(cfgs, 4, 128, 1877, 3223)
    for k in range(len(cfgs)):
        first = a[0][k] >= b[0][k]
        assert whole[0][k] == max(a[0][k], b[0][k])
        assert whole[1][k] == (a[1][k] if first else b[1][k])
    x = blocks(4, 128, 100, 5000)
    assert (whole[0][0], int(whole[1][0])) == tuple(float(v) if i == 0 else v + 100 for i, v in
                                                     enumerate(worst(round_trip_errors(x, 9, 1, 10, 0))))


def test_search_ties_go_to_the_smallest_block(ctx):
    # range 1 (inputs in {-1, 0}) and range 128: many blocks share the largest error; the first of them is reported
    for seed, rng, first, n, t in ((1, 1, 12345, 2000, (16, 8, 16, 8)), (0, 128, 500, 3000, (9, 1, 9, 1))):
        errs = round_trip_errors(blocks(seed, rng, first, n), *t)
        assert (errs == errs.max()).sum() > 1
        e, w = ctx.dct_error_search([("round_trip",) + t], seed, rng, first, n)
        assert (e[0], int(w[0])) == (float(errs.max()), first + int(np.argmax(errs == errs.max())))


def test_search_refuses_out_of_range_and_writes_nothing(ctx):
    import video_coding_amd as hvc
    arr = hvc.hvc.dct_configs([("round_trip", 12, 2, 12, 2)])
    for cfg, rng, code in (((("round_trip", 17, 0, 12, 2)), 128, -5), ((("round_trip", 12, 9, 12, 2)), 128, -5),
                           ((("inverse", 0, 0, 12, -1)), 128, -5), ((("forward", 12, 2, 0, 0)), 2049, -5),
                           ((("inverse", 0, 0, 12, 2)), 32769, -5), (((7, 12, 2, 12, 2)), 128, -1)):
        cfgs = hvc.hvc.dct_configs([("round_trip", 12, 2, 12, 2), cfg])
        res = (hvc.hvc.DctError * 2)()
        for r in res:
            r.max_error, r.worst_block = -1.0, 77
        rc = hvc.lib().hvc_dct_error_search(ctx._h, cfgs, 2, 0, rng, 0, 100, res)
        assert rc == code, cfg
        assert all(r.max_error == -1.0 and r.worst_block == 77 for r in res)
    assert len(arr) == 1


def run_cli(*args):
    r = subprocess.run([sys.executable, "-m", "video_coding_amd", "dct"] + list(args), cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_cli_search_lines():
    out = run_cli("search", "-count", "200").splitlines()
    assert len(out) == 2916
    x = blocks(0, 128, 0, 200)
    for line, t in zip(out, SEARCH):
        assert line == "%2i %2i %2i %2i - %i" % (t + (int(round_trip_errors(x, *t).max()),)), line


def test_cli_both_worst_block_reproduces():
    out = run_cli("both", "-count", "1000", "-seed", "7").strip()
    m, i = worst(round_trip_errors(blocks(7, 128, 0, 1000), 12, 2, 12, 2))
    assert out == "((max_error %d) (worst_block %d) (seed 7))" % (m, i)
    out = run_cli("both", "-seed", "7", "-block", str(i))
    assert "(max_fixed_error %d)" % m in out
    assert "(inputs ((%s)" % " ".join(str(v) for v in blocks(7, 128, i, 1)[0, 0]) in out
