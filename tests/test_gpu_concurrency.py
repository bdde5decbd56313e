"""Several contexts at once, as on a multi-GPU node with one host thread (or process) per GPU: two contexts run
their BATCH pipelines concurrently -- host worker threads, pinned rings, copy / reader / block-stage streams each --
and the host threads stay on the CPUs hvc_set_host_cpus gives them."""
import glob
import os
import threading
import time

import numpy as np
import pytest

from batch_files import frames as _frames, mixed_files as _mixed_files, uniform_files as _uniform_files
from conftest import golden_bytes
from oracle import orc
from test_host_entropy import UNUSUAL_SAMPLINGS, unusual_sampling_file

pytestmark = pytest.mark.gpu


def test_two_contexts_run_their_batch_pipelines_concurrently():
    """context A decodes a batch of files (GPU Huffman reader, then the host-reader pipeline), context B encodes raw
    frames to files (GPU coder, then host coder) at the same time, several rounds; every result against the model"""
    import video_coding_amd as hvc
    w, h, n = 640, 352, 24
    frames_a, frames_b = _frames(n, w, h, 5000), _frames(n, w, h, 7000)
    jpegs_a = [orc.encode_yuv(y, u, v, w, h, 420, 75) for y, u, v in frames_a]
    want_b = [orc.encode_yuv(y, u, v, w, h, 420, 60) for y, u, v in frames_b]
    want_a = []
    for j in jpegs_a:
        d = orc.Decoder(j)
        d.decode()
        want_a.append(np.concatenate([d.plane(i).reshape(-1) for i in range(3)]))
    raw_b = [np.concatenate([p.reshape(-1) for p in f]) for f in frames_b]
    a, b = hvc.Context(0), hvc.Context(0)
    info = hvc.hvc.jpeg_read_header(jpegs_a[0])
    fs = info.pixel_bytes
    errors = []

    def run_a():
        try:
            for rep in range(4):
                out = np.zeros(n * fs, np.uint8)
                a.jpeg_decode_batch(jpegs_a, out, fs, threads=4, frames_per_chunk=5, gpu_entropy=rep % 2 == 0)
                for f in range(n):
                    assert np.array_equal(out[f * fs:(f + 1) * fs], want_a[f]), ("decode", rep, f)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    def run_b():
        try:
            for rep in range(4):
                got, _ = b.jpeg_encode_batch(raw_b, w, h, 420, 60, threads=4, frames_per_chunk=5, gpu_entropy=rep % 2 == 0)
                assert got == want_b, ("encode", rep)
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    ta, tb = threading.Thread(target=run_a), threading.Thread(target=run_b)
    ta.start()
    tb.start()
    ta.join()
    tb.join()
    a.close()
    b.close()
    assert not errors, errors


def _thread_cpu_lists():
    out = []
    for p in glob.glob("/proc/self/task/*/status"):
        try:
            with open(p) as f:
                for line in f:
                    if line.startswith("Cpus_allowed_list:"):
                        out.append(line.split(":")[1].strip())
        except OSError:
            pass
    return out


def test_host_threads_stay_on_the_cpus_they_are_given():
    import video_coding_amd as hvc
    allowed = sorted(os.sched_getaffinity(0))
    if len(allowed) < 3:
        pytest.skip("needs three CPUs to tell a restricted thread from an unrestricted one")
    c = hvc.Context(0)
    try:
        assert c.get_host_cpus() == ("", 0) or os.environ.get("HVC_HOST_CPUS")
        for bad in ("3-1", "abc", "1,,2", "-4", "999999"):
            with pytest.raises(hvc.HvcError) as e:
                c.set_host_cpus(bad)
            assert e.value.code == -1
        pair = "%d,%d" % (allowed[0], allowed[1])
        c.set_host_cpus(pair)
        assert c.get_host_cpus() == (pair, 2)
        # a batch long enough to look at its threads while it runs
        w, h, n = 640, 352, 96
        j = [orc.encode_yuv(*f, w, h, 420, 75) for f in _frames(4, w, h, 9000)]
        jpegs = [j[i % 4] for i in range(n)]
        info = hvc.hvc.jpeg_read_header(jpegs[0])
        fs = info.pixel_bytes
        out = np.zeros(n * fs, np.uint8)
        seen, stop = set(), threading.Event()

        def watch():
            while not stop.is_set():
                seen.update(_thread_cpu_lists())
                time.sleep(0.0005)

        t = threading.Thread(target=watch)
        t.start()
        for gpu in (False, True, False):
            c.jpeg_decode_batch(jpegs, out, fs, threads=6, frames_per_chunk=8, gpu_entropy=gpu)
        stop.set()
        t.join()
        want_list = pair if allowed[1] != allowed[0] + 1 else "%d-%d" % (allowed[0], allowed[1])
        assert want_list in seen, seen  # worker threads restricted to the pair were observed
        d = orc.Decoder(jpegs[0])
        d.decode()
        assert np.array_equal(out[:fs], np.concatenate([d.plane(i).reshape(-1) for i in range(3)]))
        # "auto": the CPUs of the GPU's NUMA node (when sysfs shows them in this container)
        try:
            c.set_host_cpus("auto")
            lst, k = c.get_host_cpus()
            assert k >= 1 and lst
        except hvc.HvcError as e:
            assert e.code == -1
        c.set_host_cpus(None)
        assert c.get_host_cpus() == ("", 0)
    finally:
        c.close()


def test_batch_calls_reuse_the_contexts_threads():
    """The workers live in the context (csrc/hvc_pool.h): a loop of small batch calls starts them once.  Every kind of
    batch call, host and device side of the pool (the downloader of host output is one more thread)."""
    import video_coding_amd as hvc
    w, h, n = 320, 176, 12
    frames = _frames(n, w, h, 11000)
    jpegs = [orc.encode_yuv(y, u, v, w, h, 420, 75) for y, u, v in frames]
    raw = [np.concatenate([p.reshape(-1) for p in f]) for f in frames]
    want = []
    for j in jpegs:
        d = orc.Decoder(j)
        d.decode()
        want.append(np.concatenate([d.plane(i).reshape(-1) for i in range(3)]))
    c = hvc.Context(0)
    try:
        assert c.host_threads() == (0, 0)  # nothing until a batch call needs them
        fs = hvc.hvc.jpeg_read_header(jpegs[0]).pixel_bytes
        for rep in range(6):
            out = np.zeros(n * fs, np.uint8)
            c.jpeg_decode_batch(jpegs, out, fs, threads=5, frames_per_chunk=4, gpu_entropy=rep % 2 == 1)
            for f in range(n):
                assert np.array_equal(out[f * fs:(f + 1) * fs], want[f]), (rep, f)
            got, _ = c.jpeg_encode_batch(raw, w, h, 420, 75, threads=3, frames_per_chunk=4, gpu_entropy=rep % 2 == 0)
            assert got == jpegs, rep
        alive, ever = c.host_threads()
        assert alive == ever == 6, (alive, ever)  # 5 workers + the host-output downloader, started once in 12 calls
        c.jpeg_decode_batch(jpegs, out, fs, threads=9, frames_per_chunk=4, gpu_entropy=True)  # a wider call adds threads
        assert c.host_threads() == (10, 10)
        c.jpeg_decode_batch(jpegs, out, fs, threads=2, frames_per_chunk=4, gpu_entropy=False)  # a narrower one none
        assert c.host_threads() == (10, 10)
    finally:
        c.close()


def test_a_refused_host_thread_fails_the_call_not_the_process():
    """EAGAIN from thread creation (a pids limit: 8 ranks x 16 workers per node) inside a real batch call, with some
    workers already running: HVC_E_SYSTEM, and the same context then serves a call that fits the threads it has."""
    import subprocess
    import sys
    code = r'''
import sys
sys.path.insert(0, "tests")
import numpy as np
from helpers import synth_pixels
from oracle import orc
import video_coding_amd as hvc
w, h, n = 320, 176, 8
fr = [(synth_pixels(1 + f, h, w), synth_pixels(50 + f, h // 2, w // 2), synth_pixels(90 + f, h // 2, w // 2)) for f in range(n)]
jpegs = [orc.encode_yuv(y, u, v, w, h, 420, 75) for y, u, v in fr]
raw = [np.concatenate([p.reshape(-1) for p in f]) for f in fr]
c = hvc.Context(0)
fs = hvc.hvc.jpeg_read_header(jpegs[0]).pixel_bytes
out = np.zeros(n * fs, np.uint8)
for gpu in (False, True):
    try:
        c.jpeg_decode_batch(jpegs, out, fs, threads=8, frames_per_chunk=3, gpu_entropy=gpu)
        raise SystemExit("the call should have failed")
    except hvc.HvcError as e:
        assert e.code == -10, e
try:
    c.jpeg_encode_batch(raw, w, h, 420, 75, threads=8, frames_per_chunk=3)
    raise SystemExit("the call should have failed")
except hvc.HvcError as e:
    assert e.code == -10, e
assert c.host_threads() == (3, 3)          # the three that did start stay in the pool
c.jpeg_decode_batch(jpegs, out, fs, threads=2, frames_per_chunk=3, gpu_entropy=True)   # 2 workers + the downloader
d = orc.Decoder(jpegs[5]); d.decode()
assert np.array_equal(out[5 * fs:6 * fs], np.concatenate([d.plane(i).reshape(-1) for i in range(3)]))
got, _ = c.jpeg_encode_batch(raw, w, h, 420, 75, threads=3, frames_per_chunk=3, gpu_entropy=True)
assert got == jpegs
c.close()
print("refusal ok")
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HVC_POOL_FAIL_AFTER="3")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "refusal ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_every_context_entry_point_refuses_null_buffers():
    """The same sweep as tests/test_abi_symbols.py with a live context in front: every function that takes the context
    called with it and otherwise nothing but zeros and null pointers -- a status comes back (never a positive one), the
    process is still there, and the context then decodes a file like before.  In a child process."""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "hvc_jpeg.h")).read(), flags=re.S)
    protos = re.findall(r"HVC_API\s+int\s+(hvc_\w+)\s*\(\s*(?:const\s+)?hvc_ctx\s*\*\s*\w+\s*((?:,[^;]*?)?)\)\s*;", hdr, flags=re.S)
    calls = [(name, len(re.split(r",(?![^()]*\))", rest)) - 1 if rest.strip() else 0) for name, rest in protos]
    assert len(calls) >= 30
    code = "\n".join([
        "import ctypes as C, sys, numpy as np",
        "sys.path.insert(0, %r); sys.path.insert(0, %r)" % (root, os.path.join(root, "tests")),
        "import video_coding_amd as hvc",
        "from oracle import orc",
        "ctx = hvc.Context(0); L = hvc.lib()",
        "for name, n in %r:" % (calls,),
        "    f = getattr(L, name); f.restype = C.c_int; f.argtypes = [C.c_void_p] * (n + 1)",
        "    print(name, f(ctx._h, *([None] * n)), flush=True)",
        "data = open(%r, 'rb').read()" % os.path.join(root, "tests", "golden", "Mouse480.jpg"),
        "info, pixels = ctx.jpeg_decode(data)",
        "d = orc.Decoder(data); d.decode()",
        "assert all(np.array_equal(p, d.plane(i)) for i, p in enumerate(info.planes(pixels)))",
        "print('SWEPT')"])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    seen = dict(line.split() for line in r.stdout.splitlines() if line.startswith("hvc_"))
    assert r.returncode == 0 and "SWEPT" in r.stdout, "failed behind %s\n%s" % (list(seen)[-1:] or "the start", r.stderr[-3000:])
    assert set(seen) == {name for name, _ in calls}
    assert all(int(s) <= 0 for s in seen.values()), seen
    # what has something to refuse refuses it
    for name in ("hvc_decode_frames", "hvc_encode_frames", "hvc_jpeg_decode", "hvc_jpeg_decode_batch", "hvc_jpeg_decode_batch_gpu",
                 "hvc_jpeg_encode_batch", "hvc_huffman_encode_frames", "hvc_checksum_records"):  # (a copy of zero bytes is one)
        assert int(seen[name]) < 0, (name, seen[name])


# ---------------------------------------------------------------------------
# the pipelines' shared parts (csrc/hvc_feed.h, hvc_batch.h, the ring helper of hvc_ctx.h) through every pipeline of one context

def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else a


def _decode_uniform(c, jpegs, fs, device, **kw):
    if device:
        import torch
        out = torch.zeros(len(jpegs) * fs, dtype=torch.uint8, device="cuda")
    else:
        out = np.zeros(len(jpegs) * fs, np.uint8)
    st = c.jpeg_decode_batch(jpegs, out, fs, **kw)
    return _host(out).reshape(len(jpegs), fs), st


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_one_context_runs_every_pipeline_while_its_rings_regrow(device):
    """uniform batch (4 chunks over 3 slots, the last ragged), the same in one chunk (the coefficient ring grows), a mixed
    batch whose first file alone exceeds chunk_bytes (the ring grows inside the mixed path), its RGB form (the plane ring
    appears), the GPU-reader batch, both encode pipelines, the first call again: byte for byte what the single-file entry
    points give"""
    import video_coding_amd as hvc
    jpegs, frames = _uniform_files(7, 21000)
    mixed = _mixed_files()
    ref = hvc.Context(0)
    try:
        want = np.stack([ref.jpeg_decode(j)[1] for j in jpegs])
        want_mixed = [ref.jpeg_decode(f) for f in mixed]
        want_rgb = [ref.jpeg_decode_rgb(f)[1] for f in mixed[:2]]
        want_files = [ref.jpeg_encode(y, u, v, 64, 64, 420, 75) for y, u, v in frames[:5]]
    finally:
        ref.close()
    assert want_files == jpegs[:5]
    raw = [np.concatenate([p.reshape(-1) for p in f]) for f in frames[:5]]
    fs = want.shape[1]
    mouse_record = 2 * hvc.hvc.jpeg_read_header(mixed[0]).coef_count
    assert mouse_record > 7 * 2 * hvc.hvc.jpeg_read_header(jpegs[0]).coef_count   # larger than the ring the uniform calls leave
    c = hvc.Context(0)
    try:
        got, st = _decode_uniform(c, jpegs, fs, device, threads=3, frames_per_chunk=2)
        assert st.chunks == 4 and np.array_equal(got, want)
        got, st = _decode_uniform(c, jpegs, fs, device, threads=3, frames_per_chunk=7)
        assert st.chunks == 1 and np.array_equal(got, want)
        results = c.jpeg_decode_batch_mixed(mixed, threads=3, chunk_bytes=mouse_record - 2, device=device)
        assert c.last_batch_stats.chunks >= 2
        for (status, info, planes), (winfo, wpx) in zip(results, want_mixed):
            assert status == 0
            for a, b in zip(planes, winfo.planes(wpx)):
                assert np.array_equal(_host(a), b)
        results = c.jpeg_decode_batch_mixed_rgb(mixed, threads=3, chunk_bytes=mouse_record - 2, device=device)
        for f, wimg in enumerate(want_rgb):
            assert results[f][0] == 0 and np.array_equal(_host(results[f][2]), wimg), f
        got, st = _decode_uniform(c, jpegs, fs, device, threads=3, frames_per_chunk=2, gpu_entropy=True)
        assert st.chunks == 4 and np.array_equal(got, want)
        for gpu in (False, True):
            files, st = c.jpeg_encode_batch(raw, 64, 64, 420, 75, threads=3, frames_per_chunk=2, gpu_entropy=gpu)
            assert files == want_files and st.chunks == 3, gpu
        got, st = _decode_uniform(c, jpegs, fs, device, threads=3, frames_per_chunk=2)
        assert st.chunks == 4 and np.array_equal(got, want)
    finally:
        c.close()


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("bad_at", [6, 1], ids=["chunk3", "chunk0"])
def test_an_error_late_in_a_uniform_batch(threads, bad_at):
    """8 files in chunks of 2, one cut inside its headers (chunk 3: a slot that has come round, or chunk 0): the call returns
    that file's code, and the next call on the same context is byte-exact"""
    import video_coding_amd as hvc
    jpegs, _ = _uniform_files(8, 23000)
    bad = list(jpegs)
    bad[bad_at] = jpegs[bad_at][:100]
    with pytest.raises(hvc.HvcError) as e:
        hvc.hvc.jpeg_read_header(bad[bad_at])
    code = e.value.code
    assert code < 0
    c = hvc.Context(0)
    try:
        want = np.stack([c.jpeg_decode(j)[1] for j in jpegs])
        fs = want.shape[1]
        with pytest.raises(hvc.HvcError) as e:
            _decode_uniform(c, bad, fs, False, threads=threads, frames_per_chunk=2)
        assert e.value.code == code
        got, st = _decode_uniform(c, jpegs, fs, False, threads=threads, frames_per_chunk=2)
        assert st.chunks == 4 and np.array_equal(got, want)
    finally:
        c.close()


def test_batch_stats_are_still_filled():
    import video_coding_amd as hvc
    jpegs, _ = _uniform_files(7, 25000)
    mini, mouse = golden_bytes("mini.jpg"), golden_bytes("Mouse480.jpg")
    info = hvc.hvc.jpeg_read_header(mouse)
    # cut in its scan and followed by one-bits, which no Huffman table has a code for: the host reader fails inside the scan
    cut = mouse[:info.ecs_offset + 2000] + b"\xff\x00" * 64 + b"\xff\xd9"
    small = unusual_sampling_file(UNUSUAL_SAMPLINGS[3], 40, 24, 340)[0]
    files = [mini, cut, mini, small, small]
    coef = [2 * hvc.hvc.jpeg_read_header(f).coef_count for f in files]
    chunk = coef[0]                                       # chunks: [mini] [cut: alone, no good file] [mini] [small small]
    assert coef[1] > chunk and coef[3] + coef[4] <= chunk < coef[2] + coef[3]
    c = hvc.Context(0)
    try:
        fs = hvc.hvc.jpeg_read_header(jpegs[0]).pixel_bytes
        _, st = _decode_uniform(c, jpegs, fs, False, threads=3, frames_per_chunk=2)
        assert (st.chunks, st.threads, st.frames_per_chunk) == (4, 3, 2)
        assert st.coef_bytes == 7 * 2 * hvc.hvc.jpeg_read_header(jpegs[0]).coef_count and st.wall_ms > 0
        results = c.jpeg_decode_batch_mixed(files, threads=2, chunk_bytes=chunk)
        assert [r[0] == 0 for r in results] == [True, False, True, True, True]
        st = c.last_batch_stats
        assert (st.chunks, st.threads, st.frames_per_chunk) == (4, 2, 2)
        assert st.coef_bytes == sum(coef) - coef[1] and st.wall_ms > 0   # the chunk without a good file was not uploaded
    finally:
        c.close()
