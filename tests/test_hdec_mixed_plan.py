"""The host plan of the mixed GPU Huffman reader (csrc/hvc_hdec_mixed_plan.cpp), without a GPU: the descriptor builder through
the stand-alone program tests/host_harness/hdec_mixed_plan_harness.cpp, which runs it -- and the header parser and segment
preparation in front of it -- under AddressSanitizer and UndefinedBehaviorSanitizer (a CPU-only g++ build:
tests/host_harness/Makefile.hdec_mixed).  Nothing loaded into Python runs under a sanitizer."""
import os
import subprocess

import pytest

from mixed_reader_files import reader_set, segment_bytes, subsequences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS_DIR = os.path.join(ROOT, "tests", "host_harness")
ENV = {**os.environ, "ASAN_OPTIONS": "detect_leaks=0:halt_on_error=1", "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}
TAKEN, NO_COMPONENTS, MCU_BLOCKS, MCU_GRID, TOO_LARGE, TABLES, NO_BLOCKS, PLACE = range(8)   # HdmRefusal


@pytest.fixture(scope="module")
def hvc():
    import video_coding_amd as m
    m.build()
    return m.hvc


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("hdec_mixed") / "hdec_mixed_plan_harness")
    r = subprocess.run(["make", "-s", "-C", HARNESS_DIR, "-f", "Makefile.hdec_mixed", "OUT=" + exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return exe


@pytest.fixture(scope="module")
def paths(tmp_path_factory):
    d = tmp_path_factory.mktemp("hdec_mixed_files")
    out = []
    for k, f in enumerate(reader_set()[0]):
        p = d / ("f%02d.jpg" % k)
        p.write_bytes(f)
        out.append(str(p))
    return out


def run_plan(harness, paths, which="all"):
    r = subprocess.run([harness, "files", which] + paths, capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = dict(segments={}, files=[], map=[], refusal=[], tabsrc=[])
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "segment":
            out["segments"][int(w[1])] = tuple(map(int, w[2:]))     # (status, gpu_ok, bytes)
        elif w[0] in ("status", ):
            out["status"] = int(w[1])
        elif w[0] == "check":
            out["check"] = " ".join(w[1:])
        elif w[0] == "totals":
            out["total_sub"], out["seg_bytes"], out["dcd_entries"], out["n_tables"], out["n_units"] = map(int, w[1:])
        elif w[0] in ("refusal", "tabsrc", "map"):
            out[w[0]] = list(map(int, w[1:]))
        elif w[0] == "file":
            v = list(map(int, w[1:]))
            d = dict(zip(("file", "ecs_off", "sub0", "n_sub", "unit0", "coef_base", "need", "blocks_per_mcu", "mbs_wide", "n_comp", "selmask",
                          "tabrec", "dcd0"), v[:13]))
            d["comp"] = [tuple(v[13 + 5 * c:18 + 5 * c]) for c in range(4)]                # (h, v, bw, mcu_base, coef_off)
            d["b2"] = [tuple(v[33 + 3 * b:36 + 3 * b]) for b in range(16)]                 # (component, sx, sy)
            out["files"].append(d)
    return out


def geometry(info):
    """gd_geometry of csrc/hvc_capi_reader.hip, restated: None where the GPU reader cannot take the frame"""
    if not 1 <= info.n_comp <= 3:
        return None
    c0 = info.comp[0]
    mbs_wide, mbs_high = c0.decoded_width // (8 * c0.hscale), c0.decoded_height // (8 * c0.vscale)
    comp, b2, base = [], [], 0
    for i in range(info.n_comp):
        h, v, L = info.comp[i].hscale, info.comp[i].vscale, info.layout[i]
        if mbs_wide * h > L.blocks_w or mbs_high * v > L.blocks_h or base + h * v > 16:
            return None
        comp.append((h, v, L.blocks_w, base, L.coef_offset))
        b2 += [(i, r % h, r // h) for r in range(h * v)]
        base += h * v
    return dict(need=mbs_wide * mbs_high * base, blocks_per_mcu=base, mbs_wide=mbs_wide, n_comp=info.n_comp, comp=comp, b2=b2,
                selmask=sum(c << (2 * b) for b, (c, _, _) in enumerate(b2)))


def test_descriptors_match_the_uniform_readers_geometry(hvc, harness, paths):
    files, names, ineligible = reader_set()
    plan = run_plan(harness, paths)
    assert plan["status"] == 0 and plan["check"] == "ok"
    infos = [hvc.jpeg_read_header(f) for f in files]
    want_refusal = [TAKEN] * len(files)
    for i in ineligible:
        want_refusal[i] = NO_COMPONENTS if infos[i].n_comp > 3 else MCU_BLOCKS
    assert plan["refusal"] == want_refusal
    assert [d["file"] for d in plan["files"]] == [i for i in range(len(files)) if i not in ineligible]
    sub = unit = dcd = 0
    for d in plan["files"]:
        f = d["file"]
        g = geometry(infos[f])
        assert g is not None, names[f]
        for key in ("need", "blocks_per_mcu", "mbs_wide", "n_comp", "selmask"):
            assert d[key] == g[key], (names[f], key)
        assert d["comp"][:g["n_comp"]] == g["comp"] and d["b2"][:g["blocks_per_mcu"]] == g["b2"], names[f]
        # the segment: what the file holds between its SOS header and the marker behind the scan, unstuffed
        assert plan["segments"][f] == (0, 1, segment_bytes(files[f])), names[f]
        assert d["n_sub"] == subsequences(files[f]) and d["ecs_off"] % 128 == 0
        assert (d["sub0"], d["unit0"], d["dcd0"]) == (sub, unit, dcd), names[f]
        sub, unit, dcd = sub + d["n_sub"], unit + -(-d["n_sub"] // 64), dcd + d["need"]
    assert (plan["total_sub"], plan["n_units"], plan["dcd_entries"]) == (sub, unit, dcd)
    by_name = {names[d["file"]]: d for d in plan["files"]}
    assert by_name["grey-8x8"]["n_sub"] == 2 and by_name["grey-8x8"]["need"] == 1
    assert [by_name[n]["n_sub"] for n in ("subs64", "subs65")] == [64, 65]
    assert by_name["subs-over-512"]["n_sub"] > 512
    assert {1, 3, 4, 6, 8, 11} <= {d["blocks_per_mcu"] for d in plan["files"]}


def test_the_unit_map_follows_the_subsequence_counts(harness, paths):
    plan = run_plan(harness, paths)
    want = []
    for k, d in enumerate(plan["files"]):
        assert d["unit0"] == len(want)
        want += [k] * (-(-d["n_sub"] // 64))
    assert plan["map"] == want
    assert sorted({-(-d["n_sub"] // 64) for d in plan["files"]}) == [1, 2, 10]   # 64 subsequences: one unit; 65: two; 622: ten


def test_table_records_are_shared_by_content(hvc, harness, paths):
    files, names, ineligible = reader_set()
    # the same file three times among others: one record; the two optimised files of one geometry: one record each
    pick = [names.index("optimised-seed1"), names.index("mini"), names.index("optimised-seed2"), names.index("optimised-seed1"),
            names.index("mouse480"), names.index("optimised-seed1")]
    plan = run_plan(harness, [paths[i] for i in pick])
    assert plan["status"] == 0 and plan["check"] == "ok"
    recs = [d["tabrec"] for d in plan["files"]]
    assert recs[0] == recs[3] == recs[5] and recs[0] != recs[2] and len(set(recs)) == plan["n_tables"]
    # mini.jpg and Mouse480.jpg carry the model's default tables in different DHT layouts or not: whatever they are, equal content = one record
    assert plan["n_tables"] == len({plan["tabsrc"][r] for r in recs})
    assert all(plan["files"][k]["tabrec"] <= k for k in range(len(pick)))   # a record is named by the first file that has it


def test_a_list_leaves_the_others_out_and_an_empty_list_gives_an_empty_plan(harness, paths):
    _, names, ineligible = reader_set()
    plan = run_plan(harness, paths, "3,0,%d,2" % ineligible[0])
    assert plan["status"] == 0 and plan["check"] == "ok"
    assert [d["file"] for d in plan["files"]] == [3, 0, 2] and plan["refusal"] == [TAKEN, TAKEN, MCU_BLOCKS, TAKEN]
    assert plan["files"][0]["sub0"] == 0 and plan["files"][1]["sub0"] == plan["files"][0]["n_sub"]
    none = run_plan(harness, paths, "none")
    assert none["status"] == 0 and none["check"] == "ok" and none["files"] == [] and none["map"] == [] and none["refusal"] == []
    assert (none["total_sub"], none["seg_bytes"], none["dcd_entries"], none["n_tables"]) == (0, 0, 0, 0)
    bad = run_plan(harness, paths[:2], "0,2")                  # a list entry outside the set
    assert bad["status"] == -1


def test_seeded_random_sets_in_the_sanitizer_build(harness):
    """synthetic geometries: every refusal but the size limits (components, blocks per MCU, MCU grid, no block, tables, place;
    the limits: test_sizes_beyond_the_32_bit_indices_are_refused) is reported as expected, every plan keeps its invariants"""
    r = subprocess.run([harness, "random", "20261019", "600"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    w = r.stdout.split()
    assert w[:2] == ["ok", "600"] and int(w[3]) > 500 and int(w[5]) > 500


def test_sizes_beyond_the_32_bit_indices_are_refused(harness):
    """HDM_TOO_LARGE from both sides of every limit: per file (coef_count and a plane's coef_offset at 2^32, the frame's
    blocks at 2^31, the segment's bytes at 2^28, the end of its room at 2^32) and per chunk (the file that takes the
    subsequences to 2^31 or the DC rows to 2^32 is refused, the small file behind it is taken); the files around the refused
    one stay in a plan that keeps its invariants."""
    r = subprocess.run([harness, "limits"], capture_output=True, text=True, env=ENV)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    cases = {}
    for ln in r.stdout.splitlines():
        w = ln.split()
        if w[0] == "case":
            at = w.index("check")
            assert w[at + 1:] == ["ok"], ln
            cases[w[1]] = " ".join(w[2:at])
    taken, refused = "0 0 0", "0 %d 0" % TOO_LARGE
    assert cases == {
        "coef_count_below": taken, "coef_count_2^32": refused,
        "coef_offset_below": taken, "coef_offset_2^32": refused,
        "blocks_below": "0", "blocks_2^31": refused,
        "seg_bytes_below": taken, "seg_bytes_2^28": refused,
        "room_end_below": taken, "room_end_2^32": refused,
        # 1023 files of 2^21 + 1 subsequences stay below 2^31, the next one does not; the small last file is taken
        "chunk_subsequences": "first 1023 why %d refused 1 last 0" % TOO_LARGE,
        # 64 files of 8191 x 8192 blocks stay below 2^32 entries, the 65th does not; the one-block last file is taken
        "chunk_dc_rows": "first 64 why %d refused 1 last 0" % TOO_LARGE,
    }
    assert r.stdout.splitlines()[-1] == "ok"
