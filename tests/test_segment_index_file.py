"""The segment index's life cycle, CPU half (no GPU needed):

* the Python model tests/segment_index_file.py against the hand vectors of
  include/rpgpu.h (blob bytes, CRC, XXH64, lookups), its XXH64 against the xxhash
  module, its track against the untouched oracle on the cases of
  tests/test_segment_index.py and on random segments, and the split property: tracking [0, k) then
  [k, 12) equals tracking all 12;
* every hydrate outcome once, by name, against a table traced in the reference;
* the shared core redpanda_amd/csrc/rpgpu_segidx.h compiled for the host
  (tests/native/segidx_host.cpp) against the model over the sweep: written blobs
  byte for byte, hydrate rows and states, find rows, track; once more under
  ASan + UBSan, stand-alone, every file and slot in a heap block of exactly its size;
* struct sizes, offsets and enum values of include/rpgpu.h against redpanda_amd/abi.py;
* the compiler's resource remarks for the kernels: no scratch, no spills.
The device half is tests/test_gpu_segment_index_file.py."""
import functools
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import segment_index_file as sx  # noqa: E402
from kafka_batches import DISK, arena, batch, record  # noqa: E402
from redpanda_amd import abi  # noqa: E402

import oracle.oracle as orc  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "redpanda_amd" / "csrc"
PLAIN = ["-O2"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
STEP = 4096 * 8


# ------------------------------------------------------------- hand vectors
def test_hand_vectors():
    st = sx.hand_state()
    blob = sx.to_blob(st)
    assert blob == sx.HAND_BLOB and len(blob) == 113 == 65 + 16 * 3
    assert sx.crc32c(blob[10:-4]) == 0x0A040BB7 == int.from_bytes(blob[-4:], "little")
    assert sx.crc32c_fast(blob[10:-4]) == 0x0A040BB7
    assert sx.crc32c(b"123456789") == 0xE3069283  # the CRC-32C check value
    v3 = sx.to_v3(sx.hand_state(with_offset=False))
    assert v3 == sx.HAND_V3 and len(v3) == 101
    assert sx.xxh64(v3[13:]) == 0xFD40FABF14E63B1D == int.from_bytes(v3[5:13], "little")
    h = sx.hydrate(blob)
    assert h.row() == (sx.OK, sx.R_NONE, 5, 3) and h.state.key() == st.key()
    h3 = sx.hydrate(v3)
    assert h3.row() == (sx.OK, sx.R_NONE, 3, 3)
    assert (h3.state.monotonic, h3.state.with_offset, h3.state.non_data_timestamps) == (False, False, False)
    assert h3.state.rel_time == [0, 3, 6] and h3.state.position == st.position
    for kind, key, answer in sx.HAND_LOOKUPS:
        assert sx.find(st, kind, key) == answer, (kind, key)


def test_xxh64_digests_and_module():
    for data, digest in sx.XXH_VECTORS:
        assert sx.xxh64(data) == digest
    xxhash = pytest.importorskip("xxhash")
    rng = np.random.default_rng(3)
    for n in range(201):
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        assert sx.xxh64(data) == xxhash.xxh64(data).intdigest(), n


# --------------------------------------------------- track against the oracle
def disk_batch(base_offset, nrec=16, vlen=995, first_ts=1_700_000_000_000, max_ts=None, btype=1, crc=None):
    recs = [record(b"k" * 16, b"v" * vlen, ts_delta=j, off_delta=j) for j in range(nrec)]
    return batch(recs, fmt=DISK, base_offset=base_offset, first_ts=first_ts, max_ts=max_ts, btype=btype, crc=crc)


def segment(batches, base_offset=0, internal=False, with_offset=False, step=STEP):
    data, descs = arena(batches, fmt=DISK, ops=3)
    res, _, _ = orc.validate_arena(data, descs)
    segs = np.zeros(1, dtype=orc.SEGMENT_DTYPE)
    segs[0] = (0, len(batches), base_offset, 0, step, int(internal), int(with_offset), 0)
    return data, descs, res, segs


def oracle_cases():
    """The segments of tests/test_segment_index.py."""
    return {
        "entry_every_third_batch": segment([disk_batch(16 * i) for i in range(10)]),
        "config_batch_first": segment([disk_batch(0, nrec=1, vlen=10, first_ts=5_000, max_ts=5_000, btype=2),
                                       disk_batch(1, nrec=2, vlen=10, first_ts=9_000, max_ts=9_100)]),
        "non_monotonic": segment([disk_batch(0, nrec=1, vlen=10, first_ts=100, max_ts=200),
                                  disk_batch(1, nrec=1, vlen=10, first_ts=50, max_ts=150)], with_offset=True, step=1),
        "base_offset_assert": segment([disk_batch(100, nrec=1), disk_batch(50, nrec=1)], base_offset=100),
        "bad_batch": segment([disk_batch(0, nrec=1), disk_batch(1, nrec=1, crc=1), disk_batch(2, nrec=1)]),
    }


def split_cases():
    """12-batch segments: plain data, and a configuration batch first."""
    ts = 1_700_000_000_000
    plain = [disk_batch(100 + 16 * i, first_ts=ts + 40 * i, max_ts=ts + 40 * i + 15 - (90 if i == 7 else 0))
             for i in range(12)]
    config = [disk_batch(100, nrec=1, vlen=10, first_ts=5_000, max_ts=5_000, btype=2)] + \
             [disk_batch(101 + 16 * i, first_ts=ts + 40 * i, max_ts=ts + 40 * i + 15, btype=2 if i == 4 else 1)
              for i in range(11)]
    return {"plain": segment(plain, base_offset=100, with_offset=True),
            "config_first": segment(config, base_offset=100, with_offset=True)}


@functools.lru_cache(maxsize=None)
def random_cases(seed=23, count=60):
    """Segments of 0-12 small batches as recovery may meet them: a third of the batches no user data,
    now and then a base offset below the segment's or a bad CRC, every topic kind, time format and step.
    Built once; nobody writes to them."""
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(count):
        base, bs = int(rng.integers(0, 1000)), []
        off = base
        for _ in range(int(rng.integers(0, 13))):
            ts = 1_700_000_000_000 + int(rng.integers(-5_000_000, 5_000_000))
            bs.append(disk_batch(off if rng.integers(0, 25) else base - 1, nrec=int(rng.integers(1, 4)),
                                 vlen=int(rng.integers(0, 3000)), first_ts=ts,
                                 max_ts=ts + int(rng.integers(-10, 100_000)),
                                 btype=1 if rng.integers(0, 3) else int(rng.integers(2, 6)),
                                 crc=None if rng.integers(0, 40) else 1))
            off += int(rng.integers(1, 40))
        cases.append(segment(bs, base_offset=base, internal=bool(rng.integers(0, 2)),
                             with_offset=bool(rng.integers(0, 2)), step=int(rng.choice([1, 4096, 32768]))))
    return tuple(cases)


def model_track_all(descs, res, seg):
    st = sx.empty_state(int(seg["base_offset"]), bool(seg["with_offset"]))
    status, tracked = sx.track(st, descs, res, seg)
    return st, status, tracked


def assert_model_equals_oracle(descs, res, segs, entry_cap=None):
    """The model's track from an empty state against orc.segment_index, field for field; the status."""
    ost, oe = orc.segment_index(descs, res, segs)
    st = sx.empty_state(int(segs[0]["base_offset"]), bool(segs[0]["with_offset"]))
    status, tracked = sx.track(st, descs, res, segs[0], entry_cap=entry_cap)
    o = ost[0]
    assert (status, tracked, st.n) == (int(o["status"]), int(o["tracked"]), int(o["entries"]))
    assert (int(st.monotonic), int(st.non_data_timestamps), st.max_offset, st.base_timestamp, st.max_timestamp,
            st.acc) == (int(o["monotonic"]), int(o["non_data_timestamps"]), int(o["max_offset"]),
                        int(o["base_timestamp"]), int(o["max_timestamp"]), int(o["acc"]))
    assert st.rel_offset == [int(x) for x in oe["relative_offset"][:st.n]]
    assert st.rel_time == [int(x) for x in oe["relative_time"][:st.n]]
    assert st.position == [int(x) for x in oe["position"][:st.n]]
    return status


@pytest.mark.parametrize("name", list(oracle_cases()))
def test_model_track_equals_the_oracle(name):
    _, descs, res, segs = oracle_cases()[name]
    assert_model_equals_oracle(descs, res, segs)


def test_recovery_index_meets_neither_extra_verdict():
    """The recovery index (segment_index_kernel, rpgpu_index.hip; orc.segment_index) knows OK and
    OFFSET_BELOW_BASE only.  It is the shared recurrence started from an empty state with a slot of
    batch_count entries: from such a start NON_DATA_ASSERT and NO_ROOM are unreachable (non_data_timestamps
    is set only by the step that writes entry 0 and no non-data batch adds an entry after it; at most one
    entry per batch), so with that cap the model equals the oracle, which has neither."""
    seen = set()
    for _, descs, res, segs in random_cases():
        seen.add(assert_model_equals_oracle(descs, res, segs, entry_cap=int(segs[0]["batch_count"])))
    assert sum(1 for c in random_cases() if len(c[1])) >= 50
    assert seen == {0, sx.V_BELOW_BASE}


def split_seg(seg, lo, hi):
    s = seg.copy()
    s["first_batch"], s["batch_count"] = lo, hi - lo
    return s


@pytest.mark.parametrize("name", list(split_cases()))
def test_model_split_property(name):
    _, descs, res, segs = split_cases()[name]
    whole, status, tracked = model_track_all(descs, res, segs[0])
    assert (status, tracked) == (0, 12) and whole.n >= 3
    for k in range(13):
        st = sx.empty_state(100, True)
        assert sx.track(st, descs, res, split_seg(segs[0], 0, k)) == (0, k)
        assert sx.track(st, descs, res, split_seg(segs[0], k, 12)) == (0, 12 - k)
        assert st.key() == whole.key(), k
    if name == "config_first":
        assert whole.rel_time[0] == sx.time_index_raw(1_700_000_000_015, True) and not whole.non_data_timestamps


def test_model_track_stops_in_front_of_what_does_not_fit():
    _, descs, res, segs = split_cases()["plain"]
    whole, _, _ = model_track_all(descs, res, segs[0])
    st = sx.empty_state(100, True)
    status, tracked = sx.track(st, descs, res, segs[0], entry_cap=2)
    assert status == sx.V_NO_ROOM and st.n == 2 and 0 < tracked < 12
    assert sx.track(st, descs, res, split_seg(segs[0], tracked, 12), entry_cap=64) == (0, 12 - tracked)
    assert st.key() == whole.key()
    hostile = sx.empty_state(100, True)
    hostile.non_data_timestamps = True  # and no entry: only a hydrated blob can say so
    assert sx.track(hostile, descs, res, segs[0]) == (sx.V_NON_DATA_ASSERT, 0)


# ------------------------------------------------------------ hydrate by name
@pytest.mark.parametrize("name", list(sx.HYDRATE_EXPECT))
def test_model_hydrate_outcomes(name):
    blob, cap = sx.hydrate_cases()[name]
    h = sx.hydrate(blob, cap)
    assert (h.status, h.reason) == sx.HYDRATE_EXPECT[name]
    if h.status == sx.OK:
        want = sx.sweep_state(5, True, 91)
        assert (h.state.rel_offset, h.state.rel_time, h.state.position) == (want.rel_offset, want.rel_time,
                                                                           want.position)
        flags = (h.state.monotonic, h.state.with_offset, h.state.non_data_timestamps)
        assert flags == ((False, False, False) if h.version in (3, 4) else (want.monotonic, True, False))
        assert h.state.acc == 0 and h.state.last_batch_max_timestamp == -1


def test_hydrate_case_table_is_complete():
    assert set(sx.hydrate_cases()) == set(sx.HYDRATE_EXPECT)
    seen = {v for v in sx.HYDRATE_EXPECT.values()}
    assert {r for _, r in seen} == set(range(sx.R_ENTRY_CAP + 1)), "every reason but BAD_ROW"


# --------------------------------------------------------------- host program
def build_host(out: Path, flags, csrc: Path = CSRC) -> Path:
    subprocess.run(["g++", *flags, "-std=c++17", f"-I{csrc}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "segidx_host.cpp"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return out


def run_host(exe: Path, mode: str, inp: Path, out: Path):
    r = subprocess.run([str(exe), mode, str(inp), str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{mode}: exit {r.returncode}: {r.stderr[-1500:]}"


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("segidx_host")
    return {False: build_host(d / "segidx_host", PLAIN), True: build_host(d / "segidx_host_san", SANITIZE)}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    d = tmp_path_factory.mktemp("segidx_sweep")
    states = sx.build_sweep()
    sx.assert_sweep_classes(states)
    blobs = [sx.to_blob(s) for s in states]
    files = [(b, s.n) for b, s in zip(blobs, states)]
    files += [(sx.to_v3(s), s.n) for s in states] + [(sx.to_v4(s), s.n) for s in states[::7]]
    files += [(blob, 5 if cap is None else cap) for blob, cap in sx.hydrate_cases().values()]
    queries = sx.sweep_queries(states)
    sx.write_states_file(d / "states.bin", states)
    sx.write_files_file(d / "files.bin", files)
    sx.write_find_file(d / "find.bin", states, queries)
    return dict(dir=d, states=states, blobs=blobs, files=files, queries=queries,
                hydrated=[sx.hydrate(b, cap) for b, cap in files],
                found=[sx.find(states[i], kind, key) for i, kind, key in queries])


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_host_program_over_the_sweep(hosts, sweep, tmp_path, san):
    d = sweep["dir"]
    run_host(hosts[san], "write", d / "states.bin", tmp_path / "w.out")
    got = sx.read_blobs(tmp_path / "w.out", len(sweep["states"]))
    for s, (status, blob), want in zip(sweep["states"], got, sweep["blobs"]):
        assert status == sx.OK and blob == want, s.name
    run_host(hosts[san], "hydrate", d / "files.bin", tmp_path / "h.out")
    for k, ((row, st), want) in enumerate(zip(sx.read_hydrated(tmp_path / "h.out", len(sweep["files"])),
                                              sweep["hydrated"])):
        assert row == want.row(), k
        assert (st is None) == (want.state is None) and (st is None or st.key() == want.state.key()), k
    run_host(hosts[san], "find", d / "find.bin", tmp_path / "f.out")
    got = sx.read_found(tmp_path / "f.out", len(sweep["queries"]))
    for k, (g, w) in enumerate(zip(got, sweep["found"])):
        assert g == w, (sweep["queries"][k], sweep["states"][sweep["queries"][k][0]].name)


def track_jobs():
    """(State, cap, step, rows) with the model's outcome: the oracle's cases whole,
    the split cases at every k (the second half from the first half's state), a
    cap that runs out, the hostile state, the random segments as the recovery index
    tracks them (from empty, a slot of batch_count entries)."""
    jobs, want = [], []

    def add(st, cap, seg, descs, res):
        jobs.append((st.copy(), cap, int(seg["step"]), sx.batch_rows(descs, res, seg)))
        after = st.copy()
        status, tracked = sx.track(after, descs, res, seg, entry_cap=cap)
        want.append((status, tracked, after))
        return after

    for _, descs, res, segs in oracle_cases().values():
        add(sx.empty_state(int(segs[0]["base_offset"]), bool(segs[0]["with_offset"])), 16, segs[0], descs, res)
    for _, descs, res, segs in split_cases().values():
        for k in range(13):
            half = add(sx.empty_state(100, True), 16, split_seg(segs[0], 0, k), descs, res)
            add(half, 16, split_seg(segs[0], k, 12), descs, res)
        add(sx.empty_state(100, True), 2, segs[0], descs, res)
        hostile = sx.empty_state(100, True)
        hostile.non_data_timestamps = True
        add(hostile, 16, segs[0], descs, res)
    for _, descs, res, segs in random_cases():
        add(sx.empty_state(int(segs[0]["base_offset"]), bool(segs[0]["with_offset"])), int(segs[0]["batch_count"]),
            segs[0], descs, res)
    return jobs, want


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_host_program_tracks_like_the_model(hosts, tmp_path, san):
    jobs, want = track_jobs()
    sx.write_track_file(tmp_path / "t.bin", jobs)
    run_host(hosts[san], "track", tmp_path / "t.bin", tmp_path / "t.out")
    got = sx.read_tracked(tmp_path / "t.out", len(jobs))
    assert {w[0] for w in want} == {0, sx.V_BELOW_BASE, sx.V_NON_DATA_ASSERT, sx.V_NO_ROOM}
    for k, ((status, tracked, st), (wstatus, wtracked, wst)) in enumerate(zip(got, want)):
        assert (status, tracked) == (wstatus, wtracked) and st.key() == wst.key(), k


MUTANTS = [
    ("needle_not_truncated", "const uint32_t needle = (uint32_t)((uint64_t)key - (uint64_t)s.base_offset);",
     "const uint64_t needle = (uint64_t)key - (uint64_t)s.base_offset;"),
    ("time_lookup_answers_none", "found_entry(s, e, dist > 0 ? dist - 1 : 0, o);",
     "if (dist < n) found_entry(s, e, dist > 0 ? dist - 1 : 0, o);"),
    ("offset_time_signed", "if ((int64_t)ot < rel) {", "if ((int64_t)(int32_t)ot < rel) {"),
    ("version_4_reads_flags", "if (v->version >= 5) {", "if (v->version >= 4) {"),
    ("size_field_exact", "if (left < ld<uint32_t>(p + 2))", "if (left != ld<uint32_t>(p + 2))"),
    ("xxh_tail_dropped", "for (uint64_t at = len & ~(uint64_t)31; at < len; at += 8)",
     "for (uint64_t at = len & ~(uint64_t)31; at + 16 < len; at += 8)"),
    ("rewrite_stores_delta", "e[0].relative_time = time_index_raw(last_ts, s->with_offset);",
     "e[0].relative_time = time_index_raw(last_ts - b.first_timestamp, s->with_offset);"),
    ("no_room_after_the_write", "if (indexed && s->entries >= s->entry_cap) return RPGPU_V_INDEX_NO_ROOM;",
     "if (indexed && s->entries > s->entry_cap) return RPGPU_V_INDEX_NO_ROOM;"),
]


@pytest.mark.parametrize("name,old,new", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_sweep_rejects_one_token_changes(sweep, tmp_path, name, old, new):
    """The plain build of a header with one token changed must differ from the model somewhere."""
    text = (CSRC / "rpgpu_segidx.h").read_text()
    assert text.count(old) == 1, name
    (tmp_path / "rpgpu_segidx.h").write_text(text.replace(old, new))
    r = subprocess.run(["g++", *PLAIN, "-std=c++17", f"-I{tmp_path}", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                        str(ROOT / "tests" / "native" / "segidx_host.cpp"), "-o", str(tmp_path / "mutant")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-1500:]
    d, differs = sweep["dir"], False
    try:
        run_host(tmp_path / "mutant", "hydrate", d / "files.bin", tmp_path / "h.out")
        got = sx.read_hydrated(tmp_path / "h.out", len(sweep["files"]))
        differs |= any(row != w.row() or (st is not None and st.key() != w.state.key())
                       for (row, st), w in zip(got, sweep["hydrated"]))
        run_host(tmp_path / "mutant", "find", d / "find.bin", tmp_path / "f.out")
        differs |= sx.read_found(tmp_path / "f.out", len(sweep["queries"])) != sweep["found"]
        jobs, want = track_jobs()
        sx.write_track_file(tmp_path / "t.bin", jobs)
        run_host(tmp_path / "mutant", "track", tmp_path / "t.bin", tmp_path / "t.out")
        got = sx.read_tracked(tmp_path / "t.out", len(jobs))
        differs |= any((s, t) != (ws, wt) or st.key() != wst.key() for (s, t, st), (ws, wt, wst) in zip(got, want))
    except AssertionError:
        differs = True  # the mutant crashed or wrote a file of another shape
    assert differs, name


# ------------------------------------------------------ compiler's resources
KERNELS = ["track", "place", "emit", "crc", "hydrate", "find"]


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """The compiler's own resource remarks for rpgpu_segidx.hip (DESIGN.md §3 states the numbers)."""
    from redpanda_amd import _build

    r = subprocess.run(["hipcc", *_build.rpgpu_flags(), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", str(_build.CSRC / "rpgpu_segidx.hip"), "-o", str(tmp_path / "sx.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*([A-Za-z][A-Za-z /\[\]]*?):\s*(\S+)", line)
        if m and m.group(1).strip() == "Function Name":
            cur = kernels.setdefault(m.group(2), {})
        elif m and cur is not None and m.group(2).isdigit():
            cur[m.group(1).strip()] = int(m.group(2))
    assert len(kernels) == len(KERNELS) and all(any(f"segidx_{n}_kernel" in k for k in kernels) for n in KERNELS)
    for k, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert u["AGPRs"] == 0 and u["VGPRs"] <= 64, (k, u)


# ------------------------------------------------------------------------ ABI
ABI_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "rpgpu.h"
_Static_assert(RPGPU_ABI_VERSION == 6, "the segment index life cycle is additive");
_Static_assert(sizeof(rpgpu_segidx_state) % 16 == 0 && sizeof(rpgpu_segidx_tracked) % 16 == 0, "rows");
_Static_assert(sizeof(rpgpu_segidx_blob) % 16 == 0 && sizeof(rpgpu_segidx_file) % 16 == 0, "rows");
_Static_assert(sizeof(rpgpu_segidx_hydrated) % 16 == 0 && sizeof(rpgpu_segidx_query) % 16 == 0, "rows");
_Static_assert(sizeof(rpgpu_segidx_found) % 16 == 0, "rows");
#define OFF(T, F) printf("%s.%s %zu\n", #T, #F, offsetof(rpgpu_segidx_##T, F))
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rpgpu_segidx_state), sizeof(rpgpu_segidx_tracked),
           sizeof(rpgpu_segidx_blob), sizeof(rpgpu_segidx_file), sizeof(rpgpu_segidx_hydrated),
           sizeof(rpgpu_segidx_query), sizeof(rpgpu_segidx_found));
    printf("%d %d %d %d %d %d %d\n", RPGPU_SEGIDX_OK, RPGPU_SEGIDX_NO_ROOM, RPGPU_SEGIDX_TOO_BIG, RPGPU_SEGIDX_REBUILD,
           RPGPU_SEGIDX_THROW, RPGPU_SEGIDX_COLUMNS_DIFFER, RPGPU_SEGIDX_BAD_STATE);
    printf("%d %d %d %d %d %d\n", RPGPU_SEGIDX_R_NONE, RPGPU_SEGIDX_R_EMPTY_FILE, RPGPU_SEGIDX_R_CRC_MISMATCH,
           RPGPU_SEGIDX_R_V3_CHECKSUM, RPGPU_SEGIDX_R_ENTRY_CAP, RPGPU_SEGIDX_R_BAD_ROW);
    printf("%d %d %d %d %d %d\n", RPGPU_SEGIDX_BY_OFFSET, RPGPU_SEGIDX_BY_TIME, RPGPU_SEGIDX_TIME_BEFORE,
           RPGPU_SEGIDX_FOUND, RPGPU_SEGIDX_NONE, RPGPU_SEGIDX_BAD_QUERY);
    printf("%d %d %d %d\n", RPGPU_V_INDEX_OFFSET_BELOW_BASE, RPGPU_V_INDEX_NON_DATA_ASSERT, RPGPU_V_INDEX_NO_ROOM,
           RPGPU_V_INDEX_BAD_STATE);
    OFF(state, max_timestamp); OFF(state, bitflags); OFF(state, entries); OFF(state, entry_first);
    OFF(state, entry_cap); OFF(state, acc); OFF(state, last_batch_max_timestamp); OFF(state, monotonic);
    OFF(state, with_offset); OFF(state, non_data_timestamps); OFF(tracked, tracked); OFF(tracked, added);
    OFF(blob, entries); OFF(blob, out_bytes); OFF(blob, out_offset); OFF(file, blob_bytes); OFF(hydrated, reason);
    OFF(hydrated, version); OFF(hydrated, entries); OFF(query, kind); OFF(query, key); OFF(found, ix);
    OFF(found, offset); OFF(found, timestamp); OFF(found, filepos);
    return 0;
}
"""
NEW_SYMBOLS = {"rpgpu_segidx_track_device", "rpgpu_segidx_write_plan_device", "rpgpu_segidx_write_run_device",
               "rpgpu_segidx_hydrate_device", "rpgpu_segidx_find_device"}


def test_header_layouts_match_abi_py(tmp_path):
    (tmp_path / "a.c").write_text(ABI_C)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(tmp_path / "a.c"),
                    "-o", str(tmp_path / "a")], check=True, capture_output=True, text=True)
    lines = subprocess.run([str(tmp_path / "a")], capture_output=True, text=True, check=True).stdout.splitlines()
    dtypes = dict(state=abi.SEGIDX_STATE_DTYPE, tracked=abi.SEGIDX_TRACKED_DTYPE, blob=abi.SEGIDX_BLOB_DTYPE,
                  file=abi.SEGIDX_FILE_DTYPE, hydrated=abi.SEGIDX_HYDRATED_DTYPE, query=abi.SEGIDX_QUERY_DTYPE,
                  found=abi.SEGIDX_FOUND_DTYPE)
    assert lines[0].split() == [str(d.itemsize) for d in dtypes.values()]
    assert lines[1].split() == [str(v) for v in (abi.SEGIDX_OK, abi.SEGIDX_NO_ROOM, abi.SEGIDX_TOO_BIG,
                                                 abi.SEGIDX_REBUILD, abi.SEGIDX_THROW, abi.SEGIDX_COLUMNS_DIFFER,
                                                 abi.SEGIDX_BAD_STATE)]
    assert (sx.OK, sx.NO_ROOM, sx.TOO_BIG, sx.REBUILD, sx.THROW, sx.COLUMNS_DIFFER, sx.BAD_STATE) == tuple(range(7))
    assert lines[2].split() == [str(v) for v in (abi.SEGIDX_R_NONE, abi.SEGIDX_R_EMPTY_FILE, abi.SEGIDX_R_CRC_MISMATCH,
                                                 abi.SEGIDX_R_V3_CHECKSUM, abi.SEGIDX_R_ENTRY_CAP,
                                                 abi.SEGIDX_R_BAD_ROW)]
    assert (sx.R_CRC_MISMATCH, sx.R_V3_CHECKSUM, sx.R_ENTRY_CAP, sx.R_BAD_ROW) == (
        abi.SEGIDX_R_CRC_MISMATCH, abi.SEGIDX_R_V3_CHECKSUM, abi.SEGIDX_R_ENTRY_CAP, abi.SEGIDX_R_BAD_ROW)
    assert lines[3].split() == [str(v) for v in (abi.SEGIDX_BY_OFFSET, abi.SEGIDX_BY_TIME, abi.SEGIDX_TIME_BEFORE,
                                                 abi.SEGIDX_FOUND, abi.SEGIDX_NONE, abi.SEGIDX_BAD_QUERY)]
    assert lines[4].split() == [str(v) for v in (abi.V_INDEX_OFFSET_BELOW_BASE, abi.V_INDEX_NON_DATA_ASSERT,
                                                 abi.V_INDEX_NO_ROOM, abi.V_INDEX_BAD_STATE)]
    assert (sx.V_BELOW_BASE, sx.V_NON_DATA_ASSERT, sx.V_NO_ROOM, sx.V_BAD_STATE) == (
        abi.V_INDEX_OFFSET_BELOW_BASE, abi.V_INDEX_NON_DATA_ASSERT, abi.V_INDEX_NO_ROOM, abi.V_INDEX_BAD_STATE)
    for line in lines[5:]:
        name, off = line.split()
        row, fld = name.split(".")
        assert dtypes[row].fields[fld][1] == int(off), name
    for mine, theirs in ((sx.STATE_DTYPE, abi.SEGIDX_STATE_DTYPE), (sx.ENTRY_DTYPE, abi.INDEX_ENTRY_DTYPE),
                         (sx.HYDRATED_DTYPE, abi.SEGIDX_HYDRATED_DTYPE), (sx.QUERY_DTYPE, abi.SEGIDX_QUERY_DTYPE),
                         (sx.FOUND_DTYPE, abi.SEGIDX_FOUND_DTYPE)):
        assert mine == theirs
    assert abi.ABI_VERSION == 6 and NEW_SYMBOLS <= set(abi.EXPORTED)
