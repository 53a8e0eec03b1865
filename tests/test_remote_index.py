"""The tiered-storage offset index, CPU half (no GPU needed):

* the Python model tests/remote_index.py: decode(encode) for every row width
  0..64 with both delta kinds and the row size 1 + 2 * nbits; the hand vector of
  include/rpgpu.h;
* the shared core redpanda_amd/csrc/rpgpu_dfor.h compiled for the host
  (tests/native/rsindex_host.cpp) against the model over the sweep: blobs byte
  for byte, every result field, every lookup; once more under ASan + UBSan,
  stand-alone, every blob and row in a heap block of exactly its size;
* a table of one-token changes to rpgpu_dfor.h that the sweep must reject;
* struct sizes and enum values of include/rpgpu.h against redpanda_amd/abi.py;
* the compiler's resource remarks for the kernels: no scratch, no spills.
File-stream (delta_delta) widths above 31 cannot be reached through summed
int32 size_bytes in a test-sized arena; the host program's `rows` mode covers
every width 0..64 for both delta kinds.  The device half is
tests/test_gpu_remote_index.py."""
import random
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import remote_index as ri
from redpanda_amd import abi

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "redpanda_amd" / "csrc" / "rpgpu_dfor.h"
PLAIN = ["-O2"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_host(out: Path, flags, csrc: Path = HEADER.parent) -> Path:
    subprocess.run(["g++", *flags, "-std=c++17", f"-I{csrc}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "rsindex_host.cpp"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return out


def run_host(exe: Path, mode: str, inp: Path, out: Path):
    r = subprocess.run([str(exe), mode, str(inp), str(out)], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stderr


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("rsindex_host")
    return {False: build_host(d / "rsindex_host", PLAIN), True: build_host(d / "rsindex_host_san", SANITIZE)}


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    d = tmp_path_factory.mktemp("rsindex_sweep")
    case = ri.build_sweep()
    exp = case.expected()
    ri.assert_sweep_classes(case, exp)
    data, descs, segs = case.arena()
    inp = d / "sweep.bin"
    ri.write_build_input(inp, data, descs, segs)
    queries = ri.sweep_queries(case, exp)
    cache = {}
    want = []
    for i, by_rp, bound in queries:
        if i not in cache:
            cache[i] = ri.OffsetIndex.from_bytes(exp[i].blob)
        want.append(cache[i].find(by_rp, bound).tuple())
    bad = ri.bad_blobs(exp[[s.name for s in case.segments].index("samples17")].blob)
    fq = [(exp[i].blob, by_rp, bound) for i, by_rp, bound in queries]
    fq += [(b, by_rp, 5010) for b in bad.values() for by_rp in (True, False)]
    want += [ri.Found(ri.BAD_BLOB).tuple()] * (2 * len(bad))
    finp = d / "find.bin"
    ri.write_find_input(finp, fq)
    return case, exp, inp, finp, want


def check_build(case, exp, exe: Path, inp: Path, out: Path):
    """None when the program's output equals the model's, else what differs first."""
    rc, err = run_host(exe, "build", inp, out)
    if rc != 0:
        return f"exit {rc}: {err[-1500:]}"
    tot, res, blobs = ri.read_build_output(out, len(exp))
    if tuple(int(t) for t in tot) != ri.totals(exp):
        return f"totals {tot} vs {ri.totals(exp)}"
    want = ri.expected_results(exp)
    for f in want.dtype.names:
        bad = np.nonzero(res[f] != want[f])[0]
        if bad.size:
            return f"result field {f} differs at {case.segments[bad[0]].name}: {res[f][bad[0]]} vs {want[f][bad[0]]}"
    for i, b in enumerate(exp):
        if blobs[i] != b.blob:
            return f"blob of {case.segments[i].name} differs"
    return None


def check_find(exe: Path, finp: Path, out: Path, want):
    rc, err = run_host(exe, "find", finp, out)
    if rc != 0:
        return f"exit {rc}: {err[-1500:]}"
    got = ri.read_found(out, len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"query {k}: {g} vs {w}"
    return None


def width_rows():
    """(step or None, prev, values): a row of every width 0..64 for both delta kinds."""
    rng = random.Random(7)
    rows = []
    for w in range(65):
        prev, vals = rng.randrange(-(1 << 62), 1 << 62), []
        cur = prev
        for i in range(ri.ROW):
            d = 0 if w == 0 else rng.getrandbits(w - 1) | ((1 << (w - 1)) if i == w % ri.ROW else 0)
            cur = ri.s64((cur & ri.M64) ^ d)
            vals.append(cur)
        rows.append((None, prev, vals))
        step, prev = 4096, rng.randrange(0, 1 << 20)
        cur, vals = prev, []
        hi = min(w, 59)  # sixteen deltas below 2^59 keep the sum inside int64; the top row widths wrap below
        for i in range(ri.ROW):
            d = 0 if hi == 0 else rng.getrandbits(hi - 1) | ((1 << (hi - 1)) if i == w % ri.ROW else 0)
            cur += step + d
            vals.append(cur)
        rows.append((step, prev, vals))
    return rows


def test_rows_round_trip_at_every_width():
    seen = {None: set(), 4096: set()}
    for step, prev, vals in width_rows():
        e = ri.Encoder(prev, step)
        e.add(vals)
        nbits = e.nbits[0]
        assert len(e.data) == 1 + 2 * nbits and e.data[0] == nbits
        assert ri.decode_stream(bytes(e.data), 1, prev, step) == vals
        seen[step].add(nbits)
    assert seen[None] == set(range(65)) and seen[4096] == set(range(60))
    # delta_delta is plain 64-bit arithmetic: the widths 60..64 from raw deltas
    for w in range(60, 65):
        buf = [(1 << (w - 1)) | i for i in range(ri.ROW)]
        row = ri.row_encode(buf, w)
        assert len(row) == 1 + 2 * w and ri.row_decode(row, 0) == (buf, len(row))


def test_hand_vector():
    b = ri.build_segment(ri.hand_vector())
    x = b.index
    assert (b.status, b.samples, b.rows, len(b.blob)) == (ri.OK, 29, 1, 527) and b.blob[2:6].hex() == "09020000"
    assert [e.last for e in x.enc] == [1034, 1021, 3231]
    assert [bytes(e.data).hex() for e in x.enc] == ["0b0206021c06020e020602fe0206020e02000000c00100",
                                                     "06be6004822318822718822318", "06335dcf743dd3f54cd7335dcf"]
    assert x.samples[:4] == [(1002, 992, 201), (1004, 994, 403), (1006, 996, 606), (1010, 997, 807)]
    assert x.wb[0][13:] == [1030, 1032, 1034]
    y = ri.OffsetIndex.from_bytes(b.blob)
    assert y.to_bytes() == b.blob
    assert y.find(False, 1003).tuple() == (ri.FOUND, 0, 5, 1014, 1001, 1212)
    assert y.find(False, 1022).tuple() == (ri.FOUND, 0, 15, 1034, 1021, 3231)
    assert y.find(False, 1030).tuple() == (ri.FOUND, 1, 3, 1042, 1029, 4039)
    assert y.find(False, 992).status == ri.NONE
    assert y.find(True, 1036).tuple() == (ri.FOUND, 0, 15, 1034, 1021, 3231)
    assert y.find(True, 99999).tuple() == (ri.FOUND, 1, 12, 1060, 1047, 5857)


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_host_program_hand_vector_and_rows(hosts, tmp_path, san):
    case = ri.Case([ri.hand_vector()])
    exp = case.expected()
    ri.write_build_input(tmp_path / "hand.bin", *case.arena())
    assert check_build(case, exp, hosts[san], tmp_path / "hand.bin", tmp_path / "hand.out") is None
    rows = width_rows()
    for w in range(60, 65):  # delta_delta rows of the top widths: the sum wraps, as the 64-bit arithmetic does
        rows.append((3, 5, [ri.s64(5 + (k + 1) * (3 + (1 << (w - 1)))) for k in range(ri.ROW)]))
    ri.write_rows_input(tmp_path / "rows.bin", rows)
    rc, err = run_host(hosts[san], "rows", tmp_path / "rows.bin", tmp_path / "rows.out")
    assert rc == 0, err[-1500:]
    want = b""
    for step, prev, vals in rows:
        p, buf = prev, []
        for v in vals:
            buf.append((v ^ p) & ri.M64 if step is None else (v - p - step) & ri.M64)
            p = v
        agg = 0
        for d in buf:
            agg |= d
        want += ri.row_encode(buf, agg.bit_length())
    assert (tmp_path / "rows.out").read_bytes() == want


@pytest.mark.parametrize("san", [False, True], ids=["plain", "sanitized"])
def test_host_program_over_the_sweep(hosts, sweep, tmp_path, san):
    case, exp, inp, finp, want = sweep
    assert check_build(case, exp, hosts[san], inp, tmp_path / "sweep.out") is None
    assert check_find(hosts[san], finp, tmp_path / "find.out", want) is None


MUTANTS = [
    ("window_gt", "return window >= sampling_step;", "return window > sampling_step;"),
    ("type19_sampled", "return type == 2 || type == 19;", "return type == 2 || type == 18;"),
    ("stale_buffer_cleared", "    en.last = x->wb[s][kRow - 1];\n",
     "    en.last = x->wb[s][kRow - 1];\n        for (uint32_t e = 0; e < kRow; e++) x->wb[s][e] = 0;\n"),
    ("remainder_bit_order", "const int sh = (int)(i * r) - (int)(8 * j);",
     "const int sh = (int)((kRow - 1 - i) * r) - (int)(8 * j);"),
    ("section_order", "if (left >= 16) {\n        st<uint16_t>", "if (left >= 24) {\n        st<uint16_t>"),
    ("find_le", "if (vals[e] >= upper_bound) {", "if (vals[e] > upper_bound) {"),
    ("last_of_row", "en.last = x->wb[s][kRow - 1];", "en.last = x->wb[s][0];"),
    ("pos_is_descriptor_sum", "b->pos += (uint64_t)size_bytes;", "b->pos += 61;"),
]


@pytest.mark.parametrize("name,old,new", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_sweep_rejects_one_token_changes(sweep, tmp_path, name, old, new):
    case, exp, inp, finp, want = sweep
    text = HEADER.read_text()
    assert text.count(old) == 1, name
    (tmp_path / "rpgpu_dfor.h").write_text(text.replace(old, new))
    exe = build_host(tmp_path / "mutant", PLAIN, csrc=tmp_path)
    verdicts = [check_build(case, exp, exe, inp, tmp_path / "b.out"), check_find(exe, finp, tmp_path / "f.out", want)]
    assert any(v is not None for v in verdicts), name


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """The compiler's own resource remarks for rpgpu_rsindex.hip (DESIGN.md §3 states the numbers)."""
    from redpanda_amd import _build

    r = subprocess.run(["hipcc", *_build.rpgpu_flags(), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", str(_build.CSRC / "rpgpu_rsindex.hip"), "-o", str(tmp_path / "rs.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*([A-Za-z][A-Za-z /\[\]]*?):\s*(\S+)", line)
        if m and m.group(1).strip() == "Function Name":
            cur = kernels.setdefault(m.group(2), {})
        elif m and cur is not None and m.group(2).isdigit():
            cur[m.group(1).strip()] = int(m.group(2))
    names = ["select", "width", "place", "emit", "find"]
    assert len(kernels) == len(names) and all(any(f"rsindex_{n}_kernel" in k for k in kernels) for n in names)
    for k, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert u["AGPRs"] == 0 and u["VGPRs"] <= 128, (k, u)


ABI_C = r"""
#include <stdio.h>
#include "rpgpu.h"
_Static_assert(RPGPU_ABI_VERSION == 6, "the offset index is additive");
_Static_assert(sizeof(rpgpu_rsindex_segment) % 16 == 0 && sizeof(rpgpu_rsindex_result) % 16 == 0, "rows");
_Static_assert(sizeof(rpgpu_rsindex_query) % 16 == 0 && sizeof(rpgpu_rsindex_found) % 16 == 0, "rows");
int main(void) {
    printf("%zu %zu %zu %zu\n", sizeof(rpgpu_rsindex_segment), sizeof(rpgpu_rsindex_result),
           sizeof(rpgpu_rsindex_query), sizeof(rpgpu_rsindex_found));
    printf("%d %d %d %d\n", RPGPU_RSINDEX_OK, RPGPU_RSINDEX_NO_ROOM, RPGPU_RSINDEX_BAD_BATCH,
           RPGPU_RSINDEX_DELTA_ASSERT);
    printf("%d %d %d\n", RPGPU_RSINDEX_FOUND, RPGPU_RSINDEX_NONE, RPGPU_RSINDEX_BAD_BLOB);
    printf("%zu %zu %zu %zu %zu\n", offsetof(rpgpu_rsindex_segment, sampling_step),
           offsetof(rpgpu_rsindex_result, final_delta), offsetof(rpgpu_rsindex_result, out_offset),
           offsetof(rpgpu_rsindex_query, upper_bound), offsetof(rpgpu_rsindex_found, file_pos));
    return 0;
}
"""


def test_header_layouts_match_abi_py(tmp_path):
    (tmp_path / "a.c").write_text("#include <stddef.h>\n" + ABI_C)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(tmp_path / "a.c"),
                    "-o", str(tmp_path / "a")], check=True, capture_output=True, text=True)
    lines = subprocess.run([str(tmp_path / "a")], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[0].split() == [str(d.itemsize) for d in (abi.RSINDEX_SEGMENT_DTYPE, abi.RSINDEX_RESULT_DTYPE,
                                                           abi.RSINDEX_QUERY_DTYPE, abi.RSINDEX_FOUND_DTYPE)]
    assert lines[1].split() == [str(v) for v in (abi.RSINDEX_OK, abi.RSINDEX_NO_ROOM, abi.RSINDEX_BAD_BATCH,
                                                 abi.RSINDEX_DELTA_ASSERT)]
    assert (ri.OK, ri.NO_ROOM, ri.BAD_BATCH, ri.DELTA_ASSERT) == (abi.RSINDEX_OK, abi.RSINDEX_NO_ROOM,
                                                                   abi.RSINDEX_BAD_BATCH, abi.RSINDEX_DELTA_ASSERT)
    assert lines[2].split() == [str(v) for v in (abi.RSINDEX_FOUND, abi.RSINDEX_NONE, abi.RSINDEX_BAD_BLOB)]
    assert (ri.FOUND, ri.NONE, ri.BAD_BLOB) == (abi.RSINDEX_FOUND, abi.RSINDEX_NONE, abi.RSINDEX_BAD_BLOB)
    assert lines[3].split() == [str(v) for v in (abi.RSINDEX_SEGMENT_DTYPE.fields["sampling_step"][1],
                                                 abi.RSINDEX_RESULT_DTYPE.fields["final_delta"][1],
                                                 abi.RSINDEX_RESULT_DTYPE.fields["out_offset"][1],
                                                 abi.RSINDEX_QUERY_DTYPE.fields["upper_bound"][1],
                                                 abi.RSINDEX_FOUND_DTYPE.fields["file_pos"][1])]
    assert abi.ABI_VERSION == 6 and {"rpgpu_rsindex_scratch_bytes", "rpgpu_rsindex_plan_device",
                                     "rpgpu_rsindex_run_device", "rpgpu_rsindex_find_device"} <= set(abi.EXPORTED)
