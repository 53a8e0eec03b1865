"""Produce batches from records, without a GPU:

* murmur2 and the hand request of include/rpgpu.h against tests/produce_records.py's
  literal restatement of client::produce_records, byte for byte;
* every batch the model builds passes the untouched oracle's validation, and
  the oracle's record index gives back each row's key, value, offset delta and
  now_ms; the model's wire form equals the oracle's serializer;
* the reference's own partitioner test cases (kafka/client/test/partitioners.cc:54-78);
* rpgpu_produce.h compiled for the host (tests/native/produce_host.cpp) against
  the model over the hand cases and the sweeps, plain and under
  -fsanitize=address,undefined as a stand-alone program;
* struct layouts and enum values of include/rpgpu.h against redpanda_amd/abi.py,
  and the exported symbols."""
import os
import re
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import produce_records as pr  # noqa: E402

import oracle.oracle as orc  # noqa: E402
from redpanda_amd import abi  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "redpanda_amd" / "csrc"
PLAIN = ["-O2"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

CASES = {
    "hand": pr.hand_call,
    "keys": pr.key_geometry_call,
    "values": pr.value_call,
    "groups": lambda: pr.group_call((64, 65)),
    "round-robin": lambda: pr.round_robin_call(2100),
    "ids-6": lambda: pr.ids_call(6),
    "ids-0": lambda: pr.ids_call(0),
    "sweep-a": lambda: pr.random_call(101, 300, 5),
    "sweep-b": lambda: pr.random_call(102, 400, 65, empty_at=(0, 31, 64)),
    "sweep-uncached": lambda: pr.random_call(103, 200, 3, counts=(0,)),
    **{f"guard-{w}": (lambda w=w: pr.guard_call(w)) for w in pr.GUARDS},
}


def test_murmur2_vectors():
    for key, want in pr.MURMUR_VECTORS.items():
        assert pr.murmur2(key) == want, key
    assert pr.murmur2(b"the key") % 6 == 1 and pr.murmur2(b"k") % 6 == 4


def test_hand_request_byte_for_byte():
    a = pr.hand_call()
    m = pr.model(a["data"], a["rows"], a["requests"])
    now = int(a["requests"]["now_ms"][0])
    assert m["req_results"].tolist() == [(pr.OK, 7, 0, 4)]
    assert m["row_batch"].tolist() == [2, 1, 3, 0, 2] and m["row_delta"].tolist() == [0, 0, 0, 0, 1]
    assert len(m["batches"]) == len(pr.HAND_BODIES) == m["nbatches"]
    counts = [1, 1, 2, 1]
    for k, ((part, body), b) in enumerate(zip(pr.HAND_BODIES, m["batches"])):
        o, ln = int(b["out_offset"]), int(b["out_len"])
        assert o % 64 == 0 and ln == 61 + len(body) and (int(b["request"]), int(b["partition"])) == (0, part)
        assert int(b["record_count"]) == counts[k]
        raw = m["out"][o:o + ln].tobytes()
        assert raw[61:] == body, (part, raw[61:].hex())
        h = np.frombuffer(raw[:61], abi.RP_HEADER_DTYPE)[0]
        assert (int(h["size_bytes"]), int(h["base_offset"]), int(h["type"]), int(h["attrs"])) == (ln, 0, 1, 0)
        assert (int(h["last_offset_delta"]), int(h["record_count"])) == (counts[k] - 1, counts[k])
        assert int(h["first_timestamp"]) == int(h["max_timestamp"]) == now
        assert (int(h["producer_id"]), int(h["producer_epoch"]), int(h["base_sequence"])) == (-1, -1, -1)
        assert int(h["crc"]) & 0xFFFFFFFF == orc.crc_record_batch(h, body) & 0xFFFFFFFF
        assert int(h["header_crc"]) == orc.internal_header_only_crc(h)


def test_the_references_partitioner_cases():
    """kafka/client/test/partitioners.cc:54-78: partition 4 / key "the key" / nothing, count 6, initial 5."""
    match_partition, match_key, match_none = pr.Rec(4, None, None), pr.Rec(None, b"the key", None), pr.Rec()
    assert pr.identity_partitioner(match_none, 6) is None and pr.identity_partitioner(match_partition, 6) == 4
    assert pr.murmur2_key_partitioner(match_none, 6) is None
    assert pr.murmur2_key_partitioner(match_key, 6) == pr.murmur2(b"the key") % 6
    rr = pr.RoundRobin(5)
    assert rr(match_none, 6) == 5 and rr(match_none, 6) == (5 + 1) % 6
    d = pr.DefaultPartitioner(5)
    assert d(match_partition, 6) == 4 and d(match_key, 6) == pr.murmur2(b"the key") % 6 and d(match_none, 6) == 5


@pytest.mark.parametrize("name", ["hand", "keys", "values", "groups", "ids-6", "ids-0", "sweep-a", "sweep-b",
                                  "sweep-uncached"])
def test_model_batches_pass_the_oracle(name):
    """Verdict OK for every batch; the oracle's index gives back each row's key, value, delta and now_ms."""
    a = CASES[name]()
    m = pr.model(a["data"], a["rows"], a["requests"])
    nb = len(m["batches"])
    assert nb == m["nbatches"] and nb > 0
    res, idx, used = orc.validate_arena(m["out"], m["out_descs"][:nb])
    assert (res["verdict"] == abi.V_OK).all()
    assert used == int((m["row_batch"] != pr.NONE).sum()) == int(m["batches"]["record_count"].sum())
    out = m["out"].tobytes()
    for i, rec in enumerate(a["recs"]):
        b, d = int(m["row_batch"][i]), int(m["row_delta"][i])
        assert b != pr.NONE
        bo = int(m["batches"]["out_offset"][b])
        e = idx[int(res["index_first"][b]) + d]
        req = int(m["batches"]["request"][b])
        assert (int(e["offset"]), int(e["timestamp"])) == (d, int(a["requests"]["now_ms"][req])), i
        key = rec.key or b""                                   # an absent key is an empty one
        assert int(e["key_len"]) == len(key), i
        assert out[bo + int(e["key_off"]):bo + int(e["key_off"]) + len(key)] == key, i
        assert int(e["val_len"]) == (-1 if rec.value is None else len(rec.value)), i
        if rec.value:
            assert out[bo + int(e["val_off"]):bo + int(e["val_off"]) + len(rec.value)] == rec.value, i
    # the wire form the GPU test holds rpgpu_kafka_serialize_device against
    wire, _ = orc.kafka_serialize(m["out"], m["out_descs"][:nb])
    assert np.array_equal(wire, m["wire"])


def test_groups_and_order():
    """Requests that share partition ids give separate batches; ascending request, then signed id."""
    a = pr.ids_call(6)
    m = pr.model(a["data"], a["rows"], a["requests"])
    b = m["batches"]
    order = list(zip(b["request"].tolist(), b["partition"].tolist()))
    assert order == sorted(order) and len(set(order)) == len(order)
    assert order[0] == (0, pr.INT32_MIN) and (1, pr.INT32_MAX) == order[-1]
    assert {p for r, p in order if r == 0} == {p for r, p in order if r == 1}
    # partition_count 0: partition 0 for every row without an id, the counter stays
    a = pr.ids_call(0)
    m = pr.model(a["data"], a["rows"], a["requests"])
    assert m["req_results"]["rr_next"].tolist() == [0, 1]
    no_id = a["rows"]["flags"] == 0
    assert (m["batches"]["partition"][m["row_batch"][no_id]] == 0).all()


def test_guard_rails_in_the_model():
    for which, want in pr.GUARDS.items():
        a = pr.guard_call(which)
        m = pr.model(a["data"], a["rows"], a["requests"])
        assert m["req_results"]["status"].tolist() == [pr.OK, want, pr.OK], which
    a = pr.hand_call()
    a["requests"]["nrows"][0] = 4                              # the requests do not tile the rows
    assert pr.model(a["data"], a["rows"], a["requests"])["req_results"]["status"].tolist() == [pr.BAD_REQUEST]
    a = pr.random_call(5, 60, 4)
    m = pr.model(a["data"], a["rows"], a["requests"])
    cut = int(m["batches"]["out_offset"][int(m["req_results"]["first_batch"][2])]) + pr.TAIL_PAD
    small = pr.model(a["data"], a["rows"], a["requests"], out_cap=cut)
    assert small["req_results"]["status"].tolist()[:2] == [pr.OK, pr.OK]
    assert pr.OUT_OVERFLOW in small["req_results"]["status"].tolist()[2:]


# --------------------------------------------------------------- host program
def build_host(out: Path, flags) -> Path:
    subprocess.run(["g++", *flags, "-std=c++17", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "produce_host.cpp"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return out


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("produce_host")
    return {False: build_host(d / "produce_host", PLAIN), True: build_host(d / "produce_host_san", SANITIZE)}


def run_host(exe: Path, a, work: Path):
    inp = work / "in.bin"
    with open(inp, "wb") as f:
        f.write(np.array([len(a["data"]), len(a["rows"]), len(a["requests"])], "<u8").tobytes())
        f.write(a["data"].tobytes() + a["rows"].tobytes() + a["requests"].tobytes())
    r = subprocess.run([str(exe), str(inp)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"exit {r.returncode}: {r.stderr[-1500:]}"
    return r.stdout.splitlines()


def expected_lines(a, m):
    lines = [f"q {int(r['status'])} {int(r['rr_next'])} {int(r['nbatches'])}" for r in m["req_results"]]
    for i, w in enumerate(a["rows"]):
        b, d = int(m["row_batch"][i]), int(m["row_delta"][i])
        if b == pr.NONE:
            lines.append("r - - -")
        else:
            size = pr.record_size(d, max(int(w["key_len"]), 0), int(w["val_len"]))
            lines.append(f"r {int(m['batches']['partition'][b])} {d} {size}")
    return lines


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_host_core_equals_model(hosts, sanitized, tmp_path):
    """Every hand case and sweep; the arena is exactly data_bytes on the heap."""
    for name, make in CASES.items():
        a = make()
        m = pr.model(a["data"], a["rows"], a["requests"])
        assert run_host(hosts[sanitized], a, tmp_path) == expected_lines(a, m), name
    a = pr.hand_call()
    a["requests"]["nrows"][0] = 6                              # refused as a whole
    m = pr.model(a["data"], a["rows"], a["requests"])
    assert run_host(hosts[sanitized], a, tmp_path) == expected_lines(a, m)


# ------------------------------------------------------------------------ ABI
ABI_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "rpgpu.h"
_Static_assert(RPGPU_ABI_VERSION == 6, "the produce path is additive");
_Static_assert(sizeof(rpgpu_produce_row) == 32 && sizeof(rpgpu_produce_request) == 24, "input rows");
_Static_assert(sizeof(rpgpu_produce_result) == 16 && sizeof(rpgpu_produce_batch) == 32, "output rows");
#define OFF(T, F) printf("%s.%s %zu\n", #T, #F, offsetof(rpgpu_produce_##T, F))
int main(void) {
    printf("%zu %zu %zu %zu\n", sizeof(rpgpu_produce_row), sizeof(rpgpu_produce_request),
           sizeof(rpgpu_produce_result), sizeof(rpgpu_produce_batch));
    printf("%u\n", RPGPU_PRODUCE_HAS_PARTITION);
    printf("%d %d %d %d %d\n", RPGPU_PRODUCE_OK, RPGPU_PRODUCE_BAD_REQUEST, RPGPU_PRODUCE_BAD_ROW,
           RPGPU_PRODUCE_TOO_LARGE, RPGPU_PRODUCE_OUT_OVERFLOW);
    OFF(row, key_off); OFF(row, val_off); OFF(row, key_len); OFF(row, val_len); OFF(row, partition); OFF(row, flags);
    OFF(request, now_ms); OFF(request, nrows); OFF(request, partition_count); OFF(request, rr_initial);
    OFF(request, pad);
    OFF(result, status); OFF(result, rr_next); OFF(result, first_batch); OFF(result, nbatches);
    OFF(batch, request); OFF(batch, partition); OFF(batch, record_count); OFF(batch, pad); OFF(batch, out_offset);
    OFF(batch, out_len);
    return 0;
}
"""
NEW_SYMBOLS = {"rpgpu_produce_scratch_bytes", "rpgpu_produce_plan_device", "rpgpu_produce_run_device"}


def test_header_layouts_match_abi_py(tmp_path):
    (tmp_path / "a.c").write_text(ABI_C)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(tmp_path / "a.c"),
                    "-o", str(tmp_path / "a")], check=True, capture_output=True, text=True)
    lines = subprocess.run([str(tmp_path / "a")], capture_output=True, text=True, check=True).stdout.splitlines()
    dtypes = dict(row=abi.PRODUCE_ROW_DTYPE, request=abi.PRODUCE_REQUEST_DTYPE, result=abi.PRODUCE_RESULT_DTYPE,
                  batch=abi.PRODUCE_BATCH_DTYPE)
    assert lines[0].split() == [str(d.itemsize) for d in dtypes.values()]
    assert lines[1].split() == [str(abi.PRODUCE_HAS_PARTITION)]
    assert lines[2].split() == [str(v) for v in (abi.PRODUCE_OK, abi.PRODUCE_BAD_REQUEST, abi.PRODUCE_BAD_ROW,
                                                 abi.PRODUCE_TOO_LARGE, abi.PRODUCE_OUT_OVERFLOW)]
    assert (abi.PRODUCE_OK, abi.PRODUCE_BAD_REQUEST, abi.PRODUCE_BAD_ROW, abi.PRODUCE_TOO_LARGE,
            abi.PRODUCE_OUT_OVERFLOW) == (pr.OK, pr.BAD_REQUEST, pr.BAD_ROW, pr.TOO_LARGE, pr.OUT_OVERFLOW)
    assert len(lines) == 3 + sum(len(d.names) for d in dtypes.values())
    for line in lines[3:]:
        name, off = line.split()
        row, fld = name.split(".")
        assert dtypes[row].fields[fld][1] == int(off), name


def test_new_symbols_are_exported(built):
    from redpanda_amd import _build

    out = subprocess.run(["nm", "-D", "--defined-only", str(_build.LIBRPGPU)], capture_output=True, text=True,
                         check=True).stdout
    have = {l.split()[-1] for l in out.splitlines()}
    assert NEW_SYMBOLS <= have and NEW_SYMBOLS <= set(abi.EXPORTED)
    f = abi.lib().rpgpu_produce_scratch_bytes
    assert 0 < f(0, 0) and f(1000, 1) < f(1 << 20, 1) < 256 << 20
    assert f(1000, 1) <= f(1000, 1000)


def test_header_hand_vectors_equal_the_model():
    """The vectors written in include/rpgpu.h's comment are the model's output."""
    text = (ROOT / "include" / "rpgpu.h").read_text()
    sec = text[text.index("produce batches from records"):]
    for key, want in pr.MURMUR_VECTORS.items():
        assert re.search(r'"%s" %08x' % (re.escape(key.decode()), want), sec), key
    for part, body in pr.HAND_BODIES:
        hexed = " ".join(f"{x:02x}" for x in body)
        assert re.search(r"partition %d \([r0-4, ]+\)\s+%s" % (part, hexed), sec), part
