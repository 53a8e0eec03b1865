"""The log-append model (tests/append_log.py) on the CPU: the hand vector of
include/rpgpu.h; every log region the model produces for the sweep read back
through the oracle (the recovery parser accepts exactly the appended batches,
every emitted descriptor validates with the model's header_crc, base offsets
chain from next_offset); the row layouts against the C sizeof."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import append_log as al
import oracle.oracle as orc

ROOT = Path(__file__).resolve().parents[1]

HAND_IN = ("00000000000000000000003b0000000002d00832e900000000000000000000000003e800000000000003e8000000000000000100020000"
           "00030000000112000000026b04763100",
           "0000000000000007000000420000000002d66127c600000000000100000000000007d000000000000007d1ffffffffffffffffffffffff"
           "ffff000000021000000001047632000e000202026b0100")
HAND_OUT = ("af809a44470000002a0000000000000001e93208d0000000000000e803000000000000e8030000000000000100000000000000020003"
            "0000000100000012000000026b04763100",
            "8f4feff44e0000002b0000000000000001c62761d6000001000000d007000000000000d107000000000000ffffffffffffffffffffff"
            "ffffff020000001000000001047632000e000202026b0100")


def validated(case):
    data, descs = case.arena()
    res, _, _ = orc.validate_arena(data, descs)
    return data, descs, res


@pytest.fixture(scope="module")
def sweep():
    cases = al.build_sweep()
    inputs = {k: validated(c) for k, c in cases.items()}
    models = {k: al.model(*inputs[k], cases[k].logs, cases[k].part_lo) for k in cases}
    return cases, inputs, models


def test_hand_vector():
    c = al.hand_vector()
    assert [b.hex() for b in c.batches] == list(HAND_IN)
    data, descs, res = validated(c)
    assert (res["verdict"] == 0).all()
    m = al.model(data, descs, res, c.logs)
    assert m["regions"][0].hex() == "".join(HAND_OUT)
    for h in HAND_OUT:                                   # header_crc is CRC32C of bytes [4, 61)
        raw = bytes.fromhex(h)
        assert int.from_bytes(raw[:4], "little") == orc.crc32c(raw[4:61])
    assert [tuple(int(v) for v in r) for r in m["rows"]] == [(al.APPENDED, 0, 42, 0, 0, 0), (al.APPENDED, 1, 43, 0, 1, 0)]
    assert tuple(int(v) for v in m["log_results"][0]) == (al.OK, 2, 0, 2, 0, 0, 42, 44, 45, 149, 0)
    assert [tuple(int(v) for v in s) for s in m["segments"]] == [(0, 0, 0, 1, 42, 0, 0, 71),
                                                                 (0, al.SEG_ROLLED, 1, 1, 43, 0, 71, 78)]
    assert list(m["totals"]) == [149, 2, 2]
    # the header documents the same bytes
    text = re.sub(r"[\s*]+", "", (ROOT / "include" / "rpgpu.h").read_text())
    assert "in" + "".join(HAND_IN) + "out" + "".join(HAND_OUT) in text


def test_sweep_classes(sweep):
    cases, _, models = sweep
    al.assert_sweep_classes(cases, models)


@pytest.mark.parametrize("name", ["group-1", "group-3", "group-256", "group-257", "group-70000", "rolls", "bytes",
                                  "filter", "disk"])
def test_regions_read_back(sweep, name):
    from redpanda_amd import abi

    cases, inputs, models = sweep
    c, m = cases[name], models[name]
    data, descs, res = inputs[name]
    lr = m["log_results"]
    total = int(m["totals"][0])
    out = np.concatenate([al.expected_out(m, total, 0), np.zeros(64, np.uint8)])
    # the recovery parser accepts exactly the appended batches of each log
    logs = [k for k in range(c.nlogs) if lr["byte_size"][k]]
    reads = np.zeros(len(logs), dtype=abi.SEGMENT_READ_DTYPE)
    reads["offset"] = lr["out_offset"][logs]
    reads["length"] = lr["byte_size"][logs]
    reads["desc_first"] = lr["first_row"][logs]
    reads["desc_cap"] = lr["batches"][logs]
    reads["partition"] = np.array(logs, dtype=np.uint32) + c.part_lo
    reads["mode"] = abi.PARSE_RECOVERY
    reads["ops"] = al.OP_CRC | al.OP_HDRCRC
    pres, pdescs = orc.segment_parse(out, reads)
    assert (pres["status"] == 0).all()
    assert np.array_equal(pres["accepted"], lr["batches"][logs]) and (pres["skipped"] == 0).all()
    assert np.array_equal(pres["bytes_consumed"], lr["byte_size"][logs])
    assert np.array_equal(pdescs.view(np.uint8), m["out_descs"].view(np.uint8))
    # every emitted descriptor validates, with the model's header_crc and base offset
    vres, _, _ = orc.validate_arena(out, m["out_descs"])
    assert (vres["verdict"] == 0).all()
    for f in ("header_crc", "base_offset", "size_bytes", "type", "crc", "last_offset_delta", "attrs", "record_count",
              "first_timestamp", "max_timestamp"):
        assert np.array_equal(vres[f], m["out_results"][f]), f
    assert np.array_equal(m["out_results"]["crc"], res["crc"][m["src"]])
    # base offsets chain from next_offset by lod + 1, ghosts included
    for log, rows in enumerate(m["per_log"]):
        nxt = int(c.logs["next_offset"][log])
        for i in rows:
            assert int(m["rows"]["base_offset"][i]) == nxt
            nxt = al.wrap64(nxt + int(res["last_offset_delta"][i]) + 1)
        assert int(lr["next_offset"][log]) == nxt
        assert int(lr["last_offset"][log]) == (al.wrap64(nxt - 1) if rows else al.I64_MIN)
    # a segment is a contiguous run of rows and of bytes
    for sg in m["segments"]:
        d = m["out_descs"][int(sg["first"]):int(sg["first"]) + int(sg["count"])]
        assert int(d["length"].sum()) == int(sg["bytes"])
        if len(d):
            assert int(d["offset"][0]) == int(sg["out_offset"])


def test_filtering_by_codes(sweep):
    cases, inputs, models = sweep
    c = cases["filter"]
    data, descs, res = inputs["filter"]
    codes = al.error_codes(res, 61 + 80)
    ok = res["verdict"] == 0
    assert (codes[ok] != 0).any() and (codes[ok] == 0).any() and (~ok).any()
    m = al.model(data, descs, res, c.logs, c.part_lo, codes=codes)
    plain = models["filter"]
    assert (m["rows"]["action"][codes != 0] == al.SKIPPED).all() and (m["rows"]["action"][codes == 0] == al.APPENDED).all()
    assert (plain["rows"]["action"][ok] == al.APPENDED).all() and (plain["rows"]["action"][~ok] == al.SKIPPED).all()
    assert m["totals"][1] == (codes == 0).sum() < plain["totals"][1] == ok.sum()


def test_capacity(sweep):
    cases, inputs, _ = sweep
    c = cases["rolls"]
    full = al.model(*inputs["rolls"], c.logs, c.part_lo)
    total, rows, segs = (int(v) for v in full["totals"])
    lr = full["log_results"]
    last = max(k for k in range(c.nlogs) if lr["byte_size"][k])
    for kw, no_room in ((dict(out_cap=total), []), (dict(out_cap=total - 1), [last]),
                        (dict(rows_cap=rows - 1), [max(k for k in range(c.nlogs) if lr["batches"][k])]),
                        (dict(seg_cap=segs - 1), [max(k for k in range(c.nlogs) if lr["segments"][k])]),
                        (dict(out_cap=0), [k for k in range(c.nlogs) if lr["byte_size"][k]])):
        m = al.model(*inputs["rolls"], c.logs, c.part_lo, **kw)
        assert list(np.nonzero(m["log_results"]["status"] == al.NO_ROOM)[0]) == no_room, kw
        keep = [f for f in al.LOG_RESULT_DTYPE.names if f != "status"]
        assert all(np.array_equal(m["log_results"][f], lr[f]) for f in keep)


def test_layouts_match_the_header(tmp_path):
    from redpanda_amd import abi

    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "rpgpu.h"\n'
                   "_Static_assert(RPGPU_ABI_VERSION == 6, \"additive\");\n"
                   "int main(void) {\n"
                   '    printf("%zu %zu %zu %zu\\n", sizeof(rpgpu_append_log), sizeof(rpgpu_append_batch),\n'
                   "           sizeof(rpgpu_append_log_result), sizeof(rpgpu_append_segment));\n"
                   '    printf("%u %d %d %d %d %d %d %u\\n", RPGPU_APPEND_ROLL_FIRST, RPGPU_APPEND_SKIPPED,\n'
                   "           RPGPU_APPEND_APPENDED, RPGPU_APPEND_GHOST, RPGPU_APPEND_OK, RPGPU_APPEND_NO_ROOM,\n"
                   "           RPGPU_APPEND_BAD_CONFIG, RPGPU_APPEND_SEG_ROLLED);\n"
                   "    return 0;\n}\n")
    exe = tmp_path / "sizes"
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    dts = (abi.APPEND_LOG_DTYPE, abi.APPEND_BATCH_DTYPE, abi.APPEND_LOG_RESULT_DTYPE, abi.APPEND_SEGMENT_DTYPE)
    assert [int(v) for v in lines[0].split()] == [d.itemsize for d in dts] == [32, 32, 64, 48]
    assert [int(v) for v in lines[1].split()] == [abi.APPEND_ROLL_FIRST, abi.APPEND_SKIPPED, abi.APPEND_APPENDED,
                                                  abi.APPEND_GHOST, abi.APPEND_OK, abi.APPEND_NO_ROOM,
                                                  abi.APPEND_BAD_CONFIG, abi.APPEND_SEG_ROLLED]
    # the model's own copies name the same fields in the same places
    for mine, theirs in zip((al.LOG_DTYPE, al.BATCH_DTYPE, al.LOG_RESULT_DTYPE, al.SEGMENT_DTYPE), dts):
        assert mine == theirs
    assert (al.ROLL_FIRST, al.SKIPPED, al.APPENDED, al.GHOST, al.OK, al.NO_ROOM, al.BAD_CONFIG, al.SEG_ROLLED) == \
        (abi.APPEND_ROLL_FIRST, abi.APPEND_SKIPPED, abi.APPEND_APPENDED, abi.APPEND_GHOST, abi.APPEND_OK,
         abi.APPEND_NO_ROOM, abi.APPEND_BAD_CONFIG, abi.APPEND_SEG_ROLLED)
