"""Legacy (magic 0 / 1) MessageSets -> v2 batches, CPU half (no GPU needed):

* the restatement tests/legacy_sets.py on the hand vector of include/rpgpu.h
  and on CRC32("123456789"); its batches validate OK through the oracle;
* the shared core redpanda_amd/csrc/rpgpu_legacy.h compiled for the host
  (tests/native/legacy_host.cpp) over a seeded corpus: verdict, deciding
  message, codec, record count, timestamp and records body equal the
  restatement's; the same program once more under ASan + UBSan, stand-alone;
* the mutation corpus of the GPU test reaches every verdict (asserted on the
  restatement's side);
* rpgpu_legacy_kafka_error_code against produce.cc:440-489 restated.
The device half is tests/test_gpu_legacy_sets.py."""
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import kafka_batches as kb
import legacy_sets as ls
import oracle.oracle as orc

ROOT = Path(__file__).resolve().parents[1]
NOW = 1_700_000_123_456

HAND_A = bytes.fromhex("0000000000000000" "00000018" "5eaf63dc" "01" "00" "00000174876e8000"
                       "00000001" "6b" "00000001" "76")
HAND_B = bytes.fromhex("0000000000000001" "00000010" "fd6ebddb" "00" "00" "ffffffff" "00000002" "6869")
HAND_BODY = bytes.fromhex("10 00 00 00 02 6b 02 76 00 10 00 00 02 01 04 68 69 00".replace(" ", ""))


def test_hand_vector_through_the_restatement():
    assert zlib.crc32(b"123456789") == 0xCBF43926
    assert zlib.crc32(HAND_A[16:]) == 0x5EAF63DC
    assert ls.message(b"k", b"v", magic=1, ts=1_600_000_000_000, offset=0) == HAND_A
    assert ls.message(None, b"hi", magic=0, offset=1) == HAND_B
    v, ev, codec, batch = ls.convert(HAND_A + HAND_B, NOW)
    assert (v, ev, codec) == (ls.V_OK, -1, 0)
    assert batch[61:] == HAND_BODY
    h = np.frombuffer(batch[:61], dtype=orc.RP_HEADER_DTYPE)[0]
    assert (h["size_bytes"], h["base_offset"], h["type"], h["attrs"]) == (61 + 18, 0, 1, 0)
    assert (h["last_offset_delta"], h["record_count"]) == (1, 2)
    assert h["first_timestamp"] == h["max_timestamp"] == 1_600_000_000_000
    assert (h["producer_id"], h["producer_epoch"], h["base_sequence"]) == (-1, -1, -1)
    # an empty set is an empty batch with last_offset_delta -1 and T = now
    v, ev, codec, batch = ls.convert(b"", NOW)
    h = np.frombuffer(batch[:61], dtype=orc.RP_HEADER_DTYPE)[0]
    assert v == ls.V_OK and len(batch) == 61
    assert (h["last_offset_delta"], h["record_count"], h["first_timestamp"]) == (-1, 0, NOW)


def test_restated_batches_validate_through_the_oracle():
    rng = np.random.default_rng(7)
    sets = [HAND_A + HAND_B, b""] + [ls.message_set(ls.random_set(rng, n)) for n in (1, 5, 64, 200)]
    batches, counts = [], []
    for s in sets:
        v, _, _, batch = ls.convert(s, NOW)
        assert v == ls.V_OK
        batches.append(batch)
        counts.append(struct.unpack_from("<i", batch, 57)[0])
    data, descs = kb.arena(batches, fmt=kb.DISK)
    res, index, used = orc.validate_arena(data, descs)
    assert (res["verdict"] == 0).all()
    assert list(res["index_count"]) == counts
    assert list(res["record_count"]) == counts


def _corpus():
    rng = np.random.default_rng(11)
    sets = [HAND_A + HAND_B, b"", HAND_A[:7], HAND_A + HAND_B[:15]]
    sets += ls.mutation_corpus(0x1E6AC7, 600)
    sets += [ls.message_set(ls.random_set(rng, n, 5000)) for n in (63, 64, 65, 129)]
    return sets


def _expected_lines(sets):
    lines = []
    for s in sets:
        v, ev, codec, batch = ls.convert(s, -1)     # the program prints -1 where now_ms would go
        if v != ls.V_OK:
            lines.append(f"{v} {ev} {codec}")
        else:
            h = np.frombuffer(batch[:61], dtype=orc.RP_HEADER_DTYPE)[0]
            lines.append(f"0 -1 0 {h['record_count']} {h['first_timestamp']} {len(batch) - 61} "
                         f"{zlib.crc32(batch[61:])}")
    return lines


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_shared_core_on_the_host_matches_the_restatement(tmp_path, sanitize):
    sets = _corpus()
    corpus = tmp_path / "corpus.bin"
    with open(corpus, "wb") as f:
        f.write(struct.pack("<I", len(sets)))
        for s in sets:
            f.write(struct.pack("<I", len(s)) + s)
    exe = tmp_path / "legacy_host"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run(["g++", *flags, "-std=c++17", f"-I{ROOT / 'redpanda_amd' / 'csrc'}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "legacy_host.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe), str(corpus)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    want = _expected_lines(sets)
    assert len(got) == len(want)
    bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, bad[:5]


def verdict_histogram(sets):
    hist = {}
    for s in sets:
        v = ls.convert(s, NOW)[0]
        hist[v] = hist.get(v, 0) + 1
    return hist


def test_mutation_corpus_reaches_every_verdict():
    sets = ls.mutation_corpus(0x1E6AC7, 4000)
    hist = verdict_histogram(sets)
    for v in (ls.V_OK,) + ls.LEGACY_VERDICTS:
        assert hist.get(v, 0) >= 20, (v, hist)
    assert hist[ls.V_OK] <= len(sets) // 2, hist


# produce.cc:440-489 restated for a partition whose adapter ran adapt_with_version(version < 3)
def reference_code(verdict: int, size_bytes: int, batch_max_bytes: int) -> int:
    if verdict == ls.V_NULL_RECORDS:                       # !part.records
        return 87
    if verdict in (ls.V_LEGACY_TRUNC_THROW, ls.V_LEGACY_BAD_CODEC_THROW):
        return -1                                          # an exception escapes the decoder
    if verdict in (ls.V_LEGACY_MAGIC, ls.V_LEGACY_CRC_MISMATCH, ls.V_LEGACY_LZ4_MAGIC0,
                   ls.V_LEGACY_NULL_COMPRESSED):
        return 87                                          # adapter.legacy_error
    if verdict == ls.V_LEGACY_COMPRESSED:
        return 0x10000                                     # the nested set decides: routed, not guessed
    if verdict == ls.V_OK:                                 # valid_crc, v2_format set by the adapter
        return 10 if batch_max_bytes and size_bytes > batch_max_bytes else 0
    return -1


def test_legacy_kafka_error_code_map(built):
    from redpanda_amd import abi, engine

    assert sorted(abi.LEGACY_VERDICT_NAMES) == list(ls.LEGACY_VERDICTS)
    assert not set(abi.LEGACY_VERDICT_NAMES) & set(abi.VERDICT_NAMES)
    assert abi.LEGACY_ROUTE_TO_REFERENCE == 0x10000 and not -32768 <= abi.LEGACY_ROUTE_TO_REFERENCE <= 32767
    assert abi.ABI_VERSION == 6 == abi.lib().rpgpu_abi_version()
    lres = np.zeros(1, dtype=abi.LEGACY_RESULT_DTYPE)
    out = np.zeros(1, dtype=abi.RESULT_DTYPE)
    for v in (abi.V_OK, abi.V_NULL_RECORDS, abi.V_DECOMP_OVERFLOW, abi.V_BAD_MAGIC) + ls.LEGACY_VERDICTS:
        for size, mx in ((1000, 0), (1000, 999), (1000, 1000), (1 << 20, 1 << 20)):
            lres["verdict"], out["size_bytes"] = v, size
            assert engine.Engine.legacy_kafka_error_code(lres, out, mx) == reference_code(v, size, mx), (v, size, mx)
    lres["verdict"] = abi.V_OK
    assert engine.Engine.legacy_kafka_error_code(lres, None, 0) == 0
