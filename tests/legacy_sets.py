"""Legacy (magic 0 / 1) MessageSets: a builder and a Python restatement of the
reference's conversion to a v2 batch.  TEST INFRASTRUCTURE, independent of
the engine: CRC32 is zlib.crc32, the expected batch is built with
kafka_batches.record / kafka_batches.batch(fmt=DISK), whose CRCs come from the
oracle.

Restated (paths relative to the reference's src/v/):
  kafka_batch_adapter::convert_message_set   kafka/protocol/kafka_batch_adapter.cc:215-274
  kafka_batch_adapter::adapt_with_version    kafka/protocol/kafka_batch_adapter.cc:276-301
  decode_legacy_batch                        kafka/protocol/legacy_message.h
  iobuf_parser consume_* (out_of_range)      bytes/details/io_iterator_consumer.h:63-83
  iobuf::share (clamps)                      bytes/iobuf.cc:162-185
  crc::crc32                                 hashing/crc32.h:18-33
"""
from __future__ import annotations

import struct
import zlib

import kafka_batches as kb

V_OK = 0
V_NULL_RECORDS = 1
V_LEGACY_MAGIC = 50
V_LEGACY_CRC_MISMATCH = 51
V_LEGACY_LZ4_MAGIC0 = 52
V_LEGACY_NULL_COMPRESSED = 53
V_LEGACY_TRUNC_THROW = 54
V_LEGACY_BAD_CODEC_THROW = 55
V_LEGACY_COMPRESSED = 56
LEGACY_VERDICTS = (50, 51, 52, 53, 54, 55, 56)


def message(key: bytes | None, value: bytes | None, magic: int = 1, attrs: int = 0, ts: int = 0,
            offset: int = 0, batch_length: int | None = None, crc: int | None = None,
            following: bytes = b"") -> bytes:
    """One legacy message.  batch_length / crc override the true values; with an
    overridden batch_length and crc None, the crc is the CRC32 of the range the
    reference would hash (clamped to this message + `following`, the bytes that
    come after it in the set)."""
    body = bytes([magic & 0xFF, attrs & 0xFF])
    if magic == 1:
        body += struct.pack(">q", ts)
    body += struct.pack(">i", -1 if key is None else len(key)) + (key or b"")
    body += struct.pack(">i", -1 if value is None else len(value)) + (value or b"")
    bl = len(body) + 4 if batch_length is None else batch_length
    if crc is None:
        rest = body + following
        want = bl - 4 if bl >= 4 else len(rest)    # (size_t)batch_length - 4 wraps below 4
        crc = zlib.crc32(rest[:min(want, len(rest))])
    return struct.pack(">qiI", offset, bl, crc & 0xFFFFFFFF) + body


def message_set(msgs: list[dict]) -> bytes:
    """Messages from keyword dicts for message(); built back to front so each
    one's `following` is known."""
    out = b""
    for i in range(len(msgs) - 1, -1, -1):
        kw = dict(msgs[i])
        kw.setdefault("offset", i)
        out = message(following=out, **kw) + out
    return out


class _Throw(Exception):
    pass


def convert(set_bytes: bytes, now_ms: int):
    """(verdict, event_message, codec, batch_bytes) for one non-null set."""
    b = bytes(set_bytes)
    n = len(b)
    pos = 0
    recs: list[bytes] = []
    T = None
    i = 0

    def need(q, k):                                  # consume_*: out_of_range when bytes lack
        if n - q < k:
            raise _Throw()

    while pos < n:                                   # while (parser.bytes_left())
        try:
            need(pos, 8)                             # int64 offset
            need(pos + 8, 4)
            bl = struct.unpack_from(">i", b, pos + 8)[0]
            need(pos + 12, 4)
            crc = struct.unpack_from(">I", b, pos + 12)[0]
            q = pos + 16
            want = bl - 4 if bl >= 4 else 1 << 64    # (size_t)batch_length - 4
            crc_range = b[q:q + min(want, n - q)]    # share_no_consume clamps
            need(q, 1)
            magic = struct.unpack_from(">b", b, q)[0]
            q += 1
            if magic not in (0, 1):
                return V_LEGACY_MAGIC, i, 0, b""
            need(q, 1)
            attrs = b[q]
            q += 1
            ts = None
            if magic == 1:
                need(q, 8)
                ts = struct.unpack_from(">q", b, q)[0]
                q += 8
            if zlib.crc32(crc_range) != crc:
                return V_LEGACY_CRC_MISMATCH, i, 0, b""
            kv = []
            for _ in range(2):                       # key, then value
                need(q, 4)
                sz = struct.unpack_from(">i", b, q)[0]
                q += 4
                if sz == -1:
                    kv.append(None)
                    continue
                if sz < 0 or sz > n - q:             # share clamps, skip throws
                    raise _Throw()
                kv.append(b[q:q + sz])
                q += sz
        except _Throw:
            return V_LEGACY_TRUNC_THROW, i, 0, b""
        pos = q
        if ts is not None:
            T = ts                                   # builder.set_timestamp
        codec = attrs & 7
        if codec >= 4:
            return V_LEGACY_BAD_CODEC_THROW, i, 0, b""   # compression() throws
        if codec:
            if magic == 0 and codec == 3:
                return V_LEGACY_LZ4_MAGIC0, i, 0, b""
            if kv[1] is None:
                return V_LEGACY_NULL_COMPRESSED, i, 0, b""
            return V_LEGACY_COMPRESSED, i, codec, b""
        recs.append(kb.record(kv[0], kv[1], ts_delta=0, off_delta=i))   # add_raw_kv
        i += 1
    T = now_ms if T is None else T
    batch = kb.batch(recs, fmt=kb.DISK, base_offset=0, record_count=len(recs), attrs=0, first_ts=T, max_ts=T,
                     pid=-1, pepoch=-1, bseq=-1, lod=len(recs) - 1, btype=1)
    return V_OK, -1, 0, batch


# ---- seeded corpora ------------------------------------------------------------
def random_set(rng, nmsg: int, max_val: int = 2048) -> list[dict]:
    msgs = []
    for _ in range(nmsg):
        magic = int(rng.integers(0, 2))
        key = None if rng.random() < 0.3 else rng.bytes(int(rng.integers(0, 24)))
        value = None if rng.random() < 0.1 else rng.bytes(int(rng.integers(0, max_val + 1)))
        msgs.append(dict(key=key, value=value, magic=magic, ts=int(rng.integers(1, 1 << 41))))
    return msgs


def mutation_corpus(seed: int, count: int):
    """`count` small sets: ~10 % intact, the others with one mutation, tuned so
    that every verdict 50..56 and OK occurs often (asserted by the tests on the
    restatement's side)."""
    import numpy as np

    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        nmsg = int(rng.integers(1, 41))
        msgs = random_set(rng, nmsg, 2048 if rng.random() < 0.15 else 96)
        r = rng.random()
        j = int(rng.integers(0, nmsg))
        if r < 0.10:
            s = message_set(msgs)
        elif r < 0.22:                               # a byte flip anywhere
            s = bytearray(message_set(msgs))
            s[int(rng.integers(0, len(s)))] ^= 1 << int(rng.integers(0, 8))
            s = bytes(s)
        elif r < 0.34:                               # truncation
            s = message_set(msgs)
            s = s[:int(rng.integers(1, len(s)))]
        elif r < 0.44:                               # magic, covered by a fresh CRC
            msgs[j]["magic"] = int(rng.integers(2, 128))
            s = message_set(msgs)
        elif r < 0.54:                               # codec 4..7
            msgs[j]["attrs"] = int(rng.integers(4, 8)) | (int(rng.integers(0, 2)) << 3)
            s = message_set(msgs)
        elif r < 0.64:                               # magic 0 with lz4
            msgs[j]["magic"], msgs[j]["attrs"] = 0, 3
            s = message_set(msgs)
        elif r < 0.74:                               # compressed, null value
            msgs[j]["attrs"], msgs[j]["value"] = int(rng.integers(1, 3)), None
            s = message_set(msgs)
        elif r < 0.86:                               # a compressed wrapper
            msgs[j]["magic"], msgs[j]["attrs"] = 1, int(rng.integers(1, 4))
            if msgs[j]["value"] is None:
                msgs[j]["value"] = b"\x00"
            s = message_set(msgs)
        elif r < 0.93:                               # length-field edit: key / value size
            s = bytearray(message_set(msgs[:j + 1]))
            tail = message_set(msgs[j + 1:])
            # the last message's value size field sits 4 + len(value) from its end
            v = msgs[j]["value"]
            at = len(s) - 4 - (len(v) if v is not None else 0)
            struct.pack_into(">i", s, at, int(rng.choice([-2, -100, 1 << 20, 0x7FFFFFFF])))
            s = bytes(s) + tail
        else:                                        # batch_length edit, CRC over the clamped range
            msgs[j]["batch_length"] = int(rng.choice([4, 3, 0, -1, 1 << 30]))
            if rng.random() < 0.5:
                msgs[j]["crc"] = int(rng.integers(0, 1 << 32))
            s = message_set(msgs)
        out.append(s)
    return out


def arena(sets: list[bytes | None], align: list[int] | None = None):
    """(data, descs) with set i at an offset of alignment align[i] mod 16;
    None is a null-records descriptor."""
    import numpy as np

    import oracle.oracle as orc

    offs, cur = [], 0
    for i, s in enumerate(sets):
        a = align[i] if align else 0
        cur = ((cur + 15) & ~15) + a
        offs.append(cur)
        cur += len(s) if s is not None else 0
    data = np.zeros(cur + 64, dtype=np.uint8)
    for o, s in zip(offs, sets):
        if s:
            data[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    descs = np.zeros(len(sets), dtype=orc.DESC_DTYPE)
    descs["offset"] = offs
    descs["length"] = [len(s) if s is not None else 0 for s in sets]
    descs["partition"] = np.arange(len(sets)) % 7
    descs["format"] = 0
    descs["ops"] = 15
    descs["flags"] = [1 if s is None else 0 for s in sets]
    return data, descs
