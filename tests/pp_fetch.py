"""The REST proxy's fetch reply restated with Python's json and base64 modules
(test infrastructure, independent of the engine and of oracle/), and the
sweep the CPU and the GPU tests share.

Reference: pandaproxy/json/requests/fetch.h:46-154, pandaproxy/json/iobuf.h:70-89,
the expected string of pandaproxy/json/requests/test/fetch.cc:95-96."""
from __future__ import annotations

import base64
import json
import re
import struct
from pathlib import Path

import numpy as np

import kafka_batches as kb

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "pandaproxy_fetch.json"

OK, BAD_BATCH, COMPRESSED, NOT_INDEXED, BAD_TOPIC, BAD_RANGE, NO_ROOM = range(7)
LANE_FIELD_MAX = 128            # RPGPU_PP_LANE_FIELD_MAX (asserted against the header by the tests)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1

RANGE_DTYPE = np.dtype([("first", "<u4"), ("count", "<u4"), ("topic_off", "<u4"), ("topic_len", "<u2"),
                        ("reserved0", "<u2"), ("partition", "<i4"), ("reserved1", "<u4")])
RESPONSE_DTYPE = np.dtype([("first_range", "<u4"), ("range_count", "<u4")])
RESULT_DTYPE = np.dtype([("out_off", "<u8"), ("out_len", "<u8"), ("records", "<u4"), ("status", "<i4"),
                         ("bad_batch", "<u4"), ("reserved", "<u4")])

TOPIC_RE = re.compile(rb"[A-Za-z0-9._-]{1,249}")


def topic_ok(t: bytes) -> bool:
    """model::validate_kafka_topic_name (model/validation.cc:20-38)."""
    return TOPIC_RE.fullmatch(t) is not None and t not in (b".", b"..")


def b64(x: bytes | None):
    return base64.b64encode(x).decode() if x else None


def wrap64(v: int) -> int:
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def render(objects) -> bytes:
    """objects: (topic str, key, value, partition, offset) in order."""
    return json.dumps([{"topic": t, "key": b64(k), "value": b64(v), "partition": p, "offset": o}
                       for t, k, v, p, o in objects], separators=(",", ":")).encode()


# ---- building blocks ---------------------------------------------------------------
# A batch spec: dict(records=[(key, value)], base=int, kind=...), kind one of
#   ok | control | control_compressed | crc | codec | noindex
# A range spec: (topic bytes, partition, [batch specs]); a response spec: [range specs].
KIND_ATTRS = {"ok": 0, "control": 0x20, "control_compressed": 0x21, "crc": 0, "codec": 1, "noindex": 0}
KIND_STATUS = {"ok": OK, "control": OK, "control_compressed": OK, "crc": BAD_BATCH, "codec": COMPRESSED,
               "noindex": NOT_INDEXED}


def bspec(records, base=0, kind="ok"):
    return dict(records=list(records), base=base, kind=kind)


def pattern(n: int, salt: int) -> bytes | None:
    """n bytes that run through every byte value (-1: a null field)."""
    if n < 0:
        return None
    return bytes((salt + 7 * i + (i >> 8)) & 255 for i in range(n))


class Case:
    """Flattens response specs into an arena, a topics blob, ranges and responses,
    and states what the reference would answer."""

    def __init__(self, fmt: int):
        self.fmt = fmt
        self.batches: list[bytes] = []
        self.ops: list[int] = []
        self.kinds: list[str] = []
        self.ranges: list[tuple[int, int, bytes, int]] = []
        self.responses: list[tuple[int, int]] = []
        self.specs: list = []
        self.names: list[str] = []

    def add(self, name: str, ranges, raw=None):
        """One response.  raw: (first, count) overrides per range position (a range past n)."""
        first_range = len(self.ranges)
        for pos, (topic, partition, batches) in enumerate(ranges):
            first = len(self.batches)
            for s in batches:
                recs = [kb.record(k, v, off_delta=i, ts_delta=i) for i, (k, v) in enumerate(s["records"])]
                kind = s["kind"]
                extra = dict(crc=0x12345678) if kind == "crc" else {}
                self.batches.append(kb.batch(recs, fmt=self.fmt, base_offset=s["base"], attrs=KIND_ATTRS[kind],
                                             btype=1, **extra))
                self.ops.append(7 if kind == "noindex" else 15)
                self.kinds.append(kind)
            fc = (first, len(batches))
            if raw and pos in raw:
                fc = raw[pos]
            self.ranges.append((fc[0], fc[1], topic, partition))
        self.responses.append((first_range, len(ranges)))
        self.specs.append((ranges, raw or {}))
        self.names.append(name)

    # -- the inputs ----------------------------------------------------------------------
    def arena(self):
        data, descs = kb.arena(self.batches, fmt=self.fmt)
        descs["ops"] = self.ops
        return data, descs

    def tables(self):
        """The topics blob, the ranges and the responses."""
        blob, where = b"", {}
        for _, _, t, _ in self.ranges:
            if t not in where:
                where[t] = len(blob)
                blob += t
        rg = np.zeros(len(self.ranges), dtype=RANGE_DTYPE)
        for i, (first, count, t, part) in enumerate(self.ranges):
            rg[i] = (first, count, where[t], len(t), 0, part, 0)
        rs = np.zeros(len(self.responses), dtype=RESPONSE_DTYPE)
        for i, (fr, cnt) in enumerate(self.responses):
            rs[i] = (fr, cnt)
        return blob, rg, rs

    # -- the answer ----------------------------------------------------------------------
    def expected(self):
        """Per response: (status, bad_batch, records, body bytes, fields), fields =
        [(is_value, length, offset of its first character in the body)]."""
        n = len(self.batches)
        out = []
        g = b = 0
        for ranges, raw in self.specs:
            status, bad, objects = OK, 0, []
            for pos, (topic, partition, batches) in enumerate(ranges):
                if status == OK:
                    if not topic_ok(topic):
                        status, bad = BAD_TOPIC, g
                    elif pos in raw and raw[pos][0] + raw[pos][1] > n:
                        status, bad = BAD_RANGE, g
                for j, s in enumerate(batches):
                    if status == OK:
                        st = KIND_STATUS[s["kind"]]
                        if s["kind"] == "noindex" and not s["records"]:
                            st = OK                    # index_count == record_count == 0: nothing is missing
                        if st != OK:
                            status, bad = st, b + j
                        elif s["kind"] == "ok":
                            objects += [(topic.decode(), k, v, partition, wrap64(s["base"] + i))
                                        for i, (k, v) in enumerate(s["records"])]
                g += 1
                b += len(batches)
            if status != OK:
                out.append((status, bad, 0, b"", []))
                continue
            body, fields = b"[", []
            for i, o in enumerate(objects):
                text = render([o])[1:-1]
                at = len(body) + (1 if i else 0)       # the '{'
                kpos = at + 10 + len(o[0]) + 8 + 1
                if o[1]:
                    fields.append((0, len(o[1]), kpos))
                if o[2]:
                    klen = 2 + 4 * ((len(o[1]) + 2) // 3) if o[1] else 4
                    fields.append((1, len(o[2]), kpos - 1 + klen + 9 + 1))
                body += (b"," if i else b"") + text
            body += b"]"
            assert body == render(objects)
            out.append((OK, 0, len(objects), body, fields))
        return out

    def expected_results(self, exp=None, out_cap: int | None = None):
        exp = self.expected() if exp is None else exp
        res = np.zeros(len(exp), dtype=RESULT_DTYPE)
        cur = 0
        for i, (status, bad, records, body, _) in enumerate(exp):
            slot = (len(body) + 15) & ~15
            if status == OK and out_cap is not None and cur + slot > out_cap:
                status = NO_ROOM
            res[i] = (cur, len(body), records, status, bad, 0)
            cur += slot
        return res, cur


# ---- the sweep ---------------------------------------------------------------------
FIELD_LENS = [-1, 0, 1, 2, 3, 4, 5, 11, 12, 13, 15, 16, 17, 47, 48, 49, 63, 64, 65,
              LANE_FIELD_MAX - 1, LANE_FIELD_MAX, LANE_FIELD_MAX + 1, LANE_FIELD_MAX + 2, LANE_FIELD_MAX + 3,
              1023, 1024, 1025, 4096, 65537]
OFFSETS = sorted({0, -1, -10, -(10 ** 18), I64_MAX, I64_MIN, I64_MIN + 1}
                 | {10 ** k - 1 for k in range(1, 19)} | {10 ** k for k in range(1, 19)})
PARTITIONS = [0, 9, 10, -1, I32_MAX, I32_MIN]
TOPIC_LENS = [1, 2, 248, 249]
BAD_TOPICS = [b"", b".", b"..", b"t" * 250, b"a b", b'a"b', b"caf\xc3\xa9"]
BATCH_RECORDS = [0, 1, 63, 64, 65, 200]
RANGE_BATCHES = [0, 1, 63, 64, 65, 130]
RESPONSE_BATCHES = [1023, 1024, 1025, 2600]
MANY_RESPONSES = 1100           # more responses than the slot scan has lanes (1024)
ALIGN_FIELD = LANE_FIELD_MAX + 7  # a wave-path field whose destination is swept over 16 alignments


def small(i: int):
    return (pattern(1 + i % 5, i), pattern(i % 4 - 1, i + 1))


def build_sweep(fmt: int) -> Case:
    c = Case(fmt)
    one = lambda k, v, base=0: bspec([(k, v)], base)                     # noqa: E731
    # field lengths: every length as a key and as a value, null and empty both sides
    c.add("field-lengths", [(b"lens", 3, [bspec([(pattern(a, a), pattern(b, a + b))
                                                 for b in FIELD_LENS[(i % 7):: 7] + [FIELD_LENS[i]]], base=i * 100)
                                          for i, a in enumerate(FIELD_LENS)])])
    # destination alignment of wave-path fields: 16 consecutive topic lengths, key then value
    for tl in range(1, 17):
        c.add(f"align-{tl}", [(b"t" * tl, 7, [one(pattern(ALIGN_FIELD, tl), pattern(ALIGN_FIELD + tl, tl)),
                                              one(None, pattern(ALIGN_FIELD + 5, tl), base=10 ** (tl % 7))])])
    # offsets (base + delta, one wrapped past INT64_MAX) and partitions
    c.add("offsets", [(b"offs", 1, [one(b"k", b"v", base=o) for o in OFFSETS]
                       + [bspec([(b"a", None), (b"b", b"c")], base=I64_MAX)])])
    c.add("partitions", [(b"parts", p, [one(b"k", None, base=5)]) for p in PARTITIONS])
    c.add("topic-lengths", [(bytes(b"Az09._-"[i % 7] for i in range(tl)), 2, [one(b"key", b"value")])
                            for tl in TOPIC_LENS])
    for i, t in enumerate(BAD_TOPICS):
        c.add(f"bad-topic-{i}", [(b"good", 0, [one(b"k", b"v")]), (t, 0, [one(b"k", b"v")])])
    c.add("dots-inside", [(b"a..b", 0, [one(b"k", b"v")]), (b"...", 0, [one(b"k", b"v")])])
    # record counts per batch, batch counts per range
    c.add("batch-records", [(b"recs", 4, [bspec([small(i) for i in range(m)], base=1000 * m)
                                          for m in BATCH_RECORDS])])
    c.add("range-batches", [(b"rb%d" % m, m, [bspec([small(i + m)], base=i) for i in range(m)])
                            for m in RANGE_BATCHES])
    for total in RESPONSE_BATCHES:
        ranges, left, i = [], total, 0
        while left:
            take = min(left, (97, 130, 1, 64)[i % 4])
            ranges.append((b"big%d" % (i % 3), i, [bspec([small(i + j)], base=j) for j in range(take)]))
            left -= take
            i += 1
        c.add(f"response-{total}", ranges)
    # nothing to render
    c.add("no-ranges", [])
    c.add("empty-ranges", [(b"e1", 0, []), (b"e2", 1, [])])
    c.add("control-only", [(b"ctl", 0, [bspec([small(1)], kind="control"), bspec([small(2)], kind="control_compressed")])])
    c.add("empty-batches", [(b"eb", 0, [bspec([]), bspec([])])])
    # control batches first, last and between, one of them compressed
    c.add("control-mixed", [(b"ctl", 2, [bspec([small(1)], kind="control"), bspec([small(2), small(3)], base=7),
                                         bspec([small(4)], kind="control_compressed"), bspec([small(5)], base=9),
                                         bspec([small(6)], kind="control")])])
    # one defect per response
    nine = lambda bad_at, kind: [bspec([small(i)], base=i, kind=kind if i == bad_at else "ok")  # noqa: E731
                                 for i in range(9)]
    for at in (0, 4, 8):
        c.add(f"crc-{at}", [(b"d1", 0, nine(-1, "ok")), (b"d2", 1, nine(at, "crc"))])
    c.add("codec-bits", [(b"d3", 0, nine(3, "codec"))])
    c.add("not-indexed", [(b"d4", 0, nine(5, "noindex"))])
    c.add("noindex-but-empty", [(b"d4", 0, [bspec([], kind="noindex"), bspec([small(1)])])])
    c.add("range-past-n", [(b"d5", 0, nine(-1, "ok")), (b"d5", 1, [])], raw={1: (0xFFFFFFF0, 0x20)})
    c.add("range-at-n", [(b"d5", 1, [])], raw={0: (1 << 30, 1)})
    # two defects: the first in range order, then batch order, wins; a range's own come first
    c.add("two-batches", [(b"p1", 0, nine(6, "codec")), (b"p2", 0, nine(1, "crc"))])
    c.add("two-in-one-range", [(b"p3", 0, [bspec([small(0)]), bspec([small(1)], kind="noindex"),
                                           bspec([small(2)], kind="crc")])])
    c.add("topic-before-batches", [(b"p 4", 0, nine(0, "crc"))])
    c.add("batch-before-later-topic", [(b"p5", 0, nine(8, "crc")), (b"", 0, [])])
    c.add("topic-before-bounds", [(b"..", 0, [])], raw={0: (1 << 30, 1)})
    # many small responses
    for i in range(MANY_RESPONSES):
        c.add(f"many-{i}", [(b"m", i, [bspec([small(i)], base=i)])] if i % 3 else [])
    return c


def assert_sweep_classes(c: Case, exp) -> None:
    """Every class of the sweep is present, from the lists and the model alone."""
    lens = set(FIELD_LENS)
    assert {-1, 0, 1, 2, 3, 4, 5, 11, 12, 13, 15, 16, 17, 47, 48, 49, 63, 64, 65, 1023, 1024, 1025, 4096, 65537} <= lens
    assert {LANE_FIELD_MAX + d for d in (-1, 0, 1, 2, 3)} <= lens
    seen = {(kv, ln) for e in exp for kv, ln, _ in e[4]}
    for ln in lens:
        if ln > 0:
            assert (0, ln) in seen and (1, ln) in seen, ln
    for kv in (0, 1):                                       # all 16 destination alignments on the wave path
        assert {at % 16 for e in exp for k, ln, at in e[4] if k == kv and ln > LANE_FIELD_MAX} == set(range(16)), kv
        assert any(ln <= LANE_FIELD_MAX for e in exp for k, ln, _ in e[4] if k == kv)
    offs = set(OFFSETS)
    assert {10 ** k - 1 for k in range(1, 19)} | {10 ** k for k in range(1, 19)} | {I64_MAX, I64_MIN, -1} <= offs
    assert {len(str(abs(o))) for o in offs} == set(range(1, 20))
    assert set(PARTITIONS) == {0, 9, 10, -1, I32_MAX, I32_MIN}
    assert TOPIC_LENS == [1, 2, 248, 249] and [len(t) for t in BAD_TOPICS[:4]] == [0, 1, 2, 250]
    assert not any(topic_ok(t) for t in BAD_TOPICS) and topic_ok(b"a..b") and topic_ok(b"...")
    assert BATCH_RECORDS == [0, 1, 63, 64, 65, 200] and RANGE_BATCHES == [0, 1, 63, 64, 65, 130]
    by_name = dict(zip(c.names, zip(c.responses, exp)))
    for total in RESPONSE_BATCHES:
        (fr, cnt), e = by_name[f"response-{total}"]
        assert sum(c.ranges[g][1] for g in range(fr, fr + cnt)) == total and e[0] == OK and e[2] == total
    for name in ("no-ranges", "empty-ranges", "control-only", "empty-batches"):
        assert by_name[name][1][3] == b"[]", name
    assert [by_name[f"crc-{at}"][1][:2] for at in (0, 4, 8)] == \
        [(BAD_BATCH, c.ranges[by_name[f"crc-{at}"][0][0] + 1][0] + at) for at in (0, 4, 8)]
    assert by_name["codec-bits"][1][0] == COMPRESSED and by_name["not-indexed"][1][0] == NOT_INDEXED
    assert by_name["range-past-n"][1][0] == BAD_RANGE and by_name["range-at-n"][1][0] == BAD_RANGE
    assert by_name["two-batches"][1][0] == COMPRESSED and by_name["two-in-one-range"][1][0] == NOT_INDEXED
    assert by_name["topic-before-batches"][1][0] == BAD_TOPIC and by_name["batch-before-later-topic"][1][0] == BAD_BATCH
    assert by_name["topic-before-bounds"][1][0] == BAD_TOPIC
    assert by_name["offsets"][1][3].count(str(I64_MIN).encode()) == 2    # as a base offset and as a wrapped sum
    assert len(c.responses) > 1024


# ---- the host program's files (tests/native/pp_host.cpp) ---------------------------------
def write_host_input(path, data, descs, results, index, topics: bytes, ranges, responses) -> None:
    with open(path, "wb") as f:
        f.write(struct.pack("<6IQ", len(descs), len(index), len(topics), len(ranges), len(responses), 0, data.size))
        for a in (data, descs, results, index):
            f.write(np.ascontiguousarray(a).tobytes())
        f.write(topics)
        f.write(ranges.tobytes())
        f.write(responses.tobytes())


def read_host_output(path, nresponses: int):
    raw = Path(path).read_bytes()
    res = np.zeros(nresponses, dtype=RESULT_DTYPE)
    bodies, at = [], 0
    for i in range(nresponses):
        res[i] = np.frombuffer(raw, dtype=RESULT_DTYPE, count=1, offset=at)[0]
        at += RESULT_DTYPE.itemsize
        m = int(res[i]["out_len"]) if res[i]["status"] == OK else 0
        bodies.append(raw[at:at + m])
        at += m
    assert at == len(raw)
    return res, bodies


def golden():
    return json.loads(GOLDEN.read_text())


def golden_case(fmt: int):
    """The reference's own vector and its empty response as a Case, with the expected strings."""
    g = golden()
    unhex = lambda h: None if h is None else bytes.fromhex(h)          # noqa: E731
    c = Case(fmt)
    for key in ("ranges", "empty_ranges"):
        c.add(key, [(r["topic"].encode(), r["partition"],
                     [bspec([(unhex(x["key_hex"]), unhex(x["value_hex"])) for x in b["records"]], base=b["base_offset"])
                      for b in r["batches"]]) for r in g[key]])
    return c, [g["expected"].encode(), g["empty_expected"].encode()]
