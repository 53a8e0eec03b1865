"""The log append restated serially in Python (test infrastructure, independent
of the engine), and the cases the CPU and the GPU tests share.

Reference: disk_log_appender::operator() (storage/disk_log_appender.cc:71-135),
segment::append (storage/segment.cc:507-531), disk_header_to_iobuf and
storage::write (storage/segment_appender_utils.cc:28-61).  The model walks the
eligible batches of each log in descriptor order exactly as include/rpgpu.h
("log append") states it; headers are built with struct and header_crc comes
from oracle.internal_header_only_crc."""
from __future__ import annotations

import random
import struct

import numpy as np

import kafka_batches as kb
import oracle.oracle as orc

WIRE, DISK = kb.WIRE, kb.DISK
I64_MIN = -(1 << 63)
U32_MAX = 0xFFFFFFFF
V_OK = 0
GHOST_TYPE = 7                       # model::record_batch_type::ghost_batch
OP_CRC, OP_HDRCRC = 1, 2

ROLL_FIRST = 1                       # RPGPU_APPEND_ROLL_FIRST
SKIPPED, APPENDED, GHOST = 0, 1, 2   # rpgpu_append_batch.action
OK, NO_ROOM, BAD_CONFIG = 0, 1, 2    # rpgpu_append_log_result.status
SEG_ROLLED = 1                       # RPGPU_APPEND_SEG_ROLLED

LOG_DTYPE = np.dtype([("next_offset", "<i8"), ("file_offset", "<u8"), ("max_segment_size", "<u8"),
                      ("flags", "<u4"), ("reserved", "<u4")])
BATCH_DTYPE = np.dtype([("action", "<i4"), ("out_row", "<u4"), ("base_offset", "<i8"), ("file_pos", "<u8"),
                        ("segment", "<u4"), ("reserved", "<u4")])
LOG_RESULT_DTYPE = np.dtype([("status", "<i4"), ("batches", "<u4"), ("ghosts", "<u4"), ("segments", "<u4"),
                             ("first_row", "<u4"), ("first_segment", "<u4"), ("base_offset", "<i8"),
                             ("last_offset", "<i8"), ("next_offset", "<i8"), ("byte_size", "<u8"),
                             ("out_offset", "<u8")])
SEGMENT_DTYPE = np.dtype([("log", "<u4"), ("flags", "<u4"), ("first", "<u4"), ("count", "<u4"),
                          ("base_offset", "<i8"), ("file_pos", "<u8"), ("out_offset", "<u8"), ("bytes", "<u8")])
assert (LOG_DTYPE.itemsize, BATCH_DTYPE.itemsize, LOG_RESULT_DTYPE.itemsize, SEGMENT_DTYPE.itemsize) == (32, 32, 64, 48)


def wrap64(v: int) -> int:
    return (v + (1 << 63)) % (1 << 64) - (1 << 63)


def sort_passes(nlogs: int) -> int:
    """8-bit digits of the largest sort key, the sentinel nlogs: ceil(log2(nlogs + 1) / 8)."""
    return (max(nlogs.bit_length(), 1) + 7) // 8


def disk_header(raw: bytes, fmt: int, size: int, base: int, btype: int) -> bytes:
    """disk_header_to_iobuf: the 61 bytes written for a batch whose input header is raw[:61]."""
    tail = struct.unpack((">" if fmt == WIRE else "<") + "Ihiqqqhii", raw[17:61])
    le = struct.pack("<iqbIhiqqqhii", size, base, btype, *tail)
    hdr = np.frombuffer(bytes(4) + le, dtype=orc.RP_HEADER_DTYPE)
    return struct.pack("<I", orc.internal_header_only_crc(hdr)) + le


def error_codes(results: np.ndarray, batch_max_bytes: int) -> np.ndarray:
    """rpgpu_kafka_error_code as far as the append looks at it: nonzero = not appended."""
    ok = results["verdict"] == V_OK
    big = (results["size_bytes"].astype(np.int64) > batch_max_bytes) if batch_max_bytes else np.zeros(len(results), bool)
    return np.where(ok, np.where(big, 10, 0), 87).astype(np.int32)


def model(data: np.ndarray, descs: np.ndarray, results: np.ndarray, logs: np.ndarray, part_lo: int = 0,
          codes=None, out_cap: int | None = None, rows_cap: int | None = None, seg_cap: int | None = None) -> dict:
    """The append of one arena.  Returns rows (per descriptor), log_results,
    segments (rows of the logs that fit, others zero), totals, regions (per log:
    the bytes its files receive), out_descs / out_results (rows of the logs that
    fit), src (per output row: the input descriptor)."""
    n, nlogs = len(descs), len(logs)
    raw = np.ascontiguousarray(data, dtype=np.uint8).tobytes()
    rows = np.zeros(n, dtype=BATCH_DTYPE)
    rows["out_row"] = U32_MAX
    per_log: list[list[int]] = [[] for _ in range(nlogs)]
    for i in range(n):
        log = int(descs["partition"][i]) - part_lo
        if results["verdict"][i] == V_OK and 0 <= log < nlogs and (codes is None or codes[i] == 0) \
                and logs["max_segment_size"][log] != 0:
            per_log[log].append(i)
    lres = np.zeros(nlogs, dtype=LOG_RESULT_DTYPE)
    regions, seg_rows, out_rows = [], [], []       # per log
    for log in range(nlogs):
        lg = logs[log]
        mx, fo = int(lg["max_segment_size"]), int(lg["file_offset"])
        idx, last, byte_size, ghosts = int(lg["next_offset"]), I64_MIN, 0, 0
        left = 0 if int(lg["flags"]) & ROLL_FIRST else max(mx - fo, 0)
        pos = fo
        region, segs, written = bytearray(), [], []
        for i in per_log[log]:
            base = idx
            if left == 0:                                        # needs_to_roll_log
                segs.append(dict(log=log, flags=SEG_ROLLED, first=len(written), count=0, base_offset=idx, file_pos=0,
                                 out_offset=len(region), bytes=0))
                pos, left = 0, mx
            elif not segs:                                       # the continuing segment
                segs.append(dict(log=log, flags=0, first=0, count=0, base_offset=idx, file_pos=fo, out_offset=0,
                                 bytes=0))
            r, d = results[i], descs[i]
            lod, size, fmt = int(r["last_offset_delta"]), int(r["size_bytes"]), int(d["format"])
            if fmt == DISK and int(r["type"]) == GHOST_TYPE:
                rows[i] = (GHOST, U32_MAX, base, pos, len(segs) - 1, 0)
                ghosts += 1
            else:
                off = int(d["offset"])
                btype = 1 if fmt == WIRE else int(r["type"])
                hdr = disk_header(raw[off:off + 61], fmt, size, base, btype)
                rows[i] = (APPENDED, len(written), base, pos, len(segs) - 1, 0)
                written.append((i, len(region), hdr, btype))
                region += hdr + raw[off + 61:off + size]
                segs[-1]["count"] += 1
                segs[-1]["bytes"] += size
                pos += size
                byte_size += size
                left -= min(left, size)
            last = wrap64(base + lod)
            idx = wrap64(last + 1)
        assert byte_size == len(region)
        lres[log] = (BAD_CONFIG if mx == 0 else OK, len(written), ghosts, len(segs), 0, 0, int(lg["next_offset"]),
                     last, idx, byte_size, 0)
        regions.append(bytes(region))
        seg_rows.append(segs)
        out_rows.append(written)
    # layout: exclusive scans over the logs, regions on 16-byte boundaries
    cur = row = seg = need = 0
    for log in range(nlogs):
        lres["out_offset"][log], lres["first_row"][log], lres["first_segment"][log] = cur, row, seg
        if len(regions[log]):
            need = cur + len(regions[log])
        cur += (len(regions[log]) + 15) & ~15
        row += len(out_rows[log])
        seg += len(seg_rows[log])
    totals = np.array([need, row, seg], dtype=np.uint64)
    out_cap = need if out_cap is None else out_cap
    rows_cap = row if rows_cap is None else rows_cap
    seg_cap = seg if seg_cap is None else seg_cap
    segments = np.zeros(seg, dtype=SEGMENT_DTYPE)
    out_descs = np.zeros(row, dtype=orc.DESC_DTYPE)
    out_results = np.zeros(row, dtype=orc.RESULT_DTYPE)
    src = np.full(row, -1, dtype=np.int64)
    for log in range(nlogs):
        lr = lres[log]
        o0, r0, s0 = int(lr["out_offset"]), int(lr["first_row"]), int(lr["first_segment"])
        for i in per_log[log]:
            if rows["out_row"][i] != U32_MAX:
                rows["out_row"][i] += r0
            rows["segment"][i] += s0
        if lr["status"] == BAD_CONFIG:
            continue
        fits = (lr["byte_size"] == 0 or o0 + int(lr["byte_size"]) <= out_cap) and \
            (lr["batches"] == 0 or r0 + int(lr["batches"]) <= rows_cap) and \
            (lr["segments"] == 0 or s0 + int(lr["segments"]) <= seg_cap)
        if not fits:
            lres["status"][log] = NO_ROOM
            continue
        for k, sg in enumerate(seg_rows[log]):
            segments[s0 + k] = (log, sg["flags"], sg["first"] + r0, sg["count"], sg["base_offset"], sg["file_pos"],
                                sg["out_offset"] + o0, sg["bytes"])
        for k, (i, at, hdr, btype) in enumerate(out_rows[log]):
            size = int(results["size_bytes"][i])
            out_descs[r0 + k] = (o0 + at, size, descs["partition"][i], DISK, OP_CRC | OP_HDRCRC, 0, 0)
            res = results[i].copy()
            res["base_offset"] = rows["base_offset"][i]
            res["header_crc"] = struct.unpack("<I", hdr[:4])[0]
            res["type"] = btype
            out_results[r0 + k] = res
            src[r0 + k] = i
    return dict(rows=rows, log_results=lres, segments=segments, totals=totals, regions=regions, out_descs=out_descs,
                out_results=out_results, src=src, per_log=per_log)


def expected_out(m: dict, size: int, fill: int) -> np.ndarray:
    """The output buffer: `fill` everywhere but in the regions of the OK logs."""
    out = np.full(size, fill, dtype=np.uint8)
    for lr, region in zip(m["log_results"], m["regions"]):
        if lr["status"] == OK and region:
            a = int(lr["out_offset"])
            out[a:a + len(region)] = np.frombuffer(region, dtype=np.uint8)
    return out


# ---- building blocks ---------------------------------------------------------------
def body_bytes(n: int, salt: int) -> bytes:
    return bytes((salt * 31 + 7 * i + (i >> 8)) & 255 for i in range(n))


def raw_batch(nbody: int, salt: int = 0, fmt: int = WIRE, lod: int = 0, codec: int = 0, btype: int = 1, **kw) -> bytes:
    """A batch whose body is nbody arbitrary bytes (validated with CRC | HDRCRC only: the records are not walked)."""
    return kb.batch(body_bytes(nbody, salt), fmt=fmt, record_count=lod + 1, lod=lod, attrs=codec, btype=btype,
                    base_offset=1000 + salt, pid=salt, bseq=salt * 3, **kw)


class Case:
    """Batches in arrival order with their partitions, and the logs' state."""

    def __init__(self, nlogs: int, part_lo: int = 0):
        self.nlogs, self.part_lo = nlogs, part_lo
        self.batches: list[bytes] = []
        self.fmts: list[int] = []
        self.parts: list[int] = []
        self.trail: list[int] = []
        self.kinds: list[str] = []
        self.logs = np.zeros(nlogs, dtype=LOG_DTYPE)
        self.logs["max_segment_size"] = 1 << 30
        self.logs["next_offset"] = np.arange(nlogs) * 1000 + 5

    def add(self, log: int, b: bytes, fmt: int = WIRE, trail: int = 0, kind: str = "ok"):
        self.batches.append(b)
        self.fmts.append(fmt)
        self.parts.append(self.part_lo + log)
        self.trail.append(trail)
        self.kinds.append(kind)

    def set_log(self, log: int, next_offset: int, file_offset: int, max_segment_size: int, flags: int = 0):
        self.logs[log] = (next_offset, file_offset, max_segment_size, flags, 0)

    def reorder(self, order):
        for name in ("batches", "fmts", "parts", "trail", "kinds"):
            v = getattr(self, name)
            setattr(self, name, [v[i] for i in order])

    def arena(self):
        offs, cur = [], 0
        for b, t in zip(self.batches, self.trail):
            offs.append(cur)
            cur += len(b) + t
        data = np.full(cur + 64, 0xEE, dtype=np.uint8)
        data[cur:] = 0
        for o, b in zip(offs, self.batches):
            data[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
        descs = np.zeros(len(self.batches), dtype=orc.DESC_DTYPE)
        descs["offset"] = offs
        descs["length"] = [len(b) + t for b, t in zip(self.batches, self.trail)]
        descs["partition"] = self.parts
        descs["format"] = self.fmts
        descs["ops"] = OP_CRC | OP_HDRCRC
        return data, descs


POOL = None


def pool():
    """Small wire batches of 1..3 records, built once."""
    global POOL
    if POOL is None:
        POOL = [kb.batch([kb.record(b"k%d" % j, body_bytes(3 + 5 * (s % 7), s + j), off_delta=j, ts_delta=j)
                          for j in range(1 + s % 3)], base_offset=77 + s, pid=s) for s in range(16)]
    return POOL


GROUP_COUNTS = [0, 1, 63, 64, 65, 128, 129]
BODY_SIZES = [0, 1, 15, 16, 17, 63, 64, 65, 3000, (1 << 20) + 77]


def grouping_case(nlogs: int, counts: dict[int, int], order: str, part_lo: int, seed: int = 1) -> Case:
    c = Case(nlogs, part_lo)
    p = pool()
    per = {log: [p[(log + k) % len(p)] for k in range(m)] for log, m in counts.items()}
    # batches of the partitions just outside [part_lo, part_lo + nlogs)
    outside = [(-1, p[1]), (nlogs, p[2]), (-1, p[3]), (nlogs, p[4])] if part_lo else [(nlogs, p[2]), (nlogs, p[4])]
    seq: list[tuple[int, bytes]] = []
    if order == "round-robin":
        k = 0
        while any(k < len(v) for v in per.values()):
            seq += [(log, v[k]) for log, v in sorted(per.items()) if k < len(v)]
            k += 1
    else:                                           # blocks in reverse log order (shuffled below if asked)
        for log in sorted(per, reverse=True):
            seq += [(log, b) for b in per[log]]
    step = max(len(seq) // len(outside), 1)
    for j, o in enumerate(outside):
        seq.insert(min(j * step, len(seq)), o)
    if order == "shuffle":
        random.Random(seed).shuffle(seq)
    for log, b in seq:
        c.add(log, b, kind="ok" if 0 <= log < nlogs else "outside")
    return c


def build_sweep() -> dict[str, Case]:
    cases: dict[str, Case] = {}
    # ---- grouping: one, two and three digit passes
    cases["group-1"] = grouping_case(1, {0: 4097}, "round-robin", part_lo=0)
    cases["group-3"] = grouping_case(3, {0: 129, 2: 64}, "round-robin", part_lo=7)
    cases["group-256"] = grouping_case(256, {k: GROUP_COUNTS[k % 7] if k < 14 else (k % 3 == 0) for k in range(256)},
                                       "reverse", part_lo=1000)
    cases["group-257"] = grouping_case(257, {k: GROUP_COUNTS[(k + 3) % 7] if k > 249 else (k % 5 == 0)
                                             for k in range(257)}, "shuffle", part_lo=0xFFFF0000)
    cases["group-70000"] = grouping_case(70000, {0: 65, 255: 1, 256: 63, 257: 2, 65535: 64, 65536: 3, 69999: 129},
                                         "shuffle", part_lo=3, seed=2)
    # ---- rolls
    c = Case(12, part_lo=40)
    p = pool()
    sz = len(p[0])
    for log in range(12):
        if log not in (8, 10):
            for k in range(200 if log == 0 else 9):
                c.add(log, p[0] if log in (1, 2) else p[(log + k) % 16])
    c.set_log(0, 100, 0, 1)                             # every batch rolls (>= 3 rolls in one 64-batch step)
    c.set_log(1, 200, 0, 3 * sz)                        # lands exactly on max: the 4th batch rolls, not the 3rd
    c.set_log(2, 300, sz, 4 * sz)                       # the same from a file offset
    c.set_log(3, 400, 0, 150)
    c.set_log(4, 500, 149, 150)                         # file_offset = max - 1
    c.set_log(5, 600, 150, 150)                         # = max: rolls first
    c.set_log(6, 700, 155, 150)                         # = max + 5: rolls first
    c.set_log(7, 800, 10, 1 << 20, ROLL_FIRST)          # ROLL_FIRST with batches
    c.set_log(8, 900, 10, 1 << 20, ROLL_FIRST)          # ... without: never rolls
    c.set_log(9, -50, 0, 0)                             # BAD_CONFIG with batches
    c.set_log(10, 7, 0, 0)                              # BAD_CONFIG without
    c.set_log(11, (1 << 62), 1 << 40, (1 << 40) + 200)  # large offsets and positions
    order = list(range(len(c.batches)))
    random.Random(3).shuffle(order)
    c.reorder(order)
    cases["rolls"] = c
    # ---- bytes: body sizes, alignments, trailing bytes, codecs
    c = Case(2, part_lo=0)
    for k, nb in enumerate(BODY_SIZES):
        c.add(k % 2, raw_batch(nb, salt=k, lod=k % 3), trail=(k * 5) % 4)
    for k in range(17):                                 # one trailing byte each: (dst - src) mod 16 takes every value
        c.add(0, raw_batch(100 + k, salt=20 + k), trail=1)
    for codec in (1, 2, 3, 4):
        c.add(1, raw_batch(90 + codec, salt=40 + codec, codec=codec, lod=2))
    c.set_log(0, 0, 0, 1 << 19)
    c.set_log(1, 1 << 40, 123, 4096)
    cases["bytes"] = c
    # ---- filtering: corrupt batches between good ones, sizes on both sides of a batch_max_bytes
    c = Case(3, part_lo=5)
    for k in range(60):
        log = k % 3
        if k % 7 == 3:
            c.add(log, kb.batch([kb.record(b"k", b"v")], crc=0x12345678), kind="crc")
        elif k % 11 == 5:
            c.add(log, kb.batch([kb.record(b"k", b"v")], magic=1), kind="magic")
        else:
            c.add(log, raw_batch(20 + 30 * (k % 5), salt=k, lod=k % 4))
    c.set_log(0, 10, 0, 400)
    c.set_log(1, 20, 0, 1 << 20)
    c.set_log(2, 30, 50, 300, ROLL_FIRST)
    cases["filter"] = c
    # ---- on-disk input: types 1, 2 and the ghost batch
    c = Case(4, part_lo=0)
    d = lambda nb, salt, btype=1, lod=0: raw_batch(nb, salt=salt, fmt=DISK, btype=btype, lod=lod)   # noqa: E731
    fill = len(d(39, 0))                                # 100 bytes
    c.add(0, d(0, 1, GHOST_TYPE, lod=4), DISK)          # a ghost first, at left == 0: the row opens at its offset
    c.add(0, d(39, 2), DISK)
    c.add(0, d(10, 3, GHOST_TYPE, lod=9), DISK)         # a ghost between written batches
    c.add(0, d(39, 4, btype=2, lod=1), DISK)
    c.add(1, d(39, 5), DISK)                            # fills the segment exactly ...
    c.add(1, d(39, 6, btype=2), DISK)
    c.add(1, d(5, 7, GHOST_TYPE, lod=2), DISK)          # ... so the trailing ghost rolls: a segment with count == 0
    c.add(2, d(7, 8, GHOST_TYPE, lod=0), DISK)          # a ghost first with room left: the continuing row
    c.add(2, d(20, 9, lod=3), DISK)
    c.add(3, raw_batch(33, salt=10, lod=1), WIRE)       # wire and disk input side by side
    c.add(3, d(33, 11, btype=2), DISK)
    c.set_log(0, 1000, 0, 1 << 20, ROLL_FIRST)
    c.set_log(1, 2000, 0, 2 * fill)
    c.set_log(2, 3000, 64, 1 << 20)
    c.set_log(3, 4000, 0, 1 << 20)
    cases["disk"] = c
    return cases


def assert_sweep_classes(cases: dict[str, Case], models: dict[str, dict]) -> None:
    """Every class of the sweep is present, from the cases and the model alone."""
    assert {sort_passes(c.nlogs) for c in cases.values()} >= {1, 2, 3}
    assert [sort_passes(k) for k in (1, 3, 255, 256, 257, 65535, 65536, 70000)] == [1, 1, 1, 2, 2, 2, 3, 3]
    assert {cases[k].nlogs for k in ("group-1", "group-3", "group-256", "group-257", "group-70000")} == \
        {1, 3, 256, 257, 70000}
    counts = set()
    for name, m in models.items():
        if name.startswith("group-"):
            counts |= {len(v) for v in m["per_log"]}
            assert any(k == "outside" for k in cases[name].kinds)
            lo, hi = cases[name].part_lo, cases[name].part_lo + cases[name].nlogs
            assert hi in cases[name].parts and (lo == 0 or lo - 1 in cases[name].parts)
    assert counts >= {0, 1, 63, 64, 65, 128, 129, 4097}
    assert sum(c.part_lo != 0 for c in cases.values()) >= 3
    # rolls
    c, m = cases["rolls"], models["rolls"]
    lr, sg = m["log_results"], m["segments"]
    assert c.logs["max_segment_size"][0] == 1 and lr["segments"][0] == lr["batches"][0] == 200
    for log in (1, 2):                                   # exactly full, then the roll in front of the next batch
        s = sg[sg["log"] == log]
        fo = int(c.logs["file_offset"][log])
        assert int(s["bytes"][0]) + fo == int(c.logs["max_segment_size"][log]) and s["flags"][1] == SEG_ROLLED
        assert s["flags"][0] == 0 and s["file_pos"][0] == fo
    mx = 150
    assert [int(v) for v in c.logs["file_offset"][3:7]] == [0, mx - 1, mx, mx + 5]
    assert [int(sg[sg["log"] == k]["flags"][0]) for k in (3, 4, 5, 6)] == [0, 0, SEG_ROLLED, SEG_ROLLED]
    assert lr["segments"][7] == 1 and sg[sg["log"] == 7]["flags"][0] == SEG_ROLLED
    assert (lr["segments"][8], lr["batches"][8], lr["last_offset"][8], lr["next_offset"][8]) == (0, 0, I64_MIN, 900)
    assert list(lr["status"][[9, 10]]) == [BAD_CONFIG, BAD_CONFIG] and lr["batches"][9] == 0
    assert (m["rows"]["action"][np.array(c.parts) == c.part_lo + 9] == SKIPPED).all()
    # bytes
    c, m = cases["bytes"], models["bytes"]
    data, descs = c.arena()
    bodies = {len(b) - 61 for b in c.batches}
    assert bodies >= set(BODY_SIZES) and max(bodies) > 1 << 20
    src = descs["offset"][m["src"]].astype(np.int64) + 61
    dst = m["out_descs"]["offset"].astype(np.int64) + 61
    big = m["out_descs"]["length"] >= 61 + 32
    assert set(((dst - src) % 16)[big]) == set(range(16))
    assert any(c.trail) and {int(r["codec"]) for r in m["out_results"]} >= {0, 1, 2, 3, 4}
    # filtering
    assert {"crc", "magic", "ok"} <= set(cases["filter"].kinds)
    # on-disk input
    c, m = cases["disk"], models["disk"]
    rows, sg = m["rows"], m["segments"]
    assert rows["action"][0] == GHOST and sg[0]["flags"] == SEG_ROLLED and sg[0]["base_offset"] == 1000
    assert list(rows["action"][:4]) == [GHOST, APPENDED, GHOST, APPENDED]
    s1 = sg[sg["log"] == 1]
    assert len(s1) == 2 and s1["count"][1] == 0 and s1["bytes"][1] == 0 and rows["action"][6] == GHOST
    s2 = sg[sg["log"] == 2]
    assert s2["flags"][0] == 0 and s2["base_offset"][0] == 3000 and rows["action"][7] == GHOST
    assert {int(t) for t in m["out_results"]["type"]} == {1, 2} and m["log_results"]["ghosts"].sum() == 4


HAND_LOG = dict(next_offset=42, file_offset=0, max_segment_size=64, flags=0)


def hand_vector():
    """The vector of include/rpgpu.h: two wire batches of one log, the second one rolls."""
    c = Case(1)
    c.add(0, kb.batch([kb.record(b"k", b"v1")], base_offset=0, first_ts=1000, pid=1, pepoch=2, bseq=3))
    c.add(0, kb.batch([kb.record(None, b"v2", off_delta=0), kb.record(b"k", None, off_delta=1, ts_delta=1)],
                      base_offset=7, first_ts=2000))
    c.set_log(0, **HAND_LOG)
    return c
