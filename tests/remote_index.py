"""The tiered-storage offset index in Python: the model that the host program
(tests/native/rsindex_host.cpp over redpanda_amd/csrc/rpgpu_dfor.h) and the
device entry points (rpgpu_rsindex_*) are compared against, byte for byte.

Restated from the reference (paths relative to src/v/), written apart from
rpgpu_dfor.h: bit strings are Python integers here, the encoders keep lists.
  utils/delta_for.h                          delta_xor, delta_delta, the row format
  cloud_storage/remote_segment_index.cc      offset_index add / to_iobuf / from_iobuf /
                                             find_rp_offset / find_kaf_offset,
                                             remote_segment_index_builder
  serde/serde.h:515-565                      the envelope, vectors and iobufs of to_iobuf
"""
from __future__ import annotations

import random
import struct
from dataclasses import dataclass, field

import numpy as np

from redpanda_amd import abi

M64 = (1 << 64) - 1
ROW = 16
MIN_BLOB = 478
CONFIG_TYPES = (2, 19)  # raft_configuration, archival_metadata

OK, NO_ROOM, BAD_BATCH, DELTA_ASSERT = range(4)
FOUND, NONE, BAD_BLOB = range(3)


def s64(x: int) -> int:
    x &= M64
    return x - (1 << 64) if x >> 63 else x


class DeltaAssert(Exception):
    """delta_delta::encode's vasserts (delta_for.h:86-96)."""


class BadBlob(Exception):
    pass


# ------------------------------------------------------------------ delta-FOR
def row_encode(buf: list[int], nbits: int) -> bytes:
    """deltafor_encoder::pack (delta_for.h:515-764) behind the nbits byte."""
    assert len(buf) == ROW and all(0 <= b <= M64 for b in buf) and all(b >> nbits == 0 for b in buf)
    out = bytearray([nbits])
    if nbits == 64:
        for b in buf:
            out += b.to_bytes(8, "little")
        return bytes(out)
    vals, left = list(buf), nbits
    for width in (32, 16, 8):
        if left >= width:
            for i in range(ROW):
                out += (vals[i] & ((1 << width) - 1)).to_bytes(width // 8, "little")
                vals[i] >>= width
            left -= width
    if left:
        bits = 0
        for i in range(ROW):
            bits |= (vals[i] & ((1 << left) - 1)) << (i * left)
        out += bits.to_bytes(2 * left, "little")
    return bytes(out)


def row_decode(data: bytes, at: int) -> tuple[list[int], int]:
    """deltafor_decoder::unpack: the 16 deltas of the row at data[at], and the next row's place."""
    nbits = data[at]
    if nbits > 64 or at + 1 + 2 * nbits > len(data):
        raise BadBlob("row leaves its stream")
    p = at + 1
    if nbits == 64:
        return [int.from_bytes(data[p + 8 * i:p + 8 * i + 8], "little") for i in range(ROW)], p + 128
    vals, left, shift = [0] * ROW, nbits, 0
    for width in (32, 16, 8):
        if left >= width:
            nb = width // 8
            for i in range(ROW):
                vals[i] |= int.from_bytes(data[p + nb * i:p + nb * i + nb], "little") << shift
            p += ROW * nb
            shift += width
            left -= width
    if left:
        bits = int.from_bytes(data[p:p + 2 * left], "little")
        for i in range(ROW):
            vals[i] |= ((bits >> (i * left)) & ((1 << left) - 1)) << shift
        p += 2 * left
    return vals, p


class Encoder:
    """deltafor_encoder<int64_t> with delta_xor (step None) or delta_delta(step)."""

    def __init__(self, initial: int, step: int | None = None):
        self.initial = self.last = initial
        self.step = step
        self.data = bytearray()
        self.rows = 0
        self.nbits: list[int] = []

    def deltas(self, row: list[int]) -> list[int]:
        p, buf = self.last, []
        for v in row:
            if self.step is None:
                buf.append((v ^ p) & M64)
            else:
                if v < p or s64(v - p) < self.step:
                    raise DeltaAssert(f"{v} after {p}, step {self.step}")
                buf.append((v - p - self.step) & M64)
            p = v
        return buf

    def add(self, row: list[int]):
        buf = self.deltas(row)
        agg = 0
        for b in buf:
            agg |= b
        nbits = agg.bit_length()
        self.data += row_encode(buf, nbits)
        self.nbits.append(nbits)
        self.last = row[-1]
        self.rows += 1


def decode_stream(data: bytes, rows: int, initial: int, step: int | None) -> list[int]:
    """Every value a deltafor_decoder reads from `rows` rows."""
    out, p, at = [], initial, 0
    for _ in range(rows):
        if at >= len(data):
            raise BadBlob("row chain leaves its stream")
        vals, at = row_decode(data, at)
        for d in vals:
            p = s64(d ^ (p & M64)) if step is None else s64(d + p + step)
            out.append(p)
    return out


# --------------------------------------------------------------- offset_index
@dataclass
class Found:
    status: int
    from_write_buffer: int = 0
    ix: int = 0
    rp_offset: int = 0
    kaf_offset: int = 0
    file_pos: int = 0

    def tuple(self):
        return (self.status, self.from_write_buffer, self.ix, self.rp_offset, self.kaf_offset, self.file_pos)


class OffsetIndex:
    def __init__(self, base_rp: int, base_kaf: int, file_pos_step: int, base_file: int = 0):
        self.wb = [[0] * ROW for _ in range(3)]
        self.pos = 0
        self.step = file_pos_step
        self.enc = [Encoder(base_rp), Encoder(base_kaf), Encoder(base_file, file_pos_step)]
        self.samples: list[tuple[int, int, int]] = []
        self._decoded = None

    def add(self, rp: int, kaf: int, fpos: int):
        ix = self.pos & (ROW - 1)
        self.pos += 1
        for s, v in enumerate((rp, kaf, fpos)):
            self.wb[s][ix] = v
        self.samples.append((rp, kaf, fpos))
        if self.pos & (ROW - 1) == 0:
            for s in range(3):
                self.enc[s].add(self.wb[s])

    def to_bytes(self) -> bytes:
        body = struct.pack("<qQ", self.step, self.pos)
        for e in self.enc:
            body += struct.pack("<qq", e.initial, e.last)
        for s in range(3):
            body += struct.pack("<I16q", ROW, *self.wb[s])
        for e in self.enc:
            body += struct.pack("<I", len(e.data)) + bytes(e.data)
        return struct.pack("<BBI", 1, 1, len(body)) + body

    @classmethod
    def from_bytes(cls, blob: bytes) -> "OffsetIndex":
        """from_iobuf over exactly to_iobuf's layout; anything else is BadBlob."""
        if len(blob) < MIN_BLOB or blob[0] != 1 or blob[1] != 1:
            raise BadBlob("envelope")
        if struct.unpack_from("<I", blob, 2)[0] + 6 != len(blob):
            raise BadBlob("size")
        step, pos, brp, lrp, bkaf, lkaf, bfile, lfile = struct.unpack_from("<qQ6q", blob, 6)
        x = cls(brp, bkaf, step, bfile)
        x.pos = pos
        for s in range(3):
            if struct.unpack_from("<I", blob, 70 + 132 * s)[0] != ROW:
                raise BadBlob("write buffer count")
            x.wb[s] = list(struct.unpack_from("<16q", blob, 74 + 132 * s))
        at = 466
        for s, last in enumerate((lrp, lkaf, lfile)):
            if at + 4 > len(blob):
                raise BadBlob("stream length")
            n = struct.unpack_from("<I", blob, at)[0]
            at += 4
            if at + n > len(blob):
                raise BadBlob("stream")
            x.enc[s].data = bytearray(blob[at:at + n])
            x.enc[s].rows = pos // ROW
            x.enc[s].last = last
            at += n
        if at != len(blob):
            raise BadBlob("trailing bytes")
        x._decoded = [decode_stream(bytes(x.enc[s].data), pos // ROW, x.enc[s].initial, None if s < 2 else step)
                      for s in range(3)]
        return x

    def decoded(self, s: int) -> list[int]:
        if self._decoded is None:
            self._decoded = [decode_stream(bytes(e.data), e.rows, e.initial, e.step) for e in self.enc]
        return self._decoded[s]

    def find(self, by_rp: bool, upper_bound: int) -> Found:
        """find_rp_offset / find_kaf_offset through maybe_find_offset and _find_under."""
        q = 0 if by_rp else 1
        rows = self.enc[q].rows
        cand = None
        for ix, o in enumerate(self.decoded(q)):          # _find_under
            if o >= upper_bound:
                break
            cand = (ix, o)
        if cand is None or cand[0] == rows * ROW - 1:
            hit = None
            for i in range(self.pos & (ROW - 1)):
                if self.wb[q][i] < upper_bound:
                    hit = i
                else:
                    break
            if hit is not None:
                return Found(FOUND, 1, hit, self.wb[0][hit], self.wb[1][hit], self.wb[2][hit])
            if cand is None:
                return Found(NONE)
        ix = cand[0]
        return Found(FOUND, 0, ix, self.decoded(0)[ix], self.decoded(1)[ix], self.decoded(2)[ix])


def find_in_blob(blob: bytes, by_rp: bool, upper_bound: int) -> Found:
    try:
        return OffsetIndex.from_bytes(blob).find(by_rp, upper_bound)
    except BadBlob:
        return Found(BAD_BLOB)


# -------------------------------------------------------------------- builder
@dataclass
class Header:
    """What the builder reads of an on-disk batch header."""
    size_bytes: int
    base_offset: int
    type: int = 1
    last_offset_delta: int = 0
    # how the descriptor is forged: "wire" (not on-disk format), "short" (length < 61), None
    bad: str | None = None


@dataclass
class Segment:
    name: str
    headers: list[Header]
    base_rp: int = 0
    base_kaf: int = 0
    initial_delta: int = 0
    file_pos_step: int = 0
    sampling_step: int = 0
    past_end: int = 0  # batch_count exceeds the descriptors by this many (last segment only)


@dataclass
class Built:
    status: int = OK
    samples: int = 0
    rows: int = 0
    config_batches: int = 0
    bad_batch: int = 0
    rp_bytes: int = 0
    kaf_bytes: int = 0
    file_bytes: int = 0
    out_bytes: int = 0
    final_delta: int = 0
    stream_bytes: int = 0
    out_offset: int = 0
    blob: bytes = b""
    index: OffsetIndex | None = None
    sample_batches: list[int] = field(default_factory=list)  # batch number within the segment
    deferred: int = 0  # configuration batches met with a full window


def build_segment(seg: Segment, first_batch: int = 0) -> Built:
    """remote_segment_index_builder over the segment's headers, then to_iobuf."""
    b = Built()
    x = OffsetIndex(seg.base_rp, seg.base_kaf, seg.file_pos_step)
    delta, window, pos = seg.initial_delta, 0, 0
    try:
        for k, h in enumerate(seg.headers + [None] * seg.past_end):
            if h is None or h.bad is not None or h.size_bytes < 61:
                b.status, b.bad_batch = BAD_BATCH, first_batch + k
                break
            if h.type in CONFIG_TYPES:
                delta = s64(delta + h.last_offset_delta + 1)
                b.config_batches += 1
                b.deferred += window >= seg.sampling_step
            elif window >= seg.sampling_step:
                x.add(h.base_offset, s64(h.base_offset - delta), pos)
                b.sample_batches.append(k)
                window = 0
            window += h.size_bytes
            pos += h.size_bytes
    except DeltaAssert:
        # the reference aborts; the rows in front of the assertion do not matter
        full = build_segment(Segment(seg.name, seg.headers, seg.base_rp, seg.base_kaf, seg.initial_delta,
                                     -(1 << 62), seg.sampling_step, seg.past_end), first_batch)
        if full.status == OK:  # a bad batch behind the assertion still names the segment BAD_BATCH
            full.status = DELTA_ASSERT
        full.blob, full.index = b"", None
        full.rp_bytes = full.kaf_bytes = full.file_bytes = full.out_bytes = 0
        return full
    b.samples, b.rows = x.pos, x.pos // ROW
    b.final_delta, b.stream_bytes, b.index = delta, pos, x
    if b.status == OK:
        b.blob = x.to_bytes()
        b.rp_bytes, b.kaf_bytes, b.file_bytes = (len(e.data) for e in x.enc)
        b.out_bytes = len(b.blob)
        assert b.out_bytes == MIN_BLOB + b.rp_bytes + b.kaf_bytes + b.file_bytes
    return b


# ---------------------------------------------------------------------- arenas
@dataclass
class Case:
    segments: list[Segment]

    def arena(self):
        """(data, descs, segs): every batch is its 61-byte header alone, size_bytes forged."""
        hs = [h for s in self.segments for h in s.headers]
        hdr = np.zeros(len(hs), dtype=abi.RP_HEADER_DTYPE)
        hdr["size_bytes"] = [h.size_bytes for h in hs]
        hdr["base_offset"] = [h.base_offset for h in hs]
        hdr["type"] = [h.type for h in hs]
        hdr["last_offset_delta"] = [h.last_offset_delta for h in hs]
        hdr["record_count"] = 1
        data = np.frombuffer(hdr.tobytes(), dtype=np.uint8).copy()
        descs = np.zeros(len(hs), dtype=abi.DESC_DTYPE)
        descs["offset"] = np.arange(len(hs), dtype=np.uint64) * abi.HEADER_SIZE
        descs["length"] = [60 if h.bad == "short" else abi.HEADER_SIZE for h in hs]
        descs["format"] = [abi.FMT_KAFKA_WIRE if h.bad == "wire" else abi.FMT_RP_DISK for h in hs]
        segs = np.zeros(len(self.segments), dtype=abi.RSINDEX_SEGMENT_DTYPE)
        first = 0
        for i, s in enumerate(self.segments):
            segs[i] = (first, len(s.headers) + s.past_end, s.base_rp, s.base_kaf, s.initial_delta, s.file_pos_step,
                       s.sampling_step)
            first += len(s.headers)
        return data, descs, segs

    def expected(self) -> list[Built]:
        out, first, off = [], 0, 0
        for s in self.segments:
            b = build_segment(s, first)
            b.out_offset = off
            off += (b.out_bytes + 15) & ~15
            first += len(s.headers)
            out.append(b)
        return out


def totals(exp: list[Built]) -> tuple[int, int]:
    """d_totals: the smallest out_cap that holds every OK blob, the OK segments' samples."""
    ok = [b for b in exp if b.status == OK]
    return max((b.out_offset + b.out_bytes for b in ok), default=0), sum(b.samples for b in ok)


def expected_results(exp: list[Built], out_cap: int | None = None) -> np.ndarray:
    r = np.zeros(len(exp), dtype=abi.RSINDEX_RESULT_DTYPE)
    for i, b in enumerate(exp):
        st = b.status
        if out_cap is not None and st == OK and b.out_offset + b.out_bytes > out_cap:
            st = NO_ROOM
        r[i] = (st, b.samples, b.rows, b.config_batches, b.bad_batch, b.rp_bytes, b.kaf_bytes, b.file_bytes,
                b.out_bytes, 0, b.final_delta, b.stream_bytes, b.out_offset)
    return r


def expected_out(exp: list[Built], out_cap: int, fill: int, guard: int) -> np.ndarray:
    out = np.full(out_cap + guard, fill, dtype=np.uint8)
    for b in exp:
        if b.status == OK and b.out_offset + b.out_bytes <= out_cap:
            out[b.out_offset:b.out_offset + b.out_bytes] = np.frombuffer(b.blob, dtype=np.uint8)
    return out


# the host program's files (tests/native/rsindex_host.cpp)
def write_build_input(path, data, descs, segs):
    with open(path, "wb") as f:
        f.write(struct.pack("<IIQ", len(descs), len(segs), len(data)))
        f.write(descs.tobytes() + segs.tobytes() + data.tobytes())


def read_build_output(path, nsegs: int):
    raw = open(path, "rb").read()
    tot = struct.unpack_from("<QQ", raw, 0)
    res = np.frombuffer(raw, dtype=abi.RSINDEX_RESULT_DTYPE, count=nsegs, offset=16).copy()
    at, blobs = 16 + 64 * nsegs, []
    for r in res:
        n = int(r["out_bytes"]) if r["status"] == OK else 0
        blobs.append(raw[at:at + n])
        at += n
    assert at == len(raw)
    return tot, res, blobs


def write_find_input(path, queries: list[tuple[bytes, bool, int]]):
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(queries)))
        for blob, by_rp, bound in queries:
            f.write(struct.pack("<IIq", len(blob), int(by_rp), bound) + blob)


def read_found(path, nq: int) -> list[tuple]:
    a = np.fromfile(path, dtype=abi.RSINDEX_FOUND_DTYPE)
    assert len(a) == nq
    return [(int(r["status"]), int(r["from_write_buffer"]), int(r["ix"]), int(r["rp_offset"]), int(r["kaf_offset"]),
             int(r["file_pos"])) for r in a]


def write_rows_input(path, rows: list[tuple[int | None, int, list[int]]]):
    """(step or None for delta_xor, prev, the 16 values) per row."""
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(rows)))
        for step, prev, vals in rows:
            f.write(struct.pack("<Iqq16q", 0 if step is None else 1, step or 0, prev, *vals))


# ---------------------------------------------------------------- hand vector
def hand_vector() -> Segment:
    hs, off = [], 1000
    for k in range(60):
        cfg = k == 7
        hs.append(Header(100 + k % 3, off, 2 if cfg else 1, 2 if cfg else 0))
        off += 3 if cfg else 1
    return Segment("hand", hs, base_rp=1000, base_kaf=990, initial_delta=10, file_pos_step=150, sampling_step=150)


# ---------------------------------------------------------------------- sweep
def _uniform(name, nb, size=100, **kw) -> Segment:
    return Segment(name, [Header(size, 5000 + k) for k in range(nb)], base_rp=5000, base_kaf=5000, **kw)


def _xor_widths(name, base: int, initial_delta: int, rng: random.Random) -> Segment:
    """Row w of the rp stream has nbits w, for w in 0..64 (step 0: every batch is a sample)."""
    hs, cur = [], base
    for w in range(65):
        for _ in range(ROW):
            if w:
                cur = s64((cur & M64) ^ ((1 << (w - 1)) | rng.getrandbits(w - 1)))
            hs.append(Header(61 + rng.randrange(64), cur))
    hs += [Header(70, s64(cur + 1 + k)) for k in range(5)]   # an unflushed tail
    return Segment(name, hs, base_rp=base, base_kaf=s64(base - initial_delta), initial_delta=initial_delta,
                   file_pos_step=0, sampling_step=0)


def _file_widths(name, rng: random.Random) -> Segment:
    """Row w of the file stream has nbits w, for w in 0..31 (sampling_step 1: every batch
    but the first is a sample, so a sample's delta is the size of the batch in front)."""
    step, hs = 61, []
    for w in range(32):
        for i in range(ROW):
            d = 0
            if w:
                d = rng.getrandbits(w - 1) | ((1 << (w - 1)) if i == w % ROW else rng.getrandbits(1) << (w - 1))
                d = min(d, (1 << 31) - 1 - step)
            hs.append(Header(step + d, 9000 + len(hs)))
    hs.append(Header(61, 9000 + len(hs)))
    return Segment(name, hs, base_rp=9000, base_kaf=9000, file_pos_step=step, sampling_step=1)


def build_sweep() -> Case:
    rng = random.Random(20221)
    S: list[Segment] = []
    # sample counts 0, 1, 15, 16, 17, 63, 64, 65, 1024, 1025, 1043; step 0: one per batch
    for c in (0, 1, 15, 16, 17, 63, 64, 65, 1024, 1025, 1043):
        S.append(_uniform(f"samples{c}", c, sampling_step=0, file_pos_step=-5))
    # sampling_step equal to the batch size: every batch but the first; 129 batches
    S.append(_uniform("step_eq_size", 129, size=100, sampling_step=100, file_pos_step=100))
    S.append(_uniform("step1", 65, size=61, sampling_step=1, file_pos_step=61))
    # more than 4,096 batches, trips without a sample, samples in lane 0 and lane 63
    S.append(Segment("long", [Header(100 + k % 7, 100000 + 2 * k) for k in range(4200)], base_rp=100000,
                     base_kaf=99000, initial_delta=1000, file_pos_step=20000, sampling_step=20000))
    S.append(Segment("one", [Header(77, 42)], base_rp=42, base_kaf=40, initial_delta=2, sampling_step=0))
    # configuration batches: a run across the trip boundary, types 2 and 19, one where the window fills
    hs = []
    for k in range(200):
        t = (2 if k % 2 else 19) if 60 <= k <= 68 or k in (3, 130) else 1
        hs.append(Header(100, 7000 + 3 * k, t, 2 if t != 1 else 0))
    S.append(Segment("config_run", hs, base_rp=7000, base_kaf=6990, initial_delta=10, file_pos_step=300,
                     sampling_step=300))
    S.append(Segment("config_only", [Header(90, 10 + 4 * k, 2 if k % 3 else 19, 3) for k in range(70)],
                     base_rp=10, base_kaf=10, sampling_step=0))
    S.append(Segment("other_types", [Header(80, 300 + k, (1, 7, 99, -5, 3, 7)[k % 6]) for k in range(40)],
                     base_rp=300, base_kaf=300, file_pos_step=80, sampling_step=80))
    # every XOR width on both streams (initial_delta 0: the Kafka values are the rp values), 64 needs
    # a sign change; then the same rows under a delta and a negative base
    S.append(_xor_widths("xor_widths", 1 << 40, 0, rng))
    S.append(_xor_widths("xor_widths_neg", -(1 << 50), 12345, rng))
    S.append(_file_widths("file_widths", rng))
    # statuses
    S.append(_uniform("delta_assert", 40, size=90, sampling_step=0, file_pos_step=100))
    S.append(_uniform("delta_tail_zero", 10, size=90, sampling_step=0, file_pos_step=100))
    S.append(Segment("delta_tail", [Header(100 if k < 18 else 61, 50 + k) for k in range(22)], base_rp=50,
                     base_kaf=50, file_pos_step=100, sampling_step=61))
    for kind in ("wire", "short"):
        hs = [Header(100, 60 + k) for k in range(70)]
        hs[66].bad = kind
        S.append(Segment(f"bad_{kind}", hs, base_rp=60, base_kaf=60, sampling_step=0))
    hs = [Header(100, 60 + k) for k in range(20)]
    hs[0].size_bytes = 60
    S.append(Segment("bad_size_first", hs, base_rp=60, base_kaf=60, sampling_step=0))
    hs = [Header(100, 60 + k) for k in range(130)]
    hs[128].size_bytes = -1
    S.append(Segment("bad_size_late", hs, base_rp=60, base_kaf=60, sampling_step=150, file_pos_step=150))
    # past one scan block of segments, empty ones among them
    while len(S) < 1025:
        i = len(S)
        nb = (0, 1, 3, 18)[i % 4]
        S.append(Segment(f"small{i}", [Header(61 + (i + k) % 50, 1000 * i + 2 * k, 2 if k == 1 else 1, 1)
                                       for k in range(nb)],
                         base_rp=1000 * i, base_kaf=1000 * i - i, initial_delta=i, file_pos_step=61,
                         sampling_step=(61, 0, 200)[i % 3] if nb != 18 else 61))
    # the last one names descriptors past the arena
    S.append(Segment("past_end", [Header(100, 60 + k) for k in range(5)], base_rp=60, base_kaf=60, sampling_step=0,
                     file_pos_step=-1, past_end=3))
    return Case(S)


def assert_sweep_classes(case: Case, exp: list[Built]):
    """The geometry classes the device kernels branch on (rpgpu_rsindex.hip), from the model alone.

    File-stream widths above 31 cannot be reached through summed int32 size_bytes
    within a test-sized arena: the host program covers them (and delta_delta up to
    64 bits) through its `rows` mode, tests/test_remote_index.py."""
    segs = case.segments
    assert len(segs) == 1026 and any(not s.headers for s in segs)
    samples = {b.samples for b in exp}
    assert {0, 1, 15, 16, 17, 63, 64, 65, 1024, 1025, 1043} <= samples, sorted(samples)
    counts = {len(s.headers) for s in segs}
    assert {0, 1, 63, 64, 65, 129} <= counts and max(counts) > 4096
    lanes, full_trip, empty_trip = set(), False, False
    for s, b in zip(segs, exp):
        per_trip = {}
        for k in b.sample_batches:
            lanes.add(k % 64)
            per_trip[k // 64] = per_trip.get(k // 64, 0) + 1
        ntrips = (len(s.headers) + 63) // 64
        full_trip |= any(v == 64 for v in per_trip.values())
        empty_trip |= b.status == OK and any(t not in per_trip for t in range(ntrips)) and b.samples > 0
    assert {0, 63} <= lanes and full_trip and empty_trip
    steps = {s.sampling_step for s in segs}
    assert {0, 1} <= steps
    assert any(s.headers and s.sampling_step == s.headers[0].size_bytes and b.samples for s, b in zip(segs, exp))
    by_name = {s.name: (s, b) for s, b in zip(segs, exp)}
    s, b = by_name["config_run"]
    cfg = [k for k, h in enumerate(s.headers) if h.type in CONFIG_TYPES]
    assert {63, 64} <= set(cfg) and {s.headers[k].type for k in cfg} == {2, 19}
    assert b.deferred > 0 and b.status == OK and b.samples
    s, b = by_name["config_only"]
    assert b.config_batches == len(s.headers) and b.samples == 0 and b.status == OK
    s, b = by_name["other_types"]
    sampled_types = {s.headers[k].type for k in b.sample_batches}
    assert 7 in sampled_types and sampled_types - {1, 7, 2, 19, 3}, sampled_types
    for name in ("xor_widths", "xor_widths_neg"):
        s, b = by_name[name]
        assert set(b.index.enc[0].nbits) == set(range(65)), name
        assert any(h.base_offset < 0 for h in s.headers)
    s, b = by_name["xor_widths"]
    assert s.initial_delta == 0 and set(b.index.enc[1].nbits) == set(range(65))
    s, b = by_name["file_widths"]
    assert set(b.index.enc[2].nbits) == set(range(32)), sorted(set(b.index.enc[2].nbits))
    assert by_name["delta_assert"][1].status == DELTA_ASSERT
    for name in ("delta_tail", "delta_tail_zero"):
        s, b = by_name[name]
        assert b.status == OK
        prev, offending = 0, []
        for i, (_, _, f) in enumerate(b.index.samples):
            if f - prev < s.file_pos_step:
                offending.append(i)
            prev = f
        assert offending and min(offending) >= b.rows * ROW, (name, offending)
    kinds = {name: by_name[name][1] for name in ("bad_wire", "bad_short", "bad_size_first", "bad_size_late", "past_end")}
    assert all(b.status == BAD_BATCH for b in kinds.values())
    assert kinds["bad_size_first"].samples == 0 and kinds["bad_wire"].samples == 66
    assert any(b.status == OK and b.samples and b.samples % ROW == 0 for b in exp)
    assert any(b.status == OK and b.samples and b.rows == 0 for b in exp)


# -------------------------------------------------------------------- queries
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def sweep_queries(case: Case, exp: list[Built], dense: int = 130, sparse: int = 40) -> list[tuple[int, bool, int]]:
    """(segment, by_rp, upper_bound): every sample value and value +- 1 on both columns
    (segments of more than `dense` samples: about `sparse` evenly spaced samples and
    the ones around the last row's end; of the 1,000 small segments every eighth),
    below the first, above the last, and the ends of the int64 range."""
    out = []
    for i, (s, b) in enumerate(zip(case.segments, exp)):
        if b.status != OK or (s.name.startswith("small") and i % 8):
            continue
        smp = b.index.samples
        pick = set(range(len(smp)))
        if len(smp) > dense:
            pick = set(range(0, len(smp), len(smp) // sparse)) | {len(smp) - 1}
            pick |= {k for k in range(b.rows * ROW - 2, b.rows * ROW + 2) if 0 <= k < len(smp)}
        for by_rp in (True, False):
            col = 0 if by_rp else 1
            bounds = {I64_MIN, I64_MAX, 0}
            for k in pick:
                v = smp[k][col]
                bounds |= {max(v - 1, I64_MIN), v, min(v + 1, I64_MAX)}
            if smp:
                bounds |= {max(min(t[col] for t in smp) - 5, I64_MIN), min(max(t[col] for t in smp) + 5, I64_MAX)}
            out += [(i, by_rp, x) for x in sorted(bounds)]
    return out


def bad_blobs(blob: bytes) -> dict[str, bytes]:
    """One blob per RPGPU_RSINDEX_BAD_BLOB kind, from a blob with at least one row."""
    b = bytearray(blob)
    rp_len = struct.unpack_from("<I", b, 466)[0]
    assert struct.unpack_from("<Q", b, 14)[0] >= ROW and rp_len > 0

    def edit(at, fmt, v, src=b):
        c = bytearray(src)
        struct.pack_into(fmt, c, at, v)
        return bytes(c)

    return {
        "version": edit(0, "<B", 2), "compat": edit(1, "<B", 0),
        "size_field": edit(2, "<I", len(b) - 5),
        "truncated": bytes(b[:-1]),
        "short": edit(2, "<I", 400 - 6, b[:400]),
        "count": edit(202, "<I", 15),
        "stream_length": edit(466, "<I", rp_len + 1),
        "stream_length_past": edit(466, "<I", len(b)),
        "nbits": edit(470, "<B", 65),
        "chain": edit(14, "<Q", struct.unpack_from("<Q", b, 14)[0] + 1024),
        "row_past_stream": edit(470, "<B", min(b[470] + 1, 64)) if b[470] < 64 else edit(14, "<Q", 1 << 40),
    }
