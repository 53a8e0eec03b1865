"""kafka::client::client::produce_records restated in Python (test
infrastructure, independent of the engine): the three partitioners
(kafka/client/partitioners.cc:25-109), murmur2 (hashing/murmur.cc:384-432),
the grouping of client.cc:231-271 and record_batch_builder::build
(storage/record_batch_builder.cc:29-102), with the oracle's CRC32C for the two
checksums; the engine's guard rails and output layout (include/rpgpu.h,
"produce batches from records") on top; and the case builders of
tests/test_produce_records.py and tests/test_gpu_produce_records.py."""
from __future__ import annotations

import struct

import numpy as np

import oracle.oracle as orc
from redpanda_amd import abi

OK, BAD_REQUEST, BAD_ROW, TOO_LARGE, OUT_OVERFLOW = range(5)
ROW_DTYPE, REQUEST_DTYPE = abi.PRODUCE_ROW_DTYPE, abi.PRODUCE_REQUEST_DTYPE  # the rows a case is written in
NONE = 0xFFFFFFFF
INT32_MAX, INT32_MIN = 2**31 - 1, -(2**31)
SEED = 0x9747B28C
TAIL_PAD = 64
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------ murmur2
def murmur2(key: bytes, seed: int = SEED) -> int:
    m, r = 0x5BD1E995, 24
    n = len(key)
    h = (seed ^ n) & M32
    pos = 0
    while n >= 4:
        k = struct.unpack_from("<I", key, pos)[0]
        k = (k * m) & M32
        k ^= k >> r
        k = (k * m) & M32
        h = (h * m) & M32
        h ^= k
        pos += 4
        n -= 4
    if n == 3:
        h ^= key[pos + 2] << 16
    if n >= 2:
        h ^= key[pos + 1] << 8
    if n >= 1:
        h ^= key[pos]
        h = (h * m) & M32
    h ^= h >> 13
    h = (h * m) & M32
    h ^= h >> 15
    return h


# ------------------------------------------------------------- partitioners
class Rec:
    """record_essence: partition_id / key / value, each optional."""

    def __init__(self, partition_id=None, key=None, value=None):
        self.partition_id, self.key, self.value = partition_id, key, value


def identity_partitioner(rec, partition_count):
    return rec.partition_id


def murmur2_key_partitioner(rec, partition_count):
    if rec.key is None or len(rec.key) == 0:
        return None
    return murmur2(rec.key) % partition_count


class RoundRobin:
    def __init__(self, initial):
        self._next = initial

    def __call__(self, rec, partition_count):
        p = self._next % partition_count
        self._next += 1
        return p


class DefaultPartitioner:
    def __init__(self, initial):
        self.rr = RoundRobin(initial)
        self.impls = (identity_partitioner, murmur2_key_partitioner, self.rr)

    def __call__(self, rec, partition_count):
        p_id = None
        for impl in self.impls:
            p_id = p_id if p_id is not None else impl(rec, partition_count)
        return p_id


def partition_for(partitioner, rec, partition_count):
    """topic_cache::partition_for: a topic that is not cached throws topic_error."""
    if partition_count == 0:
        raise KeyError("topic_error")
    return partitioner(rec, partition_count)


# -------------------------------------------------------------------- batch
def zz(v: int) -> bytes:
    return orc.write_varlong(v)


def record(delta: int, key: bytes, value: bytes | None) -> bytes:
    body = b"\x00" + zz(0) + zz(delta) + zz(len(key)) + key
    body += zz(-1 if value is None else len(value)) + (value or b"") + zz(0)
    return zz(len(body)) + body


def build(records: list[tuple[bytes, bytes | None]], now_ms: int) -> bytes:
    """record_batch_builder(raft_data, offset 0)::build() with nothing set: the on-disk batch."""
    body = b"".join(record(d, k, v) for d, (k, v) in enumerate(records))
    n = len(records)
    tail = (0, n - 1, now_ms, now_ms, -1, -1, -1, n)
    crc = orc.crc32c(struct.pack(">hiqqqhii", *tail) + body)
    le = struct.pack("<iqbI", 61 + len(body), 0, 1, crc) + struct.pack("<hiqqqhii", *tail)
    return struct.pack("<I", orc.crc32c(le)) + le + body


def record_size(delta: int, klen: int, vlen: int) -> int:
    """record_batch_builder::record_size plus the length field's own varint."""
    n = 1 + 1 + len(zz(delta)) + len(zz(klen)) + klen + len(zz(vlen)) + max(vlen, 0) + 1
    return len(zz(n)) + n


def produce_records(records: list[Rec], partition_count: int, rr_initial: int):
    """One produce_records call up to the builders.  Returns ([(partition, [row numbers])] in
    the engine's order, rr_next).  The reference's order is absl::node_hash_map's (unpinned)."""
    partitioner = DefaultPartitioner(rr_initial)
    builders: dict[int, list[int]] = {}
    for i, rec in enumerate(records):
        p_id = rec.partition_id
        if p_id is None:
            try:
                p_id = partition_for(partitioner, rec, partition_count)
            except KeyError:
                p_id = 0
        builders.setdefault(p_id, []).append(i)
    return [(p_id, builders[p_id]) for p_id in sorted(builders)], partitioner.rr._next


def build_group(records: list[Rec], rows: list[int], now_ms: int) -> bytes:
    # key.value_or(iobuf{}): an absent key is an empty one
    return build([(records[i].key or b"", records[i].value) for i in rows], now_ms)


def wire(batch: bytes) -> bytes:
    """The Kafka wire form of an on-disk batch (kafka_batch_serializer without terms;
    tests/test_produce_records.py holds it against the oracle's serializer)."""
    size, base, _type, crc = struct.unpack_from("<iqbI", batch, 4)
    tail = struct.unpack_from("<hiqqqhii", batch, 21)
    return struct.pack(">qiib", base, size - 12, WIRE_LEADER_EPOCH, 2) + struct.pack(">I", crc) + \
        struct.pack(">hiqqqhii", *tail) + batch[61:]


WIRE_LEADER_EPOCH = 0  # no terms given: term 0


# -------------------------------------------------------------------- calls
class Call:
    """Builds d_data / rows / requests.  Keys and values are laid into the arena at the
    misalignment asked for (mod 16), with a guard byte pattern between them."""

    def __init__(self):
        self.data = bytearray()
        self.rows, self.reqs, self.recs = [], [], []

    def request(self, partition_count, rr_initial=0, now_ms=1_700_000_000_000, nrows=None):
        self.reqs.append([now_ms, 0, partition_count, rr_initial, nrows])
        return self

    def _put(self, b, align):
        if b is None or len(b) == 0:
            return 0
        if align is not None:
            while len(self.data) % 16 != align:
                self.data.append(0xEE)
        off = len(self.data)
        self.data += b
        return off

    def row(self, key=None, value=None, partition=None, kalign=None, valign=None, raw=None):
        """raw: a dict of row fields that overrides what key / value give (guard-rail cases)."""
        r = dict(key_off=self._put(key, kalign), val_off=self._put(value, valign),
                 key_len=-1 if key is None else len(key), val_len=-1 if value is None else len(value),
                 partition=0 if partition is None else partition,
                 flags=0 if partition is None else abi.PRODUCE_HAS_PARTITION)
        r.update(raw or {})
        self.rows.append(r)
        self.recs.append(Rec(partition, key, value))
        self.reqs[-1][1] += 1
        return self

    def build(self, pad_tail=0):
        rows = np.zeros(len(self.rows), ROW_DTYPE)
        for i, r in enumerate(self.rows):
            for f, v in r.items():
                rows[f][i] = v
        reqs = np.zeros(len(self.reqs), REQUEST_DTYPE)
        for i, (now, n, pc, rr, forced) in enumerate(self.reqs):
            reqs[i] = (now, n if forced is None else forced, pc, rr, 0)
        data = np.frombuffer(bytes(self.data) + b"\xEE" * pad_tail, np.uint8).copy()
        return dict(data=data, rows=rows, requests=reqs, recs=list(self.recs))


def row_ok(r, data_bytes):
    if r["key_len"] < -1 or r["val_len"] < -1:
        return False
    for off, ln in ((int(r["key_off"]), int(r["key_len"])), (int(r["val_off"]), int(r["val_len"]))):
        if ln > 0 and (off > data_bytes or data_bytes - off < ln):
            return False
    return True


def model(data, rows, requests, out_cap=None):
    """What the engine's plan and run leave, from the rows alone (the records are read back
    out of `data`, so a case may be written as raw rows)."""
    raw = np.ascontiguousarray(data, np.uint8).tobytes()
    n, nreq = len(rows), len(requests)
    status = [OK] * nreq
    plans = [None] * nreq
    bad_call = int(requests["nrows"].astype(np.uint64).sum()) != n
    first = 0
    for r in range(nreq):
        q = requests[r]
        cnt, pc, rr0 = int(q["nrows"]), int(q["partition_count"]), int(q["rr_initial"])
        mine = range(first, first + cnt)
        first += cnt
        if bad_call or pc > INT32_MAX or rr0 < 0:
            status[r] = BAD_REQUEST
            continue
        if not all(row_ok(rows[i], len(raw)) for i in mine):
            status[r] = BAD_ROW
            continue
        recs, lens = [], []
        for i in mine:
            w = rows[i]
            ko, kl, vo, vl = int(w["key_off"]), int(w["key_len"]), int(w["val_off"]), int(w["val_len"])
            # a key names its bytes: only the hashed ones are read before the sizes are known
            recs.append(Rec(int(w["partition"]) if int(w["flags"]) & abi.PRODUCE_HAS_PARTITION else None,
                            None if kl < 0 else raw[ko:ko + kl] if kl else b"", (vo, vl)))
            lens.append((max(kl, 0), vl))
        groups, rr_next = produce_records(recs, pc, rr0)
        if rr_next > INT32_MAX:
            status[r] = BAD_REQUEST
            continue
        if any(61 + sum(record_size(d, *lens[i]) for d, i in enumerate(members)) > INT32_MAX for _, members in groups):
            status[r] = TOO_LARGE
            continue
        for rec in recs:
            vo, vl = rec.value
            rec.value = None if vl < 0 else raw[vo:vo + vl] if vl else b""
        plans[r] = ([(p, members, build_group(recs, members, int(q["now_ms"]))) for p, members in groups],
                    rr_next, mine.start)
    # the slots, 64-byte aligned, in request order; the plan's totals
    off = 0
    slots = {}
    for r in range(nreq):
        if plans[r]:
            for g, (_, _, b) in enumerate(plans[r][0]):
                slots[r, g] = off
                off += (len(b) + 63) & ~63
    out_bytes = off
    plan_batches = len(slots)
    cap = out_bytes + TAIL_PAD if out_cap is None else out_cap
    res = np.zeros(nreq, abi.PRODUCE_RESULT_DTYPE)
    batches = []
    row_batch = np.full(n, NONE, np.uint32)
    row_delta = np.full(n, NONE, np.uint32)
    out = np.zeros(cap, np.uint8)
    wire_out = np.zeros(cap, np.uint8)
    for r in range(nreq):
        res["rr_next"][r] = requests["rr_initial"][r]
        if plans[r]:
            groups, rr_next, base = plans[r]
            end = max((slots[r, g] + ((len(b) + 63) & ~63) for g, (_, _, b) in enumerate(groups)), default=0)
            if groups and end + TAIL_PAD > cap:
                status[r] = OUT_OVERFLOW
            else:
                res["rr_next"][r], res["first_batch"][r], res["nbatches"][r] = rr_next, len(batches), len(groups)
                for g, (p_id, members, b) in enumerate(groups):
                    o = slots[r, g]
                    out[o:o + len(b)] = np.frombuffer(b, np.uint8)
                    wire_out[o:o + len(b)] = np.frombuffer(wire(b), np.uint8)
                    for d, i in enumerate(members):
                        row_batch[base + i], row_delta[base + i] = len(batches), d
                    batches.append((r, p_id, len(members), 0, o, len(b)))
        res["status"][r] = status[r]
    descs = np.zeros(n, abi.DESC_DTYPE)
    descs["format"] = abi.FMT_RP_DISK
    for k, (r, p_id, cnt, _, o, ln) in enumerate(batches):
        descs[k] = (o, ln, p_id & M32, abi.FMT_RP_DISK, 47, 0, 0)
    all_batches = np.zeros(n, abi.PRODUCE_BATCH_DTYPE)
    all_batches["request"] = NONE
    if batches:
        all_batches[:len(batches)] = np.array(batches, abi.PRODUCE_BATCH_DTYPE)
    return dict(req_results=res, batches=all_batches[:len(batches)].copy(), all_batches=all_batches,
                row_batch=row_batch, row_delta=row_delta, out=out, wire=wire_out, out_descs=descs,
                out_bytes=out_bytes, nbatches=plan_batches, out_cap=cap)


# ---------------------------------------------------------------- hand case
def hand_call():
    """The request of include/rpgpu.h's hand vectors."""
    c = Call().request(6, 5, now_ms=1_700_000_123_456)
    c.row(None, b"v0", partition=4).row(b"the key", None).row(None, b"hi").row(b"", b"").row(b"k", b"v")
    return c.build()


HAND_BODIES = [
    (0, bytes.fromhex("0c000000000000")),
    (1, bytes.fromhex("1a0000000e746865206b65790100")),
    (4, bytes.fromhex("100000000004763000" "10000002026b027600")),
    (5, bytes.fromhex("100000000004686900")),
]
MURMUR_VECTORS = {
    b"21": 0xC5F2F8EC, b"foobar": 0xD0E47BBE, b"a-little-bit-long-string": 0xC53B1DA0,
    b"a-little-bit-longer-string": 0xA768C9C3, b"lkjh234lh9fiuh90y23oiuhsafujhadof229phr9h19h89h8": 0xFC7D49CD,
    b"abc": 0x1C94221B, b"the key": 0xC4C66957, b"k": 0xA291E5E0, b"": 0x106E08D9,
}

# ------------------------------------------------------------------- sweeps
KEY_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 127, 128, 129, 4097)
VAL_LENS = (None, 0, 1, 128, 129, 70_000)


def payload(rng, n):
    return None if n is None else rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def random_call(seed, nrows, nreq, counts=(1, 2, 6, 300), empty_at=()):
    """A few hundred rows: every rule, short and long keys / values, explicit ids in and out
    of range, requests that share partition ids; zero-row requests at the positions asked for."""
    rng = np.random.default_rng(seed)
    c = Call()
    cuts = sorted(rng.integers(0, nrows + 1, max(nreq - 1 - len(empty_at), 0)).tolist()) + [nrows]
    sizes, prev = [], 0
    for x in cuts:
        sizes.append(x - prev)
        prev = x
    for at in sorted(empty_at):
        sizes.insert(min(at, len(sizes)), 0)
    for r, cnt in enumerate(sizes):
        pc = int(counts[int(rng.integers(0, len(counts)))])
        c.request(pc, int(rng.integers(0, max(pc, 1))) if r % 3 else max(pc - 1, 0), now_ms=1_700_000_000_000 + r)
        for _ in range(cnt):
            rule = int(rng.integers(0, 3))
            kl = int(rng.choice([1, 3, 4, 9, 16, 33, 130])) if rule == 1 else (None, 0)[int(rng.integers(0, 2))]
            vl = (None, 0, 1, 7, 64, 200)[int(rng.integers(0, 6))]
            part = int(rng.choice([0, 1, 5, pc, -1, 299, INT32_MIN, INT32_MAX])) if rule == 0 else None
            c.row(payload(rng, kl), payload(rng, vl), part, kalign=int(rng.integers(0, 16)))
    return c.build()


def key_geometry_call():
    """Every key length at every arena misalignment, hashed; one key ends at the last byte."""
    rng = np.random.default_rng(7)
    c = Call().request(300, 299)
    for a in range(16):
        for kl in KEY_LENS:
            c.row(payload(rng, kl), payload(rng, 3), kalign=a)
    c.row(payload(rng, 3), b"x", kalign=5).row(None, None)
    c.row(payload(rng, 21), None, kalign=11)  # the arena ends with this key
    return c.build()


def value_call():
    rng = np.random.default_rng(8)
    c = Call().request(2, 1)
    for vl in VAL_LENS:
        for a in (0, 1, 15):
            c.row(payload(rng, 4), payload(rng, vl), valign=a)
            c.row(None, payload(rng, vl), valign=a)
    # record contents of 63 and 64 bytes: the length varint goes from one byte to two
    # (framing: 00 00 delta klen vlen 00 = 6 bytes at these sizes, delta below 64)
    c.request(1, 0)
    c.row(b"", payload(rng, 57)).row(b"", payload(rng, 58)).row(payload(rng, 20), payload(rng, 37))
    return c.build()


def group_call(sizes=(64, 65, 8193)):
    """Groups whose last offset delta sits on a varint boundary: 63 -> 64, 8191 -> 8192.  A
    request per group, a second partition interleaved, values that are the row numbers."""
    c = Call()
    for n in sizes:
        c.request(6, 0)
        for i in range(n):
            c.row(None, struct.pack("<I", i), partition=3)
            if i % 7 == 0:
                c.row(b"k", struct.pack("<I", i), partition=-2 if i % 14 else 5)
    return c.build()


def round_robin_call(nrows):
    """A run of rule-3 rows across wavefront and workgroup boundaries, keyed rows between them,
    rr_initial at partition_count - 1; two requests so the second's k starts again at 0."""
    rng = np.random.default_rng(9)
    c = Call()
    half = nrows // 2
    for cnt, pc in ((half, 6), (nrows - half, 300)):
        c.request(pc, pc - 1)
        for i in range(cnt):
            if i % 5 == 3:
                c.row(payload(rng, 6), b"v")
            else:
                c.row(None if i % 2 else b"", None)
    return c.build()


def size_call(nrows, nreq=1, empty_at=()):
    return random_call(1000 + nrows + 7 * nreq, nrows, nreq, empty_at=empty_at)


def ids_call(partition_count):
    """Explicit ids -1, INT32_MIN, INT32_MAX and partition_count itself beside hashed and
    round-robin rows: the signed order and the bias.  Two requests that share ids."""
    rng = np.random.default_rng(10)
    c = Call()
    for rr in (0, 1):
        c.request(partition_count, rr)
        for p in (INT32_MAX, -1, partition_count, INT32_MIN, 0, 256, 65536, 1 << 24):
            c.row(None, b"id", partition=p)
            c.row(payload(rng, 5), b"hashed")
            c.row(None, b"rr")
    return c.build()


def guard_call(which):
    """One refused request between two that are fine."""
    c = Call().request(6, 5).row(b"a", b"first").row(None, b"x")
    if which == "partition_count":
        c.request(1 << 31, 0).row(b"k", b"v")
    elif which == "rr_negative":
        c.request(6, -1).row(b"k", b"v")
    elif which == "rr_overflow":
        c.request(6, INT32_MAX - 1).row(None, b"1").row(b"key", b"2").row(None, b"3")
    elif which == "rr_exact":  # reaches INT32_MAX and stays OK
        c.request(6, INT32_MAX - 2).row(None, b"1").row(None, b"2")
    elif which == "len_below":
        c.request(6, 0).row(b"k", b"v").row(b"k", b"v", raw=dict(val_len=-2))
    elif which == "key_range":
        c.request(6, 0).row(b"k", b"v", raw=dict(key_off=1 << 40, key_len=3))
    elif which == "val_range":
        c.request(6, 0).row(b"k", b"v", raw=dict(val_len=1 << 20))
    elif which == "too_large":  # one value, named many times: the body passes INT32_MAX
        c.request(6, 0)
        big = bytes(1 << 20)
        c.row(None, big, partition=1)
        first = dict(c.rows[-1])
        for _ in range(2047):
            c.row(None, b"", partition=1, raw=dict(val_off=first["val_off"], val_len=first["val_len"]))
        c.row(b"other", b"partition", partition=2)
    else:
        raise KeyError(which)
    c.request(6, 5).row(b"a", b"last").row(None, None)
    return c.build()


GUARDS = {"partition_count": BAD_REQUEST, "rr_negative": BAD_REQUEST, "rr_overflow": BAD_REQUEST, "rr_exact": OK,
          "len_below": BAD_ROW, "key_range": BAD_ROW, "val_range": BAD_ROW, "too_large": TOO_LARGE}
