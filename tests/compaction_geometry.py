"""Crafted arenas whose record geometry walks the boundaries of the device
compaction kernels (rpgpu_compact.hip compact_keys_kernel / key_hash /
same_key / the key table and keep set, rpgpu_compact_rw.hip WaveOut::bytes /
compact_plan_kernel's block scan / compact_write_kernel's short-buffer
branch).  Deterministic builders only; nothing here runs on a GPU.

The boundaries: 64 records per lane trip of a wave, the 8-byte word of the key
hash, the 16-byte vector, 64-lane byte tail and 1024-byte stride of the wave
copy, the 0.5 load and the wrap-around of the linear-probing tables, the
1024-batch blocks of the output-offset scan.  The serial oracle
(oracle/compact.c) and the restatements in tests/test_compaction.py have none
of them; tests/test_compaction.py states what each arena promises and
tests/test_gpu_compaction_geometry.py runs them through the engine.

Every builder returns fresh (data, descs) copies of a cached build, one scope
(descs["partition"] = 0) unless its docstring says otherwise."""
from __future__ import annotations

import functools
import struct

import numpy as np

import oracle.oracle as orc
from kafka_batches import DISK, WIRE, arena, batch, record, zz  # noqa: F401
from redpanda_amd import abi

LENS = [0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1007, 1008, 1009, 1023, 1024, 1025, 1039, 1040, 1041,
        2047, 2048, 2049, 4101]
COUNTS = [63, 64, 65, 127, 128, 129, 200]
TS_DELTAS = [0, -1, 64, -8192, 1 << 20, -(1 << 27)]  # 1, 1, 2, 2, 4 and 4 varint bytes, both signs

M64 = (1 << 64) - 1
FIRST_TS = 1_700_000_000_000


def pat(n: int, salt: int = 0) -> bytes:
    """n patterned bytes: neighbours differ, and so do runs 8, 16, 64 or 1024 apart."""
    k = np.arange(n, dtype=np.int64) + salt * 131
    return ((k * 29 + (k >> 3) * 7 + (k >> 6) * 13 + (k >> 10) * 101 + salt) & 0xFF).astype(np.uint8).tobytes()


def one_scope(batches, fmt, partitions=None):
    data, descs = arena(batches, fmt=fmt, ops=abi.OPS_PRODUCE)
    descs["partition"] = 0 if partitions is None else partitions
    return data, descs


def cached(fn):
    """Build once per argument tuple; hand out copies, so no test changes another's input."""
    build = functools.lru_cache(maxsize=None)(fn)

    @functools.wraps(fn)
    def get(*a):
        return tuple(x.copy() if isinstance(x, np.ndarray) else x for x in build(*a))
    return get


# ------------------------------------------------------------------ lengths
def length_key(li: int, j: int) -> bytes:
    return pat(LENS[li], li) + b"#%d.%d" % (li, j)


def length_round2_keep(li: int) -> list[int]:
    """Keep flags the third round leaves in the second-round batch of LENS[li]."""
    return [[1, 0, 0], [0, 0, 1], [1, 0, 1]][li % 3]


@cached
def length_arena(fmt):
    """Round 1: one 6-record batch per L in LENS (key L + suffix bytes, value
    L + j % 3 bytes, odd records one header of L % 50 / L bytes, ts deltas of
    mixed sign and size): every byte range starts at its own misalignment.
    Round 2: per L one batch re-using the keys of records 1, 2 and 5, so the
    round-1 batch is FILTERED with records 0, 3 and 4 kept.  Round 3 supersedes
    two or one of each round-2 batch's keys: first only, last only, all but one
    (length_round2_keep)."""
    bs, off = [], 0
    for li, L in enumerate(LENS):
        recs = []
        for j in range(6):
            hdrs = [(pat(L % 50, li + 3), pat(L, li + 5))] if j & 1 else []
            recs.append(record(length_key(li, j), pat(L + j % 3, li + j), ts_delta=TS_DELTAS[j], off_delta=j,
                               headers=hdrs))
        bs.append(batch(recs, fmt=fmt, base_offset=off))
        off += 6
    for li, L in enumerate(LENS):
        recs = [record(length_key(li, j), b"r2", ts_delta=k, off_delta=k) for k, j in enumerate((1, 2, 5))]
        bs.append(batch(recs, fmt=fmt, base_offset=off))
        off += 3
    for li, L in enumerate(LENS):
        gone = [j for j, k in zip((1, 2, 5), length_round2_keep(li)) if not k]
        recs = [record(length_key(li, j), b"r3", ts_delta=k, off_delta=k) for k, j in enumerate(gone)]
        bs.append(batch(recs, fmt=fmt, base_offset=off))
        off += len(recs)
    return one_scope(bs, fmt)


# ------------------------------------------------------------------ counts
DROPPED_COUNT, KEPT_COUNT, FIRST_TRIP_COUNT, LATER_TRIPS_COUNT, CUT_COUNT = 64, 65, 128, 200, 129


@cached
def count_arena(fmt):
    """One batch per COUNTS entry.  63, 127 and 129 records: ten keys per batch,
    so only the last ten records survive (FILTERED).  The others carry one key
    per record and later batches supersede all of the 64 (DROPPED), none of the
    65 (KEPT), records >= 64 of the 128 (survivors all in the first lane trip)
    and records < 64 of the 200 (survivors all in the later trips)."""
    bs, off = [], 0
    unique = (DROPPED_COUNT, KEPT_COUNT, FIRST_TRIP_COUNT, LATER_TRIPS_COUNT)
    for c in COUNTS:
        recs = [record(b"u%d.%d" % (c, j) if c in unique else b"k%d.%d" % (c, j % 10), b"v%d" % (j % 100),
                       ts_delta=j, off_delta=j) for j in range(c)]
        bs.append(batch(recs, fmt=fmt, base_offset=off))
        off += c
    for c, js in ((DROPPED_COUNT, range(64)), (FIRST_TRIP_COUNT, range(64, 128)), (LATER_TRIPS_COUNT, range(64))):
        recs = [record(b"u%d.%d" % (c, j), b"s", ts_delta=k, off_delta=k) for k, j in enumerate(js)]
        bs.append(batch(recs, fmt=fmt, base_offset=off))
        off += len(recs)
    return one_scope(bs, fmt)


def count_cut(results) -> tuple[int, int]:
    """(batch, index entries) of an index cut in the middle of the 129-record batch."""
    b = COUNTS.index(CUT_COUNT)
    return b, int(results["index_first"][b]) + CUT_COUNT // 2


# ------------------------------------------------------------------ key edges
EDGE_BASES = [-(1 << 63), -1, 0, (1 << 63) - 200]


@cached
def key_edge_arena(fmt):
    """Keys that differ only in the last byte (8, 9, 16, 17 bytes), keys that are
    prefixes of each other with zero tails, null against empty, one key under
    two batch types (1 and 5; a wire batch has no type, so there it is one key)
    and in two scopes (partitions 0 and 1), two keys whose latest records share
    an offset with a third key's older record (should_keep's duplicate-offset
    rule, by overlapping base offsets), and base offsets at the ends of int64
    (partitions 2-5)."""
    pairs = [(pat(L - 1, L) + b"\x01", pat(L - 1, L) + b"\x02") for L in (8, 9, 16, 17)]
    chain = [b"a", b"a\0", b"a\0\0", b"chain-7", b"chain-7\0", b"chain-7\0\0"]
    first = [k for p in pairs for k in p] + chain + [None, b""]
    again = [pairs[0][0], pairs[1][1], pairs[2][0], pairs[3][1], chain[1], chain[4], None]
    bs, parts = [], []

    def add(recs, base, part=0, btype=1):
        bs.append(batch(recs, fmt=fmt, base_offset=base, btype=btype))
        parts.append(part)

    add([record(k, b"one", ts_delta=j, off_delta=j) for j, k in enumerate(first)], 0)
    add([record(k, b"two", ts_delta=j, off_delta=j) for j, k in enumerate(again)], 100)
    add([record(b"typed", b"t1"), record(b"scoped", b"p0", off_delta=1)], 200)
    add([record(b"typed", b"t5")], 210, btype=5)
    add([record(b"scoped", b"p1")], 220, part=1)
    # offset 301 is the latest of both "dup-x" and "dup-y"; "dup-z" has an older record there
    add([record(b"dup-x", b"x", off_delta=0)], 301)
    add([record(b"dup-f", b"f", off_delta=0), record(b"dup-y", b"y", off_delta=1)], 300)
    add([record(b"dup-z", b"old", off_delta=0)], 301)
    add([record(b"dup-z", b"new", off_delta=0)], 305)
    for k, base in enumerate(EDGE_BASES):
        add([record(b"e1", b"a", off_delta=0), record(b"e2", b"b", off_delta=1), record(b"e1", b"c", off_delta=2)],
            base, part=2 + k)
        add([record(b"e2", b"d", off_delta=0), record(b"e3", b"e", off_delta=1)], base + 100, part=2 + k)
    return one_scope(bs, fmt, parts)


# ------------------------------------------------------------------ table load
@cached
def full_load_arena(fmt, records):
    """`records` (a power of two >= 32) distinct 8-byte keys, one record each, in
    16-record batches: index_cap == records, so the key table and the keep set
    run at exactly the 0.5 load their sizing allows."""
    assert records >= 32 and records & (records - 1) == 0
    bs = []
    for b in range(records // 16):
        recs = [record(struct.pack("<Q", ((16 * b + j) * 0x9E3779B97F4A7C15 + 1) & M64), b"v", ts_delta=j,
                       off_delta=j) for j in range(16)]
        bs.append(batch(recs, fmt=fmt, base_offset=16 * b))
    return one_scope(bs, fmt)


def mix64(h: int) -> int:
    """rpgpu_compact.hip mix64 (the splitmix64 finaliser)."""
    h ^= h >> 30
    h = h * 0xBF58476D1CE4E5B9 & M64
    h ^= h >> 27
    h = h * 0x94D049BB133111EB & M64
    return h ^ h >> 31


def key_hash(key: bytes, scope: int, btype: int) -> int:
    """rpgpu_compact.hip key_hash: 8-byte little-endian words, then a zero-padded tail."""
    h = mix64((scope << 32) ^ (btype << 24) ^ len(key) ^ 0x9E3779B97F4A7C15)
    full = len(key) & ~7
    for i in range(0, full, 8):
        h = mix64(h ^ int.from_bytes(key[i:i + 8], "little"))
    if full < len(key):
        h = mix64(h ^ int.from_bytes(key[full:], "little") ^ 0xFF51AFD7ED558CCD)
    return h


def set_hash(scope: int, offset: int) -> int:
    """rpgpu_compact.hip set_hash: the keep set's slot for (scope, offset)."""
    return mix64((offset & M64) ^ (scope * 0xC2B2AE3D27D4EB4F & M64))


def home_keys(cap, scope, btype, count, want, start=0):
    """`count` distinct 8-byte keys whose home slot (key_hash & (cap - 1)) satisfies want()."""
    out, i = [], start
    while len(out) < count:
        k = struct.pack("<Q", i)
        if want(key_hash(k, scope, btype) & (cap - 1)):
            out.append(k)
        i += 1
    return out


def wrap_keys(cap, scope, btype, count):
    """`count` distinct 8-byte keys whose home slot in a `cap`-slot key table is the last one."""
    return home_keys(cap, scope, btype, count, lambda s: s == cap - 1)


def wrap_offsets(cap, scope, count, start):
    """`count` ascending offsets >= start whose home slot in a `cap`-slot keep set is the last one."""
    out, o = [], start
    while len(out) < count:
        if set_hash(scope, o) & (cap - 1) == cap - 1:
            out.append(o)
        o += 1
    return out


WRAP_RECORDS, WRAP_CAP, WRAP_KEYS = 32, 64, 4


@cached
def wrap_arena(fmt):
    """32 records (a 64-slot table): 4 keys whose home is slot 63, twice each,
    and 24 single-record fillers whose homes lie in slots 8-55.  The 4 keys
    claim slots 63, 0, 1 and 2, so inserting and finding them steps past the
    last slot; their latest offsets are chosen to wrap the keep set as well."""
    keys = wrap_keys(WRAP_CAP, 0, 1, WRAP_KEYS)
    fill = home_keys(WRAP_CAP, 0, 1, WRAP_RECORDS - 2 * WRAP_KEYS, lambda s: 8 <= s < 56, start=1 << 20)
    late = wrap_offsets(WRAP_CAP, 0, WRAP_KEYS, 1000)
    recs = [record(k, b"old", ts_delta=j, off_delta=j) for j, k in enumerate(keys + fill[:12])]
    more = [record(k, b"new", ts_delta=j, off_delta=o - 1000) for j, (k, o) in enumerate(zip(keys, late))]
    more += [record(k, b"fill", ts_delta=4 + j, off_delta=late[-1] - 1000 + 1 + j) for j, k in enumerate(fill[12:])]
    return one_scope([batch(recs, fmt=fmt, base_offset=0), batch(more, fmt=fmt, base_offset=1000)], fmt)


# ------------------------------------------------------------------ many batches
MANY_CORRUPT = (5, 1023, 1024, 1500, 2047, 2599)
SHORT_CAP_BATCH = 1500  # the short-output-buffer test cuts the buffer at this batch's out_offset


@cached
def many_batches_arena(fmt, n=2600):
    """n small batches (1-4 records, values of 0-6 bytes, keys from a 300-key
    alphabet).  Nine in ten open with a record whose key occurs once, so they
    keep an output slot (FILTERED, or KEPT / TX_CLEARED when nothing else is
    superseded); the tenth is DROPPED unless it is late enough to survive.
    On-disk arenas mix in non-compactible batch types.  MANY_CORRUPT batches
    have a broken body CRC (SKIPPED): zero slots beside non-zero ones on both
    sides of the 1024-batch blocks of the plan's scan."""
    rng = np.random.default_rng(0xC0A7 + fmt)
    bs, off = [], 0
    for i in range(n):
        nrec = int(rng.integers(1, 5))
        recs = []
        for j in range(nrec):
            key = b"u%d" % i if j == 0 and i % 10 != 7 else b"k%03d" % int(rng.integers(0, 300))
            recs.append(record(key, b"v" * int(rng.integers(0, 7)), ts_delta=j, off_delta=j))
        bt = int(rng.choice([1, 1, 1, 1, 1, 1, 2, 19, 23, 5])) if fmt == DISK else 1
        attrs = int(rng.choice([0, 0, 0, 0x10, 0x30, 0x08]))
        b = bytearray(batch(recs, fmt=fmt, base_offset=off, btype=bt, attrs=attrs))
        if i in MANY_CORRUPT:
            b[-1] ^= 0x5A
        bs.append(bytes(b))
        off += nrec
    return one_scope(bs, fmt)


# ------------------------------------------------------------------ varints
def pad_varint(v: int) -> bytes:
    """A non-canonical encoding of v: one byte longer, the last one 0x00."""
    b = bytearray(zz(v))
    assert len(b) < 10
    b[-1] |= 0x80
    return bytes(b) + b"\0"


def raw_record(key, value, ts_delta=0, off_delta=0, headers=(), hcount=None, attrs=0, pad=()):
    """A record from raw bytes; `pad` names the varints to write non-canonically
    ("size", "ts", "off", "klen", "vlen", "hcount").  A header is (key, value)
    with None for a null (-1) length."""
    def v(name, x):
        return pad_varint(x) if name in pad else zz(x)

    body = bytes([attrs]) + v("ts", ts_delta) + v("off", off_delta)
    body += v("klen", -1 if key is None else len(key)) + (key or b"")
    body += v("vlen", -1 if value is None else len(value)) + (value or b"")
    body += v("hcount", len(headers) if hcount is None else hcount)
    for hk, hv in headers:
        body += zz(-1 if hk is None else len(hk)) + (hk or b"") + zz(-1 if hv is None else len(hv)) + (hv or b"")
    return v("size", len(body)) + body


PAST_END_KEY = b"past-end"  # key prefix of the record that declares more headers than its batch's body holds
VARINT_TS = [1, -1, 1 << 31, -(1 << 31), (1 << 63) - 1, -(1 << 63)]


@cached
def varint_arena(fmt):
    """Five batch shapes under each of the batch attributes 0, 0x08 (append
    time), 0x10 (transactional) and 0x30 (control + transactional): every
    varint of a record padded once; the extreme ts deltas; negative offset
    deltas; 0, 1, 5 and 70 headers with null values and empty keys; a last
    record declaring 4 headers the body does not hold.  Each batch opens with a
    record that a closing batch supersedes, so whatever validates OK is
    FILTERED.  No verdict is assumed: the oracle's validation decides."""
    bs, off, opened = [], 100, []
    for a, attrs in enumerate((0, 0x08, 0x10, 0x30)):
        shapes = []
        shapes.append([raw_record(b"pad-%d-%d" % (k, a), b"value", ts_delta=3 + k, off_delta=1 + k,
                                  headers=[(b"h", b"x")], pad=(name,))
                       for k, name in enumerate(("size", "ts", "off", "klen", "vlen", "hcount"))])
        shapes.append([raw_record(b"ts-%d-%d" % (k, a), b"t", ts_delta=t, off_delta=1 + k) for k, t in enumerate(VARINT_TS)])
        shapes.append([raw_record(b"neg-%d-%d" % (k, a), pat(20, k), ts_delta=k, off_delta=d)
                       for k, d in enumerate((5, -1, 3, -7, 2))])
        shapes.append([raw_record(b"hdr-%d-%d" % (hc, a), b"h", ts_delta=hc, off_delta=1 + k,
                                  headers=[(b"" if h % 3 == 0 else b"hk%d" % h, None if h % 4 == 1 else pat(h % 9, h))
                                           for h in range(hc)])
                       for k, hc in enumerate((0, 1, 5, 70))])
        shapes.append([raw_record(b"mid-%d" % a, b"m", off_delta=1),
                       raw_record(PAST_END_KEY + b"-%d" % a, b"z", ts_delta=1, off_delta=2, hcount=4)])
        for s, recs in enumerate(shapes):
            first = b"open-%d-%d" % (a, s)
            opened.append(first)
            body = raw_record(first, b"o") + b"".join(recs)
            bs.append(batch(body, fmt=fmt, base_offset=off, attrs=attrs, record_count=1 + len(recs),
                            first_ts=FIRST_TS + off, max_ts=FIRST_TS + off + 1000))
            off += 100
        opened += [b"pad-2-%d" % a, b"ts-4-%d" % a, b"hdr-5-%d" % a]  # and a record inside three of them
    bs.append(batch([record(k, b"c", ts_delta=j, off_delta=j) for j, k in enumerate(opened)], fmt=fmt,
                    base_offset=off))
    return one_scope(bs, fmt)


# ------------------------------------------------------------------ decompressed input
@cached
def compressed_keyed_arena(fmt, nb=60):
    """LZ4 and zstd batches over keyed bodies (1-11 records; a small key alphabet
    mixed with keys that occur once, so batches are dropped, filtered and
    kept), a few of them damaged or short of the records their header counts: the
    input of the decompress path, whose output compaction then reads."""
    rng = np.random.default_rng(0xDEC0 + fmt)
    keys = [None, b"", b"a", b"b", b"key-1", b"key-2", b"k" * 40]
    bs, off = [], 0
    for i in range(nb):
        nrec = int(rng.integers(1, 12))
        recs = [record(keys[int(rng.integers(0, len(keys)))] if rng.random() < 0.6 else b"once-%d.%d" % (i, j),
                       b"value-%d" % j * 3, ts_delta=j, off_delta=j) for j in range(nrec)]
        codec = 3 if i % 2 else 4
        comp = bytearray(orc.compress(codec, b"".join(recs)))
        if i % 17 == 6:  # a damaged payload: whatever the decoder makes of it
            comp[len(comp) // 2] ^= 0x5A
        # i % 13 == 4: two records more in the header than in the body -- the walk of the decoded
        # batch fails, and the rest of the index slice reserved for it stays unused
        bs.append(batch(bytes(comp), fmt=fmt, base_offset=off, record_count=nrec + (2 if i % 13 == 4 else 0),
                        attrs=codec))
        off += nrec
    data, descs = arena(bs, fmt=fmt, ops=abi.OPS_PRODUCE | abi.OP_DECOMP)
    descs["partition"] = 0
    return data, descs


BUILDERS = {
    "length": length_arena,
    "count": count_arena,
    "key_edge": key_edge_arena,
    "full_load_32": lambda fmt: full_load_arena(fmt, 32),
    "full_load_64": lambda fmt: full_load_arena(fmt, 64),
    "full_load_1024": lambda fmt: full_load_arena(fmt, 1024),
    "full_load_4096": lambda fmt: full_load_arena(fmt, 4096),
    "wrap": wrap_arena,
    "many_batches": many_batches_arena,
    "varint": varint_arena,
}


@functools.lru_cache(maxsize=None)
def oracle_chain(name, fmt):
    """The oracle's validate -> keep -> rewrite over BUILDERS[name](fmt), computed
    once and shared; callers leave it unchanged."""
    data, descs = BUILDERS[name](fmt)
    res, idx, _ = orc.validate_arena(data, descs)
    keep, nkeys = orc.compaction_keep(data, descs, res, idx)
    want = orc.compaction_rewrite(data, descs, res, idx, keep)
    return dict(data=data, descs=descs, res=res, idx=idx, keep=keep, nkeys=nkeys, want=want)
