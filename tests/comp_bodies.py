"""Record-batch bodies whose matches walk the geometry space of the device
compressors (rpgpu_lz4c.h compress_block / compress_frame, rpgpu_snappyc.h
compress_fragment / emit_literal / emit_copy / raw_compress / compress_java,
and, for the round trip, rpgpu_deflatec.h and rpgpu_zstdc.h).

A compressor cannot be handed its sequences: it finds them.  So every body
here is laid out so that liblz4's and snappy's greedy finders meet the planted
match where it was planted -- literals are random bytes (no accidental
matches), a planted match has its source inside the first positions of a block
or right after a run (where both finders still step by one), and a run of one
byte sets the anchor in front of a planted literal run.  What the reference's
compressors really emitted for these bodies is asserted by
tests/test_comp_bodies.py from the oracle's output alone; nothing here knows
how the engine decides.

families()  name -> list of (label, body); every family is deterministic.
  sizes         block / fragment / hash-table size edges, six fills each
  end_zone      matches ending at every distance from the end of a block
  stored_edge   one planted match around the compressed-size == size - 1 edge
  length_codes  one planted (ll, ml, off) per body, the largest distances,
                back-to-back matches, the catch-up back to the anchor
  skip          long incompressible stretches around compressible ones
  lane_mates    a large first tenant of a hash table, a filler, then a small
                second tenant cut from the first; `matched` pairs share
                snappy's table size class (lane_first / lane_second /
                LANE_FILLER also build the GPU lane-reuse arenas)
NAMED holds the bodies at which a sweep caught a real difference (none so far
beyond the planted ones)."""
from __future__ import annotations

import functools
import struct

import numpy as np

BLOCK = 1 << 16          # LZ4F_max64KB and snappy's kBlockSize
FRAGMENT = 128 << 10     # iobuf max_chunk_size: one snappy-java chunk
FAMILIES = ("sizes", "end_zone", "stored_edge", "length_codes", "skip", "lane_mates")

SIZES = (list(range(41))
         + [s + d for s in (256, 512, 1024, 2048, 4096, 8192, 16384) for d in (-1, 0, 1)]  # snappy's 7 tables
         + [65535, 65536, 65537, 65536 + 12, 65536 + 13, 65536 + 14, 65536 + 15]
         + [131071, 131072, 131073, 131072 + 15, 196608 + 14])
FILLS = ("const", "p2", "p3", "p5", "p37", "random")

LL = (0, 1, 14, 15, 16, 59, 60, 61, 62, 255, 256, 257, 269, 270, 271, 524, 525, 526, 65400)
ML = (4, 5, 11, 12, 13, 18, 19, 20, 60, 63, 64, 65, 66, 67, 68, 69, 70, 71, 72, 128, 131, 132, 273, 274, 275,
      528, 529, 530)
OFF = (1, 2, 3, 4, 7, 8, 2047, 2048, 2049)


def _rng(*key) -> np.random.Generator:
    return np.random.default_rng([0xC0B0D1E5, *key])


def rnd(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def other(rng, *avoid: int) -> int:
    """A byte value that is none of `avoid` (keeps a planted edge sharp)."""
    while True:
        b = int(rng.integers(0, 256))
        if b not in avoid:
            return b


def periodic(rng, n: int, period: int) -> bytes:
    """n bytes of a random period whose bytes are all distinct."""
    p = rng.permutation(256)[:period].astype(np.uint8)
    return np.resize(p, n).tobytes() if n else b""


# ---------------------------------------------------------------------- sizes
def sizes():
    out = []
    for n in SIZES:
        for fill in FILLS:
            rng = _rng(1, n, FILLS.index(fill))
            body = rnd(rng, n) if fill == "random" else periodic(rng, n, 1 if fill == "const" else int(fill[1:]))
            out.append((f"sizes/{n}/{fill}", body))
    return out


# ------------------------------------------------------------------- end zone
END_N = (40, 64, 300, 4096)
END_PERIODS = (1, 2, 3, 4, 5, 8, 16, 37)
END_LAST = 26
SPLICE_SEAMS = range(6, 21)  # the seam n - 20 .. n - 6


def splice(rng, lead: bytes, k: int, j: int) -> bytes:
    """lead + A + B + A[:k] + B[:j]: the match with A ends at the seam, where a
    match with B is waiting in the table (both sources lie where the finders
    step by one)."""
    a, b = rnd(rng, 16), rnd(rng, 24)
    return lead + a + b + a[:k] + b[:j]


def end_zone():
    out = []
    for n in END_N:
        for period in END_PERIODS:
            for back in range(1, END_LAST + 1):
                for width in (1, 2):
                    q = n - back
                    if q + width > n:
                        continue
                    rng = _rng(2, n, period, back, width)
                    b = bytearray(periodic(rng, n, period))
                    for x in range(q, q + width):
                        b[x] = other(rng, *b[max(0, x - period):x + period + 1])
                    out.append((f"end_zone/flip/{n}/p{period}/-{back}/w{width}", bytes(b)))
    for seed in range(4):
        for j in SPLICE_SEAMS:
            for k in (4, 7, 12, 16):
                for lead in (0, 200, 3000):
                    rng = _rng(3, seed, j, k, lead)
                    head = bytes([other(rng)]) * lead + (rnd(rng, 3) if lead else b"")
                    out.append((f"end_zone/splice/s{seed}/lead{lead}/k{k}/-{j}", splice(rng, head, k, j)))
    return out


# ---------------------------------------------------------------- stored edge
STORED_N = (64, 100, 200, 300, 600, 1000, 4096)
STORED_ML = range(4, 60)
STORED_POS = ("20%", "50%", "90%", "tail15", "tail270")


def planted(rng, n: int, pos: int, m: int, src: int = 1) -> bytes:
    """n random bytes with body[pos:pos+m] = body[src:src+m]; the bytes on
    both sides of the copy differ from the source's neighbours."""
    b = bytearray(rnd(rng, n))
    b[pos:pos + m] = b[src:src + m]
    if pos + m < n:
        b[pos + m] = other(rng, b[src + m])
    b[pos - 1] = other(rng, b[src - 1])
    return bytes(b)


def stored_edge_pos(n: int, m: int, where: str):
    if where.endswith("%"):
        pos = n * int(where[:-1]) // 100
    else:
        pos = n - int(where[4:]) - m
    return pos if pos >= 1 + m + 4 and pos + m <= n else None


def stored_edge():
    out = []
    for n in STORED_N:
        for where in STORED_POS:
            for m in STORED_ML:
                pos = stored_edge_pos(n, m, where)
                if pos is None:
                    continue
                # one literal stream per (n, where): neighbouring match lengths differ in the match alone
                out.append((f"stored_edge/{n}/{where}/m{m}", planted(_rng(4, n, STORED_POS.index(where)), n, pos, m)))
    return out


# --------------------------------------------------------------- length codes
def run_lead(rng, lits: bytes, length: int = 40) -> bytes:
    """8 random bytes and a run of one byte: the run is one match that ends,
    and leaves the anchor, exactly in front of `lits`."""
    return rnd(rng, 8) + bytes([other(rng, lits[0] if lits else 0)]) * length


def length_code(ll: int, ml: int, off: int, tail: int = 12) -> bytes:
    """One planted sequence: ll literals, then ml bytes from off back, then
    `tail` random bytes."""
    rng = _rng(5, ll, ml, off)
    end = rnd(rng, tail)
    if off <= 8:  # an overlapping match: the last `off` literals repeated
        lits = bytearray(rnd(rng, max(ll, off)))
        seed = rng.permutation(256)[:off].astype(np.uint8).tobytes()
        lits[len(lits) - off:] = seed
        if len(lits) > off:
            lits[len(lits) - off - 1] = other(rng, seed[-1])
        match = (seed * (ml // off + 2))[:ml]
        endb = bytearray(end)
        endb[0] = other(rng, (seed * (ml // off + 2))[ml])
        return run_lead(rng, bytes(lits)) + bytes(lits) + match + bytes(endb)
    x = rnd(rng, ml + 1)
    lits = bytearray(rnd(rng, ll))
    run = off - (ml + 1) - ll
    if run >= 8:
        fill = bytes([other(rng, x[-1], lits[0] if ll else x[0])]) * run
        if ll:
            lits[-1] = other(rng, fill[0])
    else:  # the literal run does not fit under the distance: no anchor in front of it
        fill = b""
    endb = bytearray(end)
    endb[0] = other(rng, x[ml])
    return rnd(rng, 8) + x + fill + bytes(lits) + x[:ml] + bytes(endb)


def far_match(n: int, back: int, ml: int, second_block: bool) -> bytes:
    """A block of n bytes: its first 8 bytes, a run, three literals and the
    first `ml` bytes again `back` bytes before the end: the largest distances a
    block allows, the source at index 0 (the value an empty table entry reads)."""
    rng = _rng(6, n, back, ml, int(second_block))
    x = rnd(rng, 8)
    fill = other(rng, x[-1])
    pos = n - back
    b = bytearray(x + bytes([fill]) * (pos - 3 - 8) + bytes([other(rng, fill)]) + rnd(rng, 2) + x[:ml])
    b += rnd(rng, n - len(b))
    if pos + ml < n:
        b[pos + ml] = other(rng, x[ml] if ml < 8 else fill)
    return (rnd(rng, BLOCK) if second_block else b"") + bytes(b)


def pair(ka: int, kb: int, gap: int, seed: int) -> bytes:
    """Two back-to-back matches (the second with no literals) in mid-block."""
    rng = _rng(7, ka, kb, gap, seed)
    a, b = rnd(rng, 20), rnd(rng, 20)
    return rnd(rng, 4) + a + b + rnd(rng, gap) + a[:ka] + b[:kb] + rnd(rng, 14)


def catch_up(xlen: int, seed: int) -> bytes:
    """A match that starts at the anchor but whose first position the finder
    cannot find (its source lies inside a run, which is never inserted): it is
    met one position late and walked back to the anchor."""
    rng = _rng(8, xlen, seed)
    x = rnd(rng, xlen)
    e = other(rng, x[0])
    d = other(rng, e, x[-1])
    gap = rnd(rng, 6)
    return rnd(rng, 8) + bytes([e]) * 30 + x + gap + bytes([d]) * 20 + bytes([e]) + x + rnd(rng, 13)


def length_codes():
    out = []
    for ll in LL:
        for ml in ML:
            for off in OFF:
                if ll == 65400 and (ml not in (4, 20, 70) or off not in (1, 2048)):
                    continue  # 64 KiB each: a few are enough
                if ll == 0 and off <= 8:
                    continue  # would only lengthen the lead's run
                out.append((f"length_codes/ll{ll}/ml{ml}/off{off}", length_code(ll, ml, off)))
        rng = _rng(9, ll)
        out.append((f"length_codes/literal_only/{ll}", rnd(rng, ll)))
        if ll:
            lits = rnd(rng, ll)
            out.append((f"length_codes/literal_after_run/{ll}", run_lead(rng, lits, 30) + lits))
    for n in (BLOCK, 40000):
        for second in (False, True):
            for back in (12, 13, 15, 16, 17, 24):
                for ml in (4, 7):
                    out.append((f"length_codes/far/{n}/{'b1' if second else 'b0'}/-{back}/m{ml}",
                                far_match(n, back, ml, second)))
    for seed in range(6):
        for ka in (4, 5, 12, 20):
            for kb in (4, 9, 20):
                for gap in (0, 5):
                    out.append((f"length_codes/pair/s{seed}/{ka}+{kb}/gap{gap}", pair(ka, kb, gap, seed)))
        for xlen in (4, 5, 16, 40):
            out.append((f"length_codes/catch_up/s{seed}/x{xlen}", catch_up(xlen, seed)))
    return out


# ----------------------------------------------------------------------- skip
def compressible(rng, n: int, kind: int) -> bytes:
    if kind == 0:
        return periodic(rng, n, 1)
    if kind == 1:
        return periodic(rng, n, 37)
    words = [rnd(rng, int(k)) for k in rng.integers(3, 12, 12)]
    out = b"".join(words[int(k)] for k in rng.integers(0, 12, n // 3 + 1))
    return out[:n]


def skip():
    out = []
    for kib in (2, 4, 8, 16, 32, 60):
        for kind in range(3):
            rng = _rng(10, kib, kind)
            r, c = rnd(rng, kib << 10), compressible(rng, 3000 + 17 * kib, kind)
            out.append((f"skip/{kib}k/random+tail{kind}", r + c))
            out.append((f"skip/{kib}k/tail{kind}+random", c + r))
    for kib in (8, 63, 64, 130):
        for kind in range(3):
            rng = _rng(11, kib, kind)
            parts = [rnd(rng, 1024) if k % 2 else compressible(rng, 1024, kind) for k in range(kib)]
            out.append((f"skip/alternate/{kib}k/{kind}", b"".join(parts) + rnd(rng, kib % 7)))
    return out


# ----------------------------------------------------------------- lane mates
LANE_FILLER = bytes(range(0x30, 0x30 + 24))  # a 24-byte body: one stored LZ4 block, one snappy literal
LANE_STRETCH = 3000


def lane_first(j: int, matched: bool = False) -> bytes:
    """First tenant j of a hash table: 70 KiB .. 131,092 bytes (2-3 blocks) of
    a random 3,000-byte stretch repeated, which leaves a full table with
    indices up to 65,535 behind.  matched: 64 KiB + 520..1,000 bytes, so the
    last block it leaves in the table is of the second tenant's size class."""
    rng = _rng(12, j, int(matched))
    if matched:
        n = BLOCK + int(rng.integers(520, 1001))
    else:
        n = int(rng.integers(70 << 10, 131092 + 1)) if j % 4 else (131092, 70 << 10, 131072 + 13, 131072)[j // 4 % 4]
    return np.resize(np.frombuffer(rnd(rng, LANE_STRETCH), dtype=np.uint8), n).tobytes()


def lane_second(j: int, first: bytes, matched: bool = False) -> bytes:
    """Second tenant: 300..900 bytes cut from the first tenant's body where one
    of its blocks begins (shifted by whole stretches, or by a few bytes): the
    stale entries then point at equal bytes, so a stale entry read as live
    passes the 4-byte compare.  That holds for LZ4, whose table and hash are
    the same for every block.  snappy's hash shift follows the block's table
    size (16,384 entries for the first tenant's blocks, 512 or 1,024 for these
    second tenants), so there a stale index never points at equal bytes;
    matched: the opening 513 bytes or more of the first tenant's last block,
    which snappy hashed with the same 1,024-entry shift."""
    rng = _rng(13, j, int(matched))
    if matched:
        return first[BLOCK:BLOCK + int(rng.integers(513, len(first) - BLOCK + 1))]
    n = int(rng.integers(300, 901))
    blocks = (len(first) - 1) // BLOCK
    start = BLOCK * int(rng.integers(1, blocks + 1)) % LANE_STRETCH + LANE_STRETCH * int(rng.integers(0, 4))
    if j % 4 == 3:
        start += int(rng.integers(1, 9))
    if j % 8 == 5:  # twice the same half: real matches next to the stale ones
        half = first[start:start + n // 2]
        return half + half
    return first[start:start + n]


def lane_mates(pairs: int = 8):
    out = []
    for matched in (False, True):
        kind = "matched" if matched else "plain"
        for j in range(pairs):
            first = lane_first(j, matched)
            out.append((f"lane_mates/{kind}/first/{j}", first))
            if not matched:
                out.append((f"lane_mates/{kind}/filler/{j}", LANE_FILLER))
            out.append((f"lane_mates/{kind}/second/{j}", lane_second(j, first, matched)))
    return out


# ------------------------------------------------------------------ the whole
# Bodies at which a sweep caught the engine differing from the oracle: (label, body).
NAMED: list = []


@functools.lru_cache(maxsize=None)
def family(name: str) -> tuple:
    return tuple({"sizes": sizes, "end_zone": end_zone, "stored_edge": stored_edge, "length_codes": length_codes,
                  "skip": skip, "lane_mates": lane_mates}[name]()) + (tuple(NAMED) if name == "sizes" else ())


def families() -> dict:
    return {name: family(name) for name in FAMILIES}


def all_bodies() -> list:
    return [b for name in FAMILIES for b in family(name)]


def write_file(path, bodies) -> None:
    """The --bodies file of tests/native/compress_fuzz.cpp: per body a
    little-endian uint32 length and the bytes."""
    with open(path, "wb") as f:
        for _, body in bodies:
            f.write(struct.pack("<I", len(body)))
            f.write(body)
