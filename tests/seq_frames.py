"""Crafted frames whose LZ77 sequences walk the geometry space of the device
copy engines (rpgpu_copy.h wc_exec / period16 / copy_lits / copy_seq_match /
copy_exact / match_exact / copy_match, under rpgpu_zstd.h wc_seq, rpgpu_codec.h
lz4_block_lane and the snappy decoders, rpgpu_wave.h exec_seqs /
coop_match / coop_copy, rpgpu_inflate.h Write::copy), and a plain
byte-at-a-time model of what they decode to.

A sequence is a triple (ll, ml, off): ll literal bytes, then a match of ml
bytes from off bytes back.  grid() builds, per seed, the same list of triples
for every codec (filtered only by the codec's least and greatest match length)
cut into blocks of ~40 KiB; the crafters below turn a block into an LZ4 block,
a snappy chunk, a fixed-Huffman deflate stream or a line of the geometry file
that tests/native/zstd_fuzz.cpp --dump-seqgrid turns into zstd blocks.

Nothing here knows how an engine decides between its paths: the lists are
dense where every engine branches (ll <= 34, ml <= 36, off <= 40: around the 16-
and 32-byte register widths), sparse at the larger edges (48, 64, 80, 128, 256,
1024 and the 1040 of a 1024 + 16 overshoot), and hold chains of dependent
sequences longer than a 64-sequence wave group.  check_coverage() states what
the lists promise; tests/test_seq_frames.py asserts it."""
from __future__ import annotations

import functools
import random
import struct
import zlib

import numpy as np

DENSE_LL = 34   # ll in [0, 34]
DENSE_ML = 36   # ml in [min_match, 36]
DENSE_OFF = 40  # off in [1, 40]
EDGES = (47, 48, 49, 63, 64, 65, 66, 79, 80, 81, 127, 128, 129, 255, 256, 1023, 1024, 1025, 1040)
LEAD = 1100     # literals opening a block: every off <= 1040 is expressible right after them
TAIL = 12       # literals closing a block (liblz4: last match >= 12 bytes before the end, last 5 literals)
BLOCK = 40 << 10
SEEDS = 4
PHASES = 4      # every dense triple starts at >= 4 distinct output positions mod 32

# what each codec can express: (least match, greatest match)
LZ4, SNAPPY, GZIP, ZSTD = (4, 1 << 20), (1, 64), (3, 258), (3, 1 << 20)


# ------------------------------------------------------------------ literals
def literals(n: int, salt: int = 0) -> bytes:
    """n literal bytes: one of 16 symbols chosen by a stride-11 walk, with bits
    of the position counter mixed into bits 4-6 -- neighbours always differ, and
    no copy displaced by a byte or by 1, 2 or 7 bits gives the same run."""
    k = np.arange(n, dtype=np.int64) + salt * 977
    sym = (k * 11 + (k >> 4) * 7 + (k >> 9) * 5) & 15
    mix = ((k >> 1) ^ (k >> 6) ^ (k >> 11)) & 3
    return (0x41 + sym + (mix << 4)).astype(np.uint8).tobytes()


# ------------------------------------------------------------------ geometry
class Block:
    """One block's program: sequences (the first carries the LEAD literals when
    `lead`), then `tail` literals; `salt` picks the literal stream."""

    def __init__(self, seqs, tail=TAIL, salt=0, lead=True):
        self.seqs, self.tail, self.salt, self.lead = list(seqs), tail, salt, lead

    @property
    def nlit(self):
        return sum(s[0] for s in self.seqs) + self.tail

    @property
    def size(self):
        return sum(s[0] + s[1] for s in self.seqs) + self.tail


def dense_triples(mm: int, mx: int):
    return [(ll, ml, off) for ll in range(DENSE_LL + 1) for ml in range(mm, min(DENSE_ML, mx) + 1)
            for off in range(1, DENSE_OFF + 1)]


def edge_triples(mm: int, mx: int):
    """Each edge value on each axis against a sparse set on the other two, the
    edge x edge pairs of (ml, off) and (ll, off), and every match length up to
    258 (deflate's longest) against a few distances on both sides of 16."""
    lls = (0, 1, 15, 16, 17, 33)
    mls = tuple(m for m in (mm, mm + 1, 15, 16, 17, 18, 35) if m <= mx)
    offs = (1, 2, 7, 8, 15, 16, 17, 31, 32, 33)
    out = []
    for e in EDGES:
        out += [(e, ml, off) for ml in mls for off in offs]
        out += [(e, ml, e + k) for ml in mls for k in (-1, 1, 3, 15, 16, 17)]  # rel = ll - off around 0 and -16
        if e <= mx:
            out += [(ll, e, off) for ll in lls for off in offs]
        out += [(ll, ml, e) for ll in lls for ml in mls]
        for e2 in EDGES:
            if e2 <= mx:
                out.append(((e + e2) % 23, e2, e))
            out.append((e, mls[(e + e2) % len(mls)], e2))
    for ll in range(DENSE_LL + 1, 67):  # every literal length a snappy tag holds itself (<= 60), and the next forms
        out += [(ll, mls[ll % len(mls)], off) for off in (1, 15, 16, 17, 40)]
    for ml in range(DENSE_ML + 1, min(258, mx) + 1):
        out += [((ml * 7 + off) % 20, ml, off) for off in (1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 40, 255, 256, 1024)]
    return out


def chains(rng: random.Random, mm: int, mx: int):
    """Runs of 70 and 130 consecutive dependent sequences: the match source
    starts inside the previous sequence's match ("prev"), inside this
    sequence's own literals (rel = ll - off >= 0: "own"), or less than 16 bytes
    before them (-16 < rel < 0: "straddle"), and a mix of the three."""
    out = []
    for kind in ("prev", "own", "straddle", "mixed"):
        for n in (70, 130):
            run, prev_ml = [], mm
            for _ in range(n):
                k = kind if kind != "mixed" else rng.choice(("prev", "own", "straddle"))
                ll = rng.randint(1 if k != "prev" else 0, 24)
                ml = rng.randint(mm, min(40, mx))
                if k == "prev":
                    off = ll + rng.randint(1, prev_ml)
                elif k == "own":
                    off = rng.randint(1, ll)
                else:
                    off = ll + rng.randint(1, min(15, prev_ml))
                run.append((ll, ml, off))
                prev_ml = ml
            out.append(run)
    return out


@functools.lru_cache(maxsize=None)
def grid(mm: int, mx: int):
    """[seed][block] -> Block.  Every seed holds every dense, edge and chain
    sequence once, in an order shuffled by the seed; a dense triple is placed
    only at an output position (mod 32) where no earlier seed placed it -- a
    one-sequence spacer (1, mm, 1) shifts the position when nothing in the
    look-ahead window fits."""
    dense = dense_triples(mm, mx)
    seen = {t: set() for t in dense}
    seeds = []
    for seed in range(SEEDS):
        rng = random.Random(0x5E9 + seed)
        units = [("d", t) for t in dense] + [("e", t) for t in edge_triples(mm, mx)]
        units += [("c", run) for run in chains(rng, mm, mx)]
        rng.shuffle(units)
        blocks, seqs, pos = [], None, 0
        window, it = [], iter(units)

        def open_block():
            nonlocal seqs, pos
            lead = LEAD + 3 * seed + len(blocks) % 29
            seqs, pos = [(lead, mm, 1)], lead + mm

        open_block()
        while True:
            while len(window) < 48:
                u = next(it, None)
                if u is None:
                    break
                window.append(u)
            if not window:
                break
            ph = pos % 32
            j = next((j for j, u in enumerate(window) if u[0] != "d" or ph not in seen[u[1]]), None)
            if j is None:
                seqs.append((1, mm, 1))
                pos += 1 + mm
                continue
            kind, v = window.pop(j)
            for t in ([v] if kind != "c" else v):
                if kind == "d":
                    seen[t].add(pos % 32)
                seqs.append(t)
                pos += t[0] + t[1]
            if pos >= BLOCK:
                blocks.append(Block(seqs, salt=seed * 1000 + len(blocks)))
                open_block()
        if len(seqs) > 1:
            blocks.append(Block(seqs, salt=seed * 1000 + len(blocks)))
        seeds.append(blocks)
    return seeds


def check_blocks(seeds, mm: int, mx: int, phases: int = PHASES, max_size: int = 64 << 10):
    """What the given [seed][block] lists hold, counted from the lists alone:
    every seed holds every dense and edge triple (off inside the bytes produced
    wherever the block opens its own history); over the seeds every dense
    triple starts at >= `phases` distinct output positions mod 32; a run of
    more than 64 consecutive dependent sequences exists; every edge value
    appears on every axis the codec can express.  -> (dense triples, the
    longest dependent run)."""
    dense = set(dense_triples(mm, mx))
    want = dense | set(edge_triples(mm, mx))
    seen = {t: set() for t in dense}
    longest = 0
    for blocks in seeds:
        got = set()
        for b in blocks:
            pos, run = 0, 0
            assert b.size <= max_size, b.size
            for i, (ll, ml, off) in enumerate(b.seqs):
                assert mm <= ml <= mx and off >= 1 and (not b.lead or off <= pos + ll), (ll, ml, off, pos)
                if (ll, ml, off) in dense:
                    seen[(ll, ml, off)].add(pos % 32)
                got.add((ll, ml, off))
                # a dependent sequence: its source starts at or after the previous match's start
                dep = i > 0 and off <= ll + b.seqs[i - 1][1]
                run = run + 1 if dep else 0
                longest = max(longest, run)
                pos += ll + ml
        assert want <= got, (len(want - got), sorted(want - got)[:5])
    few = [t for t, p in seen.items() if len(p) < phases]
    assert not few, (len(few), few[:5])
    assert longest > 64, longest  # crosses a 64-sequence wave group
    for e in EDGES:
        for axis in range(3):
            if axis == 1 and e > mx:
                continue
            assert any(t[axis] == e for b in seeds[0] for t in b.seqs), (axis, e)
    return len(dense), longest


def check_coverage(mm: int, mx: int):
    """What grid() promises."""
    return check_blocks(grid(mm, mx), mm, mx)


def blocks_of(frames):
    """The Blocks of a list of (frame, parts, linked)."""
    return [p for _, parts, _ in frames for p in parts if isinstance(p, Block)]


def model(block: Block, hist: bytes = b"") -> bytes:
    """The block's decoded bytes by the definition of LZ77, a byte at a time."""
    out = bytearray(hist)
    lits = literals(block.nlit, block.salt)
    lp = 0
    for ll, ml, off in block.seqs:
        out += lits[lp:lp + ll]
        lp += ll
        assert 1 <= off <= len(out), (ll, ml, off, len(out))
        for _ in range(ml):
            out.append(out[-off])
    out += lits[lp:lp + block.tail]
    return bytes(out[len(hist):])


def one_geometry(fill: int, ll: int, ml: int, off: int, mm: int = 4) -> Block:
    """A block holding the one sequence (ll, ml, off) at an output position
    that is `fill` mod 32: what a failing sweep is reduced to."""
    return Block([(LEAD + (fill - LEAD - mm) % 32, mm, 1), (ll, ml, off)], salt=fill)


# (fill, ll, ml, off): the sequences at which the sweeps caught one-token changes
# of the engines' conditions (each named for the condition it pins), kept as
# one-geometry frames of their own
NAMED = {
    "lane_period_step_off9": (14, 29, 22, 9),        # step = off * (16 / off), copy_pattern
    "lane_period_step_off13": (28, 34, 33, 13),      # the same in the lane's register path
    "lane_two_chunks_off25": (23, 12, 31, 25),       # off < 16 * nch: a 2-chunk match overlapping itself
    "lane_rel_minus17": (31, 23, 26, 40),            # rel + 16 < 0: the second chunk starts one byte before the literals
    "wc_period_step_off14": (25, 34, 21, 14),
    "wc_period_step_off7": (4, 12, 18, 7),
    "wc_rel_minus17": (25, 22, 24, 39),
    "wc_two_chunks_off27": (29, 16, 28, 27),
    "inflate_dist11_len31": (29, 21, 31, 11),        # dist >= 16 || dist >= len
}


def named_blocks(mm: int, mx: int):
    return [one_geometry(fill, ll, min(ml, mx), off, mm) for fill, ll, ml, off in NAMED.values()]


def no_lead(block: Block) -> Block:
    """The block without its opening literals (for a block that continues a
    linked LZ4 frame: its first offsets reach into the previous block)."""
    return Block(block.seqs[1:], tail=block.tail, salt=block.salt + 500, lead=False)


def fill_to(block: Block, size: int) -> Block:
    """The block extended by one long match so that it decodes to exactly `size`."""
    rest = size - block.size
    assert rest >= 4
    return Block(block.seqs + [(0, rest, 3)], tail=block.tail, salt=block.salt, lead=block.lead)


def far_block(hist: int, salt: int = 0, top: int = 65535, mx: int = 1 << 20) -> Block:
    """Sequences whose matches reach `hist` bytes of history before the block:
    the greatest offset the history allows at each position (up to `top`), and
    the 2-byte form's last values."""
    seqs, pos = [], 0
    for ll, ml in ((2, 4), (0, 5), (17, 31), (1, 16), (16, 17), (33, 64), (0, 300), (5, 18), (15, 15), (3, 7)):
        for off in (min(top, hist + pos + ll), min(top, hist + pos + ll) - 1, min(top, hist) - 13, 65535 if
                    hist + pos + ll >= 65535 and top >= 65535 else 40, 2048, 2047, 2049, 65534, 65536, 65537):
            if 1 <= off <= hist + pos + ll and off <= top:
                ml = min(ml, mx)
                seqs.append((ll, ml, off))
                pos += ll + ml
    return Block(seqs, salt=salt + 77, lead=False)


# ------------------------------------------------------------------ LZ4
def _lz4_len(r: int) -> bytes:
    return b"\xff" * (r // 255) + bytes([r % 255])


def lz4_block(block: Block) -> bytes:
    """The raw LZ4 block: token, literal length bytes, literals, offset, match
    length bytes per sequence; the tail as last literals."""
    lits = literals(block.nlit, block.salt)
    out, lp = bytearray(), 0
    for ll, ml, off in block.seqs:
        lt, mt = min(ll, 15), min(ml - 4, 15)
        out.append(lt << 4 | mt)
        if lt == 15:
            out += _lz4_len(ll - 15)
        out += lits[lp:lp + ll]
        lp += ll
        out += struct.pack("<H", off)
        if mt == 15:
            out += _lz4_len(ml - 19)
    lt = min(block.tail, 15)
    out.append(lt << 4)
    if lt == 15:
        out += _lz4_len(block.tail - 15)
    out += lits[lp:lp + block.tail]
    return bytes(out)


def lz4_run_block(n: int, c: bytes = b"a", tail: bytes = b"12345") -> bytes:
    """An LZ4 block decoding to n bytes: c, a run of it (offset 1), then tail."""
    return bytes([0x1F]) + c + struct.pack("<H", 1) + _lz4_len(n - 1 - len(tail) - 4 - 15) + bytes([len(tail) << 4]) + tail


def lz4_frame(blocks, content=None, linked=False) -> bytes:
    """An LZ4 frame (64 KiB blocks, no checksums) around the given blocks:
    bytes = a compressed block, (bytes, True) = a stored one; independent or
    linked (FLG bit 5 clear), with or without a content size."""
    import xxhash

    desc = bytes([0x40 | (0 if linked else 0x20) | (0x08 if content is not None else 0), 0x40])
    desc += struct.pack("<Q", content) if content is not None else b""
    f = struct.pack("<I", 0x184D2204) + desc + bytes([(xxhash.xxh32(desc, seed=0).intdigest() >> 8) & 0xFF])
    for b in blocks:
        if isinstance(b, tuple):
            f += struct.pack("<I", len(b[0]) | 0x80000000) + b[0]
        else:
            f += struct.pack("<I", len(b)) + b
    return f + b"\0\0\0\0"


def model_frame(parts, linked: bool = False) -> bytes:
    """What a frame of the given parts (Block, or bytes decoding to themselves)
    decodes to; `linked`: a block's matches may reach the parts before it."""
    out = b""
    for p in parts:
        out += p if isinstance(p, bytes) else model(p, hist=out if linked else b"")
    return out


def _size(parts):
    return sum(len(p) if isinstance(p, bytes) else p.size for p in parts)


def _lz4(parts, content: bool, linked: bool) -> bytes:
    return lz4_frame([(p, True) if isinstance(p, bytes) else lz4_block(p) for p in parts],
                     content=_size(parts) if content else None, linked=linked)


def lz4_lane(seed: int):
    """(frame, parts, linked) for slots the lane decoder takes: every grid block as a
    one-block frame (independent / linked, with / without a content size in
    turn); linked frames of two grid blocks, the second opening inside the
    first's bytes; a stored block of 65,530 bytes then offsets up to 65,535
    into it (history just under 64 KiB)."""
    blocks = grid(*LZ4)[seed]
    out = [(_lz4([b], bool(i & 1), bool(i & 2)), [b], bool(i & 2)) for i, b in enumerate(blocks)]
    for i in range(0, min(len(blocks) - 1, 12), 2):
        pair = [blocks[i], no_lead(blocks[i + 1])]
        out.append((_lz4(pair, bool(i & 2), True), pair, True))
    pad = literals(65530, seed + 3)
    far = [pad, far_block(65530, seed)]
    out.append((_lz4(far, bool(seed & 1), True), far, True))
    return out


def lz4_parts(seed: int, per: int = 5):
    """Independent-block frames above the split threshold holding every grid
    block of the seed: a run block of exactly 64 KiB, then `per` grid blocks,
    all but the last filled to exactly 64 KiB (each ends at its part's
    capacity), the last one short."""
    blocks = grid(*LZ4)[seed]
    run = b"a" * (65536 - 5) + b"12345"
    out = []
    for i in range(0, len(blocks), per):
        g = blocks[i:i + per]
        parts = [fill_to(b, 65536) for b in g[:-1]] + [g[-1]]
        f = lz4_frame([lz4_run_block(65536)] + [lz4_block(p) for p in parts],
                      content=65536 + _size(parts) if (i // per) & 1 else None)
        out.append((f, [run] + parts, False))
    return out


def lz4_wave(seed: int, per: int = 5):
    """Linked-block frames (a linked frame has no split plan) holding every
    grid block of the seed, five a frame (bound above 256 KiB), each block
    after the first opening inside the previous block; and two frames with a
    stored block and offsets up to 65,535 with the history just under (a stored
    block of 65,530 bytes first) and over 64 KiB."""
    blocks = grid(*LZ4)[seed]
    out = []
    for i in range(0, len(blocks) - per + 1, per):
        g = blocks[i:i + per] + (blocks[i + per:] if len(blocks) - i - per < per else [])
        parts = [g[0]] + [no_lead(b) for b in g[1:]]
        out.append((_lz4(parts, bool((i // per) & 1), True), parts, True))
    g = blocks[:4]
    pad = literals(65530, seed * 7)
    under = [pad, far_block(65530, 1), no_lead(g[0]), no_lead(g[1]), g[2], no_lead(g[3])]
    hist = g[0].size + no_lead(g[1]).size + 65530
    over = [g[0], no_lead(g[1]), pad, far_block(hist, 0), no_lead(g[2]), g[3]]
    out += [(_lz4(under, False, True), under, True), (_lz4(over, True, True), over, True)]
    return out


# ------------------------------------------------------------------ snappy
def _varint(v: int) -> bytes:
    out = bytearray()
    while v >= 128:
        out.append(v & 127 | 128)
        v >>= 7
    out.append(v)
    return bytes(out)


def snappy_literal(data: bytes, width: int = 0) -> bytes:
    """A literal tag: 1..60 in the tag itself, else (or when `width` asks) the
    60..63 forms with 1..4 length bytes."""
    n = len(data) - 1
    need = 0 if n < 60 else (n.bit_length() + 7) // 8
    w = max(need, width)
    if w == 0:
        return bytes([n << 2]) + data
    return bytes([(59 + w) << 2]) + n.to_bytes(w, "little") + data


def snappy_copy(ml: int, off: int, form: int = 0) -> bytes:
    """A copy tag in the shortest form that holds it, or a wider one (`form`
    2 / 3: the 2- / 4-byte offset forms)."""
    if form < 2 and 4 <= ml <= 11 and off < 2048:
        return bytes([1 | (ml - 4) << 2 | (off >> 8) << 5, off & 255])
    if form < 3 and off < 65536:
        return bytes([2 | (ml - 1) << 2]) + struct.pack("<H", off)
    return bytes([3 | (ml - 1) << 2]) + struct.pack("<I", off)


def snappy_chunk(block: Block, pad: bytes = b"") -> bytes:
    """The raw snappy stream of the block (length preamble, then tags; `pad` as
    one more literal at the end); the tag forms vary with the sequence's index."""
    lits = literals(block.nlit, block.salt)
    out, lp = bytearray(_varint(block.size + len(pad))), 0
    for i, (ll, ml, off) in enumerate(block.seqs):
        if ll:
            out += snappy_literal(lits[lp:lp + ll], width=(0, 0, 1, 0, 2, 0, 0, 3, 0, 0, 4)[i % 11])
            lp += ll
        out += snappy_copy(ml, off, form=(0, 0, 2, 0, 0, 0, 3)[i % 7])
    if block.tail:
        out += snappy_literal(lits[lp:lp + block.tail])
    if pad:
        out += snappy_literal(pad, width=4)
    return bytes(out)


def snappy_java(chunks) -> bytes:
    """snappy-java framing: magic, version 1, least compatible version 1, then
    {big-endian length, raw snappy chunk} -- what orc.compress(2, ...) writes."""
    f = b"\x82SNAPPY\x00" + struct.pack("<II", 1, 1)
    for c in chunks:
        f += struct.pack(">I", len(c)) + c
    return f


def snappy_lane(seed: int):
    """(frame, parts, linked=False): every grid block as a one-chunk snappy-java body (every
    fifth as a raw snappy stream without the framing), and one chunk of 66,000 literals then copies with offsets across the 2-byte
    form's end (65,535 / 65,536: the 4-byte form)."""
    blocks = grid(*SNAPPY)[seed]
    out = []
    for i, b in enumerate(blocks):
        c = snappy_chunk(b)
        out.append((c if i % 5 == 4 else snappy_java([c]), [b], False))
    far = far_block(66000 + 4, seed, top=66100, mx=64)
    far = Block([(66000, 4, 1)] + far.seqs, salt=far.salt)
    out.append((snappy_java([snappy_chunk(far)]), [far], False))
    return out


def snappy_parts(seed: int, per: int = 5):
    """snappy-java bodies above the split threshold holding every grid chunk
    of the seed: a 70,000-byte literal chunk, then `per` grid chunks (each
    part's capacity is its exact length)."""
    blocks = grid(*SNAPPY)[seed]
    out = []
    for i in range(0, len(blocks), per):
        pad = literals(70000, seed + i)
        parts = [pad] + blocks[i:i + per]
        out.append((snappy_java([_varint(len(pad)) + snappy_literal(pad, width=3 + (i // per & 1))]
                                + [snappy_chunk(b) for b in parts[1:]]), parts, False))
    return out


def merged(blocks) -> Block:
    """The blocks as one: each tail becomes part of the next block's opening literals."""
    seqs, carry = [], 0
    for b in blocks:
        ll, ml, off = b.seqs[0]
        seqs += [(ll + carry, ml, off)] + b.seqs[1:]
        carry = b.tail
    return Block(seqs, tail=carry, salt=blocks[0].salt + 300)


def snappy_wave(seed: int, per: int = 7):
    """Raw snappy streams (no snappy-java framing: no split plan) holding
    every grid block of the seed, seven merged into one stream (above 256 KiB);
    what is left over is padded with a 262,144-byte literal."""
    blocks = grid(*SNAPPY)[seed]
    out = []
    for i in range(0, len(blocks), per):
        m = merged(blocks[i:i + per])
        pad = literals(262144, seed * 5 + i) if m.size <= 262144 else b""
        out.append((snappy_chunk(m, pad), [m] + ([pad] if pad else []), False))
    return out


# ------------------------------------------------------------------ gzip
def _rev(v: int, n: int) -> int:
    r = 0
    for _ in range(n):
        r = r << 1 | v & 1
        v >>= 1
    return r


def _fixed_tables():
    lit = []
    for s in range(288):
        if s < 144:
            c, n = 0x30 + s, 8
        elif s < 256:
            c, n = 0x190 + s - 144, 9
        elif s < 280:
            c, n = s - 256, 7
        else:
            c, n = 0xC0 + s - 280, 8
        lit.append((_rev(c, n), n))
    lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    lext = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
    dbase = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073,
             4097, 6145, 8193, 12289, 16385, 24577]
    dext = [0, 0, 0, 0] + [k for k in range(1, 14) for _ in (0, 1)]
    lens = {}
    for ml in range(3, 259):
        k = max(i for i in range(29) if lbase[i] <= ml)
        code, n = lit[257 + k]
        lens[ml] = (code | (ml - lbase[k]) << n, n + lext[k])
    return lit, lens, dbase, dext


_LIT, _LEN, _DBASE, _DEXT = _fixed_tables()


def deflate_fixed(block: Block) -> bytes:
    """One final fixed-Huffman deflate block (RFC 1951 3.2.6) of the program."""
    import bisect

    lits = literals(block.nlit, block.salt)
    acc, nb = 3, 3  # BFINAL = 1, BTYPE = 01
    lp = 0
    chunks = []
    for ll, ml, off in block.seqs + [(block.tail, 0, 0)]:
        for b in lits[lp:lp + ll]:
            c, n = _LIT[b]
            acc |= c << nb
            nb += n
        lp += ll
        if ml:
            c, n = _LEN[ml]
            acc |= c << nb
            nb += n
            k = bisect.bisect_right(_DBASE, off) - 1
            acc |= (_rev(k, 5) | (off - _DBASE[k]) << 5) << nb
            nb += 5 + _DEXT[k]
        if nb >= 4096:
            chunks.append((acc & ((1 << (nb & ~7)) - 1)).to_bytes(nb >> 3, "little"))
            acc >>= nb & ~7
            nb &= 7
    nb += 7  # end of block: seven zero bits
    chunks.append(acc.to_bytes((nb + 7) >> 3, "little"))
    return b"".join(chunks)


def gzip_member(block: Block, decoded: bytes) -> bytes:
    """A gzip member around deflate_fixed(block); CRC32 and ISIZE from `decoded`."""
    return (b"\x1f\x8b\x08\x00\x00\x00\x00\x00\x00\x03" + deflate_fixed(block)
            + struct.pack("<II", zlib.crc32(decoded), len(decoded) & 0xFFFFFFFF))


def chunk_ends(n: int, total: int):
    """The ends of the wrapper's output chunks below `total` for an n-byte
    input: the first chunk holds min(128 KiB, 2 min(128 KiB, 3 n)) bytes, each
    next one twice the previous up to 128 KiB."""
    size = min(128 << 10, 2 * min(128 << 10, 3 * n))
    end, out = size, []
    while end < total:
        out.append(end)
        size = min(128 << 10, 2 * size)
        end += size
    return out


def chunk_crossings(block: Block, n: int):
    """(ll, ml, dist) of every copy of the block with a chunk end strictly inside it."""
    ends = chunk_ends(n, block.size)
    out, pos = [], 0
    for ll, ml, off in block.seqs:
        if any(pos + ll < e < pos + ll + ml for e in ends):
            out.append((ll, ml, off))
        pos += ll + ml
    return out


@functools.lru_cache(maxsize=None)
def gzip_chunk_blocks():
    """Bodies whose copies straddle the wrapper's output-chunk ends, for each
    (dist, len) of dist < 16 / >= 16 crossed with dist < len / >= len: the
    first chunk is 6 x the member's length, so `lead` literals and a run of
    258-byte copies bring the output up to it, and 120 copies of the length
    under test lie across it -- the number of long copies is searched until a
    chunk end falls strictly inside one of those (up to two more literals in
    the lead shift it by a byte)."""
    out = []
    for dist in (1, 2, 3, 7, 8, 15, 16, 17, 31, 40):
        for ml in (3, 8, 10, 15, 17, 40, 100, 258):
            for lead in (dist, 40 + dist % 3):
                for longs, extra in ((a, b) for a in range(80) for b in range(3)):
                    seqs = [(lead + extra, 258, dist)] + [(0, 258, dist)] * longs + [(0, ml, dist)] * 120
                    b = Block(seqs, tail=3, salt=lead * 41 + dist, lead=False)
                    if any(c[1] == ml for c in chunk_crossings(b, len(deflate_fixed(b)) + 18)[1 if ml == 258 else 0:]):
                        out.append(b)
                        break
                else:
                    raise AssertionError((dist, ml, lead))
    return out


def gzip_lane(seed: int):
    """(frame, parts, linked=False): every grid block as a gzip member; with seed 0 the
    chunk-end bodies as well."""
    out = []
    for b in grid(*GZIP)[seed] + (list(gzip_chunk_blocks()) if seed == 0 else []):
        out.append((gzip_member(b, model(b)), [b], False))
    return out


def named_frames():
    """(codec, frame, parts, linked=False): the NAMED geometries as one-block frames of
    LZ4, snappy-java and gzip (zstd's are in the fixture)."""
    out = [(3, _lz4([b], True, False), [b], False) for b in named_blocks(*LZ4)]
    out += [(2, snappy_java([snappy_chunk(b)]), [b], False) for b in named_blocks(*SNAPPY)]
    out += [(1, gzip_member(b, model(b)), [b], False) for b in named_blocks(*GZIP)]
    return out


# ------------------------------------------------------------------ invalid
def invalid_frames(defined_only: bool = False):
    """(codec, frame): geometries a decoder must reject or, where the library
    lets them pass, decode as the library does -- only the verdict is pinned.
    A zero offset, offsets one past the history (in a first block and, linked,
    past the previous block), matches ending inside liblz4's last-5 and
    last-12 zones.  defined_only: without the LZ4 frames with a zero offset,
    which liblz4 decodes from bytes nobody wrote (no defined content)."""
    out = []
    first = (30, 8, 1)
    for off in (0, 31 + 8 + 20 + 1, 65535):
        bad = Block([first, (20, 8, off)], salt=off)
        if off or not defined_only:
            out.append((3, lz4_frame([lz4_block(bad)])))
            out.append((3, lz4_frame([lz4_block(bad)], content=bad.size)))
        if off:
            out.append((2, snappy_java([snappy_chunk(bad)])))
            out.append((2, snappy_chunk(bad)))
            out.append((1, gzip_member(bad, b"")))
    out.append((2, snappy_java([_varint(60) + snappy_literal(literals(30)) + snappy_copy(8, 0, form=2)
                               + snappy_literal(literals(22))])))
    prev = Block([first], salt=1)
    out.append((3, lz4_frame([lz4_block(prev), lz4_block(Block([(5, 9, prev.size + 5 + 1)], salt=2, lead=False))],
                             linked=True)))
    out.append((3, lz4_frame([lz4_block(prev), lz4_block(Block([(5, 9, prev.size + 5)], salt=2, lead=False))])))
    for tail in (0, 1, 4, 5, 11):
        out.append((3, lz4_frame([lz4_block(Block([first, (7, 19, 3)], tail=tail, salt=tail))])))
        out.append((3, lz4_frame([lz4_block(Block([first, (7, 19, 3)], tail=tail, salt=tail))], content=30 + 8 + 26 + tail)))
    return out


# ------------------------------------------------------------------ zstd
def zstd_resolve(ops, rep):
    """(ll, ml, offset value) -> (ll, ml, off) under the repeat-offset rules of
    RFC 8878 3.1.1.5 (offset values 1..3 name a repeat offset, shifted by one
    when ll = 0), updating rep (a 3-list) in place."""
    out = []
    for ll, ml, ofv in ops:
        if ofv > 3:
            off = ofv - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            k = ofv - 1 + (1 if ll == 0 else 0)
            if k == 0:
                off = rep[0]
            elif k == 1:
                off = rep[1]
                rep[:] = [off, rep[0], rep[2]]
            else:
                off = rep[0] - 1 if k == 3 else rep[2]
                rep[:] = [off, rep[0], rep[1]]
        out.append((ll, ml, off))
    return out


def zstd_ops(block: Block, rep, rng: random.Random | None):
    """The block as zstd sequences (ll, ml, offset value).  Every sequence of
    the block stays what it is, at the output position (mod 32) it has: its
    offset value is off + 3, or -- with an rng -- a repeat-offset code where
    that resolves to the same offset.  With an rng, about one sequence in
    eight is preceded by two extra sequences with repeat-offset codes, the
    first with ll = 0 (which shifts the codes' meaning), the second with or
    without, 32 or 64 bytes together.  The block's first three sequences stay
    explicit, so what it decodes to does not depend on the repeat offsets
    before it.  Returns the operations and the Block they resolve to."""
    ops, res, pos = [], [], 0

    def put(op):
        nonlocal pos
        ops.append(op)
        res.append(zstd_resolve([op], rep)[0])
        pos += op[0] + op[1]

    def code_for(ll, want=None):
        for code in rng.sample((1, 2, 3), 3):
            o = zstd_resolve([(ll, 3, code)], list(rep))[0][2]
            if (1 <= o <= pos + ll) if want is None else o == want:
                return code
        return None

    for i, (ll, ml, off) in enumerate(block.seqs):
        if rng is not None and i >= 3 and rng.random() < 0.125:
            total = 32 * rng.randint(1, 2)
            ll2 = 0 if rng.random() < 0.5 else rng.randint(1, 20)
            ml1 = rng.randint(3, total - ll2 - 3)
            for ell, emm in ((0, ml1), (ll2, total - ll2 - ml1)):
                code = code_for(ell)
                put((ell, emm, code) if code else (ell, emm, rep[0] + 3))
        code = code_for(ll, off) if rng is not None and i >= 3 and rng.random() < 0.5 else None
        put((ll, ml, code if code else off + 3))
        assert res[-1] == (ll, ml, off)
    return ops, Block(res, tail=block.tail, salt=block.salt, lead=block.lead)


def zstd_geometry_file(frames) -> bytes:
    """The input of `zstd_fuzz --dump-seqgrid`: per frame u32 block count,
    flags (1: Huffman-compressed literals, 2: no content size, a 1 MiB window
    instead), pad (bytes of RLE blocks after the grid blocks); per block u32
    sequence count, literal count, the literals, then (ll, ml, offset value)
    as u32 each.  frames: (flags, pad, [(ops, Block)])."""
    out = bytearray()
    for flags, pad, blocks in frames:
        out += struct.pack("<III", len(blocks), flags, pad)
        for ops, b in blocks:
            out += struct.pack("<II", len(ops), b.nlit) + literals(b.nlit, b.salt)
            out += np.array(ops, dtype="<u4").tobytes()
    return bytes(out)


def zstd_frames(seed: int, reps: bool):
    """[(ops, resolved Block)] per frame for one seed of the grid: one grid
    block a frame."""
    rng = random.Random(0x2E9 + seed) if reps else None
    return [[zstd_ops(b, [1, 4, 8], rng)] for b in grid(*ZSTD)[seed]]


ZSTD_HUF, ZSTD_NO_FCS = 1, 2
# per seed: literal mode / header of the frames, repeat-offset codes or not
ZSTD_VARIANTS = ((0, False), (0, True), (ZSTD_HUF, True), (ZSTD_NO_FCS, True))


def zstd_lane(seed: int):
    """(flags, pad, blocks) per frame: one grid block a frame, decoded size
    below the 64 KiB at which the large-frame decoders take over."""
    flags, reps = ZSTD_VARIANTS[seed]
    return [(flags, 0, fb) for fb in zstd_frames(seed, reps)]


def zstd_splice(frames, sizes, pad: int) -> bytes:
    """One frame (with a content size) of the blocks of the given one-block
    frames and `pad` bytes of RLE blocks of up to 128 KiB: a large slot for
    four bytes per block.  sizes: what each frame decodes to."""
    body = b""
    for f in frames:
        h = 9 if f[4] == 0xA0 else 6
        bh = int.from_bytes(f[h:h + 3], "little")
        assert bh & 1 and (bh >> 1) & 3 == 2 and h + 3 + (bh >> 3) == len(f)
        body += (bh & ~1).to_bytes(3, "little") + f[h + 3:]
    left = pad
    assert pad > 0
    while left:
        n = min(left, 128 << 10)
        left -= n
        body += ((0 if left else 1) | 1 << 1 | n << 3).to_bytes(3, "little") + bytes([ord("p") + (left >> 17)])
    return b"\x28\xb5\x2f\xfd\xa0" + struct.pack("<I", sum(sizes) + pad) + body


def zstd_big(seed: int, lane_frames, per: int = 5, pad: int = 256 << 10):
    """(frame, program) holding every lane frame's block of the seed, `per` a
    frame, padded past 256 KiB (a content size above 64 KiB): for the wave and
    block-parallel decoders.  lane_frames: the seed's encoded lane frames."""
    progs = zstd_lane(seed)
    assert len(progs) == len(lane_frames)
    out = []
    for i in range(0, len(progs), per):
        blocks = [fb[0] for _, _, fb in progs[i:i + per]]
        f = zstd_splice(lane_frames[i:i + per], [b.size for _, b in blocks], pad)
        out.append((f, (progs[i][0] & ~ZSTD_NO_FCS, pad, blocks)))
    return out


def zstd_invalid():
    """Offsets one and many past the bytes produced, and a repeat-offset code
    that resolves to zero: verdicts only."""
    out = []
    for ofv in (30 + 8 + 20 + 1 + 3, 70000 + 3):
        b = Block([(30, 8, 1), (20, 8, 7)], salt=ofv)
        out.append((0, 0, [([(30, 8, 4), (20, 8, ofv)], b)]))
    b = Block([(30, 8, 1), (0, 8, 1)], salt=5)
    out.append((0, 0, [([(30, 8, 4), (0, 8, 3)], b)]))
    return out


def zstd_fixture():
    """What tests/golden/zstd_seqgrid.npz holds: every lane frame of each seed, the
    invalid ones, the named ones (the large frames are spliced from the lane
    frames: zstd_big).  -> (kind, (flags, pad, blocks)) with kind
    10 + seed: a lane frame, 2 invalid, 3 a named one-geometry frame."""
    out = []
    for seed in range(SEEDS):
        out += [(10 + seed, f) for f in zstd_lane(seed)]
    out += [(2, f) for f in zstd_invalid()]
    out += [(3, (0, 0, [zstd_ops(b, [1, 4, 8], None)])) for b in named_blocks(*ZSTD)]
    return out


def zstd_model(frame) -> bytes:
    flags, pad, blocks = frame
    out = model_frame([b for _, b in blocks], linked=True)
    left = pad
    while left:
        n = min(left, 128 << 10)
        left -= n
        out += bytes([ord("p") + (left >> 17)]) * n
    return out


def read_frames(raw: bytes):
    """Frames from a u32-length-prefixed file (what the fuzzers' --dump-* and
    --frames modes write and read)."""
    out, p = [], 0
    while p < len(raw):
        n = int.from_bytes(raw[p:p + 4], "little")
        out.append(raw[p + 4:p + 4 + n])
        p += 4 + n
    return out


def write_frames(frames) -> bytes:
    return b"".join(struct.pack("<I", len(f)) + f for f in frames)
