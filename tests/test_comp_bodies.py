"""The match-geometry bodies of tests/comp_bodies.py on the host.

  coverage    what the reference's compressors emitted for the bodies, read
              back from the oracle's output alone by two small parsers (LZ4
              frame -> blocks -> sequences, snappy-java -> chunks -> tags): the
              literal-run, match-length and offset codes, the block, table and
              fragment sizes and the stored / compressed edge the sweep
              promises to visit
  carried     the host build of the engine's restatements over every body in
              file order with one carried table per codec (tests/native/
              compress_fuzz.cpp --bodies): bytes against the oracle for LZ4 /
              snappy, twice (the second time across the generation wrap), the
              round trip for gzip / zstd
  teeth       one-token changes of rpgpu_lz4c.h / rpgpu_snappyc.h that the
              carried run must reject, each applied to a copy of the sources

Three one-token changes are equivalent and deliberately not MUTANTS:
`(mc + 239) / 255` in LZ4's match bound and `(lit + 1) / 255` in its literal
bound only make compress_block return 0 sooner than the exact last-literals
check, which every block reaches and which decides alone whether the block is
stored; `n > kInputMargin` in compress_fragment differs only for a 15-byte
block, in which ip_limit = 0 ends the search at its first step either way."""
import os
import shutil
import struct
import subprocess
import sys
from collections import Counter
from pathlib import Path

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import comp_bodies as cb  # noqa: E402
from test_compress import build_fuzzer  # noqa: E402

import oracle.oracle as orc  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]


# ------------------------------------------------------------------- parsers
def lz4_blocks(frame: bytes) -> list:
    """LZ4 frame -> per block dict(size, csize, stored, seqs [(ll, ml, off)], last)."""
    assert frame[:4] == b"\x04\x22\x4d\x18"
    flg = frame[4]
    assert flg & ~0x08 == 0x60 and frame[5] == 0x40
    pos = 7 + (8 if flg & 8 else 0)
    content = struct.unpack_from("<Q", frame, 6)[0] if flg & 8 else 0
    blocks = []
    while True:
        w, = struct.unpack_from("<I", frame, pos)
        pos += 4
        if w == 0:
            break
        n = w & 0x7FFFFFFF
        if w >> 31:
            blocks.append(dict(size=n, csize=n, stored=True, seqs=[], last=None))
            pos += n
            continue
        p, end, seqs, size = pos, pos + n, [], 0
        while True:
            tok = frame[p]
            p += 1
            ll = tok >> 4
            if ll == 15:
                while frame[p] == 255:
                    ll, p = ll + 255, p + 1
                ll, p = ll + frame[p], p + 1
            p += ll
            size += ll
            if p == end:
                last = ll
                break
            off, = struct.unpack_from("<H", frame, p)
            p += 2
            ml = tok & 15
            if ml == 15:
                while frame[p] == 255:
                    ml, p = ml + 255, p + 1
                ml, p = ml + frame[p], p + 1
            ml += 4
            assert 0 < off <= size
            size += ml
            seqs.append((ll, ml, off))
        blocks.append(dict(size=size, csize=n, stored=False, seqs=seqs, last=last))
        pos = end
    assert pos == len(frame) and sum(b["size"] for b in blocks) == content
    return blocks


def snappy_chunks(stream: bytes) -> list:
    """snappy-java -> per chunk dict(size, tags); a tag is ("lit", length,
    length bytes) or ("copy1" | "copy2", length, offset)."""
    assert stream[:16] == b"\x82SNAPPY\x00" + struct.pack("<ii", 1, 1)
    pos, chunks = 16, []
    while pos < len(stream):
        n, = struct.unpack_from(">I", stream, pos)
        pos += 4
        p, end = pos, pos + n
        size = shift = 0
        while True:
            size |= (stream[p] & 0x7F) << shift
            shift += 7
            p += 1
            if not stream[p - 1] & 0x80:
                break
        tags, done = [], 0
        while p < end:
            t = stream[p]
            p += 1
            if t & 3 == 0:
                ln, nb = t >> 2, 0
                if ln >= 60:
                    nb = ln - 59
                    ln = int.from_bytes(stream[p:p + nb], "little")
                    p += nb
                ln += 1
                p += ln
                tags.append(("lit", ln, nb))
            elif t & 3 == 1:
                ln, off = 4 + ((t >> 2) & 7), ((t >> 5) << 8) | stream[p]
                p += 1
                tags.append(("copy1", ln, off))
            else:
                assert t & 3 == 2
                ln, off = 1 + (t >> 2), struct.unpack_from("<H", stream, p)[0]
                p += 2
                tags.append(("copy2", ln, off))
            done += ln
        assert p == end and done == size
        chunks.append(dict(size=size, tags=tags))
        pos = end
    return chunks


def snappy_matches(tags) -> list:
    """Consecutive copies of one offset: the pieces EmitCopy cut one match into."""
    out, cur = [], None
    for t in tags:
        if t[0] == "lit":
            cur = None
        elif cur is not None and cur[0] == t[2]:
            cur[1].append(t[1])
        else:
            cur = (t[2], [t[1]])
            out.append(cur)
    return out


def block_sizes(n: int) -> list:
    return [min(cb.BLOCK, n - b) for b in range(0, n, cb.BLOCK)]


def snappy_table(n: int) -> int:
    """CalculateTableSize: the smallest power of two >= n in [256, 16384]."""
    t = 256
    while t < n and t < 16384:
        t *= 2
    return t


# ------------------------------------------------------------------- fixtures
@pytest.fixture(scope="module")
def bodies():
    return cb.all_bodies()


@pytest.fixture(scope="module")
def bodies_file(tmp_path_factory, bodies):
    path = tmp_path_factory.mktemp("comp_bodies") / "bodies.bin"
    cb.write_file(path, bodies)
    return path


@pytest.fixture(scope="module")
def lz4_parsed(bodies):
    return [(label, len(body), lz4_blocks(orc.compress(3, body))) for label, body in bodies]


@pytest.fixture(scope="module")
def snappy_parsed(bodies):
    return [(label, len(body), snappy_chunks(orc.compress(2, body))) for label, body in bodies]


# ------------------------------------------------------------------- coverage
def test_families_are_deterministic_and_labelled():
    fams = cb.families()
    assert tuple(fams) == cb.FAMILIES and all(len(v) > 20 for v in fams.values())
    labels = [label for v in fams.values() for label, _ in v]
    assert len(set(labels)) == len(labels)
    cb.family.cache_clear()
    again = cb.families()
    assert all(fams[k] == again[k] for k in fams)
    sizes = {len(b) for _, b in fams["sizes"]}
    assert sizes == set(cb.SIZES)


def test_lz4_coverage(lz4_parsed):
    lits, lasts, mls, offs, bsizes, nblocks = Counter(), Counter(), Counter(), Counter(), Counter(), Counter()
    stored = exact = 0
    edge = {}
    for label, n, blocks in lz4_parsed:
        assert [b["size"] for b in blocks] == block_sizes(n), label
        nblocks[len(blocks)] += 1
        for b in blocks:
            bsizes[b["size"]] += 1
            stored += b["stored"]
            exact += (not b["stored"]) and b["csize"] == b["size"] - 1
            assert b["stored"] or b["csize"] < b["size"], label
            for ll, ml, off in b["seqs"]:
                lits[ll] += 1
                mls[ml] += 1
                offs[off] += 1
            if not b["stored"]:
                lasts[b["last"]] += 1
        if label.startswith("stored_edge/"):
            _, sn, where, m = label.split("/")
            edge.setdefault((sn, where), {})[int(m[1:])] = blocks[0]["stored"]
    for ll in (0, 1, 14, 15, 16, 269, 270, 271):
        assert lits[ll], f"no literal run of {ll}"
    for ll in (5, 15, 16, 270):
        assert lasts[ll], f"no closing run of {ll}"
    for ml in (4, 18, 19, 20, 273, 274, 275, 529):
        assert mls[ml], f"no match of {ml}"
    for off in (1, 2, 3, 4, 8):
        assert offs[off], f"no offset {off}"
    # the largest a 64 KiB block allows: a match starts at most 12 bytes before the end
    assert max(offs) == cb.BLOCK - 12 and sum(v for o, v in offs.items() if o >= 65500) >= 2
    for size in (1, 12, 13):
        assert bsizes[size], f"no block of {size} bytes"
    for k in (0, 1, 2, 3, 4):
        assert nblocks[k], f"no frame of {k} blocks"
    assert stored >= 20 and exact >= 5, (stored, exact)
    # the stored / compressed switch between neighbouring match lengths
    switches = [k for k, row in edge.items() if any(row[m] and row.get(m + 1) is False for m in row)]
    assert len(switches) >= 5, switches


def test_snappy_coverage(snappy_parsed):
    lit, copy1, copy2, pieces, tables, nchunks = Counter(), Counter(), Counter(), Counter(), Counter(), Counter()
    far = 0
    for label, n, chunks in snappy_parsed:
        assert [c["size"] for c in chunks] == [min(cb.FRAGMENT, n - f) for f in range(0, n, cb.FRAGMENT)], label
        nchunks[len(chunks)] += 1
        for c in chunks:
            for size in block_sizes(c["size"]):
                tables[snappy_table(size)] += 1
            for t in c["tags"]:
                if t[0] == "lit":
                    lit[(t[1], t[2])] += 1
                else:
                    (copy1 if t[0] == "copy1" else copy2)[(t[1], t[2])] += 1
                    far += t[2] >= 65500
            for off, p in snappy_matches(c["tags"]):
                pieces[tuple(p)] += 1
    # EmitLiteral: the tag alone up to 60 bytes, then 1 and 2 length bytes
    for ln, nb in ((60, 0), (61, 1), (256, 1), (257, 2)):
        assert lit[(ln, nb)], f"no literal of {ln} with {nb} length bytes"
    for ln in (4, 11):
        assert any(k[0] == ln for k in copy1), f"no 1-byte-offset copy of {ln}"
    assert any(k[1] == 2047 for k in copy1) and max(k[1] for k in copy1) == 2047
    for ln in range(4, 12):
        assert copy2[(ln, 2048)], f"no 2-byte-offset copy of {ln} at 2048"
    assert any(k[0] == 12 for k in copy2) and any(k[0] == 64 for k in copy2)
    for want in ((60, 5), (60, 6), (60, 7), (64, 4)):
        assert pieces[want], f"no match cut into {want}"
    assert any(sum(p) >= 132 and p[:2] == (64, 64) for p in pieces)
    # the largest a 64 KiB block allows is 65,520, not n - 15 = 65,521: the search stops when the NEXT position
    # passes ip_limit = n - 15, and after a copy at ip >= ip_limit, so a match starts at n - 16 at the latest
    # (the bodies with the source's bytes again at n - 15 are there; the reference does not take them)
    assert far and max(k[1] for k in copy2) == cb.BLOCK - 16, "no offset >= 65500"
    assert sorted(tables) == [256, 512, 1024, 2048, 4096, 8192, 16384], tables
    for k in (0, 1, 2):
        assert nchunks[k], f"no stream of {k} fragments"


# -------------------------------------------------------------------- carried
def run_bodies(exe: Path, path: Path, cwd: Path, codecs: str | None = None):
    args = [str(exe), "--bodies", str(path)] + (["--codecs", codecs] if codecs else [])
    return subprocess.run(args, cwd=cwd, capture_output=True, text=True, timeout=900)


def test_carried_tables_match_oracle(tmp_path, bodies, bodies_file):
    exe = build_fuzzer(tmp_path)
    r = run_bodies(exe, bodies_file, tmp_path)
    assert r.returncode == 0, r.stderr[-4000:]
    # LZ4 and snappy twice, gzip and zstd once
    assert f"{len(bodies)} bodies, {6 * len(bodies)} cases: engine == oracle" in r.stdout


# ---------------------------------------------------------------------- teeth
LZ4C, SNAPC = "rpgpu_lz4c.h", "rpgpu_snappyc.h"
GET = "return (v >> 16) == gen ? (v & 0xFFFFu) : 0u;"
MUTANTS = [
    (LZ4C, GET, "return v & 0xFFFFu;"),
    (LZ4C, "(last + 255 - kRunMask) / 255 > cap", "(last + 254 - kRunMask) / 255 > cap"),
    (LZ4C, "if (ip >= mflimit1) break;", "if (ip > mflimit1) break;"),
    (LZ4C, "if (fwd > mflimit1) goto last_literals;", "if (fwd >= mflimit1) goto last_literals;"),
    (LZ4C, "kMinLength = kMfLimit + 1;", "kMinLength = kMfLimit + 2;"),
    (LZ4C, "matchlimit = n >= 5 ? n - kLastLiterals : 0;", "matchlimit = n >= 5 ? n - kLastLiterals - 1 : 0;"),
    (LZ4C, "dst + o + 4, sz - 1, t);", "dst + o + 4, sz, t);"),
    (LZ4C, "t.put(hpos(src, ip - 2), ip - 2);", "t.put(hpos(src, ip - 1), ip - 1);"),
    (LZ4C, "while (ip > anchor && match > 0", "while (ip > anchor + 1 && match > 0"),
    (SNAPC, GET, "return v & 0xFFFFu;"),
    (SNAPC, "while (len >= 68) {", "while (len > 68) {"),
    (SNAPC, "if (len > 64) {", "if (len >= 64) {"),
    (SNAPC, "if (lt12 && offset < 2048) {", "if (lt12 && offset <= 2048) {"),
    (SNAPC, "if (n < 60) {", "if (n <= 60) {"),
    (SNAPC, "if (len < 12) return", "if (len <= 12) return"),
    (SNAPC, "if (ip >= ip_limit) goto emit_remainder;", "if (ip > ip_limit) goto emit_remainder;"),
    (SNAPC, "if (next_ip > ip_limit) goto emit_remainder;", "if (next_ip >= ip_limit) goto emit_remainder;"),
    (SNAPC, "while (ip + m < n && in[candidate + m]", "while (ip + m + 1 < n && in[candidate + m]"),
    (SNAPC, "t.put(hash_bytes(rd32(in + ip - 1), shift), ip - 1);", ""),
    (SNAPC, "return 2u << log2_floor(n - 1);", "return 2u << log2_floor(n);"),
    (SNAPC, "kFragment = 128u << 10;", "kFragment = 64u << 10;"),
]


@pytest.mark.parametrize("row", range(len(MUTANTS)), ids=[f"{h[6:-2]}:{new or 'removed'}" for h, _, new in MUTANTS])
def test_sweep_rejects_one_token_change(tmp_path, bodies_file, row):
    header, old, new = MUTANTS[row]
    csrc = tmp_path / "csrc"
    shutil.copytree(ROOT / "redpanda_amd" / "csrc", csrc)
    text = (csrc / header).read_text()
    assert text.count(old) == 1, (header, old)
    (csrc / header).write_text(text.replace(old, new))
    exe = build_fuzzer(tmp_path, csrc=csrc)
    r = run_bodies(exe, bodies_file, tmp_path, codecs="3" if header == LZ4C else "2")
    # a difference from the oracle (exit 1); a changed rule may also run the host build out of its buffers
    assert r.returncode != 0 and "engine == oracle" not in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
