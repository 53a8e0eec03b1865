"""The device compressors (rpgpu_compress_plan_device / _run_device:
compress_caps_kernel, compress_lane_kernel<codec>, the RECRC validation and
compress_patch_kernel) on the match-geometry bodies of tests/comp_bodies.py
(tests/test_comp_bodies.py asserts on the host what the reference's compressors
emit for them, and that the sweep rejects one-token changes of the rules).

  families        every family as one arena per format: LZ4 / snappy output
                  byte for byte as the oracle's compress_batch, gzip / zstd
                  within their bound and decoded by zlib / libzstd and by the
                  GPU decoders; each arena by a plan run twice, a plan run once
                  and a second engine, all identical
  header variety  every header field with a value of its own, both formats
  lane reuse      the smallest arenas in which a compress lane takes a second
                  batch (lanes + 64 batches): the grid stride, the generation
                  carried in a lane's table, the reuse of a lane's zstd work area
  output below the plan / plan for another codec
                  the two overflow branches of compress_lane_kernel
  n = 0"""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import comp_bodies as cb  # noqa: E402
from kafka_batches import DISK, WIRE, arena, batch  # noqa: E402
from test_compress import mixed_arena  # noqa: E402
from test_gpu_decomp import OPS  # noqa: E402

import oracle.oracle as orc  # noqa: E402
from redpanda_amd import abi  # noqa: E402

pytestmark = pytest.mark.gpu

OPS_CRC = abi.OP_CRC | abi.OP_HDRCRC  # bodies are arbitrary bytes: no record walk
SAME = ("cres", "out_descs", "out_results")
LANES = {1: 32768, 2: 131072, 3: 131072, 4: 32768}  # compress_lane_kernel's lanes in flight
TENANTS = 64


@pytest.fixture(scope="module")
def eng2(built):
    from redpanda_amd import engine

    e = engine.Engine(0)
    yield e
    e.close()


def slots(got):
    c = got["cres"]
    return [got["out"][int(a):int(a) + 61 + int(n)].tobytes() if v == 0 else None
            for a, n, v in zip(c["out_offset"], c["out_len"], c["verdict"])]


def body_arena(bodies, fmt):
    bs = [batch(b, fmt=fmt, record_count=1, base_offset=7 * i) for i, b in enumerate(bodies)]
    return arena(bs, fmt=fmt, ops=OPS_CRC)


def compress_thrice(eng, eng2, data, descs, codec):
    """A plan run twice, a plan run once and a second engine: identical."""
    got = eng.compress_arena(data, descs, codec, runs=2)
    ref = slots(got)
    for o in (eng.compress_arena(data, descs, codec), eng2.compress_arena(data, descs, codec)):
        for f in SAME:
            assert np.array_equal(got[f].view(np.uint8), o[f].view(np.uint8)), f"{f} differs between runs"
        diff = [i for i, (a, b) in enumerate(zip(ref, slots(o))) if a != b]
        assert not diff, f"compressed bytes differ between runs at batches {diff[:8]}"
    assert (got["results"]["verdict"] == 0).all() and (got["results"]["codec"] == 0).all()
    assert (got["cres"]["verdict"] == 0).all(), np.nonzero(got["cres"]["verdict"])[0][:8]
    assert (got["out_results"]["verdict"] == 0).all(), np.nonzero(got["out_results"]["verdict"])[0][:8]
    return got, ref


def decode_back(eng, got, bodies):
    """The compressed batches through the GPU decoders: the original bodies."""
    od = got["out_descs"].copy()
    od["ops"] = OPS
    back = eng.decompress_arena(got["out"], od)
    d = back["dres"]
    assert (d["verdict"] == 0).all(), np.nonzero(d["verdict"])[0][:8]
    for i, body in enumerate(bodies):
        a, m = int(d["out_offset"][i]), int(d["out_len"][i])
        assert m == len(body) and back["out"][a + 61:a + 61 + m].tobytes() == body, f"batch {i} decodes differently"


def check_header(b: bytes, w: bytes, codec: int):
    """Every header field but crc / header_crc / size / attrs' codec as the
    oracle's (LZ4) rewrite; both CRCs over what was written."""
    hw = np.frombuffer(w[:61], dtype=abi.RP_HEADER_DTYPE)[0]
    hg = np.frombuffer(b[:61], dtype=abi.RP_HEADER_DTYPE)[0]
    assert int(hg["size_bytes"]) == len(b) and int(hg["attrs"]) == (int(hw["attrs"]) & ~7) | codec
    for f in ("base_offset", "type", "last_offset_delta", "first_timestamp", "max_timestamp", "producer_id",
              "producer_epoch", "base_sequence", "record_count"):
        assert hg[f] == hw[f], f
    assert int(hg["crc"]) == orc.crc_record_batch(hg, b[61:])
    assert int(hg["header_crc"]) == orc.internal_header_only_crc(hg)


# ------------------------------------------------------------------- families
@pytest.mark.parametrize("fmt", [WIRE, DISK])
@pytest.mark.parametrize("codec", [2, 3])
@pytest.mark.parametrize("name", cb.FAMILIES)
def test_family_bytes(eng, eng2, name, codec, fmt):
    bodies = [b for _, b in cb.family(name)]
    data, descs = body_arena(bodies, fmt)
    assert data.size < 32 << 20
    got, ref = compress_thrice(eng, eng2, data, descs, codec)
    want = orc.compress_batches(data, descs, got["results"], codec)
    diff = [i for i, (a, w) in enumerate(zip(ref, want)) if a != w]
    assert not diff, [cb.family(name)[i][0] for i in diff[:8]]
    decode_back(eng, got, bodies)


@pytest.mark.parametrize("fmt", [WIRE, DISK])
@pytest.mark.parametrize("codec", [1, 4])
@pytest.mark.parametrize("name", cb.FAMILIES)
def test_family_round_trip(eng, eng2, name, codec, fmt):
    bodies = [b for _, b in cb.family(name)]
    data, descs = body_arena(bodies, fmt)
    got, ref = compress_thrice(eng, eng2, data, descs, codec)
    cres = got["cres"]
    assert (cres["out_len"].astype(np.int64) <= cres["out_cap"].astype(np.int64) - 61 - 64).all()
    want = orc.compress_batches(data, descs, got["results"], 3)  # the header fields
    for i, body in enumerate(bodies):
        v, dec = orc.uncompress(codec, ref[i][61:], cap=len(body) + 1024)
        assert v == 0 and dec == body, cb.family(name)[i][0]
        check_header(ref[i], want[i], codec)
    decode_back(eng, got, bodies)


# ------------------------------------------------------------- header variety
def header_arena(fmt):
    """Every header field with a value of its own in every batch."""
    rng = np.random.default_rng(0x4EAD)
    bases = [0, 1, -1, -(1 << 63), (1 << 63) - (1 << 40), (1 << 32) + 17, -(1 << 32) - 3, 0x0102030405060708]
    bs = []
    for i in range(48):
        body = cb.periodic(rng, 40 + 11 * i, 5) + rng.integers(0, 256, 30 + i, dtype=np.uint8).tobytes()
        bs.append(batch(body, fmt=fmt, record_count=1000 + i, base_offset=bases[i % 8] + (i // 8) * 0x01010101,
                        btype=1 + i % 5, attrs=(i % 8) << 3,  # timestamp type, transactional, control
                        lod=0x11223344 - i, first_ts=0x0123456789ABCDEF - i, max_ts=-0x0FEDCBA987654321 + i,
                        pid=0x1A2B3C4D5E6F7081 + i, pepoch=0x7A5B - i, bseq=0x61626364 + i))
    return arena(bs, fmt=fmt, ops=OPS_CRC)


@pytest.mark.parametrize("fmt", [WIRE, DISK])
def test_header_variety(eng, fmt):
    data, descs = header_arena(fmt)
    for codec in (2, 3):
        got = eng.compress_arena(data, descs, codec)
        assert (got["results"]["verdict"] == 0).all() and (got["cres"]["verdict"] == 0).all()
        want = orc.compress_batches(data, descs, got["results"], codec)
        hdrs = np.frombuffer(b"".join(w[:61] for w in want), dtype=abi.RP_HEADER_DTYPE)
        assert len(set(hdrs["attrs"] >> 3)) == 8 and len(set(hdrs["type"])) == (5 if fmt == DISK else 1)
        assert (hdrs["base_offset"] < 0).any() and (hdrs["base_offset"] > 1 << 32).any()
        for f in ("producer_id", "producer_epoch", "base_sequence", "last_offset_delta", "first_timestamp",
                  "max_timestamp", "record_count", "base_offset"):
            assert len(set(hdrs[f])) == len(hdrs), f
        diff = [i for i, (a, w) in enumerate(zip(slots(got), want)) if a != w]
        assert not diff, diff[:8]
        assert (got["out_results"]["verdict"] == 0).all()


# ----------------------------------------------------------------- lane reuse
@pytest.mark.parametrize("matched", [False, True], ids=["plain", "matched"])
@pytest.mark.parametrize("codec", [3, 2, 1, 4])
def test_lane_reuse(eng, codec, matched):
    """n = lanes + 64: batches [0, 64) are the first tenants of their lanes'
    tables (2-3 blocks, a full table), [64, lanes) one filler batch repeated,
    [lanes, n) the second tenants, cut from their lane mates' bodies.  On the
    host, with the table's stale entries tagged as live, 48 of the 64 plain
    second tenants come out differently from the oracle for LZ4 and none for
    snappy (comp_bodies.lane_second says why); of the matched ones, all 64 for
    both."""
    import torch

    lanes = LANES[codec]
    n = lanes + TENANTS
    need = int(eng._lib.rpgpu_compress_scratch_bytes(n)) + (2 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip(f"{free >> 20} MiB of device memory free, the lane-reuse arena needs {need >> 20} MiB")
    firsts = [cb.lane_first(j, matched) for j in range(TENANTS)]
    seconds = [cb.lane_second(j, firsts[j], matched) for j in range(TENANTS)]
    small = [batch(b, fmt=DISK, record_count=1, base_offset=3 * j) for j, b in enumerate(firsts)] + \
        [batch(cb.LANE_FILLER, fmt=DISK, record_count=1, base_offset=24)] + \
        [batch(b, fmt=DISK, record_count=1, base_offset=5 * j) for j, b in enumerate(seconds)]
    fill = np.frombuffer(small[TENANTS], dtype=np.uint8)
    parts = [np.frombuffer(b"".join(small[:TENANTS]), dtype=np.uint8), np.tile(fill, lanes - TENANTS),
             np.frombuffer(b"".join(small[TENANTS + 1:]), dtype=np.uint8), np.zeros(64, dtype=np.uint8)]
    data = np.concatenate(parts)
    lens = np.concatenate([[len(b) for b in small[:TENANTS]], np.full(lanes - TENANTS, fill.size),
                           [len(b) for b in small[TENANTS + 1:]]]).astype(np.int64)
    descs = np.zeros(n, dtype=orc.DESC_DTYPE)
    descs["offset"] = np.cumsum(lens) - lens
    descs["length"] = lens
    descs["partition"] = np.arange(n) % 7
    descs["format"] = DISK
    descs["ops"] = OPS_CRC
    assert data.size < 64 << 20

    t0 = time.perf_counter()
    got = eng.compress_arena(data, descs, codec)
    torch.cuda.empty_cache()  # the lanes' tables: gigabytes
    cres = got["cres"]
    print(f"lane reuse codec {codec}{' matched' if matched else ''}: {n} batches, arena {data.size} bytes, compress scratch "
          f"{need - (2 << 30)} bytes ({free >> 20} MiB free), output {got['out_bytes']} bytes, "
          f"compress_arena {time.perf_counter() - t0:.2f} s, tenants' payloads "
          f"{int(cres['out_len'][:TENANTS].min())}..{int(cres['out_len'][:TENANTS].max())} and "
          f"{int(cres['out_len'][lanes:].min())}..{int(cres['out_len'][lanes:].max())} bytes")
    assert (got["results"]["verdict"] == 0).all()
    assert (cres["verdict"] == 0).all() and (got["out_results"]["verdict"] == 0).all()

    # the oracle over the tenants and one filler
    sdata, sdescs = arena(small, fmt=DISK, ops=OPS_CRC)
    sres, _, _ = orc.validate_arena(sdata, sdescs)
    want = orc.compress_batches(sdata, sdescs, sres, codec if codec in (2, 3) else 3)
    tenants = list(range(TENANTS)) + list(range(lanes, n))
    bodies = firsts + seconds
    ref = [got["out"][int(cres["out_offset"][i]):int(cres["out_offset"][i]) + 61 + int(cres["out_len"][i])].tobytes()
           for i in tenants]
    for k, (i, w) in enumerate(zip(tenants, want[:TENANTS] + want[TENANTS + 1:])):
        if codec in (2, 3):
            assert ref[k] == w, f"tenant batch {i} differs from the oracle"
        else:
            v, dec = orc.uncompress(codec, ref[k][61:], cap=len(bodies[k]) + 1024)
            assert v == 0 and dec == bodies[k], f"tenant batch {i} does not round-trip"
            check_header(ref[k], w, codec)
    # the filler: one copy against the oracle, every copy against the first
    f0, flen = int(cres["out_offset"][TENANTS]), 61 + int(cres["out_len"][TENANTS])
    one = got["out"][f0:f0 + flen]
    if codec in (2, 3):
        assert one.tobytes() == want[TENANTS]
    else:
        v, dec = orc.uncompress(codec, one[61:].tobytes(), cap=1024)
        assert v == 0 and dec == cb.LANE_FILLER
        check_header(one.tobytes(), want[TENANTS], codec)
    assert (cres["out_len"][TENANTS:lanes] == flen - 61).all()
    copies = got["out"][cres["out_offset"][TENANTS:lanes].astype(np.int64)[:, None] + np.arange(flen)[None, :]]
    bad = np.nonzero((copies != one[None, :]).any(axis=1))[0]
    assert bad.size == 0, f"filler batches {TENANTS + bad[:8]} differ from batch {TENANTS}"


# ------------------------------------------------------ the overflow branches
@pytest.mark.parametrize("codec", [2, 3, 4])
def test_output_below_plan(eng, codec):
    """The caller's capacity ends in the middle of batch k's slot: every
    wanted batch whose slot passes it reads DECOMP_OVERFLOW and writes nothing,
    every other batch is as in the full run, nothing at or past out_cap is
    written."""
    data, descs = mixed_arena(30 + codec, 200, DISK)
    full = eng.compress_arena(data, descs, codec)
    fc, fs = full["cres"], slots(full)
    wanted = np.nonzero(fc["verdict"] == 0)[0]
    assert wanted.size > 150 and (fc["verdict"] != 0).sum() > 10
    for k in (wanted[0], wanted[wanted.size // 2], wanted[-1]):
        cap = int(fc["out_offset"][k]) + int(fc["out_cap"][k]) // 2
        got = eng.compress_arena(data, descs, codec, out_cap=cap)
        c = got["cres"]
        over = (fc["verdict"] == 0) & (fc["out_offset"].astype(np.int64) + fc["out_cap"].astype(np.int64) > cap)
        assert over[k] and over.sum() >= 1
        assert (c["verdict"][over] == abi.V_DECOMP_OVERFLOW).all()
        assert (got["out_descs"]["length"][over] == 0).all() and (got["out_descs"]["ops"][over] == 0).all()
        assert (c["out_len"][over] == 0).all()
        for f in SAME:
            assert np.array_equal(got[f][~over], full[f][~over]), f
        gs = slots(got)
        assert all(gs[i] == fs[i] for i in np.nonzero(~over)[0])
        assert got["out"].size == full["out_bytes"] + 4096 and (got["out"][cap:] == 0xA5).all()


def test_plan_for_another_codec(eng):
    """A slot planned for a codec with a smaller bound than the run's (ADVICE
    r2): snappy's bound plus slack exceeds the 16-byte-rounded LZ4 slot at every
    body size (173 > 144 at size 0), so a snappy run on an LZ4 plan compresses
    nothing; an LZ4 run on a snappy plan is the oracle's LZ4."""
    data, descs = mixed_arena(41, 200, WIRE)
    plain = eng.compress_arena(data, descs, 3)
    wanted = plain["cres"]["verdict"] == 0
    assert wanted.sum() > 150
    got = eng.compress_arena(data, descs, 2, plan_codec=3, out_cap=plain["out_bytes"])
    assert (got["cres"]["verdict"][wanted] == abi.V_DECOMP_OVERFLOW).all()
    assert (got["cres"]["verdict"][~wanted] == abi.V_SKIPPED).all()
    assert (got["out_descs"]["length"] == 0).all() and (got["out_descs"]["ops"] == 0).all()
    assert (got["out"] == 0xA5).all(), "a refused run wrote into the output"
    got = eng.compress_arena(data, descs, 3, plan_codec=2)
    assert got["out_bytes"] > plain["out_bytes"]
    assert np.array_equal(got["cres"]["verdict"], plain["cres"]["verdict"])
    want = orc.compress_batches(data, descs, got["results"], 3)
    assert slots(got) == want and slots(plain) == want


def test_empty_arena(eng):
    for codec in (1, 2, 3, 4):
        got = eng.compress_arena(np.zeros(64, dtype=np.uint8), np.zeros(0, dtype=orc.DESC_DTYPE), codec)
        assert got["out_bytes"] == 0 and len(got["cres"]) == 0 and len(got["out_descs"]) == 0
