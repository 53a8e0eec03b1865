"""The device LZ77 copy engines against the oracle on crafted frames whose
sequences walk their geometry space (tests/seq_frames.py: every (ll, ml, off)
with ll <= 34, ml <= 36, off <= 40 at four output positions mod 32, the edges
up to 1040, chains of dependent sequences longer than a wave group, LZ4
offsets up to 65,535 into a previous block, every snappy tag form, deflate
copies across the wrapper's chunk ends, zstd repeat-offset codes and
Huffman-compressed literals), through each execution path:

  lane decoders     lz_lane_kernel (LZ4, snappy), ws_lane_kernel (zstd, gzip)
  split parts       part_kernel (LZ4 independent blocks, snappy-java chunks)
  wave decoders     decomp_wave_kernel (linked LZ4, raw snappy, zstd wave-only)
  block-parallel    the zblk stages (zstd, the default engine)

Verdict, length and every byte as the oracle's (tests/test_seq_frames.py pins
the oracle's bytes to a byte-at-a-time model on the host); the path is asserted
from the slot sizes the plan gave; each arena is decoded by a plan run twice,
by a plan run once and by a second engine, and the three must be identical."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import seq_frames as sf  # noqa: E402
from kafka_batches import DISK, WIRE, arena, batch  # noqa: E402
from test_gpu_decomp import OPS, compare  # noqa: E402

import oracle.oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT_MIN = 80 << 10   # LZ4 / snappy slots above it are split when the frame allows
LANE_MAX = 256 << 10   # slots above it go to the wave decoders
ZSTD_BLK_MIN = 64 << 10  # zstd frames of a known content size above it leave the lanes
SEEDS = list(range(sf.SEEDS))


@pytest.fixture(scope="module")
def eng2(built):
    from redpanda_amd import engine

    e = engine.Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def zstd_fixture():
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "zstd_seqgrid.npz"))
    ends = np.cumsum(g["lens"])
    frames = [g["data"][e - n:e].tobytes() for e, n in zip(ends, g["lens"])]
    kind = g["kind"]  # 10 + seed: a lane frame of that seed, 2: invalid, 3: a named one-geometry frame
    return dict(lane=[[f for f, k in zip(frames, kind) if k == 10 + seed] for seed in SEEDS],
                invalid=[f for f, k in zip(frames, kind) if k == 2], named=[f for f, k in zip(frames, kind) if k == 3])


def slots(got):
    """Per batch: the bytes of its output slot that hold the rewritten batch."""
    d = got["dres"]
    return [got["out"][int(a):int(a) + 61 + int(n)].tobytes() for a, n in zip(d["out_offset"], d["out_len"])]


def decode(eng, eng2, frames, codec, fmt=WIRE):
    """One arena of the frames: every verdict OK and everything as the
    oracle's; identical from a plan run twice, run once, and a second engine."""
    from redpanda_amd import abi

    bs = [batch(f, fmt=fmt, record_count=1, attrs=codec) for f in frames]
    data, descs = arena(bs, fmt=fmt, ops=OPS)
    got = eng.decompress_arena(data, descs, runs=2)
    others = [eng.decompress_arena(data, descs), eng2.decompress_arena(data, descs)]
    want = compare(got, data, descs, nthreads=8)
    bad = np.nonzero(want["verdicts"] != abi.V_OK)[0]
    assert bad.size == 0, (bad[:8], want["verdicts"][bad[:8]])
    ref = slots(got)
    for o in others:
        for f in ("dres", "out_descs", "out_results", "index"):
            assert np.array_equal(got[f].view(np.uint8), o[f].view(np.uint8)), f"{f} differs between runs"
        diff = [i for i, (a, b) in enumerate(zip(ref, slots(o))) if a != b]
        assert not diff, f"decoded bytes differ between runs at batches {diff[:8]}"
    return got


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("codec", [1, 2, 3, 4])
def test_lane_decoders(eng, eng2, zstd_fixture, codec, seed):
    """Every grid block of one seed on the lane decoders: slots of at most
    80 KiB (LZ4 / snappy: above it only linked LZ4 frames, which have no split
    plan, below 256 KiB), zstd frames below 64 KiB in slots below 256 KiB.
    gzip has no other path (every member goes to ws_lane_kernel<1>), so there
    is nothing to assert for it beyond a slot."""
    if codec == 4:
        frames = zstd_fixture["lane"][seed]
    else:
        sets = {1: sf.gzip_lane, 2: sf.snappy_lane, 3: sf.lz4_lane}[codec](seed)
        frames = [f for f, _, _ in sets]
        plan_free = [linked for _, _, linked in sets]
    assert len(frames) > 60
    got = decode(eng, eng2, frames, codec)
    cap, n = got["dres"]["out_cap"].astype(np.int64), got["dres"]["out_len"].astype(np.int64)
    assert (cap > 0).all()
    if codec in (2, 3):
        big = cap > SPLIT_MIN
        assert (cap <= LANE_MAX).all() and not (big & ~np.array(plan_free)).any()
        assert big.sum() == (7 if codec == 3 else 0)  # the linked pairs and the 64 KiB-history frame
    elif codec == 4:
        assert (cap <= LANE_MAX).all() and (n <= ZSTD_BLK_MIN).all()


@pytest.mark.parametrize("codec", [1, 2, 3, 4])
def test_lane_decoders_disk_format(eng, eng2, zstd_fixture, codec):
    """Seed 0 again as on-disk batches (the other header layout in front of
    the same bodies)."""
    if codec == 4:
        frames = zstd_fixture["lane"][0]
    else:
        frames = [f for f, _, _ in {1: sf.gzip_lane, 2: sf.snappy_lane, 3: sf.lz4_lane}[codec](0)]
    got = decode(eng, eng2, frames, codec, fmt=DISK)
    assert (got["dres"]["out_cap"].astype(np.int64) <= LANE_MAX).all()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("codec", [2, 3])
def test_split_parts(eng, eng2, codec, seed):
    """Every grid block of one seed as a part: LZ4 frames of independent
    blocks and snappy-java bodies of several chunks above the 80 KiB split
    threshold, the grid in the parts after the first (no history before a
    part; the exact copies near a part's capacity), every LZ4 block but the
    last ending exactly at its 64 KiB capacity."""
    sets = (sf.lz4_parts if codec == 3 else sf.snappy_parts)(seed)
    assert not any(linked for _, _, linked in sets)
    if codec == 3:
        assert all(p.size == 65536 for _, parts, _ in sets for p in parts[1:-1])
        assert sum(len(parts) - 2 for _, parts, _ in sets) > 60
    got = decode(eng, eng2, [f for f, _, _ in sets], codec)
    cap = got["dres"]["out_cap"].astype(np.int64)
    assert (cap > SPLIT_MIN).all()


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("codec", [2, 3])
def test_wave_decoders_lz(eng, eng2, codec, seed):
    """Every grid block of one seed in slots above 256 KiB without a split
    plan: linked-block LZ4 frames (each block opening inside the previous one;
    offsets up to 65,535 with the history just under and over 64 KiB) and raw
    snappy streams (no snappy-java framing) of seven grid blocks."""
    sets = (sf.lz4_wave if codec == 3 else sf.snappy_wave)(seed)
    if codec == 3:
        assert all(linked for _, _, linked in sets)
    else:
        assert not any(f.startswith(b"\x82SNAPPY\x00") for f, _, _ in sets)
    got = decode(eng, eng2, [f for f, _, _ in sets], codec)
    assert (got["dres"]["out_cap"].astype(np.int64) > LANE_MAX).all()


@pytest.mark.parametrize("seed", SEEDS)
def test_zstd_wave_and_block_parallel(eng, eng2, zstd_fixture, seed):
    """Every zstd grid block of one seed (raw literals without and with
    repeat-offset codes, Huffman-compressed literals), five a frame, padded
    past 256 KiB with RLE blocks: on the one-wave decoder (zstd_blocks=False)
    and block-parallel (the default engine), byte for byte equal, the
    block-parallel plan holding its literal and record regions."""
    from redpanda_amd import engine

    frames = [f for f, _ in sf.zstd_big(seed, zstd_fixture["lane"][seed])]
    assert len(frames) >= 17
    got = decode(eng, eng2, frames, 4)
    assert (got["dres"]["out_cap"].astype(np.int64) > LANE_MAX).all()
    with engine.Engine(0, zstd_blocks=False) as e:
        one = decode(e, e, frames, 4)
    for f in ("dres", "out_descs", "out_results", "index"):
        assert np.array_equal(got[f].view(np.uint8), one[f].view(np.uint8)), f
    assert slots(got) == slots(one)
    assert got["out_bytes"] > one["out_bytes"], "no frame took the block-parallel path"


@pytest.mark.parametrize("codec", [1, 2, 3, 4])
def test_named_geometries(eng, eng2, zstd_fixture, codec):
    """The one-geometry frames (seq_frames.NAMED: the sequences at which the
    sweeps caught one-token changes of the engines' conditions on the host),
    each alone in its frame, on the lane decoders."""
    frames = zstd_fixture["named"] if codec == 4 else [f for c, f, _, _ in sf.named_frames() if c == codec]
    assert len(frames) == len(sf.NAMED)
    got = decode(eng, eng2, frames, codec)
    assert (got["dres"]["out_cap"].astype(np.int64) <= SPLIT_MIN).all()


def test_invalid_geometries(eng, zstd_fixture):
    """One arena of the invalid set (a zero LZ4 offset, offsets one past the
    history, matches ending inside liblz4's last-5 / last-12 zones, a zstd
    repeat-offset code resolving to zero): the oracle's verdict for each."""
    from redpanda_amd import abi

    inv = sf.invalid_frames() + [(4, f) for f in zstd_fixture["invalid"]]
    bs = [batch(f, fmt=WIRE, record_count=1, attrs=c) for c, f in inv]
    data, descs = arena(bs, fmt=WIRE, ops=OPS)
    got = eng.decompress_arena(data, descs)
    wres, _, _ = orc.validate_arena(data, descs)
    dres = got["dres"]
    caps = np.where(dres["out_cap"] > 0, dres["out_cap"].astype(np.int64) - 61 - 128, 0).astype(np.uint64)
    want = orc.decompress_arena(data, descs, wres, caps, codecs=(1, 2, 3, 4))
    bad = np.nonzero(dres["verdict"] != want["verdicts"])[0]
    assert bad.size == 0, (bad[:8], dres["verdict"][bad[:8]], want["verdicts"][bad[:8]])
    assert (want["verdicts"] == abi.V_DECOMP_ERROR).sum() >= 10
