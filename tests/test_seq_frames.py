"""The crafted sequence-geometry frames (tests/seq_frames.py) on the host:
the geometry lists cover what they promise; the oracle (liblz4, snappy, zlib
and libzstd through the reference's wrapper loops) accepts every valid frame
and decodes it to the bytes of the helper's byte-at-a-time LZ77 model; and
the engine headers compiled for the host (tests/native/*_fuzz.cpp --frames:
rpgpu_codec.h's serial, lane and split-part decoders, rpgpu_inflate.h,
rpgpu_zstd.h's lane, ring and block-parallel decoders) give the oracle's
verdict, length and bytes on each.  No tolerance anywhere."""
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import seq_frames as sf  # noqa: E402

import oracle.oracle as orc  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.mark.parametrize("codec", ["LZ4", "SNAPPY", "GZIP", "ZSTD"])
def test_geometry_coverage(codec):
    """From the lists alone: every seed holds every dense (ll <= 34, ml <= 36,
    off <= 40) and edge triple with off inside the bytes produced; every dense
    triple starts at >= 4 distinct output positions mod 32 over the seeds; a
    run of more than 64 consecutive dependent sequences exists; every edge
    value appears on every axis the codec can express."""
    mm, mx = getattr(sf, codec)
    ndense, longest = sf.check_coverage(mm, mx)
    assert ndense == 35 * (min(36, mx) - mm + 1) * 40 and longest > 64
    assert len(sf.grid(mm, mx)) >= 4
    if codec == "ZSTD":
        # what is encoded: the blocks after the repeat-offset codes are resolved, every variant
        resolved = [[b for _, _, fb in sf.zstd_lane(seed) for _, b in fb] for seed in range(sf.SEEDS)]
        assert sf.check_blocks(resolved, mm, mx)[0] == ndense  # asserts the four phases and the long run as well
        for seed, (flags, reps) in enumerate(sf.ZSTD_VARIANTS):
            codes = sum(1 for _, _, fb in sf.zstd_lane(seed) for ops, _ in fb for _, _, ofv in ops if ofv <= 3)
            zero = sum(1 for _, _, fb in sf.zstd_lane(seed) for ops, _ in fb for ll, _, ofv in ops if ofv <= 3 and ll == 0)
            assert (codes > 5000 and 1000 < zero < codes - 1000) if reps else codes == 0, (seed, codes, zero)


@pytest.mark.parametrize("seed", range(sf.SEEDS))
def test_path_sets_hold_a_whole_seed(seed):
    """The frames of the split-part and wave paths: each seed's set holds every
    dense and edge triple and a dependent run of more than 64 sequences."""
    for name, codec in (("lz4_parts", sf.LZ4), ("lz4_wave", sf.LZ4), ("snappy_parts", sf.SNAPPY), ("snappy_wave", sf.SNAPPY)):
        blocks = sf.blocks_of(getattr(sf, name)(seed))
        assert sf.check_blocks([blocks], *codec, phases=1, max_size=320 << 10)[1] > 64, name


def test_gzip_chunk_ends_fall_inside_copies():
    """From each member's length and the wrapper's chunk rule: every chunk-end
    body has a chunk end strictly inside a copy of the length it is about, and
    every class of (dist < 16, dist < len) is crossed."""
    classes = {}
    for b in sf.gzip_chunk_blocks():
        n = len(sf.gzip_member(b, b""))
        got = sf.chunk_crossings(b, n)
        assert any(ml == b.seqs[-1][1] for _, ml, _ in got), b.seqs[-1]
        for _, ml, dist in got:
            classes[(dist < 16, dist < ml)] = classes.get((dist < 16, dist < ml), 0) + 1
    assert len(classes) == 4 and min(classes.values()) >= 10, classes


def test_literals_resist_shifts():
    """No literal run equals itself displaced by a byte, nor by 1, 2 or 7 bits."""
    a = np.frombuffer(sf.literals(1 << 16, 3), dtype=np.uint8)
    assert len(set(a.tolist())) <= 64
    for n in (16, 32):
        w = np.lib.stride_tricks.sliding_window_view(a, n)
        assert not (w[:-1] == w[1:]).all(axis=1).any()
    bits = np.unpackbits(a)
    for s in (1, 2, 7):
        shifted = np.packbits(bits[s:s - 8])
        w, v = np.lib.stride_tricks.sliding_window_view(a[:-1], 16), np.lib.stride_tricks.sliding_window_view(shifted, 16)
        assert not (w == v).all(axis=1).any()


def check_set(codec, frames):
    """Oracle V_OK on every frame, its bytes the model's."""
    for i, (f, parts, linked) in enumerate(frames):
        v, out = orc.uncompress(codec, f, cap=1 << 21)
        assert v == 0, (codec, i, v)
        assert out == sf.model_frame(parts, linked), (codec, i)


def run_frames(exe, arg, tmp, frames):
    (tmp / "frames.bin").write_bytes(sf.write_frames(frames))
    r = subprocess.run([str(exe), "--frames", arg], cwd=tmp, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-6000:]
    assert "engine == oracle" in r.stdout and f"frames: {len(frames)} cases" in r.stdout, r.stdout
    return r.stdout


def test_lz4_frames(tmp_path):
    from test_codec_fuzz import build_fuzzer

    sets = [s for seed in range(sf.SEEDS) for s in sf.lz4_lane(seed) + sf.lz4_parts(seed) + sf.lz4_wave(seed)]
    check_set(3, sets)
    assert any(linked for _, _, linked in sets) and any(not linked for _, _, linked in sets)
    out = run_frames(build_fuzzer(tmp_path), "3:frames.bin", tmp_path, [f for f, _, _ in sets])
    # every independent-block frame was decoded by parts as well, the parts giving the verdict
    plans, taken = (int(x) for x in re.search(r"(\d+) split plans \((\d+) taken\)", out).groups())
    assert plans == taken == sum(1 for _, _, linked in sets if not linked), out


@pytest.mark.parametrize("lane", [0, 1])
def test_snappy_frames(tmp_path, lane):
    """lane 1: the opt-in lane-form snappy decoder (RPGPU_SNAPPY_LANE=1)."""
    from test_codec_fuzz import build_fuzzer

    sets = [s for seed in range(sf.SEEDS) for s in sf.snappy_lane(seed) + sf.snappy_parts(seed) + sf.snappy_wave(seed)]
    if lane == 0:
        check_set(2, sets)
    exe = build_fuzzer(tmp_path, ("RPGPU_SNAPPY_LANE=1",) if lane else ())
    out = run_frames(exe, "2:frames.bin", tmp_path, [f for f, _, _ in sets])
    plans, taken = (int(x) for x in re.search(r"(\d+) split plans \((\d+) taken\)", out).groups())
    assert plans == taken >= 4 * sf.SEEDS, out


def test_gzip_frames(tmp_path):
    from test_inflate_fuzz import build_fuzzer

    sets = [s for seed in range(sf.SEEDS) for s in sf.gzip_lane(seed)]
    check_set(1, sets)
    run_frames(build_fuzzer(tmp_path), "frames.bin", tmp_path, [f for f, _, _ in sets])


def test_zstd_frames(tmp_path):
    """The committed fixture is what the geometry lists encode to today; the
    oracle decodes every valid frame of it to the model's bytes; the host
    engine agrees with the oracle on all of it, the invalid frames included."""
    from golden.make_zstd_seqgrid import encode
    from test_zstd_fuzz import build_fuzzer

    exe = build_fuzzer(tmp_path)
    fx = sf.zstd_fixture()
    frames = encode(exe, tmp_path, [f for _, f in fx])
    g = np.load(GOLDEN / "zstd_seqgrid.npz")
    assert g["data"].tobytes() == b"".join(frames) and list(g["lens"]) == [len(f) for f in frames]
    assert list(g["kind"]) == [k for k, _ in fx]
    assert (GOLDEN / "zstd_seqgrid.npz").stat().st_size <= (GOLDEN / "zstd_ring.npz").stat().st_size
    for (kind, prog), f in zip(fx, frames):
        if kind == 2:
            continue
        assert kind == 3 or 10 <= kind < 10 + sf.SEEDS
        v, out = orc.uncompress(4, f, cap=1 << 21)
        assert v == 0, (kind, v)
        assert out == sf.zstd_model(prog)
        # the literals section's type (RFC 8878 3.1.1.3.1): raw, or Huffman-compressed in that variant
        huf = kind >= 10 and sf.ZSTD_VARIANTS[kind - 10][0] & sf.ZSTD_HUF
        assert f[(9 if f[4] == 0xA0 else 6) + 3] & 3 == (2 if huf else 0), kind
    # the large frames: spliced from the lane frames, as the encoder makes them from the same programs
    big = []
    for seed in range(sf.SEEDS):
        lane = [f for (kind, _), f in zip(fx, frames) if kind == 10 + seed]
        these = sf.zstd_big(seed, lane)
        assert encode(exe, tmp_path, [these[0][1]]) == [these[0][0]]
        big += these
    for f, prog in big:
        v, out = orc.uncompress(4, f, cap=1 << 21)
        assert v == 0 and out == sf.zstd_model(prog)
        assert len(out) > 256 << 10
    out = run_frames(exe, "frames.bin", tmp_path, frames + [f for f, _ in big])
    assert int(re.search(r"(\d+) block plans", out).group(1)) >= len(big), out


def test_named_geometries():
    """The one-geometry frames: each holds its sequence at the named output
    position mod 32 and decodes, by the oracle, to the model's bytes."""
    for (fill, ll, ml, off), b in zip(sf.NAMED.values(), sf.named_blocks(*sf.LZ4)):
        assert len(b.seqs) == 2 and b.seqs[1] == (ll, ml, off) and sum(b.seqs[0][:2]) % 32 == fill
    for codec, f, parts, linked in sf.named_frames():
        check_set(codec, [(f, parts, linked)])


def test_invalid_frames_have_a_verdict(tmp_path):
    """The invalid set: the oracle gives each a verdict, some of them errors;
    the host engines (LZ4, snappy, gzip; zstd's are in test_zstd_frames) give
    the same one, and the same bytes where both decode."""
    from test_codec_fuzz import build_fuzzer

    import test_inflate_fuzz

    verdicts = [orc.uncompress(c, f, cap=1 << 20)[0] for c, f in sf.invalid_frames()]
    assert sum(v != 0 for v in verdicts) >= 10, verdicts
    # the LZ4 frames with a zero offset decode, in liblz4, from bytes nobody wrote: verdict only (above, and on
    # the device); every other one through the host engines, whether the oracle rejects it or not
    inv = sf.invalid_frames(defined_only=True)
    assert len(inv) == len(verdicts) - 2
    exe = build_fuzzer(tmp_path)
    for codec in (2, 3):
        run_frames(exe, f"{codec}:frames.bin", tmp_path, [f for c, f in inv if c == codec])
    run_frames(test_inflate_fuzz.build_fuzzer(tmp_path), "frames.bin", tmp_path, [f for c, f in inv if c == 1])
