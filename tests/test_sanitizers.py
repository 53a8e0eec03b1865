"""The engine's decoder restatements (rpgpu_codec.h, rpgpu_zstd.h,
rpgpu_inflate.h: the code the
GPU kernels run) built for the host with AddressSanitizer and
UndefinedBehaviorSanitizer, run over the differential fuzz corpora with the
device's exact buffer geometry (--exact 1: RPGPU_ARENA_TAIL_PAD readable
bytes past each input, an output slot of bound + kSlack).  The decoders copy
in 16/64-byte chunks and rely on kSlack; an access past what the GPU slot
allows would silently corrupt the neighbouring slot on the device, and is a
heap-buffer-overflow here.  The same stand-alone programs then decode the
crafted sequence-geometry frames (tests/seq_frames.py, --frames) in that
geometry.  (The reference builds its debug configuration
with -fsanitize=address,undefined, cmake/main.cmake:30-41.)"""
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
CONDA = "/opt/conda"
SAN = ["-fsanitize=address,undefined", "-static-libstdc++", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]


def build(tmp: Path, name: str, libs: list[str]) -> Path:
    import oracle.oracle as orc

    lib = orc.build()
    exe = tmp / f"{name}_san"
    r = subprocess.run(["g++", "-std=c++17", *SAN, f"-I{ROOT / 'redpanda_amd' / 'csrc'}",
                        f"-I{ROOT / 'include'}", f"-I{CONDA}/include",
                        str(ROOT / "tests" / "native" / f"{name}.cpp"), "-o", str(exe),
                        f"-L{lib.parent}", "-lrporacle", f"-Wl,-rpath,{lib.parent}",
                        f"-Wl,-rpath,{CONDA}/lib", *libs],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def run(exe: Path, cases: int, seed: int, cwd: Path):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), "--cases", str(cases), "--seed", str(seed), "--exact", "1"], cwd=cwd,
                       capture_output=True, text=True, timeout=1200, env=env)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-8000:])
    assert "engine == oracle" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-8000:]


def run_frames(exe: Path, arg: str, frames: list, cwd: Path):
    """The crafted frames (u32 length + bytes each) through the sanitized program."""
    import seq_frames as sf

    (cwd / "frames.bin").write_bytes(sf.write_frames(frames))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(exe), "--exact", "1", "--frames", arg], cwd=cwd, capture_output=True, text=True,
                       timeout=1200, env=env)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-8000:])
    assert f"frames: {len(frames)} cases" in r.stdout and "engine == oracle" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-8000:]


@pytest.mark.parametrize("seed", [31])
def test_codec_restatement_asan_ubsan(tmp_path, seed):
    import seq_frames as sf

    exe = build(tmp_path, "codec_fuzz", [f"{CONDA}/lib/liblz4.so", f"{CONDA}/lib/libsnappy.so"])
    run(exe, 4000, seed, tmp_path)
    seeds = range(sf.SEEDS)
    run_frames(exe, "3:frames.bin", [f for s in seeds for f, _, _ in sf.lz4_lane(s) + sf.lz4_parts(s) + sf.lz4_wave(s)]
               + [f for c, f in sf.invalid_frames(defined_only=True) if c == 3], tmp_path)
    run_frames(exe, "2:frames.bin", [f for s in seeds for f, _, _ in sf.snappy_lane(s) + sf.snappy_parts(s)
                                     + sf.snappy_wave(s)] + [f for c, f in sf.invalid_frames(defined_only=True) if c == 2], tmp_path)


@pytest.mark.parametrize("seed", [41])
def test_zstd_restatement_asan_ubsan(tmp_path, seed):
    import numpy as np
    import seq_frames as sf

    exe = build(tmp_path, "zstd_fuzz", [f"{CONDA}/lib/libzstd.so"])
    run(exe, 250, seed, tmp_path)
    g = np.load(ROOT / "tests" / "golden" / "zstd_seqgrid.npz")
    ends = np.cumsum(g["lens"])
    frames = [g["data"][e - n:e].tobytes() for e, n in zip(ends, g["lens"])]
    for seed in range(sf.SEEDS):  # and the large frames spliced from them
        frames += [f for f, _ in sf.zstd_big(seed, [f for f, k in zip(frames, g["kind"]) if k == 10 + seed])]
    run_frames(exe, "frames.bin", frames, tmp_path)


@pytest.mark.parametrize("seed", [61])
def test_inflate_restatement_asan_ubsan(tmp_path, seed):
    import seq_frames as sf

    exe = build(tmp_path, "inflate_fuzz", [f"{CONDA}/lib/libz.so"])
    run(exe, 2000, seed, tmp_path)
    run_frames(exe, "frames.bin", [f for s in range(sf.SEEDS) for f, _, _ in sf.gzip_lane(s)]
               + [f for c, f in sf.invalid_frames(defined_only=True) if c == 1], tmp_path)
