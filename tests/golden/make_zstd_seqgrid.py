"""Fixture generator (needs a host compiler, not a GPU): the zstd frames over
the sequence geometries of tests/seq_frames.py -- zstd_fixture(): every grid
block of every seed as a one-block frame (raw literals without and with
repeat-offset codes, Huffman-compressed literals, no content size), a few
invalid ones and the named one-geometry ones (the large frames of the wave and
block-parallel decoders are spliced from these at test time).  Encoded by tests/native/zstd_fuzz.cpp --dump-seqgrid
(the engine's own zstd encoder pieces, predefined FSE tables; libzstd's
HUF_compress for the Huffman literals); the expected outputs come from the
oracle at test time, and tests/test_seq_frames.py checks them against the
byte-at-a-time model.  Writes tests/golden/zstd_seqgrid.npz."""
import subprocess
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def encode(exe: Path, tmp: Path, frames) -> list:
    """The frames of the given (flags, pad, blocks) programs."""
    import seq_frames as sf

    (tmp / "geometry.bin").write_bytes(sf.zstd_geometry_file(frames))
    subprocess.run([str(exe), "--dump-seqgrid", "geometry.bin"], cwd=tmp, check=True)
    out = sf.read_frames((tmp / "seqgrid.bin").read_bytes())
    assert len(out) == len(frames)
    return out


def main():
    import seq_frames as sf
    from test_zstd_fuzz import build_fuzzer

    fx = sf.zstd_fixture()
    with tempfile.TemporaryDirectory() as tmp:
        frames = encode(build_fuzzer(Path(tmp)), Path(tmp), [f for _, f in fx])
    lens = np.array([len(f) for f in frames], dtype=np.int64)
    path = ROOT / "tests" / "golden" / "zstd_seqgrid.npz"
    np.savez_compressed(path, data=np.frombuffer(b"".join(frames), dtype=np.uint8), lens=lens,
                        kind=np.array([k for k, _ in fx], dtype=np.int64))
    print("wrote", len(frames), "frames,", int(lens.sum()), "bytes,", path.stat().st_size, "on disk")


if __name__ == "__main__":
    main()
