"""The LZ77 copy primitives (redpanda_amd/csrc/rpgpu_copy.h: the wild and
exact copies, period16, and the write-combined register path every lane
decoder shares) compiled for the host and compared with byte-at-a-time loops
over off 0..40, n 0..80, ll <= 34, ml <= 36 at four alignments, with guard
bytes past each copy's allowed reach -- tests/native/copy_prims.cpp."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_copy_primitives_match_byte_loops(tmp_path):
    exe = tmp_path / "copy_prims"
    subprocess.run(["g++", "-O2", "-std=c++17", f"-I{ROOT / 'redpanda_amd' / 'csrc'}",
                    str(ROOT / "tests" / "native" / "copy_prims.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cases ok" in r.stdout, r.stdout
