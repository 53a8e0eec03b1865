"""The REST proxy's fetch reply, CPU half (no GPU needed):

* the reference's own expected string (tests/golden/pandaproxy_fetch.json,
  from pandaproxy/json/requests/test/fetch.cc:77,95-96) through the Python
  model tests/pp_fetch.py and through the shared core
  redpanda_amd/csrc/rpgpu_pp.h compiled for the host (tests/native/pp_host.cpp);
* the host program over the sweep of tests/pp_fetch.py, wire and disk arenas:
  bytes, every result field and the lane / wave path counts equal the model's;
  once more under ASan + UBSan, stand-alone, with every response and every
  field encoded in isolation in a heap block of exactly its size;
* a table of one-token changes to rpgpu_pp.h that the sweep must reject.
The validation rows and the record index the host program reads come from
oracle/ (as in tests/test_legacy_sets.py).  The device half is
tests/test_gpu_pandaproxy_fetch.py."""
import base64
import re
import subprocess
from pathlib import Path

import pytest

import kafka_batches as kb
import oracle.oracle as orc
import pp_fetch as pp

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "redpanda_amd" / "csrc" / "rpgpu_pp.h"
PLAIN = ["-O2"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def build_host(out: Path, flags, csrc: Path = HEADER.parent) -> Path:
    subprocess.run(["g++", *flags, "-std=c++17", f"-I{csrc}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "pp_host.cpp"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return out


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("pp_host")
    return {False: build_host(d / "pp_host", PLAIN), True: build_host(d / "pp_host_san", SANITIZE)}


def host_input(case: pp.Case, path: Path):
    data, descs = case.arena()
    res, index, _ = orc.validate_arena(data, descs)
    topics, ranges, responses = case.tables()
    pp.write_host_input(path, data, descs, res, index, topics, ranges, responses)
    return res, index


def run_host(exe: Path, mode: str, inp: Path, out: Path):
    r = subprocess.run([str(exe), mode, str(inp), str(out)], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def check_render(case: pp.Case, exp, exe: Path, inp: Path, out: Path):
    """None when the program's output equals the model's, else what differs first."""
    rc, stdout, stderr = run_host(exe, "render", inp, out)
    if rc != 0:
        return f"exit {rc}: {stderr[-1500:]}"
    got_res, got = pp.read_host_output(out, len(exp))
    want_res, _ = case.expected_results(exp)
    for f in pp.RESULT_DTYPE.names:
        bad = (got_res[f] != want_res[f]).nonzero()[0]
        if bad.size:
            return f"result field {f} differs at response {case.names[bad[0]]}: {got_res[bad[0]]} vs {want_res[bad[0]]}"
    for i, e in enumerate(exp):
        if got[i] != e[3]:
            return f"bytes of response {case.names[i]} differ"
    lane = sum(1 for e in exp for _, ln, _ in e[4] if ln <= pp.LANE_FIELD_MAX)
    wave = sum(1 for e in exp for _, ln, _ in e[4] if ln > pp.LANE_FIELD_MAX)
    if stdout.split() != ["lane", str(lane), "wave", str(wave)]:
        return f"path counts {stdout!r}, expected lane {lane} wave {wave}"
    return None


@pytest.fixture(scope="module")
def sweeps(tmp_path_factory):
    """Per arena format: the sweep, the model's answer and the host program's input file."""
    d = tmp_path_factory.mktemp("pp_sweep")
    out = {}
    for fmt in (kb.WIRE, kb.DISK):
        case = pp.build_sweep(fmt)
        exp = case.expected()
        pp.assert_sweep_classes(case, exp)
        inp = d / f"sweep{fmt}.bin"
        res, index = host_input(case, inp)
        out[fmt] = (case, exp, inp, res, index)
    return out


def test_constants_match_the_header():
    text = (ROOT / "include" / "rpgpu.h").read_text()
    assert int(re.search(r"#define RPGPU_PP_LANE_FIELD_MAX (\d+)", text).group(1)) == pp.LANE_FIELD_MAX
    names = re.search(r"enum rpgpu_pp_status \{(.*?)\}", text, re.S).group(1)
    assert [n.strip().split(" ")[0] for n in names.split(",") if n.strip()] == \
        ["RPGPU_PP_OK", "RPGPU_PP_BAD_BATCH", "RPGPU_PP_COMPRESSED", "RPGPU_PP_NOT_INDEXED", "RPGPU_PP_BAD_TOPIC",
         "RPGPU_PP_BAD_RANGE", "RPGPU_PP_NO_ROOM"]


@pytest.mark.parametrize("fmt", [kb.WIRE, kb.DISK], ids=["wire", "disk"])
def test_reference_vector(hosts, tmp_path, fmt):
    case, want = pp.golden_case(fmt)
    exp = case.expected()
    assert [e[3] for e in exp] == want                     # the model is pinned to the reference's string
    assert want[1] == b"[]"
    for san in (False, True):
        inp = tmp_path / "golden.bin"
        host_input(case, inp)
        assert check_render(case, exp, hosts[san], inp, tmp_path / "golden.out") is None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
@pytest.mark.parametrize("fmt", [kb.WIRE, kb.DISK], ids=["wire", "disk"])
def test_host_matches_the_model_over_the_sweep(hosts, sweeps, tmp_path, fmt, sanitize):
    case, exp, inp, res, _ = sweeps[fmt]
    # the arena is what the sweep says it is: the oracle's verdicts, codecs and index counts
    for kind, r in zip(case.kinds, res):
        assert (r["verdict"] == 0) == (kind != "crc"), kind
        if kind == "noindex":
            assert r["index_count"] == 0 and r["record_count"] > 0 or r["record_count"] == 0
        if kind in ("codec", "control_compressed"):
            assert r["codec"] == 1
    assert check_render(case, exp, hosts[sanitize], inp, tmp_path / "sweep.out") is None


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_fields_encoded_in_isolation(hosts, sweeps, tmp_path, sanitize):
    case, exp, inp, res, index = sweeps[kb.DISK]
    out = tmp_path / "fields.out"
    rc, _, stderr = run_host(hosts[sanitize], "fields", inp, out)
    assert rc == 0, (rc, stderr[-1500:])
    data, descs = case.arena()
    raw = data.tobytes()
    want = []
    for b, r in enumerate(res):
        if r["verdict"] != 0 or r["attrs"] & 0x20 or r["codec"] or r["index_count"] != r["record_count"]:
            continue
        for e in index[r["index_first"]: r["index_first"] + r["index_count"]]:
            for off, ln in ((e["key_off"], e["key_len"]), (e["val_off"], e["val_len"])):
                if ln > 0:
                    at = int(descs["offset"][b]) + int(off)
                    want.append(base64.b64encode(raw[at:at + int(ln)]))
    assert len(want) > 1000 and out.read_bytes() == b"".join(want)


# one-token changes to rpgpu_pp.h the sweep must reject
MUTATIONS = [
    ("lane/wave threshold", "(uint32_t)len <= lane_max", "(uint32_t)len < lane_max"),
    ("padding count", "const uint32_t pad = 3 - rem;", "const uint32_t pad = 2 - rem;"),
    ("digit count at 10^k", "n < 20 && m >= p", "n < 20 && m > p"),
    ("sign of INT64_MIN", "RPP_HD uint64_t dec_mag(", "RPP_HD int64_t dec_mag("),
    ("comma in front of a later range's first object", "(range_off | off_in_range) == 0", "(off_in_range) == 0"),
]


def test_the_unmutated_copy_passes(sweeps, tmp_path):
    """The mutation harness itself: an unchanged copy of the header is accepted."""
    case, exp, inp, _, _ = sweeps[kb.DISK]
    (tmp_path / "rpgpu_pp.h").write_text(HEADER.read_text())
    exe = build_host(tmp_path / "pp_host_copy", PLAIN, csrc=tmp_path)
    assert check_render(case, exp, exe, inp, tmp_path / "copy.out") is None


@pytest.mark.parametrize("what,old,new", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutations_are_rejected(sweeps, tmp_path, what, old, new):
    case, exp, inp, _, _ = sweeps[kb.DISK]
    text = HEADER.read_text()
    assert text.count(old) == 1, what
    (tmp_path / "rpgpu_pp.h").write_text(text.replace(old, new))
    exe = build_host(tmp_path / "pp_host_mut", PLAIN, csrc=tmp_path)
    assert check_render(case, exp, exe, inp, tmp_path / "mut.out") is not None, what
