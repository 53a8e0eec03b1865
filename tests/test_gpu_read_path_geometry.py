"""Device side of the read-path geometry sweeps: the families of
tests/read_path_geometry.py through rpgpu_segment_parse_device,
rpgpu_remote_segment_parse_device, rpgpu_kafka_serialize_device and
rpgpu_segment_index_device, each output array compared whole with the oracle's
(unwritten descriptor, gap and kafka_base slots included: they stay zero).
tests/test_read_path_geometry.py pins the oracle on the same cases."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import read_path_geometry as g  # noqa: E402

import oracle.oracle as orc  # noqa: E402
from redpanda_amd import abi  # noqa: E402

pytestmark = pytest.mark.gpu

WAVES_PER_BLOCK = 4  # kWavesPerBlock of the two parser kernels
SERIALIZE_WAVES = 65536  # serialize_kernel: at most 16384 blocks of 4 waves


def check_segment(what, reads, names, got, want):
    wres, wdescs = want
    g.assert_struct_equal(what + " results", names, got["results"], wres)
    g.assert_struct_equal(what + " descs", g.slot_owner(reads, names, len(wdescs)), got["descs"], wdescs)
    g.assert_bytes_equal(what + " results", got["results"], wres)
    g.assert_bytes_equal(what + " descs", got["descs"], wdescs)


def check_remote(what, reads, names, got, want):
    wres, wdescs, wkb, wgaps = want
    g.assert_struct_equal(what + " results", names, got["results"], wres)
    owner = g.slot_owner(reads, names, len(wdescs))
    g.assert_struct_equal(what + " descs", owner, got["descs"], wdescs)
    i = g.first_diff(got["kafka_base"], wkb)
    assert i is None, f"{what}: {owner[i]}: kafka_base differs at slot {i}: got {got['kafka_base'][i]} want {wkb[i]}"
    i = g.first_diff(got["gaps"], wgaps)
    gowner = g.slot_owner(reads, names, len(wgaps), "gap_first", "gap_cap")
    assert i is None, f"{what}: {gowner[i // 2]}: gaps differ at {i // 2}: got {got['gaps'][i // 2]} want {wgaps[i // 2]}"
    g.assert_bytes_equal(what + " results", got["results"], wres)
    g.assert_bytes_equal(what + " descs", got["descs"], wdescs)


def run_parser(eng, kind, what, data, reads, names):
    if kind == "seg":
        check_segment(what, reads, names, eng.segment_parse(data, reads), orc.segment_parse(data, reads))
    else:
        check_remote(what, reads, names, eng.remote_segment_parse(data, reads), orc.remote_segment_parse(data, reads))


@pytest.mark.parametrize("fam", ["A", "B"])
def test_segment_parser(eng, fam):
    data, reads, names, _ = g.family_a() if fam == "A" else g.family_b("seg")
    run_parser(eng, "seg", fam, data, reads, names)


@pytest.mark.parametrize("fam", ["B", "E"])
def test_remote_parser(eng, fam):
    data, reads, names, _ = g.family_e() if fam == "E" else g.family_b("remote")
    run_parser(eng, "remote", fam, data, reads, names)


@pytest.mark.parametrize("kind", ["seg", "remote"])
@pytest.mark.parametrize("nreads", [1, 3, 4, 5, "2 * grid * 4 + 3"])
def test_parser_scheduling(eng, kind, nreads):
    """Fewer reads than one block has waves, one more, and more than twice the
    context's grid: every wave strides through at least two reads, some of them
    300 headers long."""
    _, grid = eng.device_info()
    n = 2 * grid * WAVES_PER_BLOCK + 3 if isinstance(nreads, str) else nreads
    data, reads, names, _ = g.family_c_parse(kind, n)
    assert len(reads) == n
    run_parser(eng, kind, f"C {n} reads", data, reads, names)


def test_serializer_scheduling(eng):
    n = 2 * SERIALIZE_WAVES + 5
    data, descs, terms = g.family_c_serialize(n)
    rg = np.array([(0, n), (SERIALIZE_WAVES - 1, 3), (n - 5, 5)], dtype=abi.FETCH_RANGE_DTYPE)
    out, sums = eng.kafka_serialize(data, descs, terms, rg)
    want, wsums = orc.kafka_serialize(data, descs, terms, rg)
    i = g.first_diff(out, want)
    assert i is None, f"out differs at byte {i} (batch {i // g.HDR}, header byte {i % g.HDR})"
    g.assert_bytes_equal("summaries", sums, wsums)


@pytest.mark.parametrize("kind", ["seg", "remote"])
def test_positions_past_2gib(eng, kind):
    """One read of 2^31 + 4096 bytes whose second and third headers lie at
    2^31 - 512 and 2^31 + 512.  The arena is zeroed on the device and only the
    three headers are copied in."""
    import torch

    hdrs, reads, names = g.family_d(kind)
    dev = torch.device("cuda", eng.device)
    d_data = torch.zeros(g.D_LENGTH + 64, dtype=torch.uint8, device=dev)
    for p, h in hdrs:
        d_data[p:p + g.HDR] = torch.from_numpy(np.frombuffer(h, dtype=np.uint8).copy()).to(dev)
    host, _, _ = g.family_d_host(kind)
    try:
        if kind == "seg":
            got, want = eng.segment_parse_device(d_data, reads), orc.segment_parse(host, reads)
            check_segment("D", reads, names, got, want)
            assert (got["results"]["accepted"][0], got["results"]["last_error"][0]) == (3, abi.V_END_OF_STREAM)
        else:
            got, want = eng.remote_segment_parse_device(d_data, reads), orc.remote_segment_parse(host, reads)
            check_remote("D", reads, names, got, want)
            assert list(got["results"]["accepted"]) == [2, 1]
    finally:
        del d_data
        torch.cuda.empty_cache()


def test_serializer_copy_geometry(eng):
    data, descs, terms, pairs, extras = g.family_f()
    out, _ = eng.kafka_serialize(data, descs, terms)
    want, _ = orc.kafka_serialize(data, descs, terms)
    i = g.first_diff(out, want)
    if i is not None:
        k = int(np.searchsorted(descs["offset"], i, side="right")) - 1
        o = int(descs["offset"][k])
        raise AssertionError(f"out differs at byte {i}: batch {k} at offset {o} (mod 16 = {o % 16}), "
                             f"length {int(descs['length'][k])}, byte {i - o} of it: got {out[i]} want {want[i]}")
    k = extras["distinct header"]
    o = int(descs["offset"][k])
    assert out[o:o + g.HDR].tobytes() == g.wire_header(data[o:o + g.HDR].tobytes(), int(terms[k]))


def test_summary_scans(eng):
    data, descs, ranges, names = g.family_g()
    _, sums = eng.kafka_serialize(data, descs, None, ranges)
    _, wsums = orc.kafka_serialize(data, descs, None, ranges)
    g.assert_struct_equal("G summaries", names, sums, wsums)
    g.assert_bytes_equal("G summaries", sums, wsums)
    for k, (rg, name) in enumerate(zip(ranges, names)):
        want = g.python_summary_skipping(data, descs, len(descs), int(rg["first"]), int(rg["count"]))
        if not want["has_first_tx"]:
            del want["first_tx_batch_offset"]
        assert {f: int(sums[f][k]) for f in want} == want, name


@pytest.mark.parametrize("nsegs", [None, 255, 256, 257])
def test_segment_index(eng, nsegs):
    data, descs, segs, names = g.family_h(nsegs)
    got = eng.segment_index(data, descs, segs)
    res, _, _ = orc.validate_arena(data, descs)
    g.assert_bytes_equal("H validation results", got["results"], res)
    st, e = orc.segment_index(descs, res, segs)
    g.assert_struct_equal("H states", names, got["states"], st)
    owner = [names[s] for s in range(len(segs)) for _ in range(int(segs["batch_count"][s]))]
    g.assert_struct_equal("H entries", owner, got["entries"], e)
    g.assert_bytes_equal("H states", got["states"], st)
    g.assert_bytes_equal("H entries", got["entries"], e)
