"""The tiered-storage offset index on the device (rpgpu_rsindex_plan_device /
rpgpu_rsindex_run_device / rpgpu_rsindex_find_device) against the Python model
tests/remote_index.py, field for field and byte for byte.  Outputs are
pre-filled with 0xA5 plus a guard, and nothing outside the OK blobs may change.
The sweep's geometry classes are asserted by remote_index.assert_sweep_classes
(sample, batch and segment counts, trip geometry, configuration batches, every
row width, every status); then small output buffers, determinism, lookups on
both columns with every BAD_BLOB kind, a decode check through find, and the
round trip append -> index -> find -> remote read through the engine's own
entry points."""
import numpy as np
import pytest

import remote_index as ri

pytestmark = pytest.mark.gpu

FILL, GUARD = 0xA5, 256


@pytest.fixture(scope="module")
def sweep():
    case = ri.build_sweep()
    exp = case.expected()
    ri.assert_sweep_classes(case, exp)
    return case, exp, case.arena()


def same(a, b, what):
    for f in a.dtype.names:
        bad = np.nonzero(a[f] != b[f])[0]
        assert bad.size == 0, f"{what}.{f} differs at {bad[:6]}: {a[f][bad[:6]]} vs {b[f][bad[:6]]}"


def check(exp, got, out_cap):
    assert tuple(int(t) for t in got["totals"]) == ri.totals(exp)
    same(got["plan_results"], ri.expected_results(exp), "plan_results")
    same(got["results"], ri.expected_results(exp, out_cap), "results")
    assert len(got["out"]) == out_cap + GUARD
    bad = np.nonzero(got["out"] != ri.expected_out(exp, out_cap, FILL, GUARD))[0]
    assert bad.size == 0, f"output bytes differ at {bad[:8]}"


def test_sweep_parity(eng, sweep):
    case, exp, arena = sweep
    got = eng.rsindex_build(*arena, fill=FILL, guard=GUARD)
    assert got["out_cap"] == ri.totals(exp)[0]
    check(exp, got, got["out_cap"])


@pytest.mark.parametrize("short", [0, 1, 500, None], ids=["total", "total-1", "total-500", "zero"])
def test_small_output_buffers(eng, sweep, short):
    case, exp, arena = sweep
    cap = 0 if short is None else ri.totals(exp)[0] - short
    got = eng.rsindex_build(*arena, out_cap=cap, fill=FILL, guard=GUARD)
    want = ri.expected_results(exp, cap)
    lost = int((want["status"] == ri.NO_ROOM).sum())
    assert lost == (0 if short == 0 else 1 if short == 1 else sum(b.status == ri.OK for b in exp) if short is None
                    else lost) and (lost >= 2 or short != 500)
    check(exp, got, cap)


def test_a_plan_run_twice_gives_the_same_bytes(eng, sweep):
    case, exp, arena = sweep
    a = eng.rsindex_build(*arena, plans=2, runs=2, fill=FILL, guard=GUARD)
    b = eng.rsindex_build(*arena, fill=FILL, guard=GUARD)
    check(exp, a, a["out_cap"])
    for k in ("out", "results", "plan_results", "totals"):
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


def pack_queries(blobs, queries):
    """blobs: list of bytes; queries: (blob number, by_rp, bound).  The blobs lie back to
    back at odd offsets, the last one ending the buffer."""
    offs, cur = [], 1
    for b in blobs:
        offs.append(cur)
        cur += len(b) + (1 if len(b) % 2 == 0 else 2)
    last = len(blobs) - 1
    arena = np.full(offs[last] + len(blobs[last]), 0x5A, dtype=np.uint8)
    for o, b in zip(offs, blobs):
        arena[o:o + len(b)] = np.frombuffer(b, dtype=np.uint8)
    from redpanda_amd import abi

    q = np.zeros(len(queries), dtype=abi.RSINDEX_QUERY_DTYPE)
    q["blob_offset"] = [offs[i] for i, _, _ in queries]
    q["blob_bytes"] = [len(blobs[i]) for i, _, _ in queries]
    q["by_rp"] = [int(r) for _, r, _ in queries]
    q["upper_bound"] = [b for _, _, b in queries]
    return arena, q


def found_tuples(a):
    assert (a["reserved"] == 0).all()
    return [(int(r["status"]), int(r["from_write_buffer"]), int(r["ix"]), int(r["rp_offset"]), int(r["kaf_offset"]),
             int(r["file_pos"])) for r in a]


def test_find_parity(eng, sweep):
    """Every sample value and value +- 1 on both columns (remote_index.sweep_queries), below
    the first and above the last; indexes with num_elements & 15 == 0, with no rows and with
    no samples are among the sweep's; every BAD_BLOB kind; blobs from the device's own run."""
    case, exp, arena = sweep
    got = eng.rsindex_build(*arena)
    ok = [i for i, b in enumerate(exp) if b.status == ri.OK]
    for i in ok:
        o = int(got["results"]["out_offset"][i])
        assert got["out"][o:o + exp[i].out_bytes].tobytes() == exp[i].blob
    queries = ri.sweep_queries(case, exp)
    used = {i for i, _, _ in queries}
    assert any(exp[i].samples and exp[i].samples % 16 == 0 for i in used)
    assert any(exp[i].samples and exp[i].rows == 0 for i in used) and any(exp[i].samples == 0 for i in used)
    blobs = [b.blob for b in exp]
    bad = ri.bad_blobs(exp[[s.name for s in case.segments].index("samples17")].blob)
    for b in bad.values():
        queries += [(len(blobs), True, 5010), (len(blobs), False, 5010)]
        blobs.append(b)
    keep = sorted({i for i, _, _ in queries})
    renum = {i: k for k, i in enumerate(keep)}
    barena, q = pack_queries([blobs[i] for i in keep], [(renum[i], r, b) for i, r, b in queries])
    found = found_tuples(eng.rsindex_find(barena, q))
    cache, want = {}, []
    for i, by_rp, bound in queries:
        if i not in cache:
            try:
                cache[i] = ri.OffsetIndex.from_bytes(blobs[i])
            except ri.BadBlob:
                cache[i] = None
        want.append(cache[i].find(by_rp, bound).tuple() if cache[i] else ri.Found(ri.BAD_BLOB).tuple())
    assert sum(w[0] == ri.BAD_BLOB for w in want) == 2 * len(bad)
    assert {w[0] for w in want} == {ri.FOUND, ri.NONE, ri.BAD_BLOB} and {w[1] for w in want} == {0, 1}
    wrong = [k for k in range(len(want)) if found[k] != want[k]]
    assert not wrong, [(queries[k][1:], found[k], want[k]) for k in wrong[:5]]


def test_decode_through_find(eng, sweep):
    """Looking up sample + 1 returns that sample, for every sample of the 1,043-sample segment."""
    case, exp, _ = sweep
    i = [s.name for s in case.segments].index("samples1043")
    smp = exp[i].index.samples
    assert len(smp) == 1043
    for by_rp in (True, False):
        barena, q = pack_queries([exp[i].blob], [(0, by_rp, t[0 if by_rp else 1] + 1) for t in smp])
        found = found_tuples(eng.rsindex_find(barena, q))
        for k, t in enumerate(smp):
            wb = int(k >= 1040)
            assert found[k] == (ri.FOUND, wb, k - 1040 if wb else k, *t), k


def test_round_trip_through_the_engine(eng):
    """rpgpu_append_* output of a log with configuration and data batches -> index -> find ->
    rpgpu_remote_segment_parse_device from file_pos with the found delta and offset: the first
    batch there has base offset rp_offset and Kafka base kaf_offset, and parsing from position
    0 with the segment's base delta reaches the same batch."""
    import append_log as al
    from redpanda_amd import abi
    from test_remote_parse import ARCHIVAL, RAFT_CONFIG, RAFT_DATA, rread, seg

    types = [RAFT_CONFIG if k % 11 == 3 else ARCHIVAL if k % 17 == 5 else RAFT_DATA for k in range(150)]
    base, delta0 = 5000, 37
    c = al.Case(1)
    for b in seg(types, base=base, value_len=120):
        c.add(0, b, al.DISK)
    c.set_log(0, base, 0, 1 << 30, al.ROLL_FIRST)
    data, descs = c.arena()
    res, _, _ = eng.submit(data, descs)
    ap = eng.append_arena(data, descs, res, c.logs)
    n, lr = int(ap["totals"][1]), ap["log_results"][0]
    assert n == len(types) and lr["status"] == al.OK
    out = ap["out"]
    segs = np.zeros(1, dtype=abi.RSINDEX_SEGMENT_DTYPE)
    segs[0] = (0, n, base, base - delta0, delta0, 1500, 1500)
    ix = eng.rsindex_build(out, ap["out_descs"][:n], segs)
    r = ix["results"][0]
    assert r["status"] == ri.OK and r["samples"] > 20 and r["rows"] >= 1 and r["stream_bytes"] == lr["byte_size"]
    blob = ix["out"][int(r["out_offset"]):int(r["out_offset"]) + int(r["out_bytes"])].tobytes()
    x = ri.OffsetIndex.from_bytes(blob)
    smp = x.decoded(1) + x.wb[1][:x.pos % 16]
    targets = [smp[3] + 1, smp[17] + 2, smp[-1] + 1]
    barena, q = pack_queries([blob], [(0, False, t) for t in targets])
    found = eng.rsindex_find(barena, q)
    assert set(found["from_write_buffer"]) == {0, 1}
    padded = np.concatenate([out, np.zeros(64, np.uint8)])
    for f, t in zip(found, targets):
        assert f["status"] == ri.FOUND and f["kaf_offset"] < t
        rp, kaf, fpos = int(f["rp_offset"]), int(f["kaf_offset"]), int(f["file_pos"])
        seek = rread(int(lr["out_offset"]) + fpos, int(lr["byte_size"]) - fpos, start_offset=kaf,
                     cur_delta=rp - kaf, cur_rp_offset=rp)
        full = rread(int(lr["out_offset"]), int(lr["byte_size"]), start_offset=kaf, cur_delta=delta0,
                     cur_rp_offset=base)
        a, b = eng.remote_segment_parse(padded, seek), eng.remote_segment_parse(padded, full)
        for p in (a, b):
            assert p["results"]["status"][0] == abi.V_OK and p["results"]["accepted"][0] > 0
            d0 = p["descs"][0]
            assert int(d0["offset"]) == int(lr["out_offset"]) + fpos
            hdr = np.frombuffer(out[int(d0["offset"]):int(d0["offset"]) + 61].tobytes(), dtype=abi.RP_HEADER_DTYPE)[0]
            assert int(hdr["base_offset"]) == rp and int(p["kafka_base"][0]) == kaf
        assert a["results"]["cur_delta"][0] == b["results"]["cur_delta"][0]
        assert a["results"]["cur_rp_offset"][0] == b["results"]["cur_rp_offset"][0]
