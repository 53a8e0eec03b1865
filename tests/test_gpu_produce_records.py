"""Produce batches from records on the device (rpgpu_produce_plan_device /
rpgpu_produce_run_device) against tests/produce_records.py's restatement of
client::produce_records: every array the run writes -- request results, batch
rows, row maps, the output bytes, descriptors, result rows, the index and its
count -- and two chain checks: the output through the engine's validate path,
and rpgpu_kafka_serialize_device over it against the model's wire bytes.

The shapes are the smallest at which each piece can go wrong: row counts
around a wavefront and around kScanBlock = kSortBlock = 1024; 1, 2 and 65
requests with empty ones first, in the middle and last; ids that need the
signed order, the 2^31 bias and a second radix digit; a round-robin run across
wavefront and workgroup boundaries; every key length at every misalignment;
the varint boundaries of the offset delta (64, 65, 8,193 records a group) and
of the record length (63 / 64 bytes); every guard rail beside requests that
must come out bit-exact."""

import numpy as np
import pytest

import produce_records as pr
import oracle.oracle as orc

pytestmark = pytest.mark.gpu


def compare(eng, a, out_cap=None, runs=1, chain=False):
    from redpanda_amd import abi

    m = pr.model(a["data"], a["rows"], a["requests"], out_cap)
    got = eng.produce_records(a["data"], a["rows"], a["requests"], out_cap=out_cap, runs=runs)
    n = len(a["rows"])
    assert (got["out_bytes"], got["nbatches"], got["out_cap"]) == (m["out_bytes"], m["nbatches"], m["out_cap"])
    for f in abi.PRODUCE_RESULT_DTYPE.names:
        assert np.array_equal(got["req_results"][f], m["req_results"][f]), (f, got["req_results"], m["req_results"])
    for f in abi.PRODUCE_BATCH_DTYPE.names:
        bad = np.nonzero(got["all_batches"][f] != m["all_batches"][f])[0]
        assert bad.size == 0, f"batch rows: {f} differs at {bad[:8]}"
    assert np.array_equal(got["row_batch"], m["row_batch"]), "row_batch"
    assert np.array_equal(got["row_delta"], m["row_delta"]), "row_delta"
    bad = np.nonzero(got["out"] != m["out"])[0]
    assert bad.size == 0, f"out differs at {bad[:8]} of {len(m['out'])}"
    assert (got["guard"] == 0xA5).all(), "written past out_cap"
    for f in abi.DESC_DTYPE.names:
        assert np.array_equal(got["out_descs"][f], m["out_descs"][f]), f
    want_descs = m["out_descs"].copy()
    want_descs["ops"] = np.where(want_descs["ops"] != 0, 15, 0)
    wres, windex, wused = orc.validate_arena(m["out"], want_descs)
    nb = len(m["batches"])
    assert (wres["verdict"][:nb] == abi.V_OK).all() and (wres["verdict"][nb:] == abi.V_STREAM_SHORT).all()
    for f in abi.RESULT_DTYPE.names:
        bad = np.nonzero(got["out_results"][f] != wres[f])[0]
        assert bad.size == 0, f"out_results: {f} differs at {bad[:8]}: {got['out_results'][f][bad[:8]]} vs {wres[f][bad[:8]]}"
    assert got["used"] == wused == int((m["row_batch"] != pr.NONE).sum())
    assert np.array_equal(got["index"].view(np.uint8), windex[:wused].view(np.uint8)), "index differs"
    if chain and nb:
        descs = got["out_descs"][:nb].copy()
        descs["ops"] = 15
        res, _, used = eng.submit(got["out"], descs)
        assert (res["verdict"] == abi.V_OK).all() and used == wused
        wire, _ = eng.kafka_serialize(got["out"], got["out_descs"][:nb])
        assert np.array_equal(wire, m["wire"]), "wire bytes differ"
    return got, m


def test_hand_request(eng):
    got, m = compare(eng, pr.hand_call(), chain=True)
    assert got["req_results"].tolist() == [(pr.OK, 7, 0, 4)]
    for (part, body), b in zip(pr.HAND_BODIES, got["batches"]):
        o, ln = int(b["out_offset"]), int(b["out_len"])
        assert int(b["partition"]) == part and got["out"][o + 61:o + ln].tobytes() == body


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 1023, 1024, 1025])
def test_rows_per_call(eng, nrows):
    compare(eng, pr.size_call(nrows))


@pytest.mark.parametrize("nreq,empty_at", [(2, ()), (65, (0, 31, 64)), (4, (0, 1, 3))])
def test_requests(eng, nreq, empty_at):
    got, m = compare(eng, pr.size_call(300, nreq, empty_at), chain=nreq == 65)
    for at in empty_at:
        assert got["req_results"][at].tolist()[0] == pr.OK and got["req_results"]["nbatches"][at] == 0


def test_only_empty_requests(eng):
    a = pr.Call().request(6, 2).request(0, 0).request(6, 5).build()
    got, m = compare(eng, a)
    assert got["req_results"].tolist() == [(pr.OK, 2, 0, 0), (pr.OK, 0, 0, 0), (pr.OK, 5, 0, 0)]


@pytest.mark.parametrize("partition_count", [0, 1, 2, 6, 300])
def test_partition_ids(eng, partition_count):
    """Explicit ids -1, INT32_MIN, INT32_MAX and partition_count itself beside hashed and
    round-robin rows; two requests that share their ids give separate batches."""
    got, m = compare(eng, pr.ids_call(partition_count))
    b = got["batches"]
    order = list(zip(b["request"].tolist(), b["partition"].tolist()))
    assert order == sorted(order) and order[0] == (0, pr.INT32_MIN) and order[-1] == (1, pr.INT32_MAX)


def test_uncached_topic_without_ids(eng):
    a = pr.Call().request(0, 3)
    for i in range(70):
        a.row(b"key%d" % i if i % 2 else None, b"v")
    got, m = compare(eng, a.build())
    assert got["req_results"].tolist() == [(pr.OK, 3, 0, 1)] and int(got["batches"]["partition"][0]) == 0


def test_round_robin_run(eng):
    got, m = compare(eng, pr.round_robin_call(2100))
    assert got["req_results"]["rr_next"].tolist() == m["req_results"]["rr_next"].tolist()


def test_key_geometry(eng):
    compare(eng, pr.key_geometry_call(), chain=True)


def test_values_and_length_varint(eng):
    compare(eng, pr.value_call(), chain=True)


def test_group_sizes_and_stability(eng):
    """Groups of 64, 65 and 8,193 records whose values are their row numbers, rows of other
    partitions between them."""
    a = pr.group_call()
    got, m = compare(eng, a)
    big = got["batches"][got["batches"]["record_count"] == 8193]
    assert len(big) == 1 and int(big["partition"][0]) == 3


@pytest.mark.parametrize("which", sorted(pr.GUARDS))
def test_guard_rails(eng, which):
    got, m = compare(eng, pr.guard_call(which))
    assert got["req_results"]["status"].tolist() == [pr.OK, pr.GUARDS[which], pr.OK]


def test_requests_that_do_not_tile_the_rows(eng):
    a = pr.random_call(6, 100, 3)
    a["requests"]["nrows"][1] += 1
    got, m = compare(eng, a)
    assert got["req_results"]["status"].tolist() == [pr.BAD_REQUEST] * 3 and got["used"] == 0


def test_out_overflow_writes_nothing_past_out_cap(eng):
    a = pr.random_call(5, 60, 4)
    m = pr.model(a["data"], a["rows"], a["requests"])
    cut = int(m["batches"]["out_offset"][int(m["req_results"]["first_batch"][2])]) + pr.TAIL_PAD
    got, small = compare(eng, a, out_cap=cut)
    st = got["req_results"]["status"].tolist()
    assert st[:2] == [pr.OK, pr.OK] and pr.OUT_OVERFLOW in st[2:]
    compare(eng, a, out_cap=m["out_bytes"])                  # one tail pad short: the last request


@pytest.mark.parametrize("seed", [201, 202, 203])
def test_sweep(eng, seed):
    compare(eng, pr.random_call(seed, 400, 7, empty_at=(3,)), runs=2 if seed == 201 else 1, chain=seed == 203)
