"""The planners' prefix sums at the edges of a scan block (kScanBlock = 1024
items per workgroup, 64 per wave): compress_caps_kernel, decomp_caps_kernel and
sets_count_kernel, then block_scan_kernel over the workgroups' totals.

Arenas of n one-record batches (record sets: n sets), n just below, at and
just above one block and just above two.  The items at the first and last lane
of a wave, of a block and of the arena alternate between one that gets a span
of the output and one that gets none; every other item gets one.  The scan is
checked exactly (each item starts where the spans before it end, the plan's
total is their sum), the values against the oracle as in the neighbouring
tests.  The compaction rewrite and the REST proxy have such cases in
tests/compaction_geometry.py and tests/pp_fetch.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
from kafka_batches import WIRE, arena, batch, record  # noqa: E402
from test_gpu_decomp import OPS, compare  # noqa: E402
from test_record_sets import sets_arena  # noqa: E402

import oracle.oracle as orc  # noqa: E402
from redpanda_amd import abi  # noqa: E402

pytestmark = pytest.mark.gpu

SIZES = [1023, 1024, 1025, 2049]
EDGES = [0, 63, 64, 1022, 1023, 1024, 1025, 2047, 2048]


def gets_none(n):
    """Per item: True where it gets no span (every second edge position)."""
    none = np.zeros(n, dtype=bool)
    for k, pos in enumerate(p for p in EDGES if p < n):
        none[pos] = k % 2 == 1
    return none


def recs(i):
    return [record(b"key-%d" % i, b"value %d " % i * (1 + i % 5), ts_delta=0, off_delta=0)]


def plain(i):
    return batch(recs(i), fmt=WIRE, base_offset=10 * i)


def lz4(i):
    return batch(orc.compress(3, b"".join(recs(i))), fmt=WIRE, base_offset=10 * i, record_count=1, attrs=3)


def assert_scanned(offsets, spans, total):
    spans = spans.astype(np.uint64)
    want = np.concatenate([[0], np.cumsum(spans)[:-1]]).astype(np.uint64)
    bad = np.nonzero(offsets.astype(np.uint64) != want)[0]
    assert bad.size == 0, f"offsets differ from the spans' prefix sums at {bad[:8]}"
    assert total == int(spans.sum())


@pytest.mark.parametrize("n", SIZES)
def test_compress_caps(eng, n):
    none = gets_none(n)
    data, descs = arena([lz4(i) if none[i] else plain(i) for i in range(n)], fmt=WIRE, ops=abi.OPS_PRODUCE)
    got = eng.compress_arena(data, descs, 3)
    cres = got["cres"]
    assert np.array_equal(cres["out_cap"] == 0, none)
    assert_scanned(cres["out_offset"], cres["out_cap"], got["out_bytes"])
    want = orc.compress_batches(data, descs, got["results"], 3)
    for i, w in enumerate(want):
        assert (w is None) == bool(none[i]), i
        if w is None:
            assert cres["verdict"][i] == abi.V_SKIPPED, i
            continue
        assert cres["verdict"][i] == 0, (i, cres["verdict"][i])
        o, m = int(cres["out_offset"][i]), 61 + int(cres["out_len"][i])
        assert got["out"][o:o + m].tobytes() == w, f"batch {i} differs"
        assert got["out_results"]["verdict"][i] == 0, i


@pytest.mark.parametrize("n", SIZES)
def test_decomp_caps(eng, n):
    none = gets_none(n)
    data, descs = arena([plain(i) if none[i] else lz4(i) for i in range(n)], fmt=WIRE, ops=OPS)
    got = eng.decompress_arena(data, descs)
    dres = got["dres"]
    assert np.array_equal(dres["out_cap"] == 0, none)
    assert_scanned(dres["out_offset"], dres["out_cap"], got["out_bytes"])
    compare(got, data, descs)
    assert (dres["verdict"][~none] == abi.V_OK).all()
    assert (dres["verdict"][none] != abi.V_OK).all()


@pytest.mark.parametrize("n", SIZES)
def test_sets_count(eng, n):
    none = gets_none(n)
    raw = [b"" if none[i] else b"".join(plain(2 * i + k) for k in range(1 + i % 2)) for i in range(n)]
    data, sets = sets_arena(raw)
    got = eng.record_sets(data, sets)
    s = got["sets"]
    assert np.array_equal(s["batch_count"], np.where(none, 0, 1 + np.arange(n) % 2))
    assert_scanned(s["first_batch"], s["batch_count"], len(got["batch_descs"]))
    want = orc.record_sets(data, sets)
    assert np.array_equal(s.view(np.uint8), want["sets"].view(np.uint8))
    assert np.array_equal(got["batch_descs"].view(np.uint8), want["batch_descs"].view(np.uint8))
    assert np.array_equal(got["batch_results"].view(np.uint8), want["batch_results"].view(np.uint8))
    assert got["used"] == want["used"]
    assert np.array_equal(got["index"].view(np.uint8), want["index"].view(np.uint8))
