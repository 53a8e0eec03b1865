"""rpgpu_compaction_tx_filter_device and rpgpu_compaction_keep_tx_device on the
device, field for field against the literal tx_reducer of tests/tx_compaction.py
(which tests/test_tx_compaction.py pins to hand-written expectations, to the
closed form and to the host build of the kernels' own header).

Both outputs are pre-filled with 0xA5 and carry a guard behind them (Engine.
tx_filter): nothing outside the n flags and the nscopes rows may change.

The sweep crosses what the hand cases do not: scopes on both sides of the 64
batches and 64 ranges of a wave trip, more scopes than a workgroup has waves,
more than 1,024 batches (a second sort block), more than 256 table slots in use
(a second digit pass), producers whose home slots collide."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import compaction_geometry as geo  # noqa: E402
import test_tx_compaction as cpu  # noqa: E402
import tx_compaction as tx  # noqa: E402
from kafka_batches import DISK, WIRE  # noqa: E402

import oracle.oracle as orc  # noqa: E402
from redpanda_amd import abi  # noqa: E402

pytestmark = pytest.mark.gpu

FMTS, FMT_IDS = cpu.FMTS, cpu.FMT_IDS


def run(eng, a):
    got = eng.tx_filter(*cpu.args(a))
    n, ns = len(a["descs"]), len(a["scopes"])
    assert (got["discard_raw"][n:] == 0xA5).all(), "flags written past n"
    assert (got["stats_raw"][ns * abi.TX_STATS_DTYPE.itemsize:] == 0xA5).all(), "a row written past nscopes"
    return got


def same_by_scope(a, got, want, shape):
    """Class by class: every scope's flags and row, named by its (batches, ranges)."""
    wd, ws = want
    for s, sc in enumerate(a["scopes"]):
        lo, hi = int(sc["first_batch"]), int(sc["first_batch"]) + int(sc["batch_count"])
        what = f"scope {s} {shape[s]}"
        assert np.array_equal(got["discard"][lo:hi], wd[lo:hi]), (
            f"{what}: flags differ at {np.nonzero(got['discard'][lo:hi] != wd[lo:hi])[0][:8]}")
        for f in ws.dtype.names:
            assert got["stats"][s][f] == ws[s][f], f"{what}: stats.{f} {got['stats'][s][f]} != {ws[s][f]}"
    cpu.same((got["discard"], got["stats"]), want)


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("name", cpu.SWEEP)
def test_gpu_sweep(eng, name, fmt):
    a = cpu.sweep_call(name, fmt)
    same_by_scope(a, run(eng, a), a["want"], tx.sweep_shapes()[name])


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("name", list(cpu.HAND))
def test_gpu_hand_case(eng, name, fmt):
    """Every rule of the reference and every stopping status, once per format."""
    a, flags, stats = cpu.hand_case(name, fmt)
    got = run(eng, a)
    cpu.same((got["discard"], got["stats"]), (flags, stats), name)


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_gpu_colliding_home_slots(eng, fmt):
    c, pids = tx.collision_call(fmt)
    cap = tx.table_cap(len(c.batches))
    assert len({tx.pid_hash(0, p, 0) & (cap - 1) for p in pids}) == 1
    a = c.build()
    want = tx.model(*cpu.args(a))
    assert (want[0] == abi.TX_ABORTED_DATA).any()
    got = run(eng, a)
    cpu.same((got["discard"], got["stats"]), want, "collision")


def test_gpu_no_scopes_and_no_batches(eng):
    a = cpu.sweep_call("five-a", DISK)
    empty = dict(a, scopes=a["scopes"][:0])
    got = run(eng, empty)
    assert (got["discard"] == abi.TX_NOT_REACHED).all() and len(got["stats"]) == 0


def test_gpu_two_runs_give_identical_bytes(eng):
    a = cpu.sweep_call("seventy", DISK)
    one, two = run(eng, a), run(eng, a)
    assert np.array_equal(one["discard_raw"], two["discard_raw"])
    assert np.array_equal(one["stats_raw"], two["stats_raw"])


# -------------------------------------------------------------------- keep_tx
@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_gpu_keep_tx_without_flags_is_keep(eng, fmt):
    """A null pointer and all-zero flags: rpgpu_compaction_keep_device byte for byte."""
    for a in (cpu.sweep_call("five-a", fmt), geo.oracle_chain("key_edge", fmt), geo.oracle_chain("count", fmt)):
        idx = a["idx"]
        keep, nkeys = eng.compaction_keep(a["data"], a["descs"], a["res"], idx)
        for flags in (None, np.zeros(len(a["descs"]), np.uint8), np.full(len(a["descs"]), abi.TX_NOT_REACHED, np.uint8)):
            k, nk = eng.compaction_keep_tx(a["data"], a["descs"], a["res"], idx, flags)
            assert np.array_equal(k, keep) and nk == nkeys
        wkeep, wkeys = orc.compaction_keep(a["data"], a["descs"], a["res"], idx)
        assert np.array_equal(keep, wkeep) and nkeys == wkeys


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_gpu_keep_tx_equals_model(eng, fmt):
    for a in (cpu.sweep_call("five-a", fmt), cpu.sweep_call("five-b", fmt), cpu.duplicate_offset_call(fmt)):
        discard = run(eng, a)["discard"]
        assert np.array_equal(discard, tx.model(*cpu.args(a))[0])
        keep, nkeys = eng.compaction_keep_tx(a["data"], a["descs"], a["res"], a["idx"], discard)
        wkeep, wkeys = tx.keep_tx(a["data"], a["descs"], a["res"], a["idx"], discard)
        assert np.array_equal(keep, wkeep) and nkeys == wkeys
    first = a["res"]["index_first"]  # the duplicate-offset call: the hostile duplicate is kept
    assert [int(keep[int(f)]) for f in first] == [1, 1, 1, 0, 0]


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_gpu_filter_keep_rewrite_end_to_end(eng, fmt):
    """filter -> keep_tx -> the existing rewrite: flagged batches DROPPED,
    committed transactional data TX_CLEARED, and every output batch what the
    oracle's keep and rewrite make of the arena without the flagged batches."""
    a = cpu.sweep_call("five-b", fmt)
    data, descs, res, idx = a["data"], a["descs"], a["res"], a["idx"]
    discard = run(eng, a)["discard"]
    keep, _ = eng.compaction_keep_tx(data, descs, res, idx, discard)
    got = eng.compaction_rewrite(data, descs, res, idx, keep)
    flagged = (discard >= 1) & (discard <= 3)
    assert flagged.any() and (got["cres"]["action"][flagged] == abi.COMPACT_DROPPED).all()
    sel = np.nonzero(~flagged)[0]
    wkeep, _ = orc.compaction_keep(data, descs[sel], res[sel], idx)
    want = orc.compaction_rewrite(data, descs[sel], res[sel], idx, wkeep)
    cleared = 0
    for k, b in enumerate(sel):
        g, w = got["cres"][b], want["cres"][k]
        for f in ("action", "record_count", "out_len", "removed"):
            assert g[f] == w[f], (b, f, g[f], w[f])
        gb = got["out"][int(g["out_offset"]):int(g["out_offset"]) + int(g["out_len"])]
        wb = want["out"][int(w["out_offset"]):int(w["out_offset"]) + int(w["out_len"])]
        assert np.array_equal(gb, wb), f"output of batch {b} differs"
        committed_tx_data = (res["attrs"][b] & 0x30) == 0x10 and g["action"] in (abi.COMPACT_KEPT, abi.COMPACT_TX_CLEARED)
        if committed_tx_data:
            assert g["action"] == abi.COMPACT_TX_CLEARED
            cleared += 1
    assert cleared > 0
