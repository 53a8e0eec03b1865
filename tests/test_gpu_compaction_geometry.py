"""Device compaction (rpgpu_compaction_keep_device, rpgpu_compaction_rewrite_*)
over the record-geometry arenas of tests/compaction_geometry.py, bit for bit
against the serial oracle (oracle/compact.c), which tests/test_compaction.py
pins to independent restatements on the same arenas.

The arenas cross what the small arenas of tests/test_compaction.py do not: a
second lane trip over a batch's records (> 64), key and value lengths on both
sides of the 8-byte hash word, the 16-byte copy vector and its 1024-byte
stride, the key table and keep set at 0.5 load and probing past the last slot,
output offsets past the first 1024-batch scan block, an output buffer below
the plan, an index shorter than the batches' slices, and the decompress path's
output (slack entries inside the index) as compaction's input."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import compaction_geometry as geo  # noqa: E402
from kafka_batches import DISK, WIRE  # noqa: E402

import oracle.oracle as orc  # noqa: E402
from redpanda_amd import abi  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(name, fmt) for name in geo.BUILDERS for fmt in (DISK, WIRE)]
IDS = [f"{name}-{'disk' if fmt == DISK else 'wire'}" for name, fmt in CASES]


def same_fields(got, want, what):
    for f in want.dtype.names:
        bad = np.nonzero(got[f] != want[f])[0]
        assert bad.size == 0, f"{what}.{f} differs at {bad[:8]}: gpu {got[f][bad[:8]]} oracle {want[f][bad[:8]]}"


def same_keep(got, want):
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]])


def same_out_descs(got, want):
    """The engine asks for RPGPU_OP_RECRC on its outputs (it computes their CRCs
    with the validation kernels) and the oracle, which stamps them itself, does
    not: by design the only difference between the two out_descs."""
    for f in ("offset", "length", "partition", "format", "flags"):
        bad = np.nonzero(got["out_descs"][f] != want["out_descs"][f])[0]
        assert bad.size == 0, f"out_descs.{f} differs at {bad[:8]}"
    ops = got["out_descs"]["ops"] & ~np.uint8(abi.OP_RECRC)
    assert np.array_equal(ops, want["out_descs"]["ops"])
    assert (got["out_descs"]["ops"][want["cres"]["out_len"] == 0] == 0).all()


def same_rewrite(got, want):
    same_fields(got["cres"], want["cres"], "cres")
    assert got["out_bytes"] == want["out_bytes"]
    assert np.array_equal(got["out"][:want["out_bytes"]], want["out"][:want["out_bytes"]])
    same_fields(got["out_results"], want["out_results"], "out_results")
    assert got["used"] == want["used"]
    assert np.array_equal(got["index"].view(np.uint8), want["index"].view(np.uint8))
    same_out_descs(got, want)


@pytest.mark.parametrize("name,fmt", CASES, ids=IDS)
def test_gpu_geometry_chain(eng, name, fmt):
    """submit -> compaction_keep -> compaction_rewrite, every stage fed with the
    engine's own output of the stage before."""
    c = geo.oracle_chain(name, fmt)
    res, idx, _ = eng.submit(c["data"], c["descs"])
    assert np.array_equal(res.view(np.uint8), c["res"].view(np.uint8))
    assert len(idx) == len(c["idx"])
    for b in range(len(res)):  # the entries of each batch's slice; what lies between slices is unspecified
        lo, cnt = int(res["index_first"][b]), int(res["index_count"][b])
        assert np.array_equal(idx[lo:lo + cnt], c["idx"][lo:lo + cnt]), f"index of batch {b} differs"
    keep, nkeys = eng.compaction_keep(c["data"], c["descs"], res, idx)
    assert nkeys == c["nkeys"]
    same_keep(keep, c["keep"])
    same_rewrite(eng.compaction_rewrite(c["data"], c["descs"], res, idx, keep), c["want"])


@pytest.mark.parametrize("fmt", [DISK, WIRE])
def test_gpu_truncated_index(eng, fmt):
    """index_cap in the middle of the 129-record batch: compact_keys_kernel's
    clamp of a slice's end, and the rewrite's SKIPPED for slices past the cut."""
    c = geo.oracle_chain("count", fmt)
    b, cut = geo.count_cut(c["res"])
    idx = c["idx"][:cut]
    wkeep, wkeys = orc.compaction_keep(c["data"], c["descs"], c["res"], idx)
    keep, nkeys = eng.compaction_keep(c["data"], c["descs"], c["res"], idx)
    assert nkeys == wkeys and len(keep) == cut
    same_keep(keep, wkeep)
    want = orc.compaction_rewrite(c["data"], c["descs"], c["res"], idx, wkeep)
    assert (want["cres"]["action"][b:] == abi.COMPACT_SKIPPED).all()
    same_rewrite(eng.compaction_rewrite(c["data"], c["descs"], c["res"], idx, keep), want)


@pytest.mark.parametrize("fmt", [DISK, WIRE])
def test_gpu_output_below_plan(eng, fmt):
    """out_cap = the planned offset of batch 1500 of 2600: every slot before it is
    written as planned, every later one is SKIPPED, and nothing is stored at or
    past out_cap (the buffer is larger, pre-filled with 0xA5 and compared whole)."""
    c = geo.oracle_chain("many_batches", fmt)
    full = c["want"]
    cap = int(full["cres"]["out_offset"][geo.SHORT_CAP_BATCH])
    alloc = full["out_bytes"] + 2 * abi.ARENA_TAIL_PAD
    got = eng.compaction_rewrite(c["data"], c["descs"], c["res"], c["idx"], c["keep"], out_cap=cap, alloc=alloc)
    assert got["out_bytes"] == full["out_bytes"] and got["out"].size == alloc

    slot = (full["cres"]["out_len"] + np.uint64(15)) & ~np.uint64(15)
    had = full["cres"]["out_len"] > 0
    fits = had & (full["cres"]["out_offset"] + slot <= cap)
    cut = had & ~fits
    assert fits[:geo.SHORT_CAP_BATCH][had[:geo.SHORT_CAP_BATCH]].all() and not fits[geo.SHORT_CAP_BATCH:].any()
    assert fits.sum() > 1024 and cut.sum() > 512  # both sides span a scan block's edge

    # expected: the oracle's full run with the slots past the buffer taken out
    wcres, wdescs = full["cres"].copy(), full["out_descs"].copy()
    for f, v in (("action", abi.COMPACT_SKIPPED), ("out_len", 0), ("record_count", 0), ("removed", 0)):
        wcres[f][cut] = v
    wdescs["length"][cut] = 0
    wdescs["ops"][cut] = 0
    wout = np.full(alloc, 0xA5, dtype=np.uint8)
    for i in np.nonzero(fits)[0]:
        o, n = int(full["cres"]["out_offset"][i]), int(full["cres"]["out_len"][i])
        wout[o:o + n] = full["out"][o:o + n]
    wres, widx, wused = orc.validate_arena(wout, wdescs)

    dropped = full["cres"]["action"] == abi.COMPACT_DROPPED
    assert dropped[geo.SHORT_CAP_BATCH:].any()
    assert (got["cres"]["action"][dropped] == abi.COMPACT_DROPPED).all()
    same_fields(got["cres"], wcres, "cres")
    assert (got["out"][cap:] == 0xA5).all()
    assert np.array_equal(got["out"], wout)
    same_fields(got["out_results"], wres, "out_results")
    assert got["used"] == wused
    assert np.array_equal(got["index"].view(np.uint8), widx.view(np.uint8))
    same_out_descs(got, dict(out_descs=wdescs, cres=wcres))


@pytest.mark.parametrize("fmt", [DISK, WIRE])
def test_gpu_compaction_over_decompressed(eng, fmt):
    """The decompress path's output arena (rpgpu.h names it as compaction's
    input): index slices with slack between them, so keep == 2 entries sit
    inside the index."""
    data, descs = geo.compressed_keyed_arena(fmt)
    d = eng.decompress_arena(data, descs)
    out, odescs, ores, idx = d["out"], d["out_descs"], d["out_results"], d["index"]
    ok = ores["verdict"] == abi.V_OK
    assert ok.sum() >= 50 and not ok.all() and (ores["codec"][ok] == 0).all()
    wkeep, wkeys = orc.compaction_keep(out, odescs, ores, idx)
    last = int(ores["index_first"][-1]) + int(ores["index_count"][-1])
    assert (wkeep[:last] == 2).any() and (wkeep == 0).any() and (wkeep == 1).any()
    keep, nkeys = eng.compaction_keep(out, odescs, ores, idx)
    assert nkeys == wkeys
    same_keep(keep, wkeep)
    want = orc.compaction_rewrite(out, odescs, ores, idx, wkeep)
    assert {abi.COMPACT_FILTERED, abi.COMPACT_DROPPED} <= set(int(a) for a in want["cres"]["action"])
    same_rewrite(eng.compaction_rewrite(out, odescs, ores, idx, keep), want)
