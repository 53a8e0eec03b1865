"""The checksum wave's hand-over between batches of different geometry.

A wave prefetches the next batch's header window and first rows while it
checksums the current one.  The edge tests give every wave at most one
batch, and the multi-batch parity cases use one geometry, so here an engine
of one workgroup per CU (4 waves per CU) takes an arena of 4,400 batches of
eleven kinds cycled by i % 11.  Eleven is coprime to the wave count, so each
wave meets a run of different kinds: one chunk -> two chunks with seven
phantom rows, two -> three, header-only, tiny, many-chunk, and two kinds
the reference rejects: at least one per format fails in the header, a path
that only forwards the next batch's rows.
"""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(__file__))
import edge_cases  # noqa: E402
from kafka_batches import DISK, WIRE, arena, batch, record  # noqa: E402
from test_gpu_parity import assert_same  # noqa: E402

import oracle.oracle as orc  # noqa: E402

N_BATCHES = 4400
# total batch lengths around the 8 -> 9 and 16 -> 17 row boundaries: the CRC
# region [21, n) is cut into 1 KiB rows, 8 rows to a chunk
EXACT = (8212, 8213, 8214, 16404, 16405, 16406)


def sized(fmt, total):
    """A single-record batch of exactly `total` bytes."""
    for klen in (2, 3, 4):
        for vlen in range(max(total - 90, 0), total):
            b = batch([record(b"k" * klen, b"v" * vlen, 0, 0)], fmt=fmt)
            if len(b) == total:
                return b
    raise AssertionError(total)


def kinds(fmt):
    """[(batch bytes, descriptor length)] of the eleven kinds."""
    out = [(sized(fmt, t), t) for t in EXACT]
    out.append((batch([], fmt=fmt), 61))
    out.append((sized(fmt, 70), 70))
    big = batch([record(b"key", b"x" * 70000, 0, 0)], fmt=fmt)
    out.append((big, len(big)))
    # two rejected kinds from edge_cases; bad magic / a bad header CRC / a short slot fail in
    # the header (no row of theirs is checksummed), the truncated wire body is checksummed first
    if fmt == WIRE:
        cases = {c[0]: c for c in edge_cases.wire_cases()}
        names = ("magic_1", "bl_larger")  # bad magic; batch_length past the descriptor (body truncated)
    else:
        cases = {c[0]: c for c in edge_cases.disk_cases()}
        names = ("disk_hdr_flip", "disk_body_short")  # the disk header has no magic: header CRC instead
    for nm in names:
        _, b, ln, _ = cases[nm]
        out.append((b, len(b) if ln is None else ln))
    assert len(out) == 11
    return out


@pytest.fixture(scope="module", params=[WIRE, DISK], ids=["wire", "disk"])
def handover(request):
    """(data, descs, oracle result) -- built and checked once per format."""
    fmt = request.param
    ks = kinds(fmt)
    assert [ln for _, ln in ks[:6]] == list(EXACT) and [len(b) for b, _ in ks[:6]] == list(EXACT)
    assert ks[6][1] == 61 and ks[7][1] == 70 and 70000 < ks[8][1] < 70200
    picks = [ks[i % 11] for i in range(N_BATCHES)]
    data, descs = arena([b for b, _ in picks], fmt=fmt, lengths=[ln for _, ln in picks])
    want = orc.validate_arena(data, descs)
    return data, descs, want


def test_arena_and_oracle_verdicts(handover):
    _, descs, want = handover
    assert len(descs) == N_BATCHES
    verdicts = want[0]["verdict"]
    assert len(set(verdicts.tolist())) >= 3
    # the nine well-formed kinds pass, the last two of each cycle do not
    per_kind = [set(verdicts[k::11].tolist()) for k in range(11)]
    assert all(s == {edge_cases.V_OK} for s in per_kind[:9])
    assert all(len(s) == 1 and edge_cases.V_OK not in s for s in per_kind[9:])


def check(eng, handover):
    data, descs, want = handover
    for _ in range(2):  # the second submission starts from the first one's device state
        got = eng.submit(data, descs)
        assert_same(*got, *want)


@pytest.mark.gpu
def test_handover_one_workgroup_per_cu(built, handover):
    from redpanda_amd import engine

    with engine.Engine(0, blocks_per_cu=1) as e:
        cu, grid = e.device_info()
        assert grid == cu  # 4 waves per CU: every wave takes four or five batches
        assert N_BATCHES > 4 * 4 * cu
        check(e, handover)


@pytest.mark.gpu
def test_handover_default_grid(eng, handover):
    cu, grid = eng.device_info()
    assert grid == 8 * cu  # eight workgroups per CU: validate_kernel fits eight waves per SIMD
    check(eng, handover)
