"""Aborted transactions ahead of compaction, without a GPU:

* hand cases: tests/tx_compaction.py's literal tx_reducer against flags and
  stats written out here, one named case per rule of the reference;
* the model against the closed form (a < c(r) <= i) on random segments;
* rpgpu_txfilter.h compiled for the host (tests/native/txfilter_host.cpp)
  against the model over the hand cases and the sweep, plain and under
  -fsanitize=address,undefined as a stand-alone program;
* keep_tx against the untouched oracle on well-formed segments, and the
  duplicate-offset case against the model;
* struct layouts and enum values of include/rpgpu.h against redpanda_amd/abi.py,
  the exported symbols, and the compiler's resource remarks for the kernels."""
import functools
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import tx_compaction as tx  # noqa: E402
from kafka_batches import DISK, WIRE  # noqa: E402

import oracle.oracle as orc  # noqa: E402
from redpanda_amd import abi  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "redpanda_amd" / "csrc"
PLAIN = ["-O2"]
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
OK, NONE = abi.TX_OK, tx.NONE
P, Q = 7, 8  # two producers


# ---------------------------------------------------------------- hand cases
# name -> builder(fmt) returning (Call, expected flags per batch, expected stats rows, index cut or None)
# stats row: (tx data, tx control, non-tx control, all discarded, aborted txs, all batches, processed, status, bad batch)
HAND = {}


def hand(fn):
    HAND[fn.__name__] = fn
    return fn


@hand
def range_first_below_scope(fmt):
    """first below every offset: consumed at batch 0."""
    c = tx.Call(fmt)
    c.range(P, 0, 50, 101)
    c.data(100, P, 0), c.data(101, P, 0), c.marker(102, P, 0, 0), c.data(103, P, 0)
    c.end_scope()
    return c, [1, 1, 2, 0], [(2, 1, 0, 3, 1, 4, 4, OK, NONE)], None


@hand
def range_first_beyond_every_offset(fmt):
    """never consumed, still counted."""
    c = tx.Call(fmt)
    c.range(P, 0, 1000, 2000)
    c.data(100, P, 0), c.data(101, P, 0)
    c.end_scope()
    return c, [0, 0], [(0, 0, 0, 0, 1, 2, 2, OK, NONE)], None


@hand
def abort_marker_at_consume_position(fmt):
    """the range is consumed in front of the marker's own batch, which erases it."""
    c = tx.Call(fmt)
    c.range(P, 0, 101, 101)
    c.data(100, P, 0), c.marker(101, P, 0, 0), c.data(102, P, 0)
    c.end_scope()
    return c, [0, 2, 0], [(0, 1, 0, 1, 1, 3, 3, OK, NONE)], None


@hand
def abort_marker_without_range(fmt):
    c = tx.Call(fmt)
    c.marker(100, P, 0, 0), c.data(101, P, 0)
    c.end_scope()
    return c, [2, 0], [(0, 1, 0, 1, 0, 2, 2, OK, NONE)], None


@hand
def commit_marker_between_aborted_data(fmt):
    """a commit erases nothing."""
    c = tx.Call(fmt)
    c.range(P, 0, 100, 103)
    c.data(100, P, 0), c.marker(101, P, 0, 1), c.data(102, P, 0), c.marker(103, P, 0, 0)
    c.end_scope()
    return c, [1, 2, 1, 2], [(2, 2, 0, 4, 1, 4, 4, OK, NONE)], None


@hand
def data_after_abort_kept_then_rearmed(fmt):
    c = tx.Call(fmt)
    c.range(P, 0, 100, 101), c.range(P, 0, 104, 105)
    c.data(100, P, 0), c.marker(101, P, 0, 0), c.data(102, P, 0), c.data(103, P, 0), c.data(104, P, 0)
    c.marker(105, P, 0, 0), c.data(106, P, 0)
    c.end_scope()
    return c, [1, 2, 0, 0, 1, 2, 0], [(2, 2, 0, 4, 2, 7, 7, OK, NONE)], None


@hand
def two_overlapping_ranges_of_one_pid(fmt):
    """both sit in the map under one key: one abort marker erases the pid."""
    c = tx.Call(fmt)
    c.range(P, 0, 100, 110), c.range(P, 0, 101, 105)
    c.data(100, P, 0), c.data(101, P, 0), c.marker(102, P, 0, 0), c.data(103, P, 0)
    c.end_scope()
    return c, [1, 1, 2, 0], [(2, 1, 0, 3, 2, 4, 4, OK, NONE)], None


@hand
def same_producer_id_two_epochs(fmt):
    c = tx.Call(fmt)
    c.range(P, 0, 100, 103)
    c.data(100, P, 0), c.data(101, P, 1), c.marker(102, P, 1, 0), c.data(103, P, 0)
    c.end_scope()
    return c, [1, 0, 2, 1], [(2, 1, 0, 3, 1, 4, 4, OK, NONE)], None


@hand
def same_pid_in_two_scopes(fmt):
    c = tx.Call(fmt)
    c.range(P, 0, 100, 100)
    c.data(100, P, 0)
    c.end_scope()
    c.data(200, P, 0)
    c.end_scope()
    return c, [1, 0], [(1, 0, 0, 1, 1, 1, 1, OK, NONE), (0, 0, 0, 0, 0, 1, 1, OK, NONE)], None


@hand
def non_monotone_last_offsets(fmt):
    """batch 0 ends at 110: the range with first 105 is consumed there, and batch 1 (last offset 101) reads it."""
    c = tx.Call(fmt)
    c.range(P, 0, 105, 120)
    c.data(100, tx=False, lod=10), c.data(101, P, 0)
    c.end_scope()
    return c, [0, 1], [(1, 0, 0, 1, 1, 2, 2, OK, NONE)], None


@hand
def control_type_2_kept(fmt):
    c = tx.Call(fmt)
    c.marker(100, P, 0, 2)
    c.end_scope()
    return c, [0], [(0, 0, 0, 0, 0, 1, 1, OK, NONE)], None


@hand
def fence_kept_prepare_dropped(fmt):
    """disk: batch types 10 and 9.  A wire batch has no type (raft_data): both are delegated."""
    c = tx.Call(fmt)
    c.control(100, tx.TX_FENCE, P, 0), c.control(101, tx.TX_PREPARE, P, 0)
    c.end_scope()
    if fmt == WIRE:
        return c, [0, 0], [(0, 0, 0, 0, 0, 2, 2, OK, NONE)], None
    return c, [0, 3], [(0, 0, 1, 1, 0, 2, 2, OK, NONE)], None


@hand
def transactional_batch_of_another_type(fmt):
    """disk: type 5 under an ongoing aborted range is kept (wire: it is raft_data, and discarded)."""
    c = tx.Call(fmt)
    c.range(P, 0, 100, 101)
    c.data(100, P, 0, btype=5)
    c.end_scope()
    if fmt == WIRE:
        return c, [1], [(1, 0, 0, 1, 1, 1, 1, OK, NONE)], None
    return c, [0], [(0, 0, 0, 0, 1, 1, 1, OK, NONE)], None


@hand
def non_transactional(fmt):
    c = tx.Call(fmt)
    c.range(P, 0, 100, 101)
    c.data(100, P, 0), c.marker(101, P, 0, 0)
    c.end_scope(flags=abi.TX_NON_TRANSACTIONAL)
    return c, [0, 0], [(0, 0, 0, 0, 1, 0, 2, OK, NONE)], None


def shared_rows(fmt, flags):
    c = tx.Call(fmt)
    c.range(P, 0, 100, 101), c.range(Q, 0, 200, 201)
    c.data(100, P, 0), c.data(101, Q, 0)
    c.end_scope(range_first=0, range_count=2, flags=flags, frm=100, to=101)
    c.data(200, P, 0), c.data(201, Q, 0)
    c.end_scope(range_first=0, range_count=2, flags=flags, frm=200, to=201)
    return c


@hand
def range_filter_on_shared_rows(fmt):
    return (shared_rows(fmt, abi.TX_FILTER_RANGES), [1, 0, 0, 1],
            [(1, 0, 0, 1, 1, 2, 2, OK, NONE), (1, 0, 0, 1, 1, 2, 2, OK, NONE)], None)


@hand
def range_filter_off_shared_rows(fmt):
    """scope 1 consumes the range that began in scope 0 at its first batch."""
    return (shared_rows(fmt, 0), [1, 0, 1, 1],
            [(1, 0, 0, 1, 2, 2, 2, OK, NONE), (2, 0, 0, 2, 2, 2, 2, OK, NONE)], None)


def stopping(fmt, offender, status):
    """aborted data, the offender, data behind it."""
    c = tx.Call(fmt)
    c.range(P, 0, 100, 110)
    c.data(100, P, 0)
    offender(c)
    c.data(102, P, 0)
    c.end_scope()
    return c, [1, 4, 4], [(1, 0, 0, 1, 1, 1, 1, status, 1)], None


@hand
def stop_bad_batch(fmt):
    def corrupt(c):
        c.data(101, P, 0)
        c.batches[-1] = c.batches[-1][:-1] + bytes([c.batches[-1][-1] ^ 0x5A])
    return stopping(fmt, corrupt, abi.TX_BAD_BATCH)


@hand
def stop_assert_two_records(fmt):
    return stopping(fmt, lambda c: c.marker(101, P, 0, 0, nrec=2), abi.TX_ASSERT)


@hand
def stop_assert_version(fmt):
    return stopping(fmt, lambda c: c.marker(101, P, 0, 0, version=1), abi.TX_ASSERT)


@hand
def stop_assert_version_in_two_byte_key(fmt):
    return stopping(fmt, lambda c: c.marker(101, P, 0, 0, key=b"\0\1"), abi.TX_ASSERT)


@hand
def stop_assert_control_batch_type(fmt):
    """disk: a transactional control batch that is not raft_data (wire: it is, an abort marker)."""
    c, flags, stats, cut = stopping(fmt, lambda c: c.marker(101, P, 0, 0, btype=5), abi.TX_ASSERT)
    if fmt == WIRE:
        return c, [1, 2, 0], [(1, 1, 0, 2, 1, 3, 3, OK, NONE)], None
    return c, flags, stats, cut


@hand
def stop_assert_non_tx_control_type(fmt):
    c, flags, stats, cut = stopping(fmt, lambda c: c.control(101, 5), abi.TX_ASSERT)
    if fmt == WIRE:
        return c, [1, 0, 1], [(2, 0, 0, 2, 1, 3, 3, OK, NONE)], None
    return c, flags, stats, cut


@hand
def stop_key_empty(fmt):
    return stopping(fmt, lambda c: c.marker(101, P, 0, 0, key=b""), abi.TX_KEY_SHORT_THROW)


@hand
def stop_key_null(fmt):
    return stopping(fmt, lambda c: c.marker(101, P, 0, 0, key=None), abi.TX_KEY_SHORT_THROW)


@hand
def stop_key_three_bytes(fmt):
    return stopping(fmt, lambda c: c.marker(101, P, 0, 0, key=b"\0\0\0"), abi.TX_KEY_SHORT_THROW)


@hand
def stop_not_indexed(fmt):
    """the index ends in front of the control batch's entry."""
    c = tx.Call(fmt)
    c.range(P, 0, 100, 110)
    c.data(100, P, 0), c.marker(101, P, 0, 0)
    c.end_scope()
    return c, [1, 4], [(1, 0, 0, 1, 1, 1, 1, abi.TX_NOT_INDEXED, 1)], 1


@hand
def stop_bad_scope(fmt):
    """batches past n, range rows past nranges: nothing written; the scope between them is untouched by it."""
    c = tx.Call(fmt)
    c.range(P, 0, 100, 110)
    c.data(100, P, 0), c.data(101, P, 0)
    c.scopes.append((1, 2, 0, 1, 0, 0, 0, 0))
    c.scopes.append((0, 1, 0, 1, 0, 0, 0, 0))
    c.scopes.append((1, 1, 1, 1, 0, 0, 0, 0))
    bad = (0, 0, 0, 0, 0, 0, 0, abi.TX_BAD_SCOPE, NONE)
    return c, [1, 4], [bad, (1, 0, 0, 1, 1, 1, 1, OK, NONE), bad], None


STAT_FIELDS = ("tx_data_batches_discarded", "tx_control_batches_discarded", "non_tx_control_batches_discarded",
               "all_batches_discarded", "num_aborted_txes", "all_batches", "processed", "status", "bad_batch")


@functools.lru_cache(maxsize=None)
def hand_case(name, fmt):
    """(built call, expected discard, expected stats): built once, left unchanged."""
    c, flags, rows, cut = HAND[name](fmt)
    a = c.build()
    if cut is not None:
        a["idx"] = a["idx"][:cut]
    stats = np.zeros(len(rows), abi.TX_STATS_DTYPE)
    for s, row in enumerate(rows):
        for f, v in zip(STAT_FIELDS, row):
            stats[s][f] = v
    return a, np.array(flags, np.uint8), stats


def args(a):
    return a["data"], a["descs"], a["res"], a["idx"], a["scopes"], a["ranges"]


def same(got, want, what=""):
    gd, gs = got
    wd, ws = want
    assert np.array_equal(gd, wd), f"{what} discard: got {gd.tolist()[:64]} want {wd.tolist()[:64]}"
    for f in ws.dtype.names:
        bad = np.nonzero(gs[f] != ws[f])[0]
        assert bad.size == 0, f"{what} stats.{f} differs at scopes {bad[:8]}: got {gs[f][bad[:8]]} want {ws[f][bad[:8]]}"


FMTS = [DISK, WIRE]
FMT_IDS = ["disk", "wire"]


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
@pytest.mark.parametrize("name", list(HAND))
def test_hand_case(name, fmt):
    a, flags, stats = hand_case(name, fmt)
    same(tx.model(*args(a)), (flags, stats), name)
    same(tx.model(*args(a), one=tx.closed_form), (flags, stats), name + " (closed form)")


def test_hand_cases_cover_every_status_and_flag():
    seen_status, seen_flags = set(), set()
    for name in HAND:
        _, flags, stats = hand_case(name, DISK)
        seen_status |= set(stats["status"].tolist())
        seen_flags |= set(flags.tolist())
    assert seen_status == set(range(6)) and seen_flags == set(range(5))


# ------------------------------------------------------- model vs closed form
@functools.lru_cache(maxsize=None)
def sweep_call(name, fmt):
    shape = tx.sweep_shapes()[name]
    seed = 1000 + sorted(tx.sweep_shapes()).index(name) * 2 + fmt
    a = tx.random_call(fmt, seed, shape).build()
    a["want"] = tx.model(*args(a))
    return a


SWEEP = list(tx.sweep_shapes())


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_model_equals_closed_form_on_random_segments(fmt):
    total = 0
    for name in SWEEP:
        a = sweep_call(name, fmt)
        same(tx.model(*args(a), one=tx.closed_form), a["want"], name)
        total += int((a["want"][0] == abi.TX_ABORTED_DATA).sum())
    assert total > 100, "the random segments abort something"


def test_sweep_covers_its_classes():
    shapes = tx.sweep_shapes()
    sizes = {nb for sh in shapes.values() for nb, _ in sh}
    counts = {nr for sh in shapes.values() for _, nr in sh}
    assert sizes >= set(tx.SIZES) and counts >= set(tx.RANGE_COUNTS)
    assert {len(sh) for sh in shapes.values()} == {1, 5, 70}
    a = sweep_call("seventy", DISK)
    assert len(a["descs"]) > 1024, "the sort has a second block"
    assert len(a["data"]) <= 256 << 10
    kinds = a["res"]["attrs"] & tx.ATTR_TX
    prods = {(int(p), tx.pid_of(a["data"], d)) for p, d, k in zip(a["descs"]["partition"], a["descs"], kinds) if k}
    assert len(prods) > 256 and tx.table_cap(len(a["descs"])) > 256, "the sort has a second digit pass"


def test_collision_call_collides():
    c, pids = tx.collision_call(DISK)
    cap = tx.table_cap(len(c.batches))
    assert len({tx.pid_hash(0, p, 0) & (cap - 1) for p in pids}) == 1 and len(set(pids)) == 4
    a = c.build()
    seen = {tx.pid_of(a["data"], d)[0] for d, r in zip(a["descs"], a["res"]) if r["attrs"] & tx.ATTR_TX}
    assert seen == set(pids), "every colliding producer has a batch in the scope"


# --------------------------------------------------------------- host program
def build_host(out: Path, flags) -> Path:
    subprocess.run(["g++", *flags, "-std=c++17", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "txfilter_host.cpp"), "-o", str(out)],
                   check=True, capture_output=True, text=True)
    return out


@pytest.fixture(scope="module")
def hosts(tmp_path_factory):
    d = tmp_path_factory.mktemp("txfilter_host")
    return {False: build_host(d / "txfilter_host", PLAIN), True: build_host(d / "txfilter_host_san", SANITIZE)}


def run_host(exe: Path, a, work: Path):
    inp, out = work / "in.bin", work / "out.bin"
    n, ns = len(a["descs"]), len(a["scopes"])
    data = np.ascontiguousarray(a["data"], np.uint8)
    with open(inp, "wb") as f:
        f.write(np.array([len(data), n, len(a["idx"]), ns, len(a["ranges"])], "<u8").tobytes())
        for arr, dt in ((data, np.uint8), (a["descs"], abi.DESC_DTYPE), (a["res"], abi.RESULT_DTYPE),
                        (a["idx"], abi.INDEX_DTYPE), (a["scopes"], abi.TX_SCOPE_DTYPE),
                        (a["ranges"], abi.TX_RANGE_DTYPE)):
            f.write(np.ascontiguousarray(arr, dt).tobytes())
    r = subprocess.run([str(exe), str(inp), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, f"exit {r.returncode}: {r.stderr[-1500:]}"
    raw = np.fromfile(out, np.uint8)
    return raw[:n].copy(), raw[n:].copy().view(abi.TX_STATS_DTYPE)


@pytest.mark.parametrize("sanitized", [False, True], ids=["plain", "asan-ubsan"])
def test_host_core_equals_model(hosts, sanitized, tmp_path):
    """Every hand case, the collision call and the sweep, both formats."""
    for fmt in FMTS:
        for name in HAND:
            a, flags, stats = hand_case(name, fmt)
            same(run_host(hosts[sanitized], a, tmp_path), (flags, stats), name)
        a = tx.collision_call(fmt)[0].build()
        same(run_host(hosts[sanitized], a, tmp_path), tx.model(*args(a)), "collision")
        for name in SWEEP:
            a = sweep_call(name, fmt)
            same(run_host(hosts[sanitized], a, tmp_path), a["want"], name)


# ------------------------------------------------------------------- keep_tx
def without(a, discard):
    """The arena with the flagged batches removed (their index entries stay where they are)."""
    sel = ~((discard >= 1) & (discard <= 3))
    return a["descs"][sel], a["res"][sel], sel


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_keep_tx_equals_the_oracle_without_the_flagged_batches(fmt):
    for name in ("five-a", "five-b", "one-200b"):
        a = sweep_call(name, fmt)
        discard = a["want"][0]
        assert ((discard >= 1) & (discard <= 3)).any()
        keep, nkeys = tx.keep_tx(a["data"], a["descs"], a["res"], a["idx"], discard)
        descs, res, sel = without(a, discard)
        wkeep, wkeys = orc.compaction_keep(a["data"], descs, res, a["idx"])
        assert nkeys == wkeys
        for b in range(len(a["descs"])):
            lo, cnt = int(a["res"]["index_first"][b]), int(a["res"]["index_count"][b])
            if sel[b]:
                assert np.array_equal(keep[lo:lo + cnt], wkeep[lo:lo + cnt]), (name, b)
            else:  # well-formed: no kept record shares a flagged batch's offsets
                assert (keep[lo:lo + cnt] == 0).all() and (wkeep[lo:lo + cnt] == 2).all(), (name, b)
        # and with no flags at all keep_tx is compaction_keep
        k0, n0 = tx.keep_tx(a["data"], a["descs"], a["res"], a["idx"], None)
        o0, on0 = orc.compaction_keep(a["data"], a["descs"], a["res"], a["idx"])
        assert np.array_equal(k0, o0) and n0 == on0


@functools.lru_cache(maxsize=None)
def duplicate_offset_call(fmt):
    """An aborted batch whose record shares offset 100 with a committed record of
    another key: should_keep looks at the offset alone, so the aborted record is
    kept; the aborted record at 101 shares nothing and is dropped.  The aborted
    key's older committed value at 90 is not superseded by aborted data."""
    c = tx.Call(fmt)
    c.range(P, 0, 100, 102)
    c.data(90, Q, 0, key=b"x")                       # committed, key x
    c.data(100, Q, 0, key=b"y")                      # committed, key y, offset 100
    c.data(100, P, 0, key=b"x")                      # aborted, key x, the hostile duplicate of offset 100
    c.data(101, P, 0, key=b"x")                      # aborted, key x
    c.marker(102, P, 0, 0)
    c.end_scope()
    return c.build()


@pytest.mark.parametrize("fmt", FMTS, ids=FMT_IDS)
def test_duplicate_offset_is_kept_as_the_reference_keeps_it(fmt):
    a = duplicate_offset_call(fmt)
    discard, _ = tx.model(*args(a))
    assert discard.tolist() == [0, 0, 1, 1, 2]
    keep, nkeys = tx.keep_tx(a["data"], a["descs"], a["res"], a["idx"], discard)
    first = a["res"]["index_first"]
    assert [int(keep[int(f)]) for f in first] == [1, 1, 1, 0, 0] and nkeys == 2
    k0, _ = tx.keep_tx(a["data"], a["descs"], a["res"], a["idx"], None)
    assert [int(k0[int(f)]) for f in first[:4]] == [0, 1, 1, 1], "unfiltered, the aborted x supersedes the committed one"


# ------------------------------------------------------------ ABI and resources
ABI_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "rpgpu.h"
_Static_assert(RPGPU_ABI_VERSION == 6, "the tx filter is additive");
#define OFF(T, F) printf("%s.%s %zu\n", #T, #F, offsetof(rpgpu_tx_##T, F))
int main(void) {
    printf("%zu %zu %zu\n", sizeof(rpgpu_tx_range), sizeof(rpgpu_tx_scope), sizeof(rpgpu_tx_stats));
    printf("%u %u\n", RPGPU_TX_NON_TRANSACTIONAL, RPGPU_TX_FILTER_RANGES);
    printf("%d %d %d %d %d\n", RPGPU_TX_DELEGATED, RPGPU_TX_ABORTED_DATA, RPGPU_TX_MARKER, RPGPU_TX_PREPARE,
           RPGPU_TX_NOT_REACHED);
    printf("%d %d %d %d %d %d\n", RPGPU_TX_OK, RPGPU_TX_BAD_BATCH, RPGPU_TX_ASSERT, RPGPU_TX_KEY_SHORT_THROW,
           RPGPU_TX_NOT_INDEXED, RPGPU_TX_BAD_SCOPE);
    OFF(range, producer_id); OFF(range, producer_epoch); OFF(range, first); OFF(range, last);
    OFF(scope, first_batch); OFF(scope, batch_count); OFF(scope, range_first); OFF(scope, range_count);
    OFF(scope, from); OFF(scope, to); OFF(scope, flags);
    OFF(stats, tx_data_batches_discarded); OFF(stats, tx_control_batches_discarded);
    OFF(stats, non_tx_control_batches_discarded); OFF(stats, all_batches_discarded); OFF(stats, num_aborted_txes);
    OFF(stats, all_batches); OFF(stats, processed); OFF(stats, status); OFF(stats, bad_batch);
    return 0;
}
"""
NEW_SYMBOLS = {"rpgpu_compaction_tx_scratch_bytes", "rpgpu_compaction_tx_filter_device",
               "rpgpu_compaction_keep_tx_device"}


def test_header_layouts_match_abi_py(tmp_path):
    (tmp_path / "a.c").write_text(ABI_C)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(tmp_path / "a.c"),
                    "-o", str(tmp_path / "a")], check=True, capture_output=True, text=True)
    lines = subprocess.run([str(tmp_path / "a")], capture_output=True, text=True, check=True).stdout.splitlines()
    dtypes = dict(range=abi.TX_RANGE_DTYPE, scope=abi.TX_SCOPE_DTYPE, stats=abi.TX_STATS_DTYPE)
    assert lines[0].split() == [str(d.itemsize) for d in dtypes.values()]
    assert lines[1].split() == [str(abi.TX_NON_TRANSACTIONAL), str(abi.TX_FILTER_RANGES)]
    assert lines[2].split() == [str(v) for v in (abi.TX_DELEGATED, abi.TX_ABORTED_DATA, abi.TX_MARKER, abi.TX_PREPARE,
                                                 abi.TX_NOT_REACHED)] == [str(v) for v in range(5)]
    assert lines[3].split() == [str(v) for v in (abi.TX_OK, abi.TX_BAD_BATCH, abi.TX_ASSERT, abi.TX_KEY_SHORT_THROW,
                                                 abi.TX_NOT_INDEXED, abi.TX_BAD_SCOPE)]
    for line in lines[4:]:
        name, off = line.split()
        row, fld = name.split(".")
        assert dtypes[row].fields[fld][1] == int(off), name


def test_new_symbols_are_exported(built):
    from redpanda_amd import _build

    out = subprocess.run(["nm", "-D", "--defined-only", str(_build.LIBRPGPU)], capture_output=True, text=True,
                         check=True).stdout
    have = {l.split()[-1] for l in out.splitlines()}
    assert NEW_SYMBOLS <= have and NEW_SYMBOLS <= set(abi.EXPORTED)
    f = abi.lib().rpgpu_compaction_tx_scratch_bytes
    assert f(1000, 0) == f(1000, 1 << 20), "the scratch does not grow with the ranges"
    assert f(1 << 20, 0) < 100 << 20 and f(0, 0) > 0


KERNELS = ["classify", "insert", "groups", "ranges", "decide"]


def test_kernels_use_no_scratch_and_spill_nothing(tmp_path):
    """The compiler's own resource remarks for rpgpu_txfilter.hip and the sort it shares with the append."""
    from redpanda_amd import _build

    r = subprocess.run(["hipcc", *_build.rpgpu_flags(), "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        "-c", str(_build.CSRC / "rpgpu_txfilter.hip"), "-o", str(tmp_path / "tx.o")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels, cur = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"remark: \s*([A-Za-z][A-Za-z /\[\]]*?):\s*(\S+)", line)
        if m and m.group(1).strip() == "Function Name":
            cur = kernels.setdefault(m.group(2), {})
        elif m and cur is not None and m.group(2).isdigit():
            cur[m.group(1).strip()] = int(m.group(2))
    assert all(any(f"tx_{n}_kernel" in k for k in kernels) for n in KERNELS)
    assert all(any(f"radix_{n}_kernel" in k for k in kernels) for n in ("hist", "scan", "scatter"))
    assert len(kernels) == len(KERNELS) + 3
    for k, u in kernels.items():
        assert u["ScratchSize [bytes/lane]"] == 0 and u["VGPRs Spill"] == 0 and u["SGPRs Spill"] == 0, (k, u)
        assert u["AGPRs"] == 0 and u["VGPRs"] <= 64, (k, u)
