"""CPU side of the read-path geometry sweeps (tests/read_path_geometry.py): the
oracle (oracle/parse.c, fetch.c, index.c) against restatements that share no
code with it, and the coverage the families promise -- every outcome, both
sides of every comparison, every cell of the serializer's grid -- read off the
oracle's results.  tests/test_gpu_read_path_geometry.py runs the same cases on
the device."""
import functools
import os
import re
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import read_path_geometry as g  # noqa: E402

import oracle.oracle as orc  # noqa: E402
from redpanda_amd import abi  # noqa: E402

PARSER_FAMILIES = {"A": ("seg", g.family_a), "B.seg": ("seg", lambda: g.family_b("seg")),
                   "B.remote": ("remote", lambda: g.family_b("remote")), "E": ("remote", g.family_e),
                   "D.seg": ("seg", lambda: g.family_d_host("seg") + (None,)),
                   "D.remote": ("remote", lambda: g.family_d_host("remote") + (None,)),
                   "C.seg": ("seg", lambda: g.family_c_parse("seg", 130)),
                   "C.remote": ("remote", lambda: g.family_c_parse("remote", 130))}


@functools.lru_cache(None)
def oracle_of(fam):
    kind, build = PARSER_FAMILIES[fam]
    data, reads, names, tags = build()
    out = orc.segment_parse(data, reads) if kind == "seg" else orc.remote_segment_parse(data, reads)
    return kind, data, reads, names, tags, out


@functools.lru_cache(None)
def restated(fam):
    """The restatement's outputs laid out as the oracle's arrays; raises
    OverflowError if a case leaves int64 (the no-overflow precondition)."""
    kind, data, reads, names, _, out = oracle_of(fam)
    res = np.zeros_like(out[0])
    descs = np.zeros_like(out[1])
    kb = np.zeros(len(descs), dtype=np.int64)
    gaps = np.zeros_like(out[3]) if kind == "remote" else None
    for i, rd in enumerate(reads):
        if kind == "seg":
            r, ds = g.py_segment_parse(data, rd)
        else:
            r, ds, gs = g.py_remote_parse(data, rd)
            for slot, base, last in gs:
                gaps[slot] = (base, last)
        for f, v in r.items():
            res[f][i] = v
        for d in ds:
            descs[d[0]] = (d[1], d[2], int(rd["partition"]), g.DISK, int(rd["ops"]), 0, 0)
            if kind == "remote":
                kb[d[0]] = d[3]
    return res, descs, kb, gaps


@pytest.mark.parametrize("fam", list(PARSER_FAMILIES))
def test_cases_stay_inside_int64(fam):
    """base_offset + lod, last + 1, base_offset - delta, last - delta + 1 and
    delta + lod + 1 of every header a case reaches fit int64 (the oracle is
    built without -fwrapv): _i64 in the restatement refuses anything else."""
    restated(fam)


@pytest.mark.parametrize("fam", list(PARSER_FAMILIES))
def test_restatement_agrees_with_oracle(fam):
    kind, data, reads, names, _, out = oracle_of(fam)
    res, descs, kb, gaps = restated(fam)
    assert set(res.dtype.names) == set(out[0].dtype.names)
    g.assert_struct_equal(fam + " results", names, res, out[0])
    g.assert_struct_equal(fam + " descs", g.slot_owner(reads, names, len(descs)), descs, out[1])
    if kind == "remote":
        owner = g.slot_owner(reads, names, len(kb))
        i = g.first_diff(kb, out[2])
        assert i is None, f"{fam}: {owner[i]}: kafka_base differs at slot {i}: {kb[i]} / {out[2][i]}"
        i = g.first_diff(gaps, out[3])
        assert i is None, f"{fam}: gaps differ at {i}"


def outcomes(*fams):
    got = set()
    for fam in fams:
        res = oracle_of(fam)[5][0]
        got |= set(zip(res["status"].tolist(), res["last_error"].tolist()))
    return got


def test_every_outcome_occurs():
    assert outcomes("A", "B.seg") == g.SEG_OUTCOMES
    assert outcomes("B.remote", "E") == g.REMOTE_OUTCOMES


DECISION = ("status", "last_error", "accepted", "skipped", "bytes_consumed", "over_budget", "stopped")


@pytest.mark.parametrize("fam,comparisons", [("A", g.SEG_COMPARISONS), ("E", g.REMOTE_COMPARISONS)])
def test_both_sides_of_every_comparison(fam, comparisons):
    """For each comparison there are reads with the configuration value at the
    header-derived value and one off it whose outcomes differ: `>` for `>=`
    (or the reverse) in the kernel changes one of them."""
    _, _, _, names, tags, out = oracle_of(fam)
    seen = {}
    for i, t in enumerate(tags):
        if t is not None:
            seen.setdefault(t[0], {}).setdefault(re.sub(r"[+-]\d+$", "", names[i]), {})[t[1]] = \
                tuple(int(out[0][f][i]) for f in DECISION)
    assert sorted(seen) == sorted(comparisons)
    for cmp_name in comparisons:
        witnesses = [grp for grp in seen[cmp_name].values()
                     if 0 in grp and any(s in grp and grp[s] != grp[0] for s in (-1, 1))]
        assert witnesses, f"{cmp_name}: no pair of reads across the equality differs: {seen[cmp_name]}"


def test_d_recovers_three_batches_past_2gib():
    _, _, reads, _, _, (res, descs) = oracle_of("D.seg")
    assert (res["status"][0], res["last_error"][0], res["accepted"][0]) == (abi.V_OK, abi.V_END_OF_STREAM, 3)
    assert list(descs["offset"][:3]) == list(g.D_POS) and res["bytes_consumed"][0] == g.D_LENGTH
    assert (res["accepted"][1], res["skipped"][1]) == (2, 1) and list(descs["offset"][8:10]) == list(g.D_POS[1:])
    _, _, _, _, _, (res, descs, kb, gaps) = oracle_of("D.remote")
    assert list(res["accepted"]) == [2, 1] and list(res["skipped"]) == [1, 2] and list(res["gaps"]) == [1, 1]
    assert list(descs["offset"][:2]) == list(g.D_POS[1:]) and descs["offset"][8] == g.D_POS[2]
    assert all(p + 64 > 0x7ffffff0 for p in g.D_POS[2:]) and max(g.D_POS) < 2**32


# ---- F ----------------------------------------------------------------------------------------
def test_f_grid_and_wire_headers():
    data, descs, terms, pairs, extras = g.family_f()
    assert set(pairs) >= {(m, b) for m in range(16) for b in g.F_BODIES}
    for k, (m, b) in enumerate(pairs):
        assert int(descs["offset"][k]) % 16 == m and int(descs["length"][k]) == g.HDR + b
    ends = descs["offset"][:-1] + descs["length"][:-1]
    gaps = (descs["offset"][1:] - ends)[:len(pairs) - 1]
    assert gaps.min() >= 1 and gaps.max() <= 15
    out, _ = orc.kafka_serialize(data, descs, terms)
    used = np.zeros(data.size, dtype=bool)
    for k, d in enumerate(descs):
        o = int(d["offset"])
        size = struct.unpack_from("<i", data, o + 4)[0]
        used[o:o + size] = True
        h = data[o:o + g.HDR].tobytes()
        assert out[o:o + g.HDR].tobytes() == g.wire_header(h, int(terms[k])), k
        assert np.array_equal(out[o + g.HDR:o + size], data[o + g.HDR:o + size]), k
    assert not out[~used].any() and (data[~used][:-64] == g.FILL).all()
    k = extras["distinct header"]
    h = data[int(descs["offset"][k]):][:g.HDR]
    assert len(set(h.tolist())) == g.HDR


# ---- G ----------------------------------------------------------------------------------------
def test_g_oracle_summaries_and_coverage():
    data, descs, ranges, names = g.family_g()
    _, sums = orc.kafka_serialize(data, descs, None, ranges)
    n = len(descs)
    retaken, tx_at = [], set()
    for k, (rg, name) in enumerate(zip(ranges, names)):
        want = g.python_summary_skipping(data, descs, n, int(rg["first"]), int(rg["count"]))
        if not want["has_first_tx"]:
            want["first_tx_batch_offset"] = int(sums["first_tx_batch_offset"][k])  # unset: whatever the oracle leaves
        got = {f: int(sums[f][k]) for f in want}
        assert got == want, name
        # coverage, from the headers: where the running count is back at 0 after being non-zero
        count, seen_nonzero = 0, False
        lo, hi = min(int(rg["first"]), n), min(int(rg["first"]) + int(rg["count"]), n)
        for b in range(lo, hi):
            o = int(descs["offset"][b])
            size, base = struct.unpack_from("<iq", data, o + 4)
            ok = descs["length"][b] >= g.HDR and g.HDR <= size <= descs["length"][b]
            if not ok:
                continue
            if count == 0 and seen_nonzero and got["base_offset"] == base:
                retaken.append((name, b - lo))
            rc = struct.unpack_from("<I", data, o + 57)[0]
            count = (count + rc) & 0xFFFFFFFF
            seen_nonzero |= count != 0
            if got["has_first_tx"] and got["first_tx_batch_offset"] == base and \
                    struct.unpack_from("<h", data, o + 21)[0] & 0x10:
                tx_at.add((b - lo, hi - lo))
    assert {lane for _, lane in retaken} >= {2, 63, 64, 65}, retaken
    assert {p for p, _ in tx_at} >= {0, 63, 64} and any(p == c - 1 for p, c in tx_at), tx_at
    assert sums["status"].max() >= 2 and (sums["record_count"] == 0).any()


# ---- H ----------------------------------------------------------------------------------------
def h_oracle(nsegs=None):
    data, descs, segs, names = g.family_h(nsegs)
    res, _, _ = orc.validate_arena(data, descs)
    st, e = orc.segment_index(descs, res, segs)
    return descs, res, segs, names, st, e


def test_h_reaches_every_clamp():
    descs, res, segs, names, st, e = h_oracle()
    seen = {}
    for s, name in enumerate(names):
        f, c = int(segs["first_batch"][s]), int(st["entries"][s])
        if "/acc entry" in name and c == 2:
            seen.setdefault(("acc", int(segs["with_offset"][s])), set()).add(int(e["relative_time"][f + 1]))
        if "/e[0] rewrite" in name and c >= 1:
            seen.setdefault(("e0", int(segs["with_offset"][s])), set()).add(int(e["relative_time"][f]))
    for how in ("acc", "e0"):
        for wo in (0, 1):
            assert {0, 2**32 - 1} <= seen[(how, wo)], (how, wo, seen[(how, wo)])
            # one inside the range on each side of a clamp, so that the clamp value itself is pinned
            assert {1 << 31, (1 << 31) - 1} & seen[(how, wo)], (how, wo)
    by = dict(zip(names, range(len(names))))
    assert st["entries"][by["acc = step"]] == 3 and st["entries"][by["acc = step - 1"]] == 2
    assert st["entries"][by["step = 0"]] == 4 and st["entries"][by["step = 2^32 - 1"]] == 1
    assert st["entries"][by["non-data types/internal_topic=1/step=0"]] == 6
    assert st["entries"][by["non-data types/internal_topic=0/step=0"]] == 3
    s = by["relative offset past 2^32/with_offset=0"]
    f = int(segs["first_batch"][s])
    assert list(e["relative_offset"][f:f + 4]) == [0, 2**32 - 1, 0, 7]
    assert st["tracked"][by["first batch bad"]] == 0 and st["tracked"][by["second batch bad"]] == 1
    assert st["status"][by["offset below base"]] == abi.V_INDEX_OFFSET_BELOW_BASE


@pytest.mark.parametrize("nsegs", [255, 256, 257])
def test_h_block_edge_segments(nsegs):
    descs, res, segs, names, st, e = h_oracle(nsegs)
    assert len(segs) == nsegs and st["entries"].sum() == len(descs) and st["entries"][nsegs - 1] == 1
