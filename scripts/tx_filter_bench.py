#!/usr/bin/env python
"""Times rpgpu_compaction_tx_filter_device on its own, and
rpgpu_compaction_keep_tx_device with the filter's flags beside the yardstick,
rpgpu_compaction_keep_device (the stage the filter precedes), on one arena.

The arena is C2-shaped: --gib of on-disk batches of --records x --value bytes
(16 KiB by default), validated and indexed on the device, then made
transactional where the filter and keep read it (the kernels under test read
the result rows, the index, the headers' producer identity and the control
records' keys; they do not check CRCs again): every batch gets a producer
(--producers per scope, in turn) and ascending offsets, the last batch of each
scope becomes a control batch (an abort marker for an aborted producer of the
scope, else a commit marker).  --scope-batches batches form a scope; --aborted of
the producers are aborted, each with one range over its scope.  All scopes name
the whole range list and set RPGPU_TX_FILTER_RANGES, as a caller with one
aborted list per partition would.

Seeded, reads nothing outside the tree, inputs resident in HBM, HIP events
around the calls, warmed, at least --min-ms of timed work per side, --rounds
alternating rounds.  Prints one JSON line: every round's times and each side's
run-to-run spread (max / min - 1)."""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--records", type=int, default=16)
    ap.add_argument("--value", type=int, default=995)
    ap.add_argument("--scope-batches", type=int, default=16)
    ap.add_argument("--producers", type=int, default=4, help="per scope")
    ap.add_argument("--aborted", type=float, default=0.01, help="share of the producers")
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x7AB0)
    a = ap.parse_args()

    import torch

    from redpanda_amd import abi, engine

    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream(dev).cuda_stream
    L = abi.lib()
    eng = engine.Engine(0)
    rng = np.random.default_rng(a.seed)

    def up(x):
        return torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to(dev)

    def ok(rc):
        assert rc == 0, eng.last_error()

    def timed(step, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    # ---- the arena, validated and indexed
    per = 61 + a.records * (16 + a.value + 12)
    sb = a.scope_batches
    nb = int(a.gib * (1 << 30)) // per // sb * sb
    ns = nb // sb
    spec = engine.make_spec(seed=a.seed, partitions=1, records_per_batch=a.records, key_len=16, value_len=a.value,
                            format=abi.FMT_RP_DISK, ops=abi.OPS_PRODUCE)
    data, descs = engine.build_arena(spec, nb)
    cap = nb * a.records
    d_data = torch.from_numpy(data).to(dev)
    d_descs = up(descs)
    d_res = torch.zeros(nb * 64, dtype=torch.uint8, device=dev)
    d_idx = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
    d_used = torch.zeros(1, dtype=torch.int64, device=dev)
    d_vscr = torch.zeros(eng.scratch_bytes(nb), dtype=torch.uint8, device=dev)
    eng.validate_device(d_descs.data_ptr(), nb, d_data.data_ptr(), d_res.data_ptr(), d_idx.data_ptr(), cap,
                        d_used.data_ptr(), d_vscr.data_ptr(), sh)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(abi.RESULT_DTYPE).copy()
    idx = d_idx.cpu().numpy().view(abi.INDEX_DTYPE).copy()
    assert (res["verdict"] == 0).all() and (res["index_count"] == a.records).all()
    del d_vscr

    # ---- made transactional
    b = np.arange(nb)
    scope, pos = b // sb, b % sb
    descs["partition"] = scope
    prod = scope * a.producers + pos % a.producers  # the producer id of a batch
    nprod = ns * a.producers
    is_aborted = np.zeros(nprod, bool)
    is_aborted[rng.choice(nprod, max(1, int(round(a.aborted * nprod))), replace=False)] = True
    last = pos == sb - 1
    # the marker's producer: an aborted producer of the scope if it has one, else producer 0
    ab_in_scope = is_aborted.reshape(ns, a.producers)
    mark_prod = np.arange(ns) * a.producers + np.where(ab_in_scope.any(1), ab_in_scope.argmax(1), 0)
    mark_abort = ab_in_scope.any(1)
    prod = np.where(last, mark_prod[scope], prod)
    res["base_offset"] = b * a.records
    res["last_offset_delta"] = a.records - 1
    res["attrs"] = np.where(last, 0x30, 0x10)
    res["record_count"] = np.where(last, 1, a.records)
    first = res["index_first"].astype(np.int64)
    for j in range(a.records):
        idx["offset"][first + j] = res["base_offset"] + j
    hdr = descs["offset"].astype(np.int64)
    pid_bytes = prod.astype("<i8").view(np.uint8).reshape(nb, 8)
    for k in range(8):
        data[hdr + 43 + k] = pid_bytes[:, k]
    data[hdr + 51] = 0
    data[hdr + 52] = 0
    key_at = hdr[last] + idx["key_off"][first[last]].astype(np.int64)
    for k in range(3):
        data[key_at + k] = 0
    data[key_at + 3] = np.where(mark_abort, 0, 1)  # tx_abort / tx_commit
    ab = np.nonzero(is_aborted)[0]
    ranges = np.zeros(len(ab), abi.TX_RANGE_DTYPE)
    ranges["producer_id"] = ab
    ranges["first"] = (ab // a.producers) * sb * a.records
    ranges["last"] = ranges["first"] + sb * a.records - 1
    scopes = np.zeros(ns, abi.TX_SCOPE_DTYPE)
    scopes["first_batch"], scopes["batch_count"] = np.arange(ns) * sb, sb
    scopes["range_first"], scopes["range_count"] = 0, len(ranges)
    scopes["from"] = np.arange(ns) * sb * a.records
    scopes["to"] = scopes["from"] + sb * a.records - 1
    scopes["flags"] = abi.TX_FILTER_RANGES
    # aborted data: every data batch of an aborted producer (its range is consumed at the scope's
    # first batch, and the only marker is the scope's last batch)
    want_data = int((is_aborted[prod] & ~last).sum())

    d_data = torch.from_numpy(data).to(dev)
    d_descs, d_res, d_idx = up(descs), up(res), up(idx)
    d_scopes, d_ranges = up(scopes), up(ranges)
    d_dis = torch.zeros(nb, dtype=torch.uint8, device=dev)
    d_stats = torch.zeros(ns * 64, dtype=torch.uint8, device=dev)
    d_tscr = torch.zeros(int(L.rpgpu_compaction_tx_scratch_bytes(nb, len(ranges))), dtype=torch.uint8, device=dev)
    d_keep = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_keep_y = torch.zeros(cap, dtype=torch.uint8, device=dev)
    d_nkeys = torch.zeros(2, dtype=torch.int64, device=dev)
    d_kscr = torch.zeros(int(L.rpgpu_compaction_scratch_bytes(cap)), dtype=torch.uint8, device=dev)

    def tx_filter():
        ok(L.rpgpu_compaction_tx_filter_device(eng.ctx, d_data.data_ptr(), d_descs.data_ptr(), d_res.data_ptr(), nb,
                                               d_idx.data_ptr(), cap, d_scopes.data_ptr(), ns, d_ranges.data_ptr(),
                                               len(ranges), d_dis.data_ptr(), d_stats.data_ptr(), d_tscr.data_ptr(),
                                               sh))

    def keep_tx():
        ok(L.rpgpu_compaction_keep_tx_device(eng.ctx, d_data.data_ptr(), d_descs.data_ptr(), d_res.data_ptr(), nb,
                                             d_idx.data_ptr(), cap, d_dis.data_ptr(), d_keep.data_ptr(),
                                             d_nkeys.data_ptr(), d_kscr.data_ptr(), sh))

    def keep():
        ok(L.rpgpu_compaction_keep_device(eng.ctx, d_data.data_ptr(), d_descs.data_ptr(), d_res.data_ptr(), nb,
                                          d_idx.data_ptr(), cap, d_keep_y.data_ptr(), d_nkeys.data_ptr() + 8,
                                          d_kscr.data_ptr(), sh))

    steps = (("tx_filter", tx_filter), ("keep_tx", keep_tx), ("keep", keep))
    for _ in range(a.warmup):
        for _, step in steps:
            step()
    torch.cuda.synchronize()
    stats = d_stats.cpu().numpy().view(abi.TX_STATS_DTYPE)
    dis = d_dis.cpu().numpy()
    assert (stats["status"] == abi.TX_OK).all() and int(stats["num_aborted_txes"].sum()) == len(ranges)
    assert int((dis == abi.TX_MARKER).sum()) == ns and int((dis == abi.TX_ABORTED_DATA).sum()) == want_data
    reps = {name: max(3, int(a.min_ms / max(timed(step, 1), 1e-3)) + 1) for name, step in steps}
    t = {name: [] for name, _ in steps}
    for _ in range(a.rounds):  # alternating
        for name, step in steps:
            t[name].append(timed(step, reps[name]))
    print(json.dumps(dict(
        workload=dict(batches=nb, batch_bytes=per, scopes=ns, producers=nprod, ranges=len(ranges),
                      aborted_data_batches=want_data, markers=ns, index_entries=cap, iters=reps),
        tx_filter_ms=t["tx_filter"], keep_tx_ms=t["keep_tx"], keep_ms=t["keep"],
        spread={k: max(v) / min(v) - 1 for k, v in t.items()},
        tx_filter_over_keep=min(t["tx_filter"]) / min(t["keep"]),
        keep_tx_over_keep=min(t["keep_tx"]) / min(t["keep"]))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
