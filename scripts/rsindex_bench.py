#!/usr/bin/env python
"""Times the tiered-storage offset index (rpgpu_rsindex_plan_device,
rpgpu_rsindex_run_device and 4,096 lookups with rpgpu_rsindex_find_device,
separately) over a C2-shaped arena of on-disk batches cut into --segments
equal runs of descriptors (4,096 and 8 by default: the same bytes as many
small segments and as a few large ones), both steps 64 KiB as at the
reference's call sites, beside the yardstick: rpgpu_segment_index_device over
the same descriptors, the engine's other per-segment sampling pass, with its
validation done before the clock starts.

Seeded, reads nothing outside the tree, inputs resident in HBM, HIP events
around the calls, warmed, at least --min-ms of timed work per side, --rounds
alternating rounds.  Prints one JSON line per segment count: every round's
times, each side's run-to-run spread (max / min - 1), samples, rows and blob
bytes.
"""
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
    ap.add_argument("--segments", default="4096,8")
    ap.add_argument("--records", type=int, default=16)
    ap.add_argument("--value", type=int, default=995)
    ap.add_argument("--step", type=int, default=64 << 10, help="sampling_step and file_pos_step")
    ap.add_argument("--finds", type=int, default=4096)
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x5E61DE)
    a = ap.parse_args()

    import torch

    from redpanda_amd import abi, engine

    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream(dev).cuda_stream
    L = abi.lib()
    eng = engine.Engine(0)

    def timed(step, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    per = 61 + a.records * (16 + a.value + 12)
    nb = int(a.gib * (1 << 30)) // per
    spec = engine.make_spec(seed=a.seed, partitions=1, records_per_batch=a.records, key_len=16, value_len=a.value,
                            format=abi.FMT_RP_DISK, ops=abi.OP_CRC | abi.OP_HDRCRC)
    data, descs = engine.build_arena(spec, nb)
    d_data = torch.from_numpy(data).to(dev)
    d_descs = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
    d_res = torch.zeros(nb * 64, dtype=torch.uint8, device=dev)
    d_used = torch.zeros(1, dtype=torch.int64, device=dev)
    d_vscr = torch.zeros(eng.scratch_bytes(nb), dtype=torch.uint8, device=dev)
    eng.validate_device(d_descs.data_ptr(), nb, d_data.data_ptr(), d_res.data_ptr(), 0, 0, d_used.data_ptr(),
                        d_vscr.data_ptr(), sh)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(abi.RESULT_DTYPE)
    assert (res["verdict"] == 0).all()
    del d_vscr
    base = res["base_offset"].astype(np.int64)
    rng = np.random.default_rng(a.seed)

    for ns in [int(s) for s in a.segments.split(",") if s]:
        first = (np.arange(ns, dtype=np.uint64) * nb // ns).astype(np.uint32)
        count = np.diff(np.append(first, nb)).astype(np.uint32)
        segs = np.zeros(ns, dtype=abi.RSINDEX_SEGMENT_DTYPE)
        segs["first_batch"], segs["batch_count"] = first, count
        segs["base_rp_offset"] = segs["base_kafka_offset"] = base[first]
        segs["file_pos_step"], segs["sampling_step"] = a.step, a.step
        isegs = np.zeros(ns, dtype=abi.SEGMENT_DTYPE)      # the yardstick's rows over the same runs
        isegs["first_batch"], isegs["batch_count"], isegs["base_offset"] = first, count, base[first]
        isegs["step"] = a.step
        d_segs = torch.from_numpy(segs.view(np.uint8).copy()).to(dev)
        d_isegs = torch.from_numpy(isegs.view(np.uint8).copy()).to(dev)
        d_rres = torch.zeros(ns * 64, dtype=torch.uint8, device=dev)
        d_tot = torch.zeros(2, dtype=torch.int64, device=dev)
        d_scr = torch.zeros(int(L.rpgpu_rsindex_scratch_bytes(nb, ns)), dtype=torch.uint8, device=dev)
        d_states = torch.zeros(ns * 48, dtype=torch.uint8, device=dev)
        d_entries = torch.zeros(nb * 16, dtype=torch.uint8, device=dev)

        def plan():
            rc = L.rpgpu_rsindex_plan_device(eng.ctx, d_data.data_ptr(), d_descs.data_ptr(), nb, d_segs.data_ptr(), ns,
                                             d_rres.data_ptr(), d_tot.data_ptr(), d_scr.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        plan()
        torch.cuda.synchronize()
        out_cap = int(d_tot.cpu().numpy()[0])
        d_out = torch.zeros(out_cap, dtype=torch.uint8, device=dev)

        def run():
            rc = L.rpgpu_rsindex_run_device(eng.ctx, d_segs.data_ptr(), ns, d_rres.data_ptr(), d_out.data_ptr(), out_cap,
                                            d_scr.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        run()
        torch.cuda.synchronize()
        rres = d_rres.cpu().numpy().view(abi.RSINDEX_RESULT_DTYPE)
        assert (rres["status"] == abi.RSINDEX_OK).all()
        # lookups: Kafka offsets of random batches, each in its own segment's blob
        pick = np.sort(rng.integers(0, nb, a.finds))
        owner = np.searchsorted(first, pick, side="right") - 1
        q = np.zeros(a.finds, dtype=abi.RSINDEX_QUERY_DTYPE)
        q["blob_offset"], q["blob_bytes"] = rres["out_offset"][owner], rres["out_bytes"][owner]
        q["upper_bound"] = base[pick] + 1
        d_q = torch.from_numpy(q.view(np.uint8).copy()).to(dev)
        d_found = torch.zeros(a.finds * 48, dtype=torch.uint8, device=dev)

        def find():
            rc = L.rpgpu_rsindex_find_device(eng.ctx, d_out.data_ptr(), d_q.data_ptr(), a.finds, d_found.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        def yardstick():
            rc = L.rpgpu_segment_index_device(eng.ctx, d_descs.data_ptr(), d_res.data_ptr(), d_isegs.data_ptr(), ns,
                                              d_states.data_ptr(), d_entries.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        steps = (("plan", plan), ("run", run), ("find", find), ("segment_index", yardstick))
        for _ in range(a.warmup):
            for _, step in steps:
                step()
        torch.cuda.synchronize()
        found = d_found.cpu().numpy().view(abi.RSINDEX_FOUND_DTYPE)
        hit = found["status"] == abi.RSINDEX_FOUND
        assert (found["status"] != abi.RSINDEX_BAD_BLOB).all()
        assert (found["kaf_offset"][hit] <= base[pick][hit]).all() and (found["rp_offset"][hit] >= base[first][owner][hit]).all()
        reps = {name: max(3, int(a.min_ms / max(timed(step, 1), 1e-3)) + 1) for name, step in steps}
        t = {name: [] for name, _ in steps}
        for _ in range(a.rounds):                # alternating: plan, run, find, yardstick, plan, ...
            for name, step in steps:
                t[name].append(timed(step, reps[name]))
        print(json.dumps(dict(
            segments=ns,
            workload=dict(batches=nb, arena_bytes=int(res["size_bytes"].astype(np.int64).sum()), step=a.step,
                          samples=int(rres["samples"].sum()), rows=int(rres["rows"].sum()), blob_bytes=out_cap,
                          finds=a.finds, found=int(hit.sum()), from_write_buffer=int(found["from_write_buffer"].sum()),
                          iters=reps),
            plan_ms=t["plan"], run_ms=t["run"], find_ms=t["find"], segment_index_ms=t["segment_index"],
            spread={k: max(v) / min(v) - 1 for k, v in t.items()},
            plan_over_segment_index=min(t["plan"]) / min(t["segment_index"]))), flush=True)
        del d_out
    return 0


if __name__ == "__main__":
    sys.exit(main())
