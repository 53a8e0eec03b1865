#!/usr/bin/env python
"""Times the log append (rpgpu_append_plan_device and rpgpu_append_run_device,
separately) on a C2-shaped arena of Kafka wire batches spread over
--partitions logs, on the same arena with every batch in one partition (the
skewed case: one log is walked by one wave) and, with --shapes blocked, with
every log's batches arriving together (the output order is the arrival order:
what the scatter of the spread shape costs), beside the yardstick:
rpgpu_kafka_serialize_device as shipped.  The serializer only reads on-disk
batches, so it runs over the append's own output: the same batches and the
same number of bytes, moved with an aligned copy and no CRC.

Seeded, reads nothing outside the tree, inputs resident in HBM (validated on
the device before the clock starts), HIP events around the calls, warmed, at
least --min-ms of timed work per side, --rounds alternating rounds.  Prints
one JSON line per arena: every round's times, the run's and the serializer's
bytes/s (bytes read + bytes written), their ratio, each side's run-to-run
spread (max / min - 1) and the plan's share of plan + run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--partitions", type=int, default=4096)
    ap.add_argument("--records", type=int, default=16)
    ap.add_argument("--value", type=int, default=995)
    ap.add_argument("--segment", type=int, default=128 << 20, help="max_segment_size of every log")
    ap.add_argument("--shapes", default="spread,skewed")
    ap.add_argument("--min-ms", type=float, default=400.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0xA99E4D)
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
    nb = max(a.partitions, int(a.gib * (1 << 30)) // per)
    spec = engine.make_spec(seed=a.seed, partitions=a.partitions, records_per_batch=a.records, key_len=16,
                            value_len=a.value, format=abi.FMT_KAFKA_WIRE, ops=abi.OP_CRC | abi.OP_HDRCRC)
    data, descs = engine.build_arena(spec, nb)
    nl = a.partitions
    d_data = torch.from_numpy(data).to(dev)
    d_res = torch.zeros(nb * 64, dtype=torch.uint8, device=dev)
    d_used = torch.zeros(1, dtype=torch.int64, device=dev)
    d_vscr = torch.zeros(eng.scratch_bytes(nb), dtype=torch.uint8, device=dev)
    d_descs = torch.from_numpy(descs.view(np.uint8).copy()).to(dev)
    eng.validate_device(d_descs.data_ptr(), nb, d_data.data_ptr(), d_res.data_ptr(), 0, 0, d_used.data_ptr(),
                        d_vscr.data_ptr(), sh)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(abi.RESULT_DTYPE)
    assert (res["verdict"] == 0).all()
    batch_bytes = int(res["size_bytes"].astype(np.int64).sum())
    del d_vscr

    logs = np.zeros(nl, dtype=abi.APPEND_LOG_DTYPE)
    logs["next_offset"] = np.arange(nl) * 1_000_000
    logs["file_offset"] = (np.arange(nl) * 4099) % max(a.segment // 2, 1)
    logs["max_segment_size"] = a.segment
    d_logs = torch.from_numpy(logs.view(np.uint8)).to(dev)
    d_rows = torch.zeros(nb * 32, dtype=torch.uint8, device=dev)
    d_lres = torch.zeros(nl * 64, dtype=torch.uint8, device=dev)
    d_tot = torch.zeros(3, dtype=torch.int64, device=dev)
    d_scr = torch.zeros(int(L.rpgpu_append_scratch_bytes(nb, nl)), dtype=torch.uint8, device=dev)
    d_odescs = torch.zeros(nb * 24, dtype=torch.uint8, device=dev)
    d_ores = torch.zeros(nb * 64, dtype=torch.uint8, device=dev)
    d_segs = torch.zeros((nb + nl) * 48, dtype=torch.uint8, device=dev)
    out_cap = batch_bytes + 16 * nl + 64
    d_out = torch.zeros(out_cap, dtype=torch.uint8, device=dev)
    d_wire = torch.zeros(out_cap, dtype=torch.uint8, device=dev)

    for shape in [s for s in a.shapes.split(",") if s]:
        dd = descs.copy()
        if shape == "skewed":
            dd["partition"] = 0
        elif shape == "blocked":                 # every log's batches arrive together: output order = arrival order
            dd["partition"] = (np.arange(nb, dtype=np.uint64) * nl // nb).astype(np.uint32)
        d_descs = torch.from_numpy(dd.view(np.uint8).copy()).to(dev)

        def plan():
            rc = L.rpgpu_append_plan_device(eng.ctx, d_descs.data_ptr(), d_res.data_ptr(), nb, None, d_logs.data_ptr(),
                                            0, nl, d_rows.data_ptr(), d_lres.data_ptr(), d_tot.data_ptr(),
                                            d_scr.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        def run():
            rc = L.rpgpu_append_run_device(eng.ctx, d_data.data_ptr(), d_descs.data_ptr(), d_res.data_ptr(), nb,
                                           d_logs.data_ptr(), 0, nl, d_rows.data_ptr(), d_lres.data_ptr(),
                                           d_out.data_ptr(), out_cap, d_odescs.data_ptr(), d_ores.data_ptr(), nb,
                                           d_segs.data_ptr(), nb + nl, d_scr.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        def serialize():
            rc = L.rpgpu_kafka_serialize_device(eng.ctx, d_out.data_ptr(), d_odescs.data_ptr(), None, nb,
                                                d_wire.data_ptr(), None, 0, None, sh)
            assert rc == 0, eng.last_error()

        for _ in range(a.warmup):
            plan()
            run()
            serialize()
        torch.cuda.synchronize()
        tot = d_tot.cpu().numpy()
        lres = d_lres.cpu().numpy().view(abi.APPEND_LOG_RESULT_DTYPE)
        assert (lres["status"] == abi.APPEND_OK).all() and int(tot[1]) == nb and int(tot[0]) <= out_cap
        assert int(lres["byte_size"].sum()) == batch_bytes
        # the serialized output is the produce arena again from byte 16 of every batch on
        od = d_odescs.cpu().numpy().view(abi.DESC_DTYPE)
        rows = d_rows.cpu().numpy().view(abi.APPEND_BATCH_DTYPE)
        for i in () if os.environ.get("RPGPU_DIAG_LIB") else (0, nb // 2, nb - 1):   # (a diagnostics build: times only)
            r = int(rows["out_row"][i])
            o, s, n = int(od["offset"][r]), int(dd["offset"][i]), int(od["length"][r])
            assert torch.equal(d_wire[o + 16:o + n], d_data[s + 16:s + n]), i
        reps = {}
        for name, step in (("plan", plan), ("run", run), ("serialize", serialize)):
            reps[name] = max(3, int(a.min_ms / max(timed(step, 1), 1e-3)) + 1)
        t = {"plan": [], "run": [], "serialize": []}
        for _ in range(a.rounds):                # alternating: plan, run, serialize, plan, ...
            for name, step in (("plan", plan), ("run", run), ("serialize", serialize)):
                t[name].append(timed(step, reps[name]))
        moved = 2 * batch_bytes
        best = {k: min(v) for k, v in t.items()}
        print(json.dumps(dict(
            shape=shape,
            workload=dict(batches=nb, logs=nl, batch_bytes=batch_bytes, max_segment_size=a.segment,
                          segments=int(tot[2]), iters=reps),
            plan_ms=t["plan"], run_ms=t["run"], serialize_ms=t["serialize"],
            run_tbps=moved / (best["run"] * 1e9), serialize_tbps=moved / (best["serialize"] * 1e9),
            run_over_serialize=best["run"] / best["serialize"],
            spread={k: max(v) / min(v) - 1 for k, v in t.items()},
            plan_share=best["plan"] / (best["plan"] + best["run"]))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
