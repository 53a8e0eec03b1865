#!/usr/bin/env python
"""Times building produce batches from records (rpgpu_produce_plan_device +
rpgpu_produce_run_device) on one resident arena of keys and values: 16-byte
keys, 1 KiB values, 100 rows per request, 64 partitions, one third of the rows
per partitioner rule (own id / hashed key / round robin).

Seeded, reads nothing outside the tree, inputs resident in HBM, one HIP event
pair around each plan + run step, warmed, the median of --steps steps.  Prints
one JSON line: GB/s is the input bytes the rows name (keys, values, the rows
themselves) read once plus the output bytes written once, over the time.  One
process per arena size; the caller puts each under its own time limit.  The
per-kernel split comes from a separate run under
`rocprofv3 --kernel-trace --stats -- python scripts/produce_bench.py --steps 5`.
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def build_rows(seed: int, total_bytes: int, key_len: int, value_len: int, per_request: int, partitions: int):
    from redpanda_amd import abi

    rng = np.random.default_rng(seed)
    rec = key_len + value_len
    nrows = max(per_request, total_bytes // rec // per_request * per_request)
    uniq = min(nrows, (32 << 20) // rec)
    block = rng.integers(0, 256, uniq * rec, dtype=np.uint8)
    data = np.tile(block, (nrows + uniq - 1) // uniq)[: nrows * rec]
    i = np.arange(nrows, dtype=np.uint64)
    rows = np.zeros(nrows, abi.PRODUCE_ROW_DTYPE)
    rows["key_off"] = i * rec
    rows["val_off"] = i * rec + key_len
    rule = (i % 3).astype(np.int64)
    rows["key_len"] = np.where(rule == 2, -1, key_len)       # rule 3: no key
    rows["val_len"] = value_len
    rows["flags"] = np.where(rule == 0, abi.PRODUCE_HAS_PARTITION, 0)
    rows["partition"] = np.where(rule == 0, (i * 7) % partitions, 0)
    nreq = nrows // per_request
    reqs = np.zeros(nreq, abi.PRODUCE_REQUEST_DTYPE)
    reqs["now_ms"] = 1_700_000_000_000 + np.arange(nreq)
    reqs["nrows"] = per_request
    reqs["partition_count"] = partitions
    reqs["rr_initial"] = np.arange(nreq) % partitions
    read = int(np.where(rows["key_len"] > 0, rows["key_len"], 0).sum()) + nrows * value_len + rows.nbytes + reqs.nbytes
    return data, rows, reqs, read


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=float, default=256.0, help="keys + values in the arena")
    ap.add_argument("--key", type=int, default=16)
    ap.add_argument("--value", type=int, default=1024)
    ap.add_argument("--rows", type=int, default=100, help="rows per request")
    ap.add_argument("--partitions", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x9A0D)
    a = ap.parse_args()

    import torch

    from redpanda_amd import abi, engine

    dev = torch.device("cuda", 0)
    data, rows, reqs, read = build_rows(a.seed, int(a.mib * (1 << 20)), a.key, a.value, a.rows, a.partitions)
    n, nreq = len(rows), len(reqs)
    d_data = torch.from_numpy(data).to(dev)
    d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev)
    d_reqs = torch.from_numpy(reqs.view(np.uint8)).to(dev)
    sh = torch.cuda.current_stream(dev).cuda_stream
    L = abi.lib()
    eng = engine.Engine(0)
    d_tot = torch.zeros(3, dtype=torch.int64, device=dev)
    d_scr = torch.zeros(int(L.rpgpu_produce_scratch_bytes(n, nreq)), dtype=torch.uint8, device=dev)

    def plan():
        rc = L.rpgpu_produce_plan_device(eng.ctx, d_rows.data_ptr(), n, d_reqs.data_ptr(), nreq, d_data.data_ptr(),
                                         data.nbytes, d_tot.data_ptr(), d_tot.data_ptr() + 8, d_scr.data_ptr(), sh)
        assert rc == 0, eng.last_error()

    plan()
    torch.cuda.synchronize()
    out_bytes, nbatches = int(d_tot[0].item()), int(d_tot[1].item())
    out_cap = out_bytes + abi.ARENA_TAIL_PAD
    d_out = torch.zeros(out_cap, dtype=torch.uint8, device=dev)
    d_rres = torch.zeros(nreq * 16, dtype=torch.uint8, device=dev)
    d_batches = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    d_maps = torch.zeros(2 * n, dtype=torch.int32, device=dev)
    d_od = torch.zeros(n * 24, dtype=torch.uint8, device=dev)
    d_or = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    d_index = torch.zeros(n * 32, dtype=torch.uint8, device=dev)

    def step():
        plan()
        rc = L.rpgpu_produce_run_device(eng.ctx, d_rows.data_ptr(), n, d_reqs.data_ptr(), nreq, d_data.data_ptr(),
                                        data.nbytes, d_rres.data_ptr(), d_batches.data_ptr(), d_maps.data_ptr(),
                                        d_maps.data_ptr() + 4 * n, d_out.data_ptr(), out_cap, d_od.data_ptr(),
                                        d_or.data_ptr(), d_index.data_ptr(), n, d_tot.data_ptr() + 16,
                                        d_scr.data_ptr(), sh)
        assert rc == 0, eng.last_error()

    for _ in range(a.warmup):
        step()
    torch.cuda.synchronize()
    rres = d_rres.cpu().numpy().view(abi.PRODUCE_RESULT_DTYPE)
    ores = d_or.cpu().numpy().view(abi.RESULT_DTYPE)[:nbatches]
    assert (rres["status"] == 0).all() and int(rres["nbatches"].sum()) == nbatches
    assert (ores["verdict"] == 0).all() and int(d_tot[2].item()) == n == int(ores["record_count"].sum())
    ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    med = statistics.median(ms)
    print(json.dumps(dict(
        workload=dict(mib=a.mib, rows=n, requests=nreq, batches=nbatches, key=a.key, value=a.value,
                      rows_per_request=a.rows, partitions=a.partitions, read_bytes=read, out_bytes=out_bytes),
        steps=a.steps, ms_median=med, ms_min=min(ms), ms_max=max(ms),
        gbps=(read + out_bytes) / (med * 1e6))))
    eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
