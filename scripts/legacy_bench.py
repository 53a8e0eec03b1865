#!/usr/bin/env python
"""Times the legacy MessageSet conversion (rpgpu_legacy_plan_device +
rpgpu_legacy_run_device) on one arena of uncompressed magic-1 sets, beside the
yardstick: rpgpu_validate_device over an arena of v2 wire batches of the same
byte volume, in the same process, alternating.

Seeded, reads nothing outside the tree, inputs resident in HBM, HIP events
around the calls, warmed, at least --min-ms of timed work per side.  Prints
one JSON line.  --lane-crc sweeps the lane / wave crossover of the CRC32
kernel (RPGPU_LEGACY_LANE_CRC, read when a context opens).  The per-kernel
split comes from a separate run under `rocprofv3 --kernel-trace --stats` with
--no-yardstick --iters N.
"""
from __future__ import annotations

import argparse
import json
import os
import struct
import sys
import zlib
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))


def build_sets(seed: int, total_bytes: int, msgs_per_set: int, key_len: int, value_len: int):
    """Sets of msgs_per_set magic-1 messages; a 32 MiB seeded block of messages
    tiled up to total_bytes (whole sets)."""
    rng = np.random.default_rng(seed)
    msg = 16 + 1 + 1 + 8 + 4 + key_len + 4 + value_len
    set_len = msg * msgs_per_set
    nsets = max(1, total_bytes // set_len)
    uniq = max(1, min(nsets, (32 << 20) // set_len))
    block = rng.integers(0, 256, uniq * set_len, dtype=np.uint8)
    m = block.reshape(uniq * msgs_per_set, msg)
    idx = np.arange(uniq * msgs_per_set) % msgs_per_set
    m[:, 0:8] = np.frombuffer(idx.astype(">i8").tobytes(), dtype=np.uint8).reshape(-1, 8)
    m[:, 8:12] = np.frombuffer(struct.pack(">i", msg - 12), dtype=np.uint8)
    m[:, 16] = 1                                           # magic
    m[:, 17] = 0                                           # attributes: uncompressed
    ts = (1_650_000_000_000 + np.arange(len(m))).astype(">i8")
    m[:, 18:26] = np.frombuffer(ts.tobytes(), dtype=np.uint8).reshape(-1, 8)
    m[:, 26:30] = np.frombuffer(struct.pack(">i", key_len), dtype=np.uint8)
    m[:, 30 + key_len:34 + key_len] = np.frombuffer(struct.pack(">i", value_len), dtype=np.uint8)
    raw = m.tobytes()
    crcs = np.array([zlib.crc32(raw[i * msg + 16:(i + 1) * msg]) for i in range(len(m))], dtype=">u4")
    m[:, 12:16] = np.frombuffer(crcs.tobytes(), dtype=np.uint8).reshape(-1, 4)
    reps = (nsets + uniq - 1) // uniq
    data = np.tile(m.reshape(-1), reps)[: nsets * set_len]
    return np.concatenate([data, np.zeros(64, dtype=np.uint8)]), nsets, set_len


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--msgs", type=int, default=100)
    ap.add_argument("--key", type=int, default=16)
    ap.add_argument("--value", type=int, default=1024)
    ap.add_argument("--min-ms", type=float, default=400.0)
    ap.add_argument("--iters", type=int, default=0, help="fixed iteration count (0: until --min-ms)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--lane-crc", default="", help="comma-separated RPGPU_LEGACY_LANE_CRC values to sweep")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--seed", type=int, default=0x1E6AC7)
    a = ap.parse_args()

    import torch

    from redpanda_amd import abi, engine

    dev = torch.device("cuda", 0)
    total = int(a.gib * (1 << 30))
    data, nsets, set_len = build_sets(a.seed, total, a.msgs, a.key, a.value)
    wire = nsets * set_len
    sets = np.zeros(nsets, dtype=abi.DESC_DTYPE)
    sets["offset"] = np.arange(nsets, dtype=np.uint64) * set_len
    sets["length"] = set_len
    sets["partition"] = np.arange(nsets) % 64
    sets["ops"] = abi.OPS_PRODUCE
    d_data = torch.from_numpy(data).to(dev)
    d_sets = torch.from_numpy(sets.view(np.uint8)).to(dev)
    sh = torch.cuda.current_stream(dev).cuda_stream
    L = abi.lib()

    def legacy_side(eng):
        d_tot = torch.zeros(3, dtype=torch.int64, device=dev)
        d_scr = torch.zeros(int(L.rpgpu_legacy_scratch_bytes(nsets)), dtype=torch.uint8, device=dev)

        def plan():
            rc = L.rpgpu_legacy_plan_device(eng.ctx, d_sets.data_ptr(), nsets, d_data.data_ptr(), d_tot.data_ptr(),
                                            d_tot.data_ptr() + 8, d_scr.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        plan()
        torch.cuda.synchronize()
        out_cap = int(d_tot[0].item()) + abi.ARENA_TAIL_PAD
        index_cap = int(d_tot[1].item()) + 1
        d_out = torch.zeros(out_cap, dtype=torch.uint8, device=dev)
        d_lres = torch.zeros(nsets * 48, dtype=torch.uint8, device=dev)
        d_od = torch.zeros(nsets * 24, dtype=torch.uint8, device=dev)
        d_or = torch.zeros(nsets * 64, dtype=torch.uint8, device=dev)
        d_index = torch.zeros(index_cap * 32, dtype=torch.uint8, device=dev)

        def step():
            plan()
            rc = L.rpgpu_legacy_run_device(eng.ctx, d_sets.data_ptr(), nsets, d_data.data_ptr(), 1_700_000_000_000,
                                           d_lres.data_ptr(), d_out.data_ptr(), out_cap, d_od.data_ptr(),
                                           d_or.data_ptr(), d_index.data_ptr(), index_cap, d_tot.data_ptr() + 16,
                                           d_scr.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        def check():
            lres = d_lres.cpu().numpy().view(abi.LEGACY_RESULT_DTYPE)
            ores = d_or.cpu().numpy().view(abi.RESULT_DTYPE)
            assert (lres["verdict"] == 0).all() and (ores["verdict"] == 0).all()
            assert (lres["record_count"] == a.msgs).all() and int(d_tot[2].item()) == nsets * a.msgs

        return step, check, (d_tot, d_scr, d_out, d_lres, d_od, d_or, d_index)

    def yardstick_side(eng):
        per = 61 + a.msgs * (a.key + a.value + 12)
        nb = max(1, wire // per)
        spec = engine.make_spec(seed=a.seed, partitions=64, records_per_batch=a.msgs, key_len=a.key,
                                value_len=a.value)
        vdata, vdescs = engine.build_arena(spec, nb)
        vbytes = int(vdescs["length"].astype(np.uint64).sum())
        dv = torch.from_numpy(vdata).to(dev)
        dd = torch.from_numpy(vdescs.view(np.uint8)).to(dev)
        d_res = torch.zeros(nb * 64, dtype=torch.uint8, device=dev)
        cap = nb * a.msgs + 1
        d_index = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        d_used = torch.zeros(1, dtype=torch.int64, device=dev)
        d_scr = torch.zeros(eng.scratch_bytes(nb), dtype=torch.uint8, device=dev)

        def step():
            eng.validate_device(dd.data_ptr(), nb, dv.data_ptr(), d_res.data_ptr(), d_index.data_ptr(), cap,
                                d_used.data_ptr(), d_scr.data_ptr(), sh)

        def check():
            assert (d_res.cpu().numpy().view(abi.RESULT_DTYPE)["verdict"] == 0).all()

        return step, check, vbytes, (dv, dd, d_res, d_index, d_used, d_scr)

    def timed(step, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    result = dict(workload=dict(sets=nsets, msgs_per_set=a.msgs, key=a.key, value=a.value, wire_bytes=wire))
    lanes = [int(x) for x in a.lane_crc.split(",") if x] or [None]
    eng0 = engine.Engine(0)
    ystep = None
    if not a.no_yardstick:
        ystep, ycheck, vbytes, _ykeep = yardstick_side(eng0)
        for _ in range(a.warmup):
            ystep()
        torch.cuda.synchronize()
        ycheck()
    runs = []
    for lm in lanes:
        if lm is not None:
            os.environ["RPGPU_LEGACY_LANE_CRC"] = str(lm)
        eng = engine.Engine(0) if lm is not None else eng0
        step, check, _keep = legacy_side(eng)
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        check()
        one = max(timed(step, 1), 1e-3)
        n = a.iters or max(3, int(a.min_ms / one) + 1)
        # alternating: legacy, yardstick, legacy, yardstick
        lt, yt = [], []
        for _ in range(2):
            lt.append(timed(step, n) / n)
            if ystep:
                yt.append(timed(ystep, n) / n)
        r = dict(lane_crc=lm, iters=n, legacy_ms=lt, legacy_gbps=wire / (min(lt) * 1e6))
        if ystep:
            r.update(validate_ms=yt, validate_gbps=vbytes / (min(yt) * 1e6),
                     ratio=(wire / min(lt)) / (vbytes / min(yt)))
        runs.append(r)
        if lm is not None:
            eng.close()
        del _keep
        torch.cuda.empty_cache()
    result["runs"] = runs
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
