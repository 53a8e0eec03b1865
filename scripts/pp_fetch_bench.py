#!/usr/bin/env python
"""Times the REST proxy fetch rendering (rpgpu_pp_fetch_plan_device +
rpgpu_pp_fetch_run_device) on one arena of uncompressed on-disk v2 batches,
rendered as one response per --per-response batches, beside the yardstick:
rpgpu_kafka_serialize_device over the same arena (it also reads and writes
the arena once), in the same process, alternating.

Seeded, reads nothing outside the tree, inputs resident in HBM (validated and
indexed on the device before the clock starts), HIP events around the calls,
warmed, at least --min-ms of timed work per side.  Prints one JSON line per
arena.  --values sweeps the value size; each size is rendered with every
field on its record's lane and with the values on the wave path
(RPGPU_PP_LANE_FIELD, a diagnostics variable read when a context opens).
The byte-count bound is field bytes in + 32 B of index per record + the JSON
bytes out, at --copy-tbps (the measured copy rate DESIGN.md §3 uses).
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
    ap.add_argument("--records", type=int, default=100)
    ap.add_argument("--key", type=int, default=16)
    ap.add_argument("--values", default="1024", help="comma-separated value sizes, an arena each")
    ap.add_argument("--per-response", type=int, default=64)
    ap.add_argument("--paths", default="default", help="comma-separated: default, lane, wave")
    ap.add_argument("--min-ms", type=float, default=400.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--copy-tbps", type=float, default=6.3)
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--seed", type=int, default=0x1E6AC7)
    a = ap.parse_args()

    import torch

    from redpanda_amd import abi, engine

    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream(dev).cuda_stream
    L = abi.lib()

    def timed(step, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    eng0 = engine.Engine(0)
    for value in [int(v) for v in a.values.split(",") if v]:
        per = 61 + a.records * (a.key + value + 12)
        nb = max(a.per_response, int(a.gib * (1 << 30)) // per)
        spec = engine.make_spec(seed=a.seed, partitions=64, records_per_batch=a.records, key_len=a.key,
                                value_len=value, format=abi.FMT_RP_DISK)
        data, descs = engine.build_arena(spec, nb)
        arena_bytes = int(descs["length"].astype(np.uint64).sum())
        d_data = torch.from_numpy(data).to(dev)
        d_descs = torch.from_numpy(descs.view(np.uint8)).to(dev)
        d_res = torch.zeros(nb * 64, dtype=torch.uint8, device=dev)
        cap = nb * a.records + 1
        d_index = torch.zeros(cap * 32, dtype=torch.uint8, device=dev)
        d_used = torch.zeros(1, dtype=torch.int64, device=dev)
        d_vscr = torch.zeros(eng0.scratch_bytes(nb), dtype=torch.uint8, device=dev)
        eng0.validate_device(d_descs.data_ptr(), nb, d_data.data_ptr(), d_res.data_ptr(), d_index.data_ptr(), cap,
                             d_used.data_ptr(), d_vscr.data_ptr(), sh)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(abi.RESULT_DTYPE)
        assert (res["verdict"] == 0).all() and (res["index_count"] == a.records).all()
        del d_vscr

        topic = b"bench-topic"
        nr = (nb + a.per_response - 1) // a.per_response
        ranges = np.zeros(nr, dtype=abi.PP_RANGE_DTYPE)
        ranges["first"] = np.arange(nr) * a.per_response
        ranges["count"] = np.minimum(a.per_response, nb - ranges["first"])
        ranges["topic_len"] = len(topic)
        ranges["partition"] = np.arange(nr) % 64
        responses = np.zeros(nr, dtype=abi.PP_RESPONSE_DTYPE)
        responses["first_range"] = np.arange(nr)
        responses["range_count"] = 1
        d_top = torch.from_numpy(np.frombuffer(topic, dtype=np.uint8).copy()).to(dev)
        d_rg = torch.from_numpy(ranges.view(np.uint8)).to(dev)
        d_rs = torch.from_numpy(responses.view(np.uint8)).to(dev)
        d_pres = torch.zeros(nr * 32, dtype=torch.uint8, device=dev)
        d_bytes = torch.zeros(1, dtype=torch.int64, device=dev)
        d_scr = torch.zeros(int(L.rpgpu_pp_fetch_scratch_bytes(nb, nr, nr)), dtype=torch.uint8, device=dev)

        def plan(eng):
            rc = L.rpgpu_pp_fetch_plan_device(eng.ctx, d_descs.data_ptr(), d_res.data_ptr(), nb, d_index.data_ptr(),
                                              d_top.data_ptr(), len(topic), d_rg.data_ptr(), nr, d_rs.data_ptr(), nr,
                                              abi.PP_FMT_BINARY_V2, d_pres.data_ptr(), d_bytes.data_ptr(),
                                              d_scr.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        plan(eng0)
        torch.cuda.synchronize()
        out_cap = int(d_bytes.item())
        d_out = torch.zeros(out_cap, dtype=torch.uint8, device=dev)

        def pp_step(eng):
            plan(eng)
            rc = L.rpgpu_pp_fetch_run_device(eng.ctx, d_data.data_ptr(), d_descs.data_ptr(), d_res.data_ptr(), nb,
                                             d_index.data_ptr(), d_top.data_ptr(), d_rg.data_ptr(), nr,
                                             d_rs.data_ptr(), nr, d_out.data_ptr(), out_cap, d_pres.data_ptr(),
                                             d_scr.data_ptr(), sh)
            assert rc == 0, eng.last_error()

        ystep = None
        if not a.no_yardstick:
            d_wire = torch.zeros_like(d_data)

            def ystep():
                rc = L.rpgpu_kafka_serialize_device(eng0.ctx, d_data.data_ptr(), d_descs.data_ptr(), None, nb,
                                                    d_wire.data_ptr(), None, 0, None, sh)
                assert rc == 0, eng0.last_error()

            for _ in range(a.warmup):
                ystep()
            torch.cuda.synchronize()

        records = nb * a.records
        field_bytes = records * (a.key + value)
        runs = []
        for path in a.paths.split(","):
            lane_max = {"default": None, "lane": max(a.key, value), "wave": max(value - 1, 0)}[path]
            if lane_max is None:
                os.environ.pop("RPGPU_PP_LANE_FIELD", None)
            else:
                os.environ["RPGPU_PP_LANE_FIELD"] = str(lane_max)
            eng = engine.Engine(0)
            step = lambda: pp_step(eng)          # noqa: E731
            for _ in range(a.warmup):
                step()
            torch.cuda.synchronize()
            pres = d_pres.cpu().numpy().view(abi.PP_RESULT_DTYPE)
            assert (pres["status"] == 0).all() and int(pres["records"].sum()) == records
            json_bytes = int(pres["out_len"].sum())
            first = bytes(d_out[: int(pres["out_len"][0])].cpu().numpy())
            assert len(json.loads(first)) == int(pres["records"][0])      # a well-formed array
            one = max(timed(step, 1), 1e-3)
            n = max(3, int(a.min_ms / one) + 1)
            pt, yt = [], []
            for _ in range(2):                   # alternating: render, yardstick, render, yardstick
                pt.append(timed(step, n) / n)
                if ystep:
                    yt.append(timed(ystep, n) / n)
            bound_bytes = field_bytes + 32 * records + json_bytes
            bound_ms = bound_bytes / (a.copy_tbps * 1e9)
            r = dict(path=path, lane_field_max=lane_max, iters=n, render_ms=pt,
                     json_gbps=json_bytes / (min(pt) * 1e6), bound_ms=bound_ms, of_bound=bound_ms / min(pt))
            if ystep:
                r.update(serialize_ms=yt, ratio_to_serialize=min(yt) / min(pt))
            runs.append(r)
            eng.close()
        print(json.dumps(dict(workload=dict(batches=nb, records_per_batch=a.records, key=a.key, value=value,
                                            arena_bytes=arena_bytes, responses=nr, json_bytes=json_bytes,
                                            field_bytes=field_bytes), runs=runs)), flush=True)
        del d_data, d_descs, d_res, d_index, d_out, d_scr
        if ystep:
            del d_wire
        torch.cuda.empty_cache()
    os.environ.pop("RPGPU_PP_LANE_FIELD", None)
    return 0


if __name__ == "__main__":
    sys.exit(main())
