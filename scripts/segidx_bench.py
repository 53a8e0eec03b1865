#!/usr/bin/env python
"""Times the segment index's life cycle on the device, each entry point on its
own: rpgpu_segidx_write_plan_device, rpgpu_segidx_write_run_device,
rpgpu_segidx_hydrate_device (of the blobs the run wrote) and --finds lookups
with rpgpu_segidx_find_device (a third of each kind), over --shapes "states x
entries" (8 x 32,768 and 4,096 x 64 by default: the same number of entries as a
few large indexes and as many small ones); then rpgpu_segidx_track_device from
empty states beside the yardstick, the parent's rpgpu_segment_index_device, over
the same validated on-disk arena cut into --segments equal runs.  Tracking
continues its state rows in place, so every timed track call gets fresh rows of
its own from a pool of --pool copies that is refilled, outside the clock, before
each timed run; a run makes at most --pool calls.

Seeded, reads nothing outside the tree, inputs resident in HBM, HIP events
around the calls, warmed, at least --min-ms of timed work per side, --rounds
alternating rounds.  Prints one JSON line per shape and per segment count:
every round's times and each side's run-to-run spread (max / min - 1).
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
    ap.add_argument("--shapes", default="8x32768,4096x64")
    ap.add_argument("--finds", type=int, default=4096)
    ap.add_argument("--gib", type=float, default=1.0, help="arena of the track comparison")
    ap.add_argument("--segments", default="4096,8")
    ap.add_argument("--records", type=int, default=16)
    ap.add_argument("--value", type=int, default=995)
    ap.add_argument("--step", type=int, default=4096 * 8, help="segment_index step")
    ap.add_argument("--pool", type=int, default=1024, help="copies of the fresh state rows per timed run")
    ap.add_argument("--min-ms", type=float, default=200.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x5E61D8)
    a = ap.parse_args()

    import torch

    from redpanda_amd import abi, engine

    dev = torch.device("cuda", 0)
    sh = torch.cuda.current_stream(dev).cuda_stream
    L = abi.lib()
    eng = engine.Engine(0)
    rng = np.random.default_rng(a.seed)

    def timed(step, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            step()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n

    def up(x):
        return torch.from_numpy(x.view(np.uint8).reshape(-1).copy()).to(dev)

    def measure(steps, prepare=None, cap=None):
        """prepare: called (untimed, then synchronized) before every timed run; cap: most calls per run."""
        def ready():
            if prepare:
                prepare()
                torch.cuda.synchronize()

        for _ in range(a.warmup):
            for _, step in steps:
                step()
        torch.cuda.synchronize()
        reps = {}
        for name, step in steps:
            ready()
            reps[name] = max(3, int(a.min_ms / max(timed(step, 1), 1e-3)) + 1)
            if cap:
                reps[name] = min(reps[name], cap)
        t = {name: [] for name, _ in steps}
        for _ in range(a.rounds):  # alternating
            for name, step in steps:
                ready()
                t[name].append(timed(step, reps[name]))
        return t, reps

    def ok(rc):
        assert rc == 0, eng.last_error()

    # ---- write, hydrate, find
    for shape in [s for s in a.shapes.split(",") if s]:
        ns, per = (int(x) for x in shape.split("x"))
        ne = ns * per
        states = np.zeros(ns, dtype=abi.SEGIDX_STATE_DTYPE)
        states["base_offset"] = np.arange(ns, dtype=np.int64) * 10_000_000
        states["base_timestamp"] = 1_700_000_000_000
        states["entries"] = states["entry_cap"] = per
        states["entry_first"] = np.arange(ns, dtype=np.uint64) * per
        states["monotonic"] = states["with_offset"] = 1
        ent = np.zeros(ne, dtype=abi.INDEX_ENTRY_DTYPE)
        ent["relative_offset"] = np.cumsum(rng.integers(1, 200, (ns, per)), axis=1).reshape(-1)
        deltas = np.cumsum(rng.integers(0, 40, (ns, per)), axis=1)
        ent["relative_time"] = (deltas + (1 << 31)).reshape(-1)
        ent["position"] = np.cumsum(rng.integers(61, 40_000, (ns, per)), axis=1).reshape(-1)
        states["max_offset"] = states["base_offset"] + ent["relative_offset"].reshape(ns, per)[:, -1]
        states["max_timestamp"] = states["base_timestamp"] + deltas[:, -1]
        d_states, d_ent = up(states), up(ent)
        d_blobs = torch.zeros(ns * 32, dtype=torch.uint8, device=dev)
        d_tot = torch.zeros(1, dtype=torch.int64, device=dev)

        def plan():
            ok(L.rpgpu_segidx_write_plan_device(eng.ctx, d_states.data_ptr(), ns, ne, d_blobs.data_ptr(),
                                                d_tot.data_ptr(), sh))

        plan()
        torch.cuda.synchronize()
        out_cap = int(d_tot.cpu().numpy()[0])
        d_out = torch.zeros(out_cap, dtype=torch.uint8, device=dev)

        def run():
            ok(L.rpgpu_segidx_write_run_device(eng.ctx, d_states.data_ptr(), ns, d_ent.data_ptr(), ne,
                                               d_blobs.data_ptr(), d_out.data_ptr(), out_cap, sh))

        run()
        torch.cuda.synchronize()
        blobs = d_blobs.cpu().numpy().view(abi.SEGIDX_BLOB_DTYPE)
        assert (blobs["status"] == abi.SEGIDX_OK).all()
        files = np.zeros(ns, dtype=abi.SEGIDX_FILE_DTYPE)
        files["blob_offset"], files["blob_bytes"] = blobs["out_offset"], blobs["out_bytes"]
        d_files = up(files)
        h_states = np.zeros(ns, dtype=abi.SEGIDX_STATE_DTYPE)
        h_states["entry_first"], h_states["entry_cap"] = states["entry_first"], per
        d_hstates = up(h_states)
        d_hent = torch.zeros(ne * 16, dtype=torch.uint8, device=dev)
        d_hyd = torch.zeros(ns * 16, dtype=torch.uint8, device=dev)

        def hydrate():
            ok(L.rpgpu_segidx_hydrate_device(eng.ctx, d_out.data_ptr(), out_cap, d_files.data_ptr(), ns,
                                             d_hstates.data_ptr(), d_hent.data_ptr(), ne, d_hyd.data_ptr(), sh))

        hydrate()
        torch.cuda.synchronize()
        assert (d_hyd.cpu().numpy().view(abi.SEGIDX_HYDRATED_DTYPE)["status"] == abi.SEGIDX_OK).all()
        assert np.array_equal(d_hent.cpu().numpy(), ent.view(np.uint8).reshape(-1))
        q = np.zeros(a.finds, dtype=abi.SEGIDX_QUERY_DTYPE)
        q["state"] = rng.integers(0, ns, a.finds)
        q["kind"] = np.arange(a.finds) % 3
        pick = rng.integers(0, per, a.finds)
        row = ent.reshape(ns, per)[q["state"], pick]
        q["key"] = np.where(q["kind"] == 0, states["base_offset"][q["state"]] + row["relative_offset"],
                            states["base_timestamp"][q["state"]] + row["relative_time"].astype(np.int64) - (1 << 31) + 1)
        d_q = up(q)
        d_found = torch.zeros(a.finds * 32, dtype=torch.uint8, device=dev)

        def find():
            ok(L.rpgpu_segidx_find_device(eng.ctx, d_hstates.data_ptr(), ns, d_hent.data_ptr(), ne, d_q.data_ptr(),
                                          a.finds, d_found.data_ptr(), sh))

        t, reps = measure((("plan", plan), ("run", run), ("hydrate", hydrate), ("find", find)))
        found = d_found.cpu().numpy().view(abi.SEGIDX_FOUND_DTYPE)
        assert (found["status"] != abi.SEGIDX_BAD_QUERY).all()
        by_offset = q["kind"] == 0
        assert (found["status"][by_offset] == abi.SEGIDX_FOUND).all() and (found["ix"][by_offset] == pick[by_offset]).all()
        print(json.dumps(dict(
            shape=shape, workload=dict(states=ns, entries=ne, blob_bytes=out_cap, finds=a.finds,
                                       found=int((found["status"] == abi.SEGIDX_FOUND).sum()), iters=reps),
            plan_ms=t["plan"], run_ms=t["run"], hydrate_ms=t["hydrate"], find_ms=t["find"],
            spread={k: max(v) / min(v) - 1 for k, v in t.items()},
            run_gb_per_s=out_cap / min(t["run"]) / 1e6, hydrate_gb_per_s=out_cap / min(t["hydrate"]) / 1e6)), flush=True)
        del d_out, d_ent, d_hent

    # ---- track from empty states beside rpgpu_segment_index_device
    per = 61 + a.records * (16 + a.value + 12)
    nb = int(a.gib * (1 << 30)) // per
    spec = engine.make_spec(seed=a.seed, partitions=1, records_per_batch=a.records, key_len=16, value_len=a.value,
                            format=abi.FMT_RP_DISK, ops=abi.OP_CRC | abi.OP_HDRCRC)
    data, descs = engine.build_arena(spec, nb)
    d_data = torch.from_numpy(data).to(dev)
    d_descs = up(descs)
    d_res = torch.zeros(nb * 64, dtype=torch.uint8, device=dev)
    d_used = torch.zeros(1, dtype=torch.int64, device=dev)
    d_vscr = torch.zeros(eng.scratch_bytes(nb), dtype=torch.uint8, device=dev)
    eng.validate_device(d_descs.data_ptr(), nb, d_data.data_ptr(), d_res.data_ptr(), 0, 0, d_used.data_ptr(),
                        d_vscr.data_ptr(), sh)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(abi.RESULT_DTYPE)
    assert (res["verdict"] == 0).all()
    del d_vscr, d_data
    base = res["base_offset"].astype(np.int64)
    for ns in [int(s) for s in a.segments.split(",") if s]:
        first = (np.arange(ns, dtype=np.uint64) * nb // ns).astype(np.uint32)
        count = np.diff(np.append(first, nb)).astype(np.uint32)
        segs = np.zeros(ns, dtype=abi.SEGMENT_DTYPE)
        segs["first_batch"], segs["batch_count"], segs["base_offset"] = first, count, base[first]
        segs["file_base"], segs["step"], segs["with_offset"] = descs["offset"][first], a.step, 1
        fresh = np.zeros(ns, dtype=abi.SEGIDX_STATE_DTYPE)
        fresh["base_offset"], fresh["with_offset"], fresh["monotonic"] = base[first], 1, 1
        fresh["last_batch_max_timestamp"] = -1
        fresh["entry_first"], fresh["entry_cap"] = first, count  # the yardstick's slots: one row per batch
        d_segs, d_fresh = up(segs), up(fresh)
        d_pool = torch.zeros(a.pool * ns * 80, dtype=torch.uint8, device=dev)
        turn = [0]
        d_trk = torch.zeros(ns * 16, dtype=torch.uint8, device=dev)
        d_entries = torch.zeros(nb * 16, dtype=torch.uint8, device=dev)
        d_ystates = torch.zeros(ns * 48, dtype=torch.uint8, device=dev)
        d_yentries = torch.zeros(nb * 16, dtype=torch.uint8, device=dev)

        def refill():
            d_pool.view(a.pool, ns * 80).copy_(d_fresh)
            turn[0] = 0

        def track():
            rows = d_pool.data_ptr() + (turn[0] % a.pool) * ns * 80
            turn[0] += 1
            ok(L.rpgpu_segidx_track_device(eng.ctx, d_descs.data_ptr(), d_res.data_ptr(), nb, d_segs.data_ptr(), ns,
                                           rows, d_entries.data_ptr(), nb, d_trk.data_ptr(), sh))

        def yardstick():
            ok(L.rpgpu_segment_index_device(eng.ctx, d_descs.data_ptr(), d_res.data_ptr(), d_segs.data_ptr(), ns,
                                            d_ystates.data_ptr(), d_yentries.data_ptr(), sh))

        refill()
        t, reps = measure((("track", track), ("segment_index", yardstick)), prepare=refill, cap=a.pool - a.warmup)
        assert turn[0] <= a.pool, "every timed call had fresh rows"
        refill()  # the yardstick's last run refilled the pool too
        track()
        torch.cuda.synchronize()
        st = d_pool.cpu().numpy()[:ns * 80].view(abi.SEGIDX_STATE_DTYPE)
        yst = d_ystates.cpu().numpy().view(abi.SEGMENT_STATE_DTYPE)
        trk = d_trk.cpu().numpy().view(abi.SEGIDX_TRACKED_DTYPE)
        assert (trk["status"] == 0).all() and np.array_equal(trk["tracked"], yst["tracked"])
        assert np.array_equal(st["entries"], yst["entries"]) and np.array_equal(st["max_timestamp"], yst["max_timestamp"])
        e, ye = d_entries.cpu().numpy().view(abi.INDEX_ENTRY_DTYPE), d_yentries.cpu().numpy().view(abi.INDEX_ENTRY_DTYPE)
        live = np.concatenate([np.arange(f, f + c) for f, c in zip(first, st["entries"])])
        assert np.array_equal(e[live], ye[live])
        print(json.dumps(dict(
            segments=ns, workload=dict(batches=nb, step=a.step, entries=int(st["entries"].sum()), iters=reps),
            track_ms=t["track"], segment_index_ms=t["segment_index"],
            spread={k: max(v) / min(v) - 1 for k, v in t.items()},
            track_over_segment_index=min(t["track"]) / min(t["segment_index"]))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
