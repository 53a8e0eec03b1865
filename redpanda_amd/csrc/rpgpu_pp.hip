// rpgpu_pp.hip — the REST proxy's fetch reply on the device:
// rjson_serialize_impl<kafka::fetch_response> (pandaproxy/json/requests/fetch.h:94-154)
// over validated and indexed batches.  Sizes, verdicts, base64, decimals and
// the object writer are the host/device functions of rpgpu_pp.h.
//
// Plan
//   pp_ranges_kernel    one wave per response, 64 ranges per trip: each range's
//                       response and its own defect (topic, bounds).
//   pp_batch_kernel     one wave per batch, 64 records per trip: what the batch
//                       does to its response (batch_status) and the sum of its
//                       records' variable object bytes; each index entry is
//                       read once.
//   pp_range_kernel     one wave per range, 64 batches per trip: each batch's
//                       offset in the range (adding what the range decides:
//                       topic, partition, lead byte), the batch's range, the
//                       range's bytes and records.
//   pp_response_kernel  one wave per response: each range's offset in the
//                       response, then the result row from the totals and
//                       from the response's smallest event key.
//   block_scan_kernel   the slots: an exclusive scan of the 16-byte rounded
//                       lengths (rpgpu_kernels.hip), then pp_publish_kernel.
// A defect is an atomicMin of (range position, 0 | 1 + batch position) on the
// response's key, so its first offender wins whatever the scheduling.
// Run
//   pp_open_kernel      the result rows again (NO_ROOM against out_cap), ']'
//                       and the '[' of an empty array.
//   pp_emit_kernel<0>   one wave per batch, a lane per record: lead byte,
//                       skeleton, topic, the two integers and every key or
//                       value of at most lane_max bytes.  A batch holding a
//                       longer field goes on the work list, one atomic per wave.
//   pp_emit_kernel<1>   the listed batches, a wave each: the same walk finds
//                       the places, then every long field is encoded by the
//                       whole wave, 12 bytes to 16 characters per lane and step
//                       (b64_encode_wave).
// The list names batches, not fields: the scratch is sized by batches, ranges
// and responses, none of which bounds the number of records.
// Bound: HBM.  Key and value bytes and 32 B of index per record are read
// (the index twice: plan and run), 4/3 of the field bytes and the skeleton
// are written.
#include "rpgpu_device.h"
#include "rpgpu_launch.h"
#include "rpgpu_scan.h"
#include "rpgpu_pp.h"

namespace rpgpu {

namespace {

using rppp::kNone;

// scratch: 64 B (the work list's length) | b_off[n] | r_off[nranges] | key[nresponses] |
//          slot[nresponses] (u64 each) | plan_res[nresponses] | b_recs, b_stat, b_range, list [n] |
//          r_recs, r_resp, r_stat [nranges] (u32 each)
struct Parts {
    uint64_t* count;
    uint64_t *b_off, *r_off, *key, *slot;
    rpgpu_pp_result* plan_res;
    uint32_t *b_recs, *b_stat, *b_range, *list;
    uint32_t *r_recs, *r_resp, *r_stat;
};
size_t scratch_bytes(uint32_t n, uint32_t nranges, uint32_t nresponses) {
    return 64 + (size_t)n * (8 + 4 * 4) + (size_t)nranges * (8 + 3 * 4) +
           (size_t)nresponses * (8 + 8 + sizeof(rpgpu_pp_result));
}
Parts parts(void* d_scratch, uint32_t n, uint32_t nranges, uint32_t nresponses) {
    uint8_t* sc = static_cast<uint8_t*>(d_scratch);
    Parts p;
    p.count = reinterpret_cast<uint64_t*>(sc);
    p.b_off = reinterpret_cast<uint64_t*>(sc + 64);
    p.r_off = p.b_off + n;
    p.key = p.r_off + nranges;
    p.slot = p.key + nresponses;
    p.plan_res = reinterpret_cast<rpgpu_pp_result*>(p.slot + nresponses);
    p.b_recs = reinterpret_cast<uint32_t*>(p.plan_res + nresponses);
    p.b_stat = p.b_recs + n;
    p.b_range = p.b_stat + n;
    p.list = p.b_range + n;
    p.r_recs = p.list + n;
    p.r_resp = p.r_recs + nranges;
    p.r_stat = p.r_resp + nranges;
    return p;
}
static_assert(sizeof(rpgpu_pp_result) == 32 && sizeof(rpgpu_pp_range) == 24 && sizeof(rpgpu_pp_response) == 8,
              "ABI layouts");

__device__ __forceinline__ uint32_t wave_index() { return (blockIdx.x * blockDim.x + threadIdx.x) >> 6; }
__device__ __forceinline__ uint32_t wave_count() { return (gridDim.x * blockDim.x) >> 6; }
__device__ __forceinline__ unsigned long long* ull(uint64_t* p) { return reinterpret_cast<unsigned long long*>(p); }

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

__global__ __launch_bounds__(256) void pp_ranges_kernel(const rpgpu_pp_range* __restrict__ ranges, uint32_t nranges,
                                                        const rpgpu_pp_response* __restrict__ responses,
                                                        uint32_t nresponses, const uint8_t* __restrict__ topics,
                                                        uint32_t topics_len, uint32_t n, Parts p) {
    const uint32_t l = lane_id();
    for (uint32_t r = wave_index(); r < nresponses; r += wave_count()) {
        const rpgpu_pp_response R = responses[r];
        if ((uint64_t)R.first_range + R.range_count > nranges) continue;  // pp_response_kernel reports it
        for (uint64_t c = 0; c < R.range_count; c += 64) {
            const uint64_t pos = c + l;
            if (pos >= R.range_count) continue;
            const uint32_t g = R.first_range + (uint32_t)pos;
            const int32_t st = rppp::range_status(ranges[g], topics, topics_len, n);
            p.r_resp[g] = r;
            p.r_stat[g] = (uint32_t)st;
            if (st != RPGPU_PP_OK) atomicMin(ull(p.key + r), (unsigned long long)rppp::event_key((uint32_t)pos, 0));
        }
    }
}

__global__ __launch_bounds__(256) void pp_batch_kernel(const rpgpu_batch_result* __restrict__ results, uint32_t n,
                                                       const rpgpu_record_index* __restrict__ index, Parts p) {
    const uint32_t l = lane_id();
    for (uint32_t b = wave_index(); b < n; b += wave_count()) {
        const rpgpu_batch_result r = results[b];
        uint32_t recs;
        const int32_t st = rppp::batch_status(r, &recs);
        uint64_t var = 0;
        for (uint64_t c = 0; c < recs; c += 64)
            if (c + l < recs) var += rppp::object_var(index[(uint64_t)r.index_first + c + l]);
        var = wave_sum(var);
        if (l == 0) {
            p.b_off[b] = var;
            p.b_recs[b] = recs;
            p.b_stat[b] = (uint32_t)st;
            p.b_range[b] = kNone;
        }
    }
}

__global__ __launch_bounds__(256) void pp_range_kernel(const rpgpu_pp_range* __restrict__ ranges, uint32_t nranges,
                                                       const rpgpu_pp_response* __restrict__ responses, Parts p) {
    const uint32_t l = lane_id();
    for (uint32_t g = wave_index(); g < nranges; g += wave_count()) {
        const uint32_t r = p.r_resp[g];
        uint64_t run = 0;
        uint32_t recs = 0;
        if (r != kNone && p.r_stat[g] == RPGPU_PP_OK) {
            const rpgpu_pp_range rg = ranges[g];
            const uint32_t pos = g - responses[r].first_range;
            const uint64_t each = 1ull + rppp::object_fixed(rg.topic_len, rg.partition);
            for (uint64_t c = 0; c < rg.count; c += 64) {
                const uint64_t j = c + l;
                const bool live = j < rg.count;
                const uint32_t b = rg.first + (uint32_t)j;
                uint64_t sz = 0;
                uint32_t rc = 0, st = RPGPU_PP_OK;
                if (live) {
                    rc = p.b_recs[b];
                    st = p.b_stat[b];
                    sz = p.b_off[b] + rc * each;
                }
                const uint64_t bad = __ballot(live && st != RPGPU_PP_OK);
                if (bad) {  // the response has failed: its first offender, nothing behind it
                    if (l == (uint32_t)__builtin_ctzll(bad))
                        atomicMin(ull(p.key + r), (unsigned long long)rppp::event_key(pos, (uint32_t)j + 1));
                    break;
                }
                const uint64_t inc = wave_scan_incl(sz, l);
                if (live) {
                    p.b_off[b] = run + inc - sz;
                    p.b_range[b] = g;
                }
                run += __shfl(inc, 63, 64);
                recs += (uint32_t)wave_sum(rc);
            }
        }
        if (l == 0) {
            p.r_off[g] = run;
            p.r_recs[g] = recs;
        }
    }
}

__global__ __launch_bounds__(256) void pp_response_kernel(const rpgpu_pp_range* __restrict__ ranges, uint32_t nranges,
                                                          const rpgpu_pp_response* __restrict__ responses,
                                                          uint32_t nresponses, Parts p) {
    const uint32_t l = lane_id();
    for (uint32_t r = wave_index(); r < nresponses; r += wave_count()) {
        const rpgpu_pp_response R = responses[r];
        const bool past = (uint64_t)R.first_range + R.range_count > nranges;
        uint64_t run = 0;
        uint32_t recs = 0;
        for (uint64_t c = 0; !past && c < R.range_count; c += 64) {
            const uint64_t pos = c + l;
            const bool live = pos < R.range_count;
            const uint32_t g = R.first_range + (uint32_t)pos;
            const uint64_t sz = live ? p.r_off[g] : 0;
            const uint32_t rc = live ? p.r_recs[g] : 0;
            const uint64_t inc = wave_scan_incl(sz, l);
            if (live) p.r_off[g] = run + inc - sz;
            run += __shfl(inc, 63, 64);
            recs += (uint32_t)wave_sum(rc);
        }
        if (l != 0) continue;
        rpgpu_pp_result res = {0, 0, 0, RPGPU_PP_OK, 0, 0};
        const uint64_t key = p.key[r];
        if (past) {
            res.status = RPGPU_PP_BAD_RANGE;
            res.bad_batch = nranges;
        } else if (key != rppp::kNoEvent) {
            const uint32_t g = R.first_range + (uint32_t)(key >> 32), sub = (uint32_t)key;
            if (sub == 0) {
                res.status = (int32_t)p.r_stat[g];
                res.bad_batch = g;
            } else {
                res.bad_batch = ranges[g].first + sub - 1;
                res.status = (int32_t)p.b_stat[res.bad_batch];
            }
        } else {
            res.out_len = rppp::response_len(run);
            res.records = recs;
        }
        p.slot[r] = rppp::slot_size(res.out_len);
        p.plan_res[r] = res;
    }
}

__global__ __launch_bounds__(256) void pp_publish_kernel(Parts p, uint32_t nresponses, rpgpu_pp_result* out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nresponses) return;
    rpgpu_pp_result res = p.plan_res[r];
    res.out_off = p.slot[r];
    p.plan_res[r] = res;
    out[r] = res;
}

__global__ __launch_bounds__(256) void pp_open_kernel(Parts p, uint32_t nresponses, uint8_t* __restrict__ out,
                                                      uint64_t out_cap, rpgpu_pp_result* results) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nresponses) return;
    rpgpu_pp_result res = p.plan_res[r];
    if (res.status == RPGPU_PP_OK) {
        if (res.out_off + rppp::slot_size(res.out_len) > out_cap) {
            res.status = RPGPU_PP_NO_ROOM;
        } else {
            if (res.records == 0) out[res.out_off] = '[';
            out[res.out_off + res.out_len - 1] = ']';
        }
    }
    results[r] = res;
}

// a value every lane holds, as a wave-uniform one
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32)) << 32) |
           (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
}

// kWave 0: every batch, the objects.  kWave 1: the listed batches, their long fields.
template <int kWave>
__global__ __launch_bounds__(256) void pp_emit_kernel(const uint8_t* __restrict__ data,
                                                      const rpgpu_batch_desc* __restrict__ descs,
                                                      const rpgpu_batch_result* __restrict__ results, uint32_t n,
                                                      const rpgpu_record_index* __restrict__ index,
                                                      const uint8_t* __restrict__ topics,
                                                      const rpgpu_pp_range* __restrict__ ranges, Parts p,
                                                      const rpgpu_pp_result* __restrict__ pres, uint8_t* out,
                                                      uint32_t lane_max) {
    const uint32_t l = lane_id();
    const uint32_t work = kWave ? (uint32_t)*p.count : n;
    for (uint32_t w = wave_index(); w < work; w += wave_count()) {
        const uint32_t b = kWave ? p.list[w] : w;
        const uint32_t g = p.b_range[b], recs = p.b_recs[b];
        if (g == kNone || recs == 0) continue;
        const rpgpu_pp_result res = pres[p.r_resp[g]];
        if (res.status != RPGPU_PP_OK) continue;
        const rpgpu_pp_range rg = ranges[g];
        const uint8_t* topic = topics + rg.topic_off;
        const uint8_t* batch = data + descs[b].offset;
        const uint64_t each = 1ull + rppp::object_fixed(rg.topic_len, rg.partition);
        const uint64_t range_off = p.r_off[g];
        uint8_t* base = out + res.out_off + range_off;  // the range's first lead byte
        const rpgpu_record_index* ix = index + results[b].index_first;
        uint64_t run = p.b_off[b];
        bool any_long = false;
        for (uint64_t c = 0; c < recs; c += 64) {
            const bool live = c + l < recs;
            rpgpu_record_index e = {0, 0, 0, 0, 0, 0};
            if (live) e = ix[c + l];
            const uint64_t sz = live ? rppp::object_var(e) + each : 0;
            const uint64_t inc = wave_scan_incl(sz, l);
            const uint64_t at = run + inc - sz;
            run += __shfl(inc, 63, 64);
            rppp::Fields f = {nullptr, nullptr};
            if (live) f = rppp::locate_fields(base + at, rg.topic_len, e, lane_max);
            if (!kWave) {
                if (live)
                    (void)rppp::put_object(base + at, rppp::lead_byte(range_off, at), topic, rg.topic_len,
                                           rg.partition, e, batch, lane_max);
                any_long = any_long || __ballot(f.kdst || f.vdst) != 0;
                continue;
            }
            // the long keys, then the long values, each by the whole wave
            for (int kv = 0; kv < 2; kv++) {
                uint8_t* dst = kv ? f.vdst : f.kdst;
                const uint8_t* src = batch + (kv ? e.val_off : e.key_off);
                const uint32_t len = (uint32_t)(kv ? e.val_len : e.key_len);
                for (uint64_t m = __ballot(dst != nullptr); m; m &= m - 1) {
                    const int from = __builtin_ctzll(m);
                    rppp::b64_encode_wave((uint8_t*)uniform64(__shfl((uint64_t)dst, from, 64)),
                                          (const uint8_t*)uniform64(__shfl((uint64_t)src, from, 64)),
                                          (uint32_t)__builtin_amdgcn_readfirstlane((int)__shfl(len, from, 64)), l);
                }
            }
        }
        if (!kWave && any_long && l == 0) p.list[atomicAdd(ull(p.count), 1ull)] = b;
    }
}

uint32_t wave_blocks(uint64_t waves) {
    const uint64_t want = (waves * 64 + 255) / 256;
    return (uint32_t)(want < 1 ? 1 : want < 16384 ? want : 16384);
}

}  // namespace

size_t pp_fetch_scratch_bytes(uint32_t n, uint32_t nranges, uint32_t nresponses) {
    return scratch_bytes(n, nranges, nresponses);
}

hipError_t launch_pp_fetch_plan(const rpgpu_batch_result* d_results, uint32_t n, const rpgpu_record_index* d_index,
                                const uint8_t* d_topics, uint32_t topics_len, const rpgpu_pp_range* d_ranges,
                                uint32_t nranges, const rpgpu_pp_response* d_responses, uint32_t nresponses,
                                rpgpu_pp_result* d_out_results, uint64_t* d_out_bytes, void* d_scratch,
                                hipStream_t s) {
    if (nresponses == 0) return d_out_bytes ? hipMemsetAsync(d_out_bytes, 0, sizeof(uint64_t), s) : hipSuccess;
    const Parts p = parts(d_scratch, n, nranges, nresponses);
    hipError_t e;
    if ((e = hipMemsetAsync(p.key, 0xff, (size_t)nresponses * 8, s)) != hipSuccess) return e;
    if (nranges && (e = hipMemsetAsync(p.r_resp, 0xff, (size_t)nranges * 4, s)) != hipSuccess) return e;
    pp_ranges_kernel<<<wave_blocks(nresponses), 256, 0, s>>>(d_ranges, nranges, d_responses, nresponses, d_topics,
                                                            topics_len, n, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (n) {
        pp_batch_kernel<<<wave_blocks(n), 256, 0, s>>>(d_results, n, d_index, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (nranges) {
        pp_range_kernel<<<wave_blocks(nranges), 256, 0, s>>>(d_ranges, nranges, d_responses, p);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    pp_response_kernel<<<wave_blocks(nresponses), 256, 0, s>>>(d_ranges, nranges, d_responses, nresponses, p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = launch_block_scan(p.slot, nresponses, d_out_bytes, s)) != hipSuccess) return e;
    pp_publish_kernel<<<(nresponses + 255) / 256, 256, 0, s>>>(p, nresponses, d_out_results);
    return hipGetLastError();
}

hipError_t launch_pp_fetch_run(const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                               const rpgpu_batch_result* d_results, uint32_t n, const rpgpu_record_index* d_index,
                               const uint8_t* d_topics, const rpgpu_pp_range* d_ranges, uint32_t nranges,
                               const rpgpu_pp_response* d_responses, uint32_t nresponses, uint8_t* d_out,
                               uint64_t out_cap, rpgpu_pp_result* d_out_results, void* d_scratch, uint32_t lane_max,
                               hipStream_t s) {
    (void)d_responses;
    if (nresponses == 0) return hipSuccess;
    const Parts p = parts(d_scratch, n, nranges, nresponses);
    hipError_t e;
    if ((e = hipMemsetAsync(p.count, 0, sizeof(uint64_t), s)) != hipSuccess) return e;
    pp_open_kernel<<<(nresponses + 255) / 256, 256, 0, s>>>(p, nresponses, d_out, out_cap, d_out_results);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (n == 0 || nranges == 0) return hipSuccess;
    pp_emit_kernel<0><<<wave_blocks(n), 256, 0, s>>>(d_data, d_descs, d_results, n, d_index, d_topics, d_ranges, p,
                                                    d_out_results, d_out, lane_max);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    pp_emit_kernel<1><<<wave_blocks(n), 256, 0, s>>>(d_data, d_descs, d_results, n, d_index, d_topics, d_ranges, p,
                                                    d_out_results, d_out, lane_max);
    return hipGetLastError();
}

}  // namespace rpgpu
