// rpgpu_produce.hip — produce batches from records on the device:
// kafka::client::client::produce_records (kafka/client/client.cc:231-271) over
// many requests (include/rpgpu.h, "produce batches from records").  The
// partitioners, murmur2, the record sizes and the guard rails are the
// host/device functions of rpgpu_produce.h; the record writer is rpgpu_emit.h,
// shared with the legacy conversion; DESIGN.md §3 has the argument.
//
// Plan:
//   produce_requests_kernel   one workgroup: the scan of the requests' nrows
//                             (where each request's rows begin), the guard
//                             rails on the requests themselves.
//   produce_partition_kernel  one lane per row: its request (a binary search
//                             in that scan), the row's guard rails, rules 1 and
//                             2 (murmur2 is a serial multiply / xor chain per
//                             key: one lane per key, so its time follows the
//                             longest key, not the bytes), the flag of a rule-3
//                             row and the block scan of the flags.
//   produce_keys_kernel       one lane per row: k = the flags' scan minus its
//                             value at the request's first row, rule 3, the
//                             sort key; the request's last row leaves rr_next.
//   radix_sort_items          (rpgpu_sort.h) twice, chained: the rows by
//                             partition id biased by 2^31, then by request.
//                             Stable, so a group keeps request order.
//   produce_heads_kernel      one lane per sorted position: head flags where
//                             (request, partition) changes, their block scan.
//   produce_groups_kernel     the group of each position, each group's head.
//   produce_sizes_kernel      offset delta = position - head, the record's
//                             bytes, their block scan; the tail leaves the count.
//   produce_bodies_kernel     one lane per group: the body, TOO_LARGE.
//   produce_slots_kernel      one lane per group: the 64-byte aligned slot and
//                             the batch number of the requests still OK, their
//                             block scans.
//   produce_ends_kernel       one lane per group: each request's first and last
//                             batch and where the last ends; *d_out_bytes,
//                             *d_nbatches.
// Run:
//   produce_results_kernel    one workgroup: which requests fit out_cap, the
//                             scan of their batch counts, the result rows.
//   produce_finish_kernel     one lane per batch row: the header with zero
//                             CRCs, the descriptor, the rpgpu_produce_batch row;
//                             the unused rows.
//   produce_emit_kernel       64 records per wave (emit_record_lane), the row
//                             maps; long keys / values are listed.
//   produce_copy_wave_kernel  the listed keys and values, a wave each.
//   then launch_revalidate (rpgpu_rewrite.h): both CRCs, the result rows and
//   the index.
//
// The run changes nothing the plan left in the scratch, so a plan may be run
// any number of times.
#include <type_traits>

#include "rpgpu_device.h"
#include "rpgpu_launch.h"
#include "rpgpu_rewrite.h"
#include "rpgpu_scan.h"
#include "rpgpu_sort.h"
#include "rpgpu_emit.h"
#include "rpgpu_produce.h"

namespace rpgpu {
namespace {

using rpproduce::kNone;

static_assert(sizeof(rpgpu_produce_row) == 32 && sizeof(rpgpu_produce_request) == 24 &&
                  sizeof(rpgpu_produce_result) == 16 && sizeof(rpgpu_produce_batch) == 32,
              "produce row layouts");

enum : int { kRowSum = 0, kGroups = 1, kBodyBytes = 2, kSlotBytes = 3, kBatches = 4, kLong = 5, kEmitted = 6 };

struct PParts {
    uint64_t* totals;  // kRowSum .. kEmitted
    // per request
    uint64_t *req_first, *req_end, *run_nb, *run_first;
    int32_t* status;
    uint32_t *rr_count, *req_gfirst, *req_glast;
    // per row / sorted position / group
    uint64_t *sz_local, *g_body, *slot_sz, *slot_local, *list;
    uint32_t *row_req, *key_part, *idx_a, *idx_b, *rr_local, *head_local, *pos_group, *g_head, *g_count, *g_req;
    uint32_t *emitf, *fin_local;
    int32_t* part;
    // per block of kScanBlock rows
    uint64_t *rr_bsum, *head_bsum, *sz_bsum, *slot_bsum, *fin_bsum;
    uint32_t* table;
    void* vscratch;
};
size_t pr_al(size_t x) { return (x + 255) & ~(size_t)255; }
uint32_t scan_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + kScanBlock - 1) / kScanBlock); }
size_t pr_layout(void* base, uint32_t n, uint32_t nreq, PParts* out) {
    uint8_t* b = static_cast<uint8_t*>(base);
    size_t o = 0;
    PParts p;
    const size_t nb = scan_blocks(n);
    auto take = [&](auto*& ptr, size_t count) {
        ptr = reinterpret_cast<std::remove_reference_t<decltype(ptr)>>(b + o);
        o += pr_al(count * sizeof(*ptr));
    };
    take(p.totals, 8);
    take(p.req_first, nreq), take(p.req_end, nreq), take(p.run_nb, nreq), take(p.run_first, nreq);
    take(p.status, nreq), take(p.rr_count, nreq), take(p.req_gfirst, nreq), take(p.req_glast, nreq);
    take(p.sz_local, n), take(p.g_body, n), take(p.slot_sz, n), take(p.slot_local, n), take(p.list, 2 * (size_t)n);
    take(p.row_req, n), take(p.key_part, n), take(p.idx_a, n), take(p.idx_b, n), take(p.rr_local, n);
    take(p.head_local, n), take(p.pos_group, n), take(p.g_head, n), take(p.g_count, n), take(p.g_req, n);
    take(p.emitf, n), take(p.fin_local, n), take(p.part, n);
    take(p.rr_bsum, nb), take(p.head_bsum, nb), take(p.sz_bsum, nb), take(p.slot_bsum, nb), take(p.fin_bsum, nb);
    take(p.table, (size_t)sort_blocks(n) * 256);
    p.vscratch = b + o;
    if (out) *out = p;
    return o;
}

// a request keeps the first status that applies: later stages only replace OK
__device__ __forceinline__ void refuse(int32_t* status, int32_t why) { atomicCAS(status, RPGPU_PRODUCE_OK, why); }

__global__ __launch_bounds__(kScanBlock) void produce_requests_kernel(const rpgpu_produce_request* __restrict__ reqs,
                                                                      uint32_t nreq, uint32_t n, PParts p) {
    __shared__ uint64_t part[kScanBlock];
    for (uint32_t r = threadIdx.x; r < nreq; r += kScanBlock) p.req_first[r] = reqs[r].nrows;
    __syncthreads();
    const uint64_t sum = array_scan_excl(p.req_first, p.req_first, nreq, part);
    for (uint32_t r = threadIdx.x; r < nreq; r += kScanBlock) {
        p.status[r] = (sum != n || !rpproduce::request_ok(reqs[r])) ? RPGPU_PRODUCE_BAD_REQUEST : RPGPU_PRODUCE_OK;
        p.rr_count[r] = 0;
        p.req_end[r] = 0;
        p.req_gfirst[r] = 0;
        p.req_glast[r] = kNone;
    }
    if (threadIdx.x == 0) p.totals[kRowSum] = sum;
}

__global__ __launch_bounds__(kScanBlock) void produce_partition_kernel(const rpgpu_produce_row* __restrict__ rows,
                                                                       uint32_t n,
                                                                       const rpgpu_produce_request* __restrict__ reqs,
                                                                       uint32_t nreq, const uint8_t* __restrict__ data,
                                                                       uint64_t data_bytes, PParts p) {
    __shared__ uint32_t wsum[kScanBlock / 64];
    const uint64_t i = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t flag = 0;
    if (i < n) {
        uint32_t r = kNone;
        int32_t partition = 0;
        if (p.totals[kRowSum] == n) {  // else no row has a request: the whole call is refused
            uint32_t lo = 0, hi = nreq;  // the last request that begins at or in front of row i
            while (hi - lo > 1) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (p.req_first[mid] <= i) lo = mid;
                else hi = mid;
            }
            r = lo;
            if (p.status[r] == RPGPU_PRODUCE_OK) {
                const rpgpu_produce_row row = rows[i];
                if (!rpproduce::row_ok(row, data_bytes)) refuse(p.status + r, RPGPU_PRODUCE_BAD_ROW);
                else flag = rpproduce::row_rule(row, data, reqs[r].partition_count, &partition) == rpproduce::kRuleRoundRobin;
            }
        }
        p.row_req[i] = r;
        p.part[i] = partition;
        p.key_part[i] = flag;  // until produce_keys_kernel
    }
    const uint32_t e = block_scan_excl(flag, wsum, p.rr_bsum);
    if (i < n) p.rr_local[i] = e;
}

__global__ __launch_bounds__(256) void produce_keys_kernel(uint32_t n, const rpgpu_produce_request* __restrict__ reqs,
                                                           PParts p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = p.row_req[i];
    int32_t partition = p.part[i];
    if (r != kNone) {
        const rpgpu_produce_request q = reqs[r];
        const uint32_t first = (uint32_t)p.req_first[r];
        const uint32_t flag = p.key_part[i];
        const uint32_t k = (uint32_t)(slot_offset(p.rr_bsum, p.rr_local, i) - slot_offset(p.rr_bsum, p.rr_local, first));
        if (flag) partition = rpproduce::round_robin(q.rr_initial, k, q.partition_count);
        if (i == first + q.nrows - 1) {  // the request's last row: what rr_next adds
            p.rr_count[r] = k + flag;
            if ((uint64_t)(uint32_t)q.rr_initial + k + flag > 0x7fffffffull) refuse(p.status + r, RPGPU_PRODUCE_BAD_REQUEST);
        }
    }
    p.part[i] = partition;
    p.key_part[i] = rpproduce::partition_key(partition);
}

// the row at a sorted position, and whether its request is still OK
__device__ __forceinline__ bool live_row(const PParts& p, uint32_t row, uint32_t* req) {
    const uint32_t r = p.row_req[row];
    *req = r;
    return r != kNone && p.status[r] == RPGPU_PRODUCE_OK;
}

__global__ __launch_bounds__(kScanBlock) void produce_heads_kernel(const uint32_t* __restrict__ sorted, uint32_t n,
                                                                   PParts p) {
    __shared__ uint32_t wsum[kScanBlock / 64];
    const uint64_t pos = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t head = 0;
    if (pos < n) {
        const uint32_t row = sorted[pos];
        uint32_t r;
        if (live_row(p, row, &r)) {
            head = 1;
            if (pos) {
                const uint32_t prev = sorted[pos - 1];
                head = p.row_req[prev] != r || p.part[prev] != p.part[row];
            }
        }
        p.pos_group[pos] = head;  // until produce_groups_kernel
    }
    const uint32_t e = block_scan_excl(head, wsum, p.head_bsum);
    if (pos < n) p.head_local[pos] = e;
}

__global__ __launch_bounds__(256) void produce_groups_kernel(const uint32_t* __restrict__ sorted, uint32_t n, PParts p) {
    const uint32_t pos = blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n) return;
    uint32_t r;
    if (!live_row(p, sorted[pos], &r)) {
        p.pos_group[pos] = kNone;
        return;
    }
    const uint32_t head = p.pos_group[pos];
    const uint32_t g = (uint32_t)slot_offset(p.head_bsum, p.head_local, pos) + head - 1;
    p.pos_group[pos] = g;
    if (head) {
        p.g_head[g] = pos;
        p.g_req[g] = r;
    }
}

__global__ __launch_bounds__(kScanBlock) void produce_sizes_kernel(const rpgpu_produce_row* __restrict__ rows,
                                                                   const uint32_t* __restrict__ sorted, uint32_t n,
                                                                   PParts p) {
    __shared__ uint64_t wsum[kScanBlock / 64];
    const uint64_t pos = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint64_t sz = 0;
    if (pos < n) {
        const uint32_t g = p.pos_group[pos];
        if (g != kNone) {
            const uint32_t delta = (uint32_t)pos - p.g_head[g];
            sz = rpproduce::record_bytes(delta, rows[sorted[pos]]);
            if (pos + 1 == n || p.pos_group[pos + 1] != g) p.g_count[g] = delta + 1;
        }
    }
    const uint64_t e = block_scan_excl(sz, wsum, p.sz_bsum);
    if (pos < n) p.sz_local[pos] = e;
}

// where the record at a sorted position begins in the bodies laid end to end
__device__ __forceinline__ uint64_t body_at(const PParts& p, uint32_t pos) { return slot_offset(p.sz_bsum, p.sz_local, pos); }

__global__ __launch_bounds__(256) void produce_bodies_kernel(uint32_t n, PParts p) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t groups = p.totals[kGroups];
    if (g >= n || g >= groups) return;
    const uint64_t start = body_at(p, p.g_head[g]);
    const uint64_t end = g + 1 < groups ? body_at(p, p.g_head[g + 1]) : p.totals[kBodyBytes];
    p.g_body[g] = end - start;
    if (!rpproduce::body_fits(end - start)) refuse(p.status + p.g_req[g], RPGPU_PRODUCE_TOO_LARGE);
}

__global__ __launch_bounds__(kScanBlock) void produce_slots_kernel(uint32_t n, PParts p) {
    __shared__ uint64_t wsum[kScanBlock / 64];
    __shared__ uint32_t wcnt[kScanBlock / 64];
    const uint64_t g = (uint64_t)blockIdx.x * kScanBlock + threadIdx.x;
    uint64_t sz = 0;
    uint32_t ok = 0;
    if (g < n && g < p.totals[kGroups]) {
        ok = p.status[p.g_req[g]] == RPGPU_PRODUCE_OK;
        sz = ok ? ((uint64_t)kHeaderSize + p.g_body[g] + 63) & ~(uint64_t)63 : 0;
    }
    const uint64_t at = block_scan_excl(sz, wsum, p.slot_bsum);
    const uint32_t nth = block_scan_excl(ok, wcnt, p.fin_bsum);
    if (g < n) {
        p.slot_sz[g] = sz;
        p.slot_local[g] = at;
        p.emitf[g] = ok;
        p.fin_local[g] = nth;
    }
}
// a group's slot in d_out and its batch number (emitted groups only)
__device__ __forceinline__ uint64_t slot_at(const PParts& p, uint32_t g) { return slot_offset(p.slot_bsum, p.slot_local, g); }
__device__ __forceinline__ uint32_t batch_of(const PParts& p, uint32_t g) {
    return (uint32_t)slot_offset(p.fin_bsum, p.fin_local, g);
}

// the batches of a request: rows [number of its first group, number of its last] and where the last ends
__global__ __launch_bounds__(256) void produce_ends_kernel(uint32_t n, PParts p, uint64_t* out_bytes,
                                                           uint32_t* nbatches) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g == 0) {
        if (out_bytes) *out_bytes = p.totals[kSlotBytes];
        if (nbatches) *nbatches = (uint32_t)p.totals[kBatches];
    }
    const uint64_t groups = p.totals[kGroups];
    if (g >= n || g >= groups || !p.emitf[g]) return;
    const uint32_t r = p.g_req[g];
    if (g == 0 || p.g_req[g - 1] != r) p.req_gfirst[r] = batch_of(p, g);
    if (g + 1 == groups || p.g_req[g + 1] != r) {
        p.req_glast[r] = batch_of(p, g);
        p.req_end[r] = slot_at(p, g) + p.slot_sz[g];
    }
}

__global__ __launch_bounds__(kScanBlock) void produce_results_kernel(const rpgpu_produce_request* __restrict__ reqs,
                                                                     uint32_t nreq, PParts p, uint64_t out_cap,
                                                                     rpgpu_produce_result* __restrict__ res) {
    __shared__ uint64_t part[kScanBlock];
    for (uint32_t r = threadIdx.x; r < nreq; r += kScanBlock) {
        int32_t st = p.status[r];
        const bool has = st == RPGPU_PRODUCE_OK && p.req_glast[r] != kNone;
        // the validation reads up to the tail pad past a batch
        if (has && p.req_end[r] + RPGPU_ARENA_TAIL_PAD > out_cap) st = RPGPU_PRODUCE_OUT_OVERFLOW;
        res[r].status = st;
        p.run_nb[r] = has && st == RPGPU_PRODUCE_OK ? (uint64_t)(p.req_glast[r] - p.req_gfirst[r]) + 1 : 0;
    }
    __syncthreads();
    const uint64_t emitted = array_scan_excl(p.run_nb, p.run_first, nreq, part);
    for (uint32_t r = threadIdx.x; r < nreq; r += kScanBlock) {
        const bool ok = res[r].status == RPGPU_PRODUCE_OK;
        res[r].rr_next = reqs[r].rr_initial + (ok ? (int32_t)p.rr_count[r] : 0);
        res[r].first_batch = ok ? (uint32_t)p.run_first[r] : 0u;
        res[r].nbatches = (uint32_t)p.run_nb[r];
    }
    if (threadIdx.x == 0) {
        p.totals[kEmitted] = emitted;
        p.totals[kLong] = 0;
    }
}

__global__ __launch_bounds__(256) void produce_finish_kernel(uint32_t n, const rpgpu_produce_request* __restrict__ reqs,
                                                             PParts p, const uint32_t* __restrict__ sorted,
                                                             const rpgpu_produce_result* __restrict__ res,
                                                             rpgpu_produce_batch* __restrict__ batches,
                                                             uint8_t* __restrict__ out,
                                                             rpgpu_batch_desc* __restrict__ out_descs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (i >= p.totals[kEmitted]) {  // an unused row
        rpgpu_produce_batch b;
        b.request = kNone, b.partition = 0, b.record_count = 0, b.pad = 0, b.out_offset = 0, b.out_len = 0;
        batches[i] = b;
        out_descs[i] = out_desc(0, 0, 0, 0);
    }
    if (i >= p.totals[kGroups] || !p.emitf[i]) return;
    const uint32_t r = p.g_req[i];
    if (res[r].status != RPGPU_PRODUCE_OK) return;
    // the fitting requests are the first ones: their batch numbers are the plan's
    const uint32_t at = batch_of(p, i);
    rpgpu_produce_batch b;
    b.request = r;
    b.partition = p.part[sorted[p.g_head[i]]];
    b.record_count = p.g_count[i];
    b.pad = 0;
    b.out_offset = slot_at(p, i);
    b.out_len = (uint64_t)kHeaderSize + p.g_body[i];
    rplegacy::put_header(out + b.out_offset, (uint32_t)p.g_body[i], b.record_count, reqs[r].now_ms);
    batches[at] = b;
    out_descs[at] = out_desc(b.out_offset, (uint32_t)b.out_len, (uint32_t)b.partition,
                             (uint8_t)(RPGPU_OP_CRC | RPGPU_OP_HDRCRC | RPGPU_OP_RECRC | RPGPU_OP_PARSE | RPGPU_OP_INDEX));
}

// the record at a sorted position of an emitted batch
__device__ __forceinline__ RecordPlace place(const PParts& p, const rpgpu_produce_row& row, uint32_t pos, uint32_t g,
                                             const uint8_t* __restrict__ data, uint8_t* out, uint32_t* delta_out,
                                             uint32_t* rec_len_out) {
    const uint32_t hp = p.g_head[g];
    const uint32_t delta = pos - hp;
    const uint32_t rec_len = (uint32_t)rpproduce::record_len(delta, row);
    *delta_out = delta;
    *rec_len_out = rec_len;
    return place_record(out + slot_at(p, g) + kHeaderSize + (body_at(p, pos) - body_at(p, hp)), data + row.key_off,
                        data + row.val_off, rec_len, delta, rpproduce::encoded_key_len(row.key_len), row.val_len);
}
__device__ __forceinline__ bool emitted_pos(const PParts& p, const rpgpu_produce_result* __restrict__ res, uint32_t pos,
                                            uint32_t* g) {
    *g = p.pos_group[pos];
    return *g != kNone && res[p.g_req[*g]].status == RPGPU_PRODUCE_OK;
}

__global__ __launch_bounds__(256) void produce_emit_kernel(const rpgpu_produce_row* __restrict__ rows, uint32_t n,
                                                           const uint32_t* __restrict__ sorted,
                                                           const uint8_t* __restrict__ data, PParts p,
                                                           const rpgpu_produce_result* __restrict__ res, uint8_t* out,
                                                           uint32_t* __restrict__ row_batch,
                                                           uint32_t* __restrict__ row_delta) {
    const uint32_t l = lane_id();
    const uint64_t gw = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t base = gw * 64; base < n; base += nw * 64) {
        const uint64_t pos = base + l;
        bool klong = false, vlong = false;
        if (pos < n) {
            const uint32_t ri = sorted[pos];
            uint32_t g, batch = kNone, delta = kNone;
            if (emitted_pos(p, res, (uint32_t)pos, &g)) {
                const rpgpu_produce_row row = rows[ri];
                uint32_t rec_len;
                const RecordPlace q = place(p, row, (uint32_t)pos, g, data, out, &delta, &rec_len);
                emit_record_lane(q, rec_len, delta, rpproduce::encoded_key_len(row.key_len), row.val_len, klong, vlong);
                batch = batch_of(p, g);
            }
            row_batch[ri] = batch;
            row_delta[ri] = delta;
        }
        list_append(p.list, p.totals + kLong, klong, pos << 1, l);
        list_append(p.list, p.totals + kLong, vlong, (pos << 1) | 1, l);
    }
}

__global__ __launch_bounds__(256) void produce_copy_wave_kernel(const rpgpu_produce_row* __restrict__ rows,
                                                                const uint32_t* __restrict__ sorted,
                                                                const uint8_t* __restrict__ data, PParts p,
                                                                uint8_t* out) {
    const uint64_t count = p.totals[kLong];
    const uint32_t l = lane_id();
    const uint64_t gw = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t i = gw; i < count; i += nw) {
        const uint64_t item = p.list[i];
        const uint32_t pos = (uint32_t)(item >> 1);
        uint32_t delta, rec_len;
        const RecordPlace q = place(p, rows[sorted[pos]], pos, p.pos_group[pos], data, out, &delta, &rec_len);
        copy_listed(q, (item & 1) != 0, l);
    }
}

// the rows sorted by (request, partition id as a signed int32), stable
hipError_t sort_rows(const PParts& p, uint32_t n, uint32_t nreq, const uint32_t** sorted, hipStream_t s) {
    hipError_t e = radix_sort_items(p.key_part, n, 0xffffffffu, p.idx_a, p.idx_b, p.table, sorted, s);
    if (e != hipSuccess || nreq < 2) return e;
    // the second chain starts from the first one's order and must not scatter into it
    const bool in_a = *sorted == p.idx_a;
    return radix_sort_items(p.row_req, n, nreq - 1, in_a ? p.idx_b : p.idx_a, in_a ? p.idx_a : p.idx_b, p.table,
                            sorted, s, *sorted);
}
// where sort_rows leaves the result: a function of the pass counts alone
const uint32_t* sorted_rows(const PParts& p, uint32_t nreq) {
    const bool first_in_a = (sort_passes(0xffffffffu) & 1u) != 0;
    if (nreq < 2) return first_in_a ? p.idx_a : p.idx_b;
    const bool second_in_first = (sort_passes(nreq - 1) & 1u) != 0;  // an odd chain ends in its idx_a argument
    return second_in_first == first_in_a ? p.idx_b : p.idx_a;
}

}  // namespace

size_t produce_scratch_bytes(uint32_t nrows, uint32_t nrequests) {
    return pr_layout(nullptr, nrows, nrequests, nullptr) + validate_scratch_bytes(nrows);
}

hipError_t launch_produce_plan(const rpgpu_produce_row* d_rows, uint32_t n, const rpgpu_produce_request* d_requests,
                               uint32_t nreq, const uint8_t* d_data, uint64_t data_bytes, uint64_t* d_out_bytes,
                               uint32_t* d_nbatches, void* d_scratch, hipStream_t s) {
    PParts p;
    (void)pr_layout(d_scratch, n, nreq, &p);
    hipError_t e;
    if ((e = hipMemsetAsync(p.totals, 0, 8 * sizeof(uint64_t), s)) != hipSuccess) return e;
    if (nreq) {
        produce_requests_kernel<<<1, kScanBlock, 0, s>>>(d_requests, nreq, n, p);
        RPGPU_LAUNCH_CHECK();
    }
    if (n) {
        const uint32_t nsb = scan_blocks(n), nb = (n + 255) / 256;
        produce_partition_kernel<<<nsb, kScanBlock, 0, s>>>(d_rows, n, d_requests, nreq, d_data, data_bytes, p);
        RPGPU_LAUNCH_CHECK();
        if ((e = launch_block_scan(p.rr_bsum, nsb, nullptr, s)) != hipSuccess) return e;
        produce_keys_kernel<<<nb, 256, 0, s>>>(n, d_requests, p);
        RPGPU_LAUNCH_CHECK();
        const uint32_t* sorted = nullptr;
        if ((e = sort_rows(p, n, nreq, &sorted, s)) != hipSuccess) return e;
        if (sorted != sorted_rows(p, nreq)) return hipErrorUnknown;
        produce_heads_kernel<<<nsb, kScanBlock, 0, s>>>(sorted, n, p);
        RPGPU_LAUNCH_CHECK();
        if ((e = launch_block_scan(p.head_bsum, nsb, p.totals + kGroups, s)) != hipSuccess) return e;
        produce_groups_kernel<<<nb, 256, 0, s>>>(sorted, n, p);
        RPGPU_LAUNCH_CHECK();
        produce_sizes_kernel<<<nsb, kScanBlock, 0, s>>>(d_rows, sorted, n, p);
        RPGPU_LAUNCH_CHECK();
        if ((e = launch_block_scan(p.sz_bsum, nsb, p.totals + kBodyBytes, s)) != hipSuccess) return e;
        produce_bodies_kernel<<<nb, 256, 0, s>>>(n, p);
        RPGPU_LAUNCH_CHECK();
    }
    if (n == 0) {
        if (d_out_bytes && (e = hipMemsetAsync(d_out_bytes, 0, sizeof(uint64_t), s)) != hipSuccess) return e;
        return d_nbatches ? hipMemsetAsync(d_nbatches, 0, sizeof(uint32_t), s) : hipSuccess;
    }
    const uint32_t nsb = scan_blocks(n);
    produce_slots_kernel<<<nsb, kScanBlock, 0, s>>>(n, p);
    RPGPU_LAUNCH_CHECK();
    if ((e = launch_block_scan(p.slot_bsum, nsb, p.totals + kSlotBytes, s)) != hipSuccess) return e;
    if ((e = launch_block_scan(p.fin_bsum, nsb, p.totals + kBatches, s)) != hipSuccess) return e;
    produce_ends_kernel<<<(n + 255) / 256, 256, 0, s>>>(n, p, d_out_bytes, d_nbatches);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_produce_run(const rpgpu_produce_row* d_rows, uint32_t n, const rpgpu_produce_request* d_requests,
                              uint32_t nreq, const uint8_t* d_data, rpgpu_produce_result* d_req_results,
                              rpgpu_produce_batch* d_batches, uint32_t* d_row_batch, uint32_t* d_row_delta,
                              uint8_t* d_out, uint64_t out_cap, rpgpu_batch_desc* d_out_descs,
                              rpgpu_batch_result* d_vres2, rpgpu_record_index* d_index, uint64_t index_cap,
                              uint64_t* d_index_used, void* d_scratch, const uint32_t* d_tables, int grid,
                              hipStream_t s) {
    PParts p;
    (void)pr_layout(d_scratch, n, nreq, &p);
    if (nreq) {
        produce_results_kernel<<<1, kScanBlock, 0, s>>>(d_requests, nreq, p, out_cap, d_req_results);
        RPGPU_LAUNCH_CHECK();
    }
    if (n == 0) return d_index_used ? hipMemsetAsync(d_index_used, 0, sizeof(uint64_t), s) : hipSuccess;
    const uint32_t* sorted = sorted_rows(p, nreq);
    produce_finish_kernel<<<(n + 255) / 256, 256, 0, s>>>(n, d_requests, p, sorted, d_req_results, d_batches, d_out,
                                                          d_out_descs);
    RPGPU_LAUNCH_CHECK();
    produce_emit_kernel<<<grid, 256, 0, s>>>(d_rows, n, sorted, d_data, p, d_req_results, d_out, d_row_batch,
                                             d_row_delta);
    RPGPU_LAUNCH_CHECK();
    produce_copy_wave_kernel<<<grid, 256, 0, s>>>(d_rows, sorted, d_data, p, d_out);
    RPGPU_LAUNCH_CHECK();
    return launch_revalidate(d_out_descs, n, d_out, d_batches, d_vres2, d_index, index_cap, d_index_used, p.vscratch,
                             d_tables, grid, s);
}

}  // namespace rpgpu
