// rpgpu_txfilter.hip — storage::internal::tx_reducer over the scopes of a
// validated, indexed arena (include/rpgpu.h, "aborted transactions ahead of
// compaction").  The per-batch decision, the consume position, the interval
// search and the producer hash live in rpgpu_txfilter.h, which the host program
// tests/native/txfilter_host.cpp compiles too; DESIGN.md §3 has the argument.
//
//   tx_classify_kernel  one wavefront per scope, 64 batches per trip: the
//                       classification of every batch from its result row, its
//                       header's producer identity and its control record's key;
//                       a ballot finds the first batch that stops the scope; a
//                       wave max-scan carried across the trips gives M, the
//                       running maximum of the last offsets.  Writes the flags
//                       that need no history (0, 2, 3) and the scope's counters.
//   tx_insert_kernel    one lane per batch: the (scope, producer) of every
//                       transactional data batch and abort marker into an
//                       open-addressing table, by CAS claim as in
//                       compact_insert_kernel.  At most n keys in >= 2n slots.
//   radix_sort_items    (rpgpu_sort.h) the abort markers sorted by table slot,
//                       stable: each producer's markers in file order.  Batches
//                       that are no abort marker carry the sentinel key.
//   tx_groups_kernel    one lane per sorted position: where each slot's run of
//                       markers begins and ends.
//   tx_ranges_kernel    one wavefront per scope, 64 ranges per trip: the range
//                       filter, the consume position c(r) (a binary search on
//                       M), the producer's slot, the interval c(r) falls into (a
//                       binary search over the producer's markers), and an
//                       atomic min of c(r) into that interval's cell.
//   tx_decide_kernel    one lane per batch: a transactional data batch finds
//                       its interval the same way and is discarded iff the
//                       cell's minimum is at or in front of it.
//
// Nothing is kept per (scope, range): a range that several scopes name is read
// by each of them and leaves only a minimum in a cell, so the scratch is a
// function of n alone.  The table's slot numbers depend on which lane claims a
// slot first and differ from run to run; every output is a min, a sum or a
// value looked up by key, so no output byte does.
//
// Known bound: one scope is classified by one wave, and its
// ranges are read by one wave.
#include "rpgpu_device.h"
#include "rpgpu_launch.h"
#include "rpgpu_scan.h"
#include "rpgpu_sort.h"
#include "rpgpu_txfilter.h"

namespace rptx {
// MaxOp under wave_scan_incl (rpgpu_scan.h)
__device__ __forceinline__ MaxOp operator+(MaxOp a, MaxOp b) { return max_combine(a, b); }
__device__ __forceinline__ MaxOp shfl_up(MaxOp x, int s) { return MaxOp{(int64_t)rpgpu::shfl_up((uint64_t)x.v, s)}; }
}  // namespace rptx

namespace rpgpu {
namespace {

static_assert(sizeof(rpgpu_tx_range) == 32 && sizeof(rpgpu_tx_scope) == 40 && sizeof(rpgpu_tx_stats) == 64,
              "tx filter row layouts");

struct TxParts {
    int64_t *M, *pid;
    uint32_t *bscope, *slot, *key, *idx_a, *idx_b, *table;
    int16_t* epoch;
    uint8_t* kind;
    uint32_t *rep, *gstart, *gend;  // per table slot: claiming batch + 1; the slot's run of sorted markers
    uint32_t *cellm, *cellh;        // interval minima: behind marker b; in front of a slot's first marker
    uint32_t cap;
    size_t cells_at, cells_bytes;
};
size_t tx_al(size_t x) { return (x + 255) & ~(size_t)255; }
uint32_t tx_table_cap(uint32_t n) {
    uint64_t c = 64;
    while (c < 2 * (uint64_t)n) c <<= 1;
    return (uint32_t)c;  // n < 2^30 (launch_tx_filter)
}
size_t tx_layout(void* p, uint32_t n, TxParts* out) {
    uint8_t* b = static_cast<uint8_t*>(p);
    size_t o = 0;
    TxParts s;
    const size_t cap = s.cap = tx_table_cap(n);
    s.M = reinterpret_cast<int64_t*>(b + o), o += tx_al((size_t)n * 8);
    s.pid = reinterpret_cast<int64_t*>(b + o), o += tx_al((size_t)n * 8);
    s.bscope = reinterpret_cast<uint32_t*>(b + o), o += tx_al((size_t)n * 4);
    s.slot = reinterpret_cast<uint32_t*>(b + o), o += tx_al((size_t)n * 4);
    s.key = reinterpret_cast<uint32_t*>(b + o), o += tx_al((size_t)n * 4);
    s.idx_a = reinterpret_cast<uint32_t*>(b + o), o += tx_al((size_t)n * 4);
    s.idx_b = reinterpret_cast<uint32_t*>(b + o), o += tx_al((size_t)n * 4);
    s.table = reinterpret_cast<uint32_t*>(b + o), o += tx_al((size_t)sort_blocks(n) * 256 * 4);
    s.epoch = reinterpret_cast<int16_t*>(b + o), o += tx_al((size_t)n * 2);
    s.kind = b + o, o += tx_al((size_t)n);
    s.rep = reinterpret_cast<uint32_t*>(b + o), o += tx_al(cap * 4);
    s.gstart = reinterpret_cast<uint32_t*>(b + o), o += tx_al(cap * 4);
    s.gend = reinterpret_cast<uint32_t*>(b + o), o += tx_al(cap * 4);
    s.cells_at = o;
    s.cellm = reinterpret_cast<uint32_t*>(b + o), o += tx_al((size_t)n * 4);
    s.cellh = reinterpret_cast<uint32_t*>(b + o), o += tx_al(cap * 4);
    s.cells_bytes = o - s.cells_at;
    if (out) *out = s;
    return o;
}

__device__ __forceinline__ bool scope_ok(const rpgpu_tx_scope& sc, uint32_t n, uint32_t nranges) {
    return (uint64_t)sc.first_batch + sc.batch_count <= n && (uint64_t)sc.range_first + sc.range_count <= nranges;
}

__global__ __launch_bounds__(256) void tx_classify_kernel(
    const uint8_t* __restrict__ data, const rpgpu_batch_desc* __restrict__ descs,
    const rpgpu_batch_result* __restrict__ res, uint32_t n, const rpgpu_record_index* __restrict__ index,
    uint64_t index_cap, const rpgpu_tx_scope* __restrict__ scopes, uint32_t nscopes, uint32_t nranges,
    uint8_t* __restrict__ discard, rpgpu_tx_stats* __restrict__ stats, int64_t* __restrict__ M,
    int64_t* __restrict__ pid, int16_t* __restrict__ epoch, uint8_t* __restrict__ kind,
    uint32_t* __restrict__ bscope) {
    const uint32_t s = wave_item();
    if (s >= nscopes) return;
    const uint32_t l = lane_id();
    const rpgpu_tx_scope sc = scopes[s];
    rpgpu_tx_stats st;
    st.tx_data_batches_discarded = 0, st.tx_control_batches_discarded = 0, st.non_tx_control_batches_discarded = 0;
    st.all_batches_discarded = 0, st.num_aborted_txes = 0, st.all_batches = 0;
    st.processed = 0, st.status = RPGPU_TX_OK, st.bad_batch = UINT32_MAX, st.reserved = 0;
    if (!scope_ok(sc, n, nranges)) {
        st.status = RPGPU_TX_BAD_SCOPE;
        if (l == 0) stats[s] = st;
        return;
    }
    const bool nontx = (sc.flags & RPGPU_TX_NON_TRANSACTIONAL) != 0;
    rptx::MaxOp carry = rptx::max_identity();
    for (uint32_t base = 0; base < sc.batch_count; base += 64) {
        const uint32_t left = sc.batch_count - base, nlive = left < 64 ? left : 64;
        const bool live = l < nlive;
        const uint32_t b = sc.first_batch + base + l;
        rptx::Class c;
        c.stop = RPGPU_TX_OK, c.flag = RPGPU_TX_DELEGATED, c.kind = rptx::kKindNone, c.epoch = 0, c.pid = 0;
        rptx::MaxOp x = rptx::max_identity();
        if (live) {
            const rpgpu_batch_result r = res[b];
            const rpgpu_batch_desc d = descs[b];
            c = rptx::classify(r, d, data + d.offset, index, index_cap, nontx);
            x.v = rptx::last_offset(r);
        }
        const uint64_t stops = __ballot(live && c.stop != RPGPU_TX_OK);
        const uint32_t upto = stops ? (uint32_t)__builtin_ctzll(stops) : nlive;
        const bool ok = l < upto;
        if (!ok) x = rptx::max_identity();
        x = rptx::max_combine(carry, wave_scan_incl(x, l));
        carry.v = (int64_t)shfl64((uint64_t)x.v, 63);
        if (ok) {
            M[b] = x.v;
            pid[b] = c.pid;
            epoch[b] = c.epoch;
            kind[b] = c.kind;
            bscope[b] = s;
            discard[b] = c.flag;
        }
        st.tx_control_batches_discarded += __popcll(__ballot(ok && c.flag == RPGPU_TX_MARKER));
        st.non_tx_control_batches_discarded += __popcll(__ballot(ok && c.flag == RPGPU_TX_PREPARE));
        st.processed += upto;
        if (stops) {
            st.status = __builtin_amdgcn_readlane(c.stop, upto);
            st.bad_batch = sc.first_batch + base + upto;
            break;
        }
    }
    st.all_batches_discarded = st.tx_control_batches_discarded + st.non_tx_control_batches_discarded;
    st.all_batches = nontx ? 0 : st.processed;
    if (l == 0) stats[s] = st;  // tx_ranges_kernel and tx_decide_kernel add what depends on the ranges
}

__device__ __forceinline__ bool same_producer(const uint32_t* __restrict__ bscope, const int64_t* __restrict__ pid,
                                              const int16_t* __restrict__ epoch, uint32_t o, uint32_t scope,
                                              int64_t p, int16_t e) {
    return bscope[o] == scope && pid[o] == p && epoch[o] == e;
}

__global__ __launch_bounds__(256) void tx_insert_kernel(uint32_t n, const uint8_t* __restrict__ kind,
                                                        const uint32_t* __restrict__ bscope,
                                                        const int64_t* __restrict__ pid,
                                                        const int16_t* __restrict__ epoch, uint32_t* rep,
                                                        uint32_t cap, uint32_t* __restrict__ slot,
                                                        uint32_t* __restrict__ key) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n) return;
    const uint8_t k = kind[b];
    if (k == rptx::kKindNone) {
        key[b] = cap;  // the sentinel: sorted behind every marker
        return;
    }
    const uint32_t scope = bscope[b];
    const int64_t p = pid[b];
    const int16_t e = epoch[b];
    const uint32_t mask = cap - 1;
    uint32_t pos = (uint32_t)rptx::pid_hash(scope, p, e) & mask;
    // the table has at least 2x as many slots as batches: a free slot is always found
    for (uint32_t probe = 0; probe < cap; probe++, pos = (pos + 1) & mask) {
        uint32_t cur = __hip_atomic_load(rep + pos, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(rep + pos, 0u, b + 1);
            if (cur == 0) break;  // claimed: this batch represents the producer
        }
        if (same_producer(bscope, pid, epoch, cur - 1, scope, p, e)) break;
    }
    slot[b] = pos;
    key[b] = k == rptx::kKindAbort ? pos : cap;
}

__global__ __launch_bounds__(256) void tx_groups_kernel(const uint32_t* __restrict__ sorted,
                                                        const uint32_t* __restrict__ key, uint32_t n, uint32_t cap,
                                                        uint32_t* __restrict__ gstart, uint32_t* __restrict__ gend) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t ky = key[sorted[k]];
    if (ky >= cap) return;
    if (k == 0 || key[sorted[k - 1]] != ky) gstart[ky] = k;
    if (k + 1 == n || key[sorted[k + 1]] != ky) gend[ky] = k + 1;
}

struct TxTable {
    const uint32_t *rep, *gstart, *gend, *sorted, *bscope;
    const int64_t* pid;
    const int16_t* epoch;
    uint32_t *cellm, *cellh;
    uint32_t cap;
};

// the cell of the interval that position x of the slot's producer falls into
__device__ __forceinline__ uint32_t* interval_cell(const TxTable& t, uint32_t slot, uint32_t x) {
    const uint32_t iv = rptx::interval_of(t.sorted, t.gstart[slot], t.gend[slot], x);
    return iv == rptx::kNone ? t.cellh + slot : t.cellm + t.sorted[iv];
}

__global__ __launch_bounds__(256) void tx_ranges_kernel(const rpgpu_tx_scope* __restrict__ scopes, uint32_t nscopes,
                                                        const rpgpu_tx_range* __restrict__ ranges,
                                                        rpgpu_tx_stats* __restrict__ stats,
                                                        const int64_t* __restrict__ M, TxTable t) {
    const uint32_t s = wave_item();
    if (s >= nscopes) return;
    const uint32_t l = lane_id();
    const int32_t status = stats[s].status;
    if (status == RPGPU_TX_BAD_SCOPE) return;
    const uint32_t m = stats[s].processed;
    const rpgpu_tx_scope sc = scopes[s];
    const bool nontx = (sc.flags & RPGPU_TX_NON_TRANSACTIONAL) != 0;
    const uint32_t mask = t.cap - 1;
    uint64_t taking = 0;
    for (uint32_t base = 0; base < sc.range_count; base += 64) {
        const bool live = base + l < sc.range_count;
        rpgpu_tx_range r;
        r.producer_id = 0, r.producer_epoch = 0, r.first = 0, r.last = 0;
        if (live) r = ranges[sc.range_first + base + l];
        const bool part = live && rptx::takes_part(r, sc);
        taking += __popcll(__ballot(part));
        const uint32_t c = part && !nontx ? rptx::consume_pos(M + sc.first_batch, m, r.first) : m;
        uint32_t pos = (uint32_t)rptx::pid_hash(s, r.producer_id, r.producer_epoch) & mask;
        // c == m: never consumed
        for (uint32_t probe = 0; c < m && probe < t.cap; probe++, pos = (pos + 1) & mask) {
            const uint32_t cur = t.rep[pos];
            if (cur == 0) break;  // no batch of this producer in the scope
            if (same_producer(t.bscope, t.pid, t.epoch, cur - 1, s, r.producer_id, r.producer_epoch)) {
                const uint32_t x = sc.first_batch + c;
                atomicMin(interval_cell(t, pos, x), x);
                break;
            }
        }
    }
    if (l == 0) stats[s].num_aborted_txes = taking;
}

__global__ __launch_bounds__(256) void tx_decide_kernel(uint32_t n, const uint8_t* __restrict__ kind,
                                                        const uint32_t* __restrict__ slot, TxTable t,
                                                        uint8_t* __restrict__ discard, rpgpu_tx_stats* stats) {
    const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t l = lane_id();
    bool dis = false;
    uint32_t scope = 0;
    if (b < n && kind[b] == rptx::kKindData) {
        dis = rptx::aborted(*interval_cell(t, slot[b], b), b);
        scope = t.bscope[b];
        if (dis) discard[b] = RPGPU_TX_ABORTED_DATA;
    }
    // the counters: one add per wave where its discarded batches share a scope
    const uint64_t m = __ballot(dis);
    if (m == 0) return;
    const uint32_t first = (uint32_t)__builtin_ctzll(m);
    const uint32_t s0 = __builtin_amdgcn_readlane(scope, first);
    const bool one = __ballot(dis && scope == s0) == m;
    if (one ? l == first : dis) {
        const unsigned long long add = one ? (unsigned long long)__popcll(m) : 1ull;
        atomicAdd(reinterpret_cast<unsigned long long*>(&stats[scope].tx_data_batches_discarded), add);
        atomicAdd(reinterpret_cast<unsigned long long*>(&stats[scope].all_batches_discarded), add);
    }
}

}  // namespace

size_t compaction_tx_scratch_bytes(uint32_t n, uint32_t nranges) {
    (void)nranges;  // a range leaves a minimum in a cell of its producer: nothing is kept per range
    return tx_layout(nullptr, n, nullptr);
}

hipError_t launch_tx_filter(const uint8_t* d_data, const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res,
                            uint32_t n, const rpgpu_record_index* d_index, uint64_t index_cap,
                            const rpgpu_tx_scope* d_scopes, uint32_t nscopes, const rpgpu_tx_range* d_ranges,
                            uint32_t nranges, uint8_t* d_discard, rpgpu_tx_stats* d_stats, void* d_scratch,
                            hipStream_t s) {
    hipError_t e;
    if (n && (e = hipMemsetAsync(d_discard, RPGPU_TX_NOT_REACHED, n, s)) != hipSuccess) return e;
    if (nscopes == 0) return hipSuccess;
    TxParts p;
    const size_t bytes = tx_layout(d_scratch, n, &p);
    if ((e = hipMemsetAsync(d_scratch, 0, bytes, s)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(static_cast<uint8_t*>(d_scratch) + p.cells_at, 0xff, p.cells_bytes, s)) != hipSuccess)
        return e;
    tx_classify_kernel<<<wave_grid(nscopes), 256, 0, s>>>(d_data, d_descs, d_res, n, d_index, index_cap, d_scopes,
                                                          nscopes, nranges, d_discard, d_stats, p.M, p.pid, p.epoch,
                                                          p.kind, p.bscope);
    RPGPU_LAUNCH_CHECK();
    TxTable t;
    t.rep = p.rep, t.gstart = p.gstart, t.gend = p.gend, t.sorted = nullptr, t.bscope = p.bscope;
    t.pid = p.pid, t.epoch = p.epoch, t.cellm = p.cellm, t.cellh = p.cellh, t.cap = p.cap;
    const uint32_t nb = (n + 255) / 256;
    if (n) {
        tx_insert_kernel<<<nb, 256, 0, s>>>(n, p.kind, p.bscope, p.pid, p.epoch, p.rep, p.cap, p.slot, p.key);
        RPGPU_LAUNCH_CHECK();
        // the largest key is the sentinel, the table's capacity
        if ((e = radix_sort_items(p.key, n, p.cap, p.idx_a, p.idx_b, p.table, &t.sorted, s)) != hipSuccess) return e;
        tx_groups_kernel<<<nb, 256, 0, s>>>(t.sorted, p.key, n, p.cap, p.gstart, p.gend);
        RPGPU_LAUNCH_CHECK();
    }
    tx_ranges_kernel<<<wave_grid(nscopes), 256, 0, s>>>(d_scopes, nscopes, d_ranges, d_stats, p.M, t);
    RPGPU_LAUNCH_CHECK();
    if (n) {
        tx_decide_kernel<<<nb, 256, 0, s>>>(n, p.kind, p.slot, t, d_discard, d_stats);
        RPGPU_LAUNCH_CHECK();
    }
    return hipSuccess;
}

}  // namespace rpgpu
