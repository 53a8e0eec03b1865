// rpgpu_append.hip — the produce path's log append (the last
// two lines of the call stack): disk_log_appender::operator()
// (storage/disk_log_appender.cc:71-135) and storage::write ->
// disk_header_to_iobuf (storage/segment_appender_utils.cc:28-61) over a
// validated arena.  Eligible batches are grouped by log in descriptor order,
// get their offsets, file positions and segment rolls, and leave as the bytes
// each log's segment files receive (include/rpgpu.h, "log append").
//
// Plan (descriptors, result rows, codes and logs only):
//   append_classify_kernel  one lane per batch: the sort key (the log, or the
//                           sentinel nlogs for a batch that is not appended)
//                           and the per-log batch counts
//   radix_sort_items        (rpgpu_sort.h) a stable LSD radix sort of the batch
//                           indices on the key, 8-bit digits,
//                           ceil(log2(nlogs + 1) / 8) passes; no atomic
//                           ticket, the order is the descriptors'.
//   append_walk_kernel      one wavefront per log, 64 batches per step: wave
//                           scans of lod + 1 and of size_bytes carry the next
//                           offset, the file position and the bytes left
//                           before the roll; rolls inside a step are resolved
//                           by a ballot loop (first lane whose running bytes
//                           exhaust `left`, open a segment there, rebase the
//                           lanes behind it), one iteration per roll
//   append_log_scan_kernel  exclusive scans over the logs: output region,
//                           first row, first segment; the totals
//   append_fixup_kernel     one lane per batch: log-relative row, segment and
//                           output offset made absolute
// Run:
//   append_write_kernel     one wavefront per appended batch: lanes 0..60 make
//                           the little-endian header (wire input: fields
//                           [17, 61) byte-reversed in place), the header CRC
//                           goes through the one-byte-per-lane tables, the
//                           body is copied with destination-aligned 16-byte
//                           stores and unaligned 16-byte loads.
//                           Bound: HBM, size_bytes read + size_bytes written.
//                           One lane of wave i also settles log i's status
//                           (does it fit the caller's buffers) and emits
//                           segment row i of the plan.
//
// Known bound: one log is walked by one wave, so an arena whose
// batches nearly all belong to one log is walked serially, 64 batches a step.
#include "rpgpu_device.h"
#include "rpgpu_launch.h"
#include "rpgpu_scan.h"
#include "rpgpu_sort.h"

namespace rpgpu {
namespace {

constexpr uint32_t kScanThreads = 1024;
constexpr uint8_t kGhostBatch = 7;  // model::record_batch_type::ghost_batch
static_assert(sizeof(rpgpu_append_log) == 32 && sizeof(rpgpu_append_batch) == 32 &&
                  sizeof(rpgpu_append_log_result) == 64 && sizeof(rpgpu_append_segment) == 48,
              "append row layouts");

struct ApParts {
    uint32_t *key, *idx_a, *idx_b, *starts, *table;
    uint64_t* dst;
    rpgpu_append_segment* segs;
};
size_t ap_al(size_t x) { return (x + 255) & ~(size_t)255; }
size_t ap_layout(void* p, uint32_t n, uint32_t nlogs, ApParts* out) {
    uint8_t* b = static_cast<uint8_t*>(p);
    size_t o = 0;
    ApParts s;
    s.key = reinterpret_cast<uint32_t*>(b + o), o += ap_al((size_t)n * 4);
    s.idx_a = reinterpret_cast<uint32_t*>(b + o), o += ap_al((size_t)n * 4);
    s.idx_b = reinterpret_cast<uint32_t*>(b + o), o += ap_al((size_t)n * 4);
    s.dst = reinterpret_cast<uint64_t*>(b + o), o += ap_al((size_t)n * 8);
    s.segs = reinterpret_cast<rpgpu_append_segment*>(b + o), o += ap_al((size_t)n * sizeof(rpgpu_append_segment));
    s.starts = reinterpret_cast<uint32_t*>(b + o), o += ap_al(((size_t)nlogs + 1) * 4);
    s.table = reinterpret_cast<uint32_t*>(b + o), o += ap_al((size_t)sort_blocks(n) * 256 * 4);
    if (out) *out = s;
    return o;
}
__global__ __launch_bounds__(256) void append_classify_kernel(const rpgpu_batch_desc* __restrict__ descs,
                                                              const rpgpu_batch_result* __restrict__ res, uint32_t n,
                                                              const int32_t* __restrict__ codes,
                                                              const rpgpu_append_log* __restrict__ logs,
                                                              uint32_t part_lo, uint32_t nlogs,
                                                              uint32_t* __restrict__ key, uint32_t* __restrict__ counts,
                                                              rpgpu_append_batch* __restrict__ rows) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rpgpu_batch_desc d = descs[i];
    const rpgpu_batch_result& r = res[i];
    const uint32_t log = d.partition - part_lo;  // below part_lo: wraps past nlogs
    // RPGPU_V_OK implies 61 <= size_bytes <= desc.length; checked again because
    // the write pass reads that many bytes
    bool el = r.verdict == RPGPU_V_OK && log < nlogs && (!codes || codes[i] == 0) &&
              r.size_bytes >= kHeaderSize && (uint32_t)r.size_bytes <= d.length;
    if (el && logs[log].max_segment_size == 0) el = false;  // RPGPU_APPEND_BAD_CONFIG: nothing is appended
    key[i] = el ? log : nlogs;
    if (el) {
        atomicAdd(&counts[log], 1u);
    } else {
        rpgpu_append_batch b;
        b.action = RPGPU_APPEND_SKIPPED;
        b.out_row = UINT32_MAX;
        b.base_offset = 0;
        b.file_pos = 0;
        b.segment = 0;
        b.reserved = 0;
        rows[i] = b;
    }
}

// disk_log_appender::operator() per log (disk_log_appender.cc:71-135); rows,
// segments and output offsets relative to the log's own
__global__ __launch_bounds__(256) void append_walk_kernel(const rpgpu_batch_desc* __restrict__ descs,
                                                          const rpgpu_batch_result* __restrict__ res,
                                                          const rpgpu_append_log* __restrict__ logs, uint32_t nlogs,
                                                          const uint32_t* __restrict__ sorted,
                                                          const uint32_t* __restrict__ starts,
                                                          rpgpu_append_batch* __restrict__ rows,
                                                          uint64_t* __restrict__ dst,
                                                          rpgpu_append_segment* __restrict__ segs,
                                                          rpgpu_append_log_result* __restrict__ lres) {
    const uint32_t log = wave_item();
    if (log >= nlogs) return;
    const uint32_t l = lane_id();
    const rpgpu_append_log lg = logs[log];
    const uint32_t s0 = starts[log], s1 = starts[log + 1];
    uint64_t idx = (uint64_t)lg.next_offset;  // _idx, wrapping
    uint64_t byte_size = 0;
    // bytes_left_before_roll (:61), 0 when the caller asks for a roll first
    uint64_t left = (lg.flags & RPGPU_APPEND_ROLL_FIRST)
                        ? 0
                        : (lg.max_segment_size > lg.file_offset ? lg.max_segment_size - lg.file_offset : 0);
    uint64_t pos = lg.file_offset;
    uint32_t nseg = 0, nrows = 0, nghost = 0;
    bool open = false, any = false;
    uint32_t sg_flags = 0, sg_first = 0;  // the open segment row
    uint64_t sg_base = 0, sg_fpos = 0, sg_off = 0;
    rpgpu_append_segment* my = segs + s0;  // at most one row per batch of the log
    for (uint64_t c = s0; c < s1; c += 64) {
        const uint64_t j = c + l;
        const bool live = j < s1;
        uint32_t b = 0;
        uint64_t w = 0, sz = 0;
        bool ghost = false;
        if (live) {
            b = sorted[j];
            const rpgpu_batch_result& r = res[b];
            ghost = descs[b].format == RPGPU_FMT_RP_DISK && r.type == kGhostBatch;
            w = (uint64_t)((int64_t)r.last_offset_delta + 1);
            sz = ghost ? 0 : (uint64_t)(uint32_t)r.size_bytes;
        }
        const uint64_t W = wave_scan_incl(w, l), S = wave_scan_incl(sz, l);  // wrapping
        const uint64_t E = S - sz;  // bytes of this step in front of the batch
        const uint64_t wm = __ballot(live && !ghost);
        const uint64_t lanes_below = (1ull << l) - 1;
        if (!open && left > 0) {  // the continuing segment, reached by the log's first batch
            sg_flags = 0, sg_first = 0, sg_base = idx, sg_fpos = pos, sg_off = 0;
            nseg = 1;
            open = true;
        }
        uint32_t my_seg = nseg - 1;  // (no row yet: lane 0 rolls below)
        uint64_t my_rb = 0, my_p0 = pos;
        uint64_t rb = 0, L = left, p0 = pos;  // the current segment began at step byte rb with L left, at p0
        uint32_t from = 0;
        for (;;) {
            // needs_to_roll_log in front of the batch: left - min(left, bytes since) == 0
            const uint64_t m = __ballot(live && l >= from && E - rb >= L);
            if (!m) break;
            const int k = __builtin_ctzll(m);
            const uint64_t Ek = shfl64(E, k);
            const uint64_t base_k = idx + shfl64(W - w, k);
            const uint32_t first_k = nrows + (uint32_t)__popcll(wm & ((1ull << k) - 1));
            if (open && l == 0) {
                rpgpu_append_segment sg;
                sg.log = log, sg.flags = sg_flags, sg.first = sg_first, sg.count = first_k - sg_first;
                sg.base_offset = (int64_t)sg_base, sg.file_pos = sg_fpos, sg.out_offset = sg_off;
                sg.bytes = byte_size + Ek - sg_off;
                my[nseg - 1] = sg;
            }
            sg_flags = RPGPU_APPEND_SEG_ROLLED, sg_first = first_k, sg_base = base_k, sg_fpos = 0;
            sg_off = byte_size + Ek;
            open = true;
            nseg++;
            rb = Ek, L = lg.max_segment_size, p0 = 0;  // initialize() -> bytes_left_before_roll()
            from = (uint32_t)k + 1;
            if (l >= (uint32_t)k) my_seg = nseg - 1, my_rb = rb, my_p0 = 0;
        }
        if (live) {
            rpgpu_append_batch o;
            o.action = ghost ? RPGPU_APPEND_GHOST : RPGPU_APPEND_APPENDED;
            o.out_row = ghost ? UINT32_MAX : nrows + (uint32_t)__popcll(wm & lanes_below);
            o.base_offset = (int64_t)(idx + W - w);
            o.file_pos = my_p0 + (E - my_rb);
            o.segment = my_seg;
            o.reserved = 0;
            rows[b] = o;
            dst[b] = byte_size + E;
        }
        const uint64_t T = shfl64(S, 63), used = T - rb;
        left = L - (L < used ? L : used);
        pos = p0 + used;
        byte_size += T;
        nrows += (uint32_t)__popcll(wm);
        nghost += (uint32_t)__popcll(__ballot(live && ghost));
        idx += shfl64(W, 63);
        any = true;
    }
    if (l != 0) return;
    if (open) {
        rpgpu_append_segment sg;
        sg.log = log, sg.flags = sg_flags, sg.first = sg_first, sg.count = nrows - sg_first;
        sg.base_offset = (int64_t)sg_base, sg.file_pos = sg_fpos, sg.out_offset = sg_off;
        sg.bytes = byte_size - sg_off;
        my[nseg - 1] = sg;
    }
    rpgpu_append_log_result o;
    o.status = lg.max_segment_size == 0 ? RPGPU_APPEND_BAD_CONFIG : RPGPU_APPEND_OK;
    o.batches = nrows, o.ghosts = nghost, o.segments = nseg;
    o.first_row = 0, o.first_segment = 0;
    o.base_offset = lg.next_offset;
    o.last_offset = any ? (int64_t)(idx - 1) : INT64_MIN;  // model::offset{}
    o.next_offset = (int64_t)idx;
    o.byte_size = byte_size;
    o.out_offset = 0;
    lres[log] = o;
}

// first_row, first_segment and out_offset (regions on 16-byte boundaries) as
// exclusive scans over the logs; totals: the smallest out_cap that holds
// every log, the output rows, the segment rows
__global__ __launch_bounds__(kScanThreads) void append_log_scan_kernel(rpgpu_append_log_result* __restrict__ lres,
                                                                       uint32_t nlogs, uint64_t* __restrict__ totals) {
    __shared__ uint64_t pb[kScanThreads], pe[kScanThreads];
    __shared__ uint32_t pr[kScanThreads], ps[kScanThreads];
    const uint32_t t = threadIdx.x;
    const uint64_t c = ((uint64_t)nlogs + kScanThreads - 1) / kScanThreads;
    const uint64_t lo = t * c < nlogs ? t * c : nlogs, hi = lo + c < nlogs ? lo + c : nlogs;
    uint64_t sb = 0;
    uint32_t sr = 0, ss = 0;
    for (uint64_t k = lo; k < hi; k++) {
        sb += (lres[k].byte_size + 15) & ~(uint64_t)15;
        sr += lres[k].batches;
        ss += lres[k].segments;
    }
    pb[t] = sb, pr[t] = sr, ps[t] = ss;
    __syncthreads();
    for (uint32_t off = 1; off < kScanThreads; off <<= 1) {
        const uint64_t vb = t >= off ? pb[t - off] : 0;
        const uint32_t vr = t >= off ? pr[t - off] : 0, vs = t >= off ? ps[t - off] : 0;
        __syncthreads();
        pb[t] += vb, pr[t] += vr, ps[t] += vs;
        __syncthreads();
    }
    uint64_t rbytes = pb[t] - sb, end = 0;
    uint32_t rrows = pr[t] - sr, rsegs = ps[t] - ss;
    for (uint64_t k = lo; k < hi; k++) {
        rpgpu_append_log_result& o = lres[k];
        o.out_offset = rbytes, o.first_row = rrows, o.first_segment = rsegs;
        if (o.byte_size && rbytes + o.byte_size > end) end = rbytes + o.byte_size;
        rbytes += (o.byte_size + 15) & ~(uint64_t)15;
        rrows += o.batches;
        rsegs += o.segments;
    }
    pe[t] = end;
    __syncthreads();
    if (t == 0) {
        uint64_t mx = 0;
        for (uint32_t k = 0; k < kScanThreads; k++) mx = pe[k] > mx ? pe[k] : mx;
        totals[0] = mx;
        totals[1] = pr[kScanThreads - 1];
        totals[2] = ps[kScanThreads - 1];
    }
}

__global__ __launch_bounds__(256) void append_fixup_kernel(const uint32_t* __restrict__ key, uint32_t n, uint32_t nlogs,
                                                           const rpgpu_append_log_result* __restrict__ lres,
                                                           rpgpu_append_batch* __restrict__ rows,
                                                           uint64_t* __restrict__ dst) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t log = key[i];
    if (log >= nlogs) return;
    const rpgpu_append_log_result& lr = lres[log];
    if (rows[i].out_row != UINT32_MAX) rows[i].out_row += lr.first_row;
    rows[i].segment += lr.first_segment;
    dst[i] += lr.out_offset;
}

// a log is written whole or not at all
__device__ __forceinline__ bool log_fits(const rpgpu_append_log_result& lr, uint64_t out_cap, uint64_t rows_cap,
                                         uint64_t seg_cap) {
    return (lr.byte_size == 0 || (lr.out_offset <= out_cap && lr.byte_size <= out_cap - lr.out_offset)) &&
           (lr.batches == 0 || (uint64_t)lr.first_row + lr.batches <= rows_cap) &&
           (lr.segments == 0 || (uint64_t)lr.first_segment + lr.segments <= seg_cap);
}

// what the run pass adds to the plan's rows
struct ApRun {
    uint64_t out_cap, rows_cap, seg_cap;
    const uint32_t *key, *sorted, *starts;
    const rpgpu_append_segment* segs;  // the plan's rows, log-relative
    rpgpu_append_segment* out_segs;
};

// storage::write (segment_appender_utils.cc:53-61): header, then the records.
// Item i of the grid-stride loop is batch i, and on one lane log i's status
// and segment row i of the plan (separate launches for those two cost ~20 us
// each behind a kernel that left 1 GiB of dirty lines).  Whether a log fits is
// recomputed from its row, so no wave waits for another one's status store.
__global__ __launch_bounds__(256) void append_write_kernel(
    const uint8_t* __restrict__ data, const rpgpu_batch_desc* __restrict__ descs,
    const rpgpu_batch_result* __restrict__ res, uint32_t n, uint32_t part_lo, uint32_t nlogs,
    const rpgpu_append_batch* __restrict__ rows, rpgpu_append_log_result* lres, const uint64_t* __restrict__ dst,
    const uint32_t* __restrict__ tables, uint8_t* __restrict__ out, rpgpu_batch_desc* __restrict__ out_descs,
    rpgpu_batch_result* __restrict__ out_res, ApRun a) {
    const uint32_t lid = lane_id();
    const uint32_t nw = gridDim.x * (blockDim.x / 64);
    const uint32_t items = n > nlogs ? n : nlogs;
    for (uint64_t it = __builtin_amdgcn_readfirstlane(blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6)); it < items;
         it += nw) {
        const uint32_t i = (uint32_t)it;
        if (lid == 0 && i < nlogs && lres[i].status != RPGPU_APPEND_BAD_CONFIG)
            lres[i].status = log_fits(lres[i], a.out_cap, a.rows_cap, a.seg_cap) ? RPGPU_APPEND_OK : RPGPU_APPEND_NO_ROOM;
        if (lid == 1 && i < n && i < a.starts[nlogs]) {  // slot i of the sorted order: a segment row of its log?
            const uint32_t log = a.key[a.sorted[i]];
            const uint32_t k = i - a.starts[log];
            if (k < lres[log].segments && log_fits(lres[log], a.out_cap, a.rows_cap, a.seg_cap)) {
                rpgpu_append_segment sg = a.segs[i];
                sg.first += lres[log].first_row;
                sg.out_offset += lres[log].out_offset;
                a.out_segs[lres[log].first_segment + k] = sg;
            }
        }
        if (i >= n) continue;
        const rpgpu_append_batch row = rows[i];
        if (row.action != RPGPU_APPEND_APPENDED) continue;
        const rpgpu_batch_desc d = descs[i];
        const uint32_t log = d.partition - part_lo;
        if (log >= nlogs || !log_fits(lres[log], a.out_cap, a.rows_cap, a.seg_cap)) continue;
        rpgpu_batch_result r = res[i];
        const uint8_t* p = data + d.offset;
        const uint64_t off = dst[i];
        uint8_t* o = out + off;
        const uint32_t size = (uint32_t)r.size_bytes;
        const bool wire = d.format == RPGPU_FMT_KAFKA_WIRE;
        const uint32_t type = wire ? 1u : (uint32_t)r.type;  // read_header: raft_data
        // ---- header (disk_header_to_iobuf, segment_appender_utils.cc:28-51)
        uint32_t v = 0;
        if (lid >= 4 && lid < 8) {
            v = (size >> (8 * (lid - 4))) & 255u;
        } else if (lid < 16) {
            v = (uint32_t)((uint64_t)row.base_offset >> (8 * (lid - 8))) & 255u;
        } else if (lid == 16) {
            v = type;
        } else if (lid < kHeaderSize) {
            uint32_t at = lid;
            if (wire) {
                // crc 17+4, attrs 21+2, lod 23+4, first_ts 27+8, max_ts 35+8,
                // producer id 43+8, epoch 51+2, base sequence 53+4, count 57+4
                int s, len;
                if (lid < 21) s = 17, len = 4;
                else if (lid < 23) s = 21, len = 2;
                else if (lid < 27) s = 23, len = 4;
                else if (lid < 35) s = 27, len = 8;
                else if (lid < 43) s = 35, len = 8;
                else if (lid < 51) s = 43, len = 8;
                else if (lid < 53) s = 51, len = 2;
                else if (lid < 57) s = 53, len = 4;
                else s = 57, len = 4;
                at = (uint32_t)(2 * s + len - 1 - (int)lid);
            }
            v = p[at];
        }
        // internal_header_only_crc (record_utils.cc:34-55) over bytes [4, 61): lane l
        // hashes byte l - 3 of the header in the right-aligned 64-byte window, the
        // initial value folded into the first four bytes
        uint32_t hb = (uint32_t)__shfl((int)v, (int)(lid >= 3 ? lid - 3 : 0), 64);
        hb = lid < 7 ? 0u : (lid < 11 ? hb ^ 255u : hb);
#ifdef RPGPU_DIAG_APPEND_NO_HCRC  // diagnostics build: time everything but the header CRC
        const uint32_t hcrc = hb;
#else
        const uint32_t* t = tables + kOffHB + lid;
        uint32_t c = t[(hb & 15u) * 64] ^ t[(16u + (hb >> 4)) * 64];
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) c ^= (uint32_t)__shfl_xor((int)c, s, 64);
        const uint32_t hcrc = ~c;
#endif
        if (lid < 4) v = (hcrc >> (8 * lid)) & 255u;
        if (lid < kHeaderSize) o[lid] = (uint8_t)v;
        // ---- records bytes [61, size): aligned 16-byte stores, unaligned loads
        const uint8_t* sb = p + kHeaderSize;
        uint8_t* ob = o + kHeaderSize;
        const uint64_t nb = size - kHeaderSize;
        const uint64_t head = (16 - ((uintptr_t)ob & 15)) & 15;
        if (nb < head + 16) {
            for (uint64_t q = lid; q < nb; q += 64) ob[q] = sb[q];
        } else {
            const uint64_t mid = (nb - head) & ~(uint64_t)15;
            if (lid < head) ob[lid] = sb[lid];
            for (uint64_t q = head + 16ull * lid; q < head + mid; q += 1024)
#ifdef RPGPU_DIAG_APPEND_ALIGNED  // diagnostics build: the copy with aligned loads (wrong bytes)
                *reinterpret_cast<u32x4*>(ob + q) =
                    *reinterpret_cast<const u32x4*>((uintptr_t)(sb + q) & ~(uintptr_t)15);
#else
                *reinterpret_cast<u32x4*>(ob + q) = ld16(sb + q);
#endif
            const uint64_t tail = head + mid;
            if (tail + lid < nb) ob[tail + lid] = sb[tail + lid];
        }
        if (lid == 0) {
            rpgpu_batch_desc od;
            od.offset = off;
            od.length = size;
            od.partition = d.partition;
            od.format = RPGPU_FMT_RP_DISK;
            od.ops = (uint8_t)(RPGPU_OP_CRC | RPGPU_OP_HDRCRC);
            od.flags = 0;
            od.reserved = 0;
            out_descs[row.out_row] = od;
            r.base_offset = row.base_offset;
            r.header_crc = hcrc;
            r.type = (uint8_t)type;
            out_res[row.out_row] = r;
        }
    }
}

}  // namespace

size_t append_scratch_bytes(uint32_t n, uint32_t nlogs) { return ap_layout(nullptr, n, nlogs, nullptr); }

hipError_t launch_append_plan(const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res, uint32_t n,
                              const int32_t* d_codes, const rpgpu_append_log* d_logs, uint32_t part_lo,
                              uint32_t nlogs, rpgpu_append_batch* d_rows, rpgpu_append_log_result* d_lres,
                              uint64_t* d_totals, void* d_scratch, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_totals, 0, 3 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    if (n == 0 && nlogs == 0) return hipSuccess;
    ApParts p;
    ap_layout(d_scratch, n, nlogs, &p);
    if ((e = hipMemsetAsync(p.starts, 0, ((size_t)nlogs + 1) * 4, s)) != hipSuccess) return e;
    if (n) {
        append_classify_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_descs, d_res, n, d_codes, d_logs, part_lo, nlogs,
                                                               p.key, p.starts, d_rows);
        RPGPU_LAUNCH_CHECK();
    }
    if (nlogs == 0) return hipSuccess;
    radix_scan_kernel<<<1, kScanBlock, 0, s>>>(p.starts, nlogs + 1);
    RPGPU_LAUNCH_CHECK();
    const uint32_t* in = nullptr;  // the largest key is the sentinel nlogs
    if ((e = radix_sort_items(p.key, n, nlogs, p.idx_a, p.idx_b, p.table, &in, s)) != hipSuccess) return e;
    append_walk_kernel<<<wave_grid(nlogs), 256, 0, s>>>(d_descs, d_res, d_logs, nlogs, in, p.starts, d_rows, p.dst,
                                                        p.segs, d_lres);
    RPGPU_LAUNCH_CHECK();
    append_log_scan_kernel<<<1, kScanThreads, 0, s>>>(d_lres, nlogs, d_totals);
    RPGPU_LAUNCH_CHECK();
    if (n) {
        append_fixup_kernel<<<(n + 255) / 256, 256, 0, s>>>(p.key, n, nlogs, d_lres, d_rows, p.dst);
        RPGPU_LAUNCH_CHECK();
    }
    return hipSuccess;
}

hipError_t launch_append_run(const uint8_t* d_data, const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res,
                             uint32_t n, uint32_t part_lo, uint32_t nlogs, const rpgpu_append_batch* d_rows,
                             rpgpu_append_log_result* d_lres, uint8_t* d_out, uint64_t out_cap,
                             rpgpu_batch_desc* d_out_descs, rpgpu_batch_result* d_out_res, uint32_t rows_cap,
                             rpgpu_append_segment* d_segments, uint32_t seg_cap, void* d_scratch,
                             const uint32_t* d_tables, hipStream_t s) {
    if (nlogs == 0) return hipSuccess;
    ApParts p;
    ap_layout(d_scratch, n, nlogs, &p);
    ApRun r;
    r.out_cap = out_cap, r.rows_cap = rows_cap, r.seg_cap = seg_cap;
    r.key = p.key, r.sorted = (sort_passes(nlogs) & 1) ? p.idx_a : p.idx_b, r.starts = p.starts;
    r.segs = p.segs, r.out_segs = d_segments;
    const uint32_t items = n > nlogs ? n : nlogs;
    const uint32_t waves = items < 65536u ? items : 65536u;
    append_write_kernel<<<(waves + 3) / 4, 256, 0, s>>>(d_data, d_descs, d_res, n, part_lo, nlogs, d_rows, d_lres,
                                                        p.dst, d_tables, d_out, d_out_descs, d_out_res, r);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace rpgpu
