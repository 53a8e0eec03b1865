// rpgpu_rsindex.hip — the tiered-storage offset index (include/rpgpu.h,
// "tiered-storage offset index"): remote_segment_index_builder over a segment's
// batch headers, offset_index::to_iobuf, and find_rp_offset / find_kaf_offset on
// a serialized index.  The row format and the blob layout live in rpgpu_dfor.h,
// which the host program tests/native/rsindex_host.cpp compiles too.
//
// Plan:
//   rsindex_select_kernel  one wavefront per segment, 64 batch headers per trip:
//                          wave scans of size_bytes and of the configuration
//                          batches' last_offset_delta + 1 carry the parser's
//                          position and the running delta; the samples inside
//                          a trip are resolved by a ballot loop (first lane
//                          that is no configuration batch and whose window is
//                          full, restart the window there, repeat), one
//                          iteration per sample.  The triples go to the
//                          segment's slice of the scratch (slot first_batch +
//                          sample number: at most one sample per batch).
//   rsindex_width_kernel   one wavefront per segment, 16 lanes per row, four
//                          rows per trip: each lane's delta against its left
//                          neighbour (the row's first lane: the previous row's
//                          last sample or the initial value), nbits as an
//                          OR-reduction over the row's 16 lanes; one byte per
//                          row and stream, the three stream sizes per segment.
//   rsindex_place_kernel   the blobs' places: an exclusive scan of the
//                          16-byte-rounded sizes (rpgpu_scan.h), the totals.
// Run:
//   rsindex_emit_kernel    one wavefront per segment.  Header fields and write
//                          buffers: one int64 field per lane.  Rows: offsets
//                          from an exclusive wave scan of 1 + 2 * nbits over 64
//                          rows with a carry; then four rows per trip, each
//                          lane stores its value's 8 / 4 / 2 / 1-byte pieces
//                          and the lanes below 2r assemble one byte each of the
//                          remainder bit string from their row's lanes.  Plain
//                          stores, every output byte written once.
// Find:
//   rsindex_find_kernel    one wavefront per query.  The chain of nbits bytes is
//                          walked over a 256-byte chunk of the stream held in a
//                          register per lane (a wave-uniform read of one lane
//                          per row, not a dependent global load); 64 row
//                          starts are collected, then decoded four rows per
//                          trip: unpack, prefix XOR / prefix sum with a carry,
//                          compare, ballot.
//
// Known bound: one segment is selected, measured and emitted by
// one wave, so a single huge segment is walked 64 headers a trip.
#include "rpgpu_device.h"
#include "rpgpu_dfor.h"
#include "rpgpu_launch.h"
#include "rpgpu_scan.h"

namespace rpgpu {
namespace {

static_assert(sizeof(rpgpu_rsindex_segment) == 48 && sizeof(rpgpu_rsindex_result) == 64 &&
                  sizeof(rpgpu_rsindex_query) == 32 && sizeof(rpgpu_rsindex_found) == 48,
              "offset index row layouts");

struct RsParts {
    int64_t* val[3];   // n each: the samples' rp, Kafka and file columns
    uint8_t* nbits[3]; // n / 16 + 1 each: one byte per row
    uint64_t* place;   // nsegs: rounded blob sizes, then their exclusive scan
};
// The scratch begins with n (the run has no other way to learn the plan's
// layout), so the kernels lay it out themselves.
__host__ __device__ inline size_t rs_al(size_t x) { return (x + 255) & ~(size_t)255; }
__host__ __device__ inline size_t rs_layout(void* p, uint32_t n, uint32_t nsegs, RsParts* out) {
    uint8_t* b = static_cast<uint8_t*>(p);
    size_t o = 256;
    RsParts s;
    for (int k = 0; k < 3; k++) s.val[k] = reinterpret_cast<int64_t*>(b + o), o += rs_al((size_t)n * 8);
    for (int k = 0; k < 3; k++) s.nbits[k] = b + o, o += rs_al((size_t)n / 16 + 1);
    s.place = reinterpret_cast<uint64_t*>(b + o), o += rs_al((size_t)nsegs * 8);
    if (out) *out = s;
    return o;
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int m) {
    const uint32_t lo = __shfl_xor((uint32_t)v, m, 64), hi = __shfl_xor((uint32_t)(v >> 32), m, 64);
    return ((uint64_t)hi << 32) | lo;
}
// OR over the lane's 16-lane row
__device__ __forceinline__ uint64_t row_or(uint64_t v) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) v |= shfl_xor64(v, m);
    return v;
}
// inclusive XOR scan over the wave
__device__ __forceinline__ uint64_t wave_xor_incl(uint64_t x, uint32_t lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const uint64_t y = shfl_up(x, s);
        if (lane >= (uint32_t)s) x ^= y;
    }
    return x;
}

// remote_segment_index_builder::consume_batch_start per segment
__global__ __launch_bounds__(256) void rsindex_select_kernel(const uint8_t* __restrict__ data,
                                                             const rpgpu_batch_desc* __restrict__ descs, uint32_t n,
                                                             const rpgpu_rsindex_segment* __restrict__ segs,
                                                             uint32_t nsegs, rpgpu_rsindex_result* __restrict__ results,
                                                             void* scratch) {
    // wave_item() written out: through the call, the `seg == 0 && l == 0` test below compiles differently
    const uint32_t seg = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (seg >= nsegs) return;
    const uint32_t l = lane_id();
    RsParts p;
    rs_layout(scratch, n, nsegs, &p);
    if (seg == 0 && l == 0) *static_cast<uint32_t*>(scratch) = n;
    const rpgpu_rsindex_segment sg = segs[seg];
    uint64_t delta = (uint64_t)sg.initial_delta, pos = 0;
    uint64_t wbase = 0;  // where the window restarted: the last sample's position
    uint32_t ns = 0, ncfg = 0, bad_at = 0;
    bool bad_seg = false;
    for (uint64_t c = 0; c < sg.batch_count && !bad_seg; c += 64) {
        const uint64_t k = c + l, gi = (uint64_t)sg.first_batch + k;
        bool live = k < sg.batch_count, bad = false;
        int type = 0;
        int64_t base = 0;
        uint64_t sz = 0, dl = 0;
        if (live) {
            bad = true;
            if (gi < n) {
                const rpgpu_batch_desc d = descs[gi];
                if (d.format == RPGPU_FMT_RP_DISK && d.length >= (uint32_t)kHeaderSize) {
                    const uint8_t* h = data + d.offset;
                    const int32_t size = rpdf::ld<int32_t>(h + 4);
                    if (size >= kHeaderSize) {
                        bad = false;
                        sz = (uint64_t)size;
                        base = rpdf::ld<int64_t>(h + 8);
                        type = (int8_t)h[16];
                        dl = (uint64_t)((int64_t)rpdf::ld<int32_t>(h + 23) + 1);
                    }
                }
            }
        }
        const uint64_t badm = __ballot(live && bad);
        if (badm) {  // the batches in front of the first bad one still count
            const uint32_t kb = (uint32_t)__builtin_ctzll(badm);
            bad_seg = true, bad_at = (uint32_t)(sg.first_batch + c + kb);
            live = live && l < kb;
        }
        if (!live) sz = 0;
        const bool cfg = live && rpdf::is_config(type);
        if (!cfg) dl = 0;
        const uint64_t D = wave_scan_incl(dl, l), S = wave_scan_incl(sz, l);  // wrapping
        const uint64_t mypos = pos + S - sz, mydelta = delta + D;
        const bool cand = live && !cfg;
        uint32_t from = 0;
        for (;;) {
            const uint64_t m = __ballot(cand && l >= from && rpdf::window_full(mypos - wbase, sg.sampling_step));
            if (!m) break;
            const int ks = __builtin_ctzll(m);
            if (l == (uint32_t)ks) {
                const uint64_t at = (uint64_t)sg.first_batch + ns;  // < n: one slot per live batch at most
                p.val[0][at] = base;
                p.val[1][at] = (int64_t)((uint64_t)base - mydelta);
                p.val[2][at] = (int64_t)mypos;
            }
            wbase = shfl64(mypos, ks);
            ns++;
            from = (uint32_t)ks + 1;
        }
        pos += shfl64(S, 63);
        delta += shfl64(D, 63);
        ncfg += (uint32_t)__popcll(__ballot(cfg));
    }
    if (l != 0) return;
    rpgpu_rsindex_result o;
    o.status = bad_seg ? RPGPU_RSINDEX_BAD_BATCH : RPGPU_RSINDEX_OK;
    o.samples = ns, o.rows = ns / rpdf::kRow, o.config_batches = ncfg, o.bad_batch = bad_at;
    o.rp_bytes = 0, o.kaf_bytes = 0, o.file_bytes = 0, o.out_bytes = 0, o.reserved = 0;
    o.final_delta = (int64_t)delta;
    o.stream_bytes = pos;
    o.out_offset = 0;
    results[seg] = o;
}

// The lane's sample of row `row` (element e) and the one in front of it, per
// stream, as the deltas delta_xor / delta_delta encode.  dok: the file delta
// passes delta_delta::encode's assertions.
struct RsDeltas {
    uint64_t b[3];
    bool dok;
};
__device__ __forceinline__ RsDeltas row_deltas(const RsParts& p, const rpgpu_rsindex_segment& sg, uint64_t row,
                                               uint32_t e, bool live) {
    RsDeltas r;
    r.dok = true;
    const uint64_t idx = row * rpdf::kRow + e, at = (uint64_t)sg.first_batch + idx;
    const int64_t init[3] = {sg.base_rp_offset, sg.base_kafka_offset, 0};
#pragma unroll
    for (int s = 0; s < 3; s++) {
        const uint64_t v = live ? (uint64_t)p.val[s][at] : 0;
        uint64_t prev = shfl_up(v, 1);
        if (live && e == 0) prev = idx == 0 ? (uint64_t)init[s] : (uint64_t)p.val[s][at - 1];
        if (s == 2) {
            r.b[s] = rpdf::delta_delta(v, prev, (uint64_t)sg.file_pos_step);
            r.dok = !live || rpdf::delta_ok((int64_t)v, (int64_t)prev, sg.file_pos_step);
        } else {
            r.b[s] = rpdf::delta_xor(v, prev);
        }
        if (!live) r.b[s] = 0;
    }
    return r;
}

__global__ __launch_bounds__(256) void rsindex_width_kernel(const rpgpu_rsindex_segment* __restrict__ segs,
                                                            uint32_t nsegs, rpgpu_rsindex_result* __restrict__ results,
                                                            void* scratch, uint32_t n) {
    const uint32_t seg = wave_item();
    if (seg >= nsegs) return;
    const uint32_t l = lane_id(), e = l & 15u;
    RsParts p;
    rs_layout(scratch, n, nsegs, &p);
    const rpgpu_rsindex_segment sg = segs[seg];
    const rpgpu_rsindex_result r = results[seg];
    if (r.status != RPGPU_RSINDEX_OK) {
        if (l == 0) p.place[seg] = 0;
        return;
    }
    const uint64_t slot = sg.first_batch / rpdf::kRow;  // rows <= batch_count / 16: slices do not meet
    uint64_t sum[3] = {0, 0, 0};
    bool asserted = false;
    for (uint64_t R = 0; R < r.rows; R += 4) {
        const uint64_t row = R + (l >> 4);
        const bool live = row < r.rows;
        const RsDeltas d = row_deltas(p, sg, row, e, live);
        asserted = asserted || __ballot(!d.dok) != 0;
#pragma unroll
        for (int s = 0; s < 3; s++) {
            const uint32_t nb = rpdf::width(row_or(d.b[s]));
            if (live && e == 0) {
                p.nbits[s][slot + row] = (uint8_t)nb;
                sum[s] += rpdf::row_bytes(nb);
            }
        }
    }
#pragma unroll
    for (int s = 0; s < 3; s++) sum[s] = shfl64(wave_scan_incl(sum[s], l), 63);
    if (l != 0) return;
    rpgpu_rsindex_result& o = results[seg];
    if (asserted) {
        o.status = RPGPU_RSINDEX_DELTA_ASSERT;
        p.place[seg] = 0;
        return;
    }
    o.rp_bytes = (uint32_t)sum[0], o.kaf_bytes = (uint32_t)sum[1], o.file_bytes = (uint32_t)sum[2];
    const uint64_t total = rpdf::kMinBlob + sum[0] + sum[1] + sum[2];
    o.out_bytes = (uint32_t)total;
    p.place[seg] = (total + 15) & ~(uint64_t)15;
}

__global__ __launch_bounds__(kScanBlock) void rsindex_place_kernel(rpgpu_rsindex_result* __restrict__ results,
                                                                   uint32_t nsegs, uint64_t* __restrict__ place,
                                                                   uint64_t* __restrict__ totals) {
    __shared__ uint64_t part[kScanBlock];
    __shared__ unsigned long long need, samples;
    if (threadIdx.x == 0) need = 0, samples = 0;
    (void)array_scan_excl(place, place, nsegs, part);  // ends in a barrier
    for (uint32_t k = threadIdx.x; k < nsegs; k += kScanBlock) {
        rpgpu_rsindex_result& o = results[k];
        o.out_offset = place[k];
        if (o.status == RPGPU_RSINDEX_OK) {
            atomicMax(&need, (unsigned long long)(place[k] + o.out_bytes));
            atomicAdd(&samples, (unsigned long long)o.samples);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) totals[0] = need, totals[1] = samples;
}

// offset_index::to_iobuf per segment
__global__ __launch_bounds__(256) void rsindex_emit_kernel(const rpgpu_rsindex_segment* __restrict__ segs,
                                                           uint32_t nsegs, rpgpu_rsindex_result* __restrict__ results,
                                                           uint8_t* __restrict__ out, uint64_t out_cap, void* scratch) {
    const uint32_t seg = wave_item();
    if (seg >= nsegs) return;
    const uint32_t l = lane_id(), e = l & 15u;
    RsParts p;
    rs_layout(scratch, *static_cast<const uint32_t*>(scratch), nsegs, &p);
    const rpgpu_rsindex_segment sg = segs[seg];
    const rpgpu_rsindex_result r = results[seg];
    if (r.status != RPGPU_RSINDEX_OK && r.status != RPGPU_RSINDEX_NO_ROOM) return;
    const bool fits = r.out_offset <= out_cap && r.out_bytes <= out_cap - r.out_offset;
    if (l == 0) results[seg].status = fits ? RPGPU_RSINDEX_OK : RPGPU_RSINDEX_NO_ROOM;
    if (!fits) return;
    uint8_t* o = out + r.out_offset;
    const uint64_t first = sg.first_batch;
    // ---- envelope, header fields, write buffers: one int64 field per lane
    if (l < rpdf::kFields) {
        int64_t v = 0;
        // the lane's stream: fields 2..7 are base and last per stream, 8.. the write buffers
        const uint32_t s = l < 8 ? (l - 2) >> 1 : (l - 8) / rpdf::kRow;
        const int64_t* col = s == 0 ? p.val[0] : (s == 1 ? p.val[1] : p.val[2]);
        if (l < 8) {
            if (l == 0) v = sg.file_pos_step;
            else if (l == 1) v = (int64_t)r.samples;
            else if (!(l & 1u)) v = s == 0 ? sg.base_rp_offset : (s == 1 ? sg.base_kafka_offset : 0);
            else if (r.rows) v = col[first + (uint64_t)r.rows * rpdf::kRow - 1];
            else v = s == 0 ? sg.base_rp_offset : (s == 1 ? sg.base_kafka_offset : 0);
        } else {
            uint64_t idx;
            if (rpdf::slot_sample(r.samples, (l - 8) % rpdf::kRow, &idx)) v = col[first + idx];
        }
        rpdf::st<int64_t>(o + rpdf::field_offset(l), v);
    } else if (l == 56) {
        o[0] = 1, o[1] = 1;
        rpdf::st<uint32_t>(o + 2, r.out_bytes - 6);
    } else if (l < 60) {
        rpdf::st<uint32_t>(o + rpdf::count_offset(l - 57), rpdf::kRow);
    } else if (l == 60) {
        rpdf::st<uint32_t>(o + rpdf::kHeaderEnd, r.rp_bytes);
    } else if (l == 61) {
        rpdf::st<uint32_t>(o + rpdf::kHeaderEnd + 4 + r.rp_bytes, r.kaf_bytes);
    } else if (l == 62) {
        rpdf::st<uint32_t>(o + rpdf::kHeaderEnd + 8 + (uint64_t)r.rp_bytes + r.kaf_bytes, r.file_bytes);
    }
    // ---- the three streams
    const uint64_t sbase[3] = {rpdf::kHeaderEnd + 4, rpdf::kHeaderEnd + 8 + (uint64_t)r.rp_bytes,
                               rpdf::kHeaderEnd + 12 + (uint64_t)r.rp_bytes + r.kaf_bytes};
    const uint64_t slot = first / rpdf::kRow;
    uint64_t carry[3] = {0, 0, 0};
    for (uint64_t G = 0; G < r.rows; G += 64) {
        uint32_t nbw[3];
        uint64_t off[3];
#pragma unroll
        for (int s = 0; s < 3; s++) {
            nbw[s] = G + l < r.rows ? p.nbits[s][slot + G + l] : 0u;
            const uint64_t sz = G + l < r.rows ? rpdf::row_bytes(nbw[s]) : 0u;
            const uint64_t inc = wave_scan_incl(sz, l);
            off[s] = carry[s] + inc - sz;
            carry[s] += shfl64(inc, 63);
        }
        for (uint32_t t = 0; t < 16 && G + 4 * t < r.rows; t++) {
            const int src = (int)(4 * t + (l >> 4));
            const uint64_t row = G + (uint32_t)src;
            const bool live = row < r.rows;
            const RsDeltas d = row_deltas(p, sg, row, e, live);
#pragma unroll
            for (int s = 0; s < 3; s++) {
                const uint32_t nb = (uint32_t)__shfl((int)nbw[s], src, 64);
                uint8_t* rowp = o + sbase[s] + shfl64(off[s], src);
                uint32_t rem = 0;
                if (live) {
                    if (e == 0) rowp[0] = (uint8_t)nb;
                    rem = (uint32_t)rpdf::elem_put(rowp + 1, nb, e, d.b[s]);
                }
                const uint32_t rb = rpdf::rem_bits(nb);
                const uint32_t byte = rpdf::rem_byte(rb ? rb : 1u, e, [&](uint32_t i) {
                    return (uint32_t)__shfl((int)rem, (int)((l & ~15u) + i), 64);
                });
                if (live && e < 2 * rb) rowp[1 + rpdf::rem_offset(nb) + e] = (uint8_t)byte;
            }
        }
    }
}

// ------------------------------------------------------------------- find
// A stream's nbits chain, walked over a 256-byte window held one dword per lane.
struct RsWalk {
    const uint8_t* s;
    uint32_t len;
    uint64_t p;       // the next row's start
    uint64_t cbase;   // stream offset of the window
    uint32_t chunk;
    bool loaded;
};
__device__ __forceinline__ uint32_t walk_byte(RsWalk& w, uint32_t l) {  // w.p < w.len
    if (!w.loaded || w.p < w.cbase || w.p >= w.cbase + 256) {
        w.cbase = w.p, w.loaded = true;
        const uint64_t at = w.cbase + 4ull * l;
        uint32_t v = 0;
        if (at + 4 <= w.len) {
            v = rpdf::ld<uint32_t>(w.s + at);
        } else {
            for (uint32_t k = 0; k < 4; k++)
                if (at + k < w.len) v |= (uint32_t)w.s[at + k] << (8 * k);
        }
        w.chunk = v;
    }
    const uint32_t rel = __builtin_amdgcn_readfirstlane((uint32_t)(w.p - w.cbase));
    return (__builtin_amdgcn_readlane(w.chunk, rel >> 2) >> (8 * (rel & 3u))) & 255u;
}

enum { kRsValidate = 0, kRsSearch = 1, kRsFetch = 2 };
struct RsHit {
    bool have;
    uint64_t ix;
    int64_t value;
};
// Walks all `rows` rows of a stream (false: the chain leaves it) and decodes
// while the mode needs it: kRsSearch: the last element < bound, stopping at the
// first >= bound (_find_under); kRsFetch: element `target` (_fetch_ix).
template <bool FILE_STREAM>
__device__ __forceinline__ bool scan_stream(const uint8_t* s, uint32_t len, uint64_t rows, int64_t initial,
                                            int64_t step, int mode, int64_t bound, uint64_t target, RsHit* hit,
                                            uint32_t l) {
    RsWalk w{s, len, 0, 0, 0, false};
    uint64_t carry = (uint64_t)initial;
    bool active = mode != kRsValidate;
    const uint32_t e = l & 15u;
    for (uint64_t R = 0; R < rows; R += 64) {
        uint32_t cnt = 0, mystart = 0, mynb = 0;
        while (cnt < 64 && R + cnt < rows) {
            if (w.p >= len) return false;
            const uint32_t nb = walk_byte(w, l);
            if (nb > 64 || w.p + rpdf::row_bytes(nb) > len) return false;
            if (l == cnt) mystart = (uint32_t)w.p, mynb = nb;
            w.p += rpdf::row_bytes(nb);
            cnt++;
        }
        for (uint32_t t = 0; active && 4 * t < cnt; t++) {
            const int src = (int)(4 * t + (l >> 4));
            const bool live = (uint32_t)src < cnt;
            const uint32_t st = (uint32_t)__shfl((int)mystart, src, 64), nb = (uint32_t)__shfl((int)mynb, src, 64);
            uint64_t x = live ? rpdf::elem_get(s + st + 1, nb, e) : 0;
            uint64_t v;
            if (FILE_STREAM) {
                if (live) x += (uint64_t)step;
                v = carry + wave_scan_incl(x, l);
            } else {
                v = carry ^ wave_xor_incl(x, l);
            }
            const uint32_t left = cnt - 4 * t, nlive = (left < 4 ? left : 4) * rpdf::kRow;
            carry = shfl64(v, (int)nlive - 1);
            const uint64_t first = (R + 4 * t) * rpdf::kRow;
            if (mode == kRsSearch) {
                const uint64_t ge = __ballot(live && (int64_t)v >= bound);
                const uint32_t below = ge ? (uint32_t)__builtin_ctzll(ge) : nlive;
                if (below) {
                    hit->have = true, hit->ix = first + below - 1;
                    hit->value = (int64_t)shfl64(v, (int)below - 1);
                }
                if (ge) active = false;
            } else if (target < first + nlive) {
                hit->have = true, hit->ix = target;
                hit->value = (int64_t)shfl64(v, (int)(target - first));
                active = false;
            }
        }
    }
    return true;
}

__global__ __launch_bounds__(256) void rsindex_find_kernel(const uint8_t* __restrict__ blobs,
                                                           const rpgpu_rsindex_query* __restrict__ queries, uint32_t nq,
                                                           rpgpu_rsindex_found* __restrict__ found) {
    const uint32_t qi = wave_item();
    if (qi >= nq) return;
    const uint32_t l = lane_id();
    const rpgpu_rsindex_query q = queries[qi];
    rpgpu_rsindex_found o;
    o.status = RPGPU_RSINDEX_BAD_BLOB, o.from_write_buffer = 0, o.ix = 0;
    o.rp_offset = 0, o.kaf_offset = 0, o.file_pos = 0, o.reserved = 0;
    rpdf::View v;
    bool ok = rpdf::blob_parse(blobs + q.blob_offset, q.blob_bytes, &v);
    if (ok) {
        const uint64_t rows = v.elements / rpdf::kRow;
        const uint32_t qs = q.by_rp ? 0u : 1u, other = 1u - qs;
        RsHit hit{false, 0, 0};
        ok = scan_stream<false>(v.stream[qs], v.len[qs], rows, v.base[qs], 0, kRsSearch, q.upper_bound, 0, &hit, l);
        bool from_wb = false;
        uint32_t slot = 0;
        if (ok && (!hit.have || hit.ix == rows * rpdf::kRow - 1)) {
            const uint32_t end = (uint32_t)(v.elements & (rpdf::kRow - 1));
            const bool under = l < end && rpdf::ld<int64_t>(v.wb[qs] + 8 * (l & 15u)) < q.upper_bound;
            const uint32_t run = (uint32_t)__builtin_ctzll(~__ballot(under) | (1ull << 16));
            if (run) from_wb = true, slot = run - 1;
        }
        const bool fetch = ok && hit.have && !from_wb;
        RsHit ho{false, 0, 0}, hf{false, 0, 0};
        ok = ok && scan_stream<false>(v.stream[other], v.len[other], rows, v.base[other], 0,
                                      fetch ? kRsFetch : kRsValidate, 0, hit.ix, &ho, l);
        ok = ok && scan_stream<true>(v.stream[2], v.len[2], rows, v.base[2], v.step, fetch ? kRsFetch : kRsValidate, 0,
                                     hit.ix, &hf, l);
        if (ok) {
            if (from_wb) {
                o.status = RPGPU_RSINDEX_FOUND, o.from_write_buffer = 1, o.ix = slot;
                o.rp_offset = rpdf::ld<int64_t>(v.wb[0] + 8 * slot);
                o.kaf_offset = rpdf::ld<int64_t>(v.wb[1] + 8 * slot);
                o.file_pos = rpdf::ld<int64_t>(v.wb[2] + 8 * slot);
            } else if (hit.have) {
                o.status = RPGPU_RSINDEX_FOUND, o.ix = hit.ix;
                o.rp_offset = qs == 0 ? hit.value : ho.value;
                o.kaf_offset = qs == 0 ? ho.value : hit.value;
                o.file_pos = hf.value;
            } else {
                o.status = RPGPU_RSINDEX_NONE;
            }
        }
    }
    if (l == 0) found[qi] = o;
}

}  // namespace

size_t rsindex_scratch_bytes(uint32_t n, uint32_t nsegs) { return rs_layout(nullptr, n, nsegs, nullptr); }

hipError_t launch_rsindex_plan(const uint8_t* d_data, const rpgpu_batch_desc* d_descs, uint32_t n,
                               const rpgpu_rsindex_segment* d_segs, uint32_t nsegs, rpgpu_rsindex_result* d_results,
                               uint64_t* d_totals, void* d_scratch, hipStream_t s) {
    hipError_t e = hipMemsetAsync(d_totals, 0, 2 * sizeof(uint64_t), s);
    if (e != hipSuccess) return e;
    if (nsegs == 0) return hipSuccess;
    RsParts p;
    rs_layout(d_scratch, n, nsegs, &p);
    const uint32_t grid = wave_grid(nsegs);
    rsindex_select_kernel<<<grid, 256, 0, s>>>(d_data, d_descs, n, d_segs, nsegs, d_results, d_scratch);
    RPGPU_LAUNCH_CHECK();
    rsindex_width_kernel<<<grid, 256, 0, s>>>(d_segs, nsegs, d_results, d_scratch, n);
    RPGPU_LAUNCH_CHECK();
    rsindex_place_kernel<<<1, kScanBlock, 0, s>>>(d_results, nsegs, p.place, d_totals);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_rsindex_run(const rpgpu_rsindex_segment* d_segs, uint32_t nsegs, rpgpu_rsindex_result* d_results,
                              uint8_t* d_out, uint64_t out_cap, void* d_scratch, hipStream_t s) {
    if (nsegs == 0) return hipSuccess;
    rsindex_emit_kernel<<<wave_grid(nsegs), 256, 0, s>>>(d_segs, nsegs, d_results, d_out, out_cap, d_scratch);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_rsindex_find(const uint8_t* d_blobs, const rpgpu_rsindex_query* d_queries, uint32_t nq,
                               rpgpu_rsindex_found* d_found, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    rsindex_find_kernel<<<wave_grid(nq), 256, 0, s>>>(d_blobs, d_queries, nq, d_found);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace rpgpu
