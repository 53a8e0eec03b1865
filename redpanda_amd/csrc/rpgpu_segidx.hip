// rpgpu_segidx.hip — the segment index's life cycle (include/rpgpu.h, "segment
// index life cycle"): maybe_track from any state, serde::to_iobuf(index_state),
// materialize_index_from_file, and the three lookups.  The recurrence, the blob
// layout, the parser's order of events, XXH64 and the lookups live in
// rpgpu_segidx.h, which the host program tests/native/segidx_host.cpp compiles too.
//
// Track:
//   segidx_track_kernel    one lane per segment, as segment_index_kernel
//                          (rpgpu_index.hip): a scan with data-dependent resets.
//                          The state row is read, carried in registers, written
//                          back; entries go behind the ones the slot holds.
// Write plan:
//   segidx_place_kernel    one workgroup: a contiguous run of states per thread,
//                          the 16-byte-rounded blob sizes through block_scan_excl
//                          (rpgpu_scan.h), the rows, the total.
// Write run:
//   segidx_emit_kernel     one wavefront per state.  The twelve scalar pieces of the
//                          envelope and of tmp: one per lane.  The columns are
//                          the transposition of the 16-byte entries: 64 entries
//                          per trip, one dwordx4 load per lane, then one store
//                          per lane and column, so each column's stores cover
//                          256 / 256 / 512 contiguous bytes.
//   segidx_crc_kernel      one wavefront per written blob: crc_range_wave over
//                          tmp (the strided rows of the validation kernel), the
//                          CRC behind it.  A launch of its own, so the bytes it
//                          reads are the emit kernel's finished stores.
// Hydrate:
//   segidx_hydrate_kernel  one wavefront per file.  parse_head on every lane
//                          (wave-uniform), then the checksum: crc_range_wave over
//                          tmp, or XXH64's four accumulators on lanes 0..3 and
//                          the merge; parse_body; then the columns back into
//                          16-byte entries, 64 per trip, one dwordx4 store per
//                          lane.  State row and entries are written on OK only.
// Find:
//   segidx_find_kernel     one lane per query (rpsx::find).
//
// Known bound: one state is written and hydrated by one wave.
#include "rpgpu_device.h"
#include "rpgpu_launch.h"
#include "rpgpu_scan.h"
#include "rpgpu_segidx.h"

namespace rpgpu {
namespace {

static_assert(sizeof(rpgpu_segidx_state) == 80 && sizeof(rpgpu_segidx_tracked) == 16 &&
                  sizeof(rpgpu_segidx_blob) == 32 && sizeof(rpgpu_segidx_file) == 16 &&
                  sizeof(rpgpu_segidx_hydrated) == 16 && sizeof(rpgpu_segidx_query) == 16 &&
                  sizeof(rpgpu_segidx_found) == 32 && sizeof(rpgpu_index_entry) == 16,
              "segment index row layouts");

// segment_index::maybe_track per segment, from the segment's state
__global__ __launch_bounds__(256) void segidx_track_kernel(const rpgpu_batch_desc* __restrict__ descs,
                                                           const rpgpu_batch_result* __restrict__ res, uint32_t n,
                                                           const rpgpu_segment* __restrict__ segs, uint32_t nsegs,
                                                           rpgpu_segidx_state* __restrict__ states,
                                                           rpgpu_index_entry* __restrict__ entries, uint64_t nentries,
                                                           rpgpu_segidx_tracked* __restrict__ tracked) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsegs) return;
    const rpgpu_segment g = segs[s];
    rpgpu_segidx_state st = states[s];
    rpgpu_segidx_tracked o;
    o.status = RPGPU_V_OK, o.tracked = 0, o.added = 0, o.reserved = 0;
    if (!rpsx::slot_ok(st, nentries) || (uint64_t)g.first_batch + g.batch_count > n) {
        o.status = RPGPU_V_INDEX_BAD_STATE;
        tracked[s] = o;
        return;
    }
    rpgpu_index_entry* e = entries + st.entry_first;
    const uint32_t had = st.entries;
    for (uint32_t k = 0; k < g.batch_count; k++) {
        const rpgpu_batch_result r = res[g.first_batch + k];
        if (r.verdict != RPGPU_V_OK) break;  // recovery stops at the first bad batch
        rpsx::Batch b;
        b.base_offset = r.base_offset, b.first_timestamp = r.first_timestamp, b.max_timestamp = r.max_timestamp;
        b.size_bytes = r.size_bytes, b.last_offset_delta = r.last_offset_delta;
        b.user_data = g.internal_topic || r.type == 1;  // raft_data
        b.position = descs[g.first_batch + k].offset - g.file_base;
        o.status = rpsx::track_step(&st, e, g.step, b);
        if (o.status != RPGPU_V_OK) break;
        o.tracked++;
    }
    o.added = st.entries - had;
    states[s] = st;
    tracked[s] = o;
}

// the blobs' places: status, size, an exclusive scan of the rounded sizes, the total
__global__ __launch_bounds__(kScanBlock) void segidx_place_kernel(const rpgpu_segidx_state* __restrict__ states,
                                                                  uint32_t nstates, uint64_t nentries,
                                                                  rpgpu_segidx_blob* __restrict__ blobs,
                                                                  uint64_t* __restrict__ totals) {
    __shared__ uint64_t wsum[kScanBlock / 64];
    __shared__ unsigned long long need;
    if (threadIdx.x == 0) need = 0;
    const uint32_t per = (nstates + kScanBlock - 1) / kScanBlock;
    const uint64_t lo64 = (uint64_t)threadIdx.x * per;
    const uint32_t lo = lo64 < nstates ? (uint32_t)lo64 : nstates, hi = nstates - lo < per ? nstates : lo + per;
    auto size_of = [&](uint32_t k, int32_t* status, uint32_t* entries) -> uint64_t {
        const rpgpu_segidx_state st = states[k];
        *entries = st.entries;
        *status = !rpsx::slot_ok(st, nentries) ? RPGPU_SEGIDX_BAD_STATE
                                               : (rpsx::too_big(st.entries) ? RPGPU_SEGIDX_TOO_BIG : RPGPU_SEGIDX_OK);
        return *status == RPGPU_SEGIDX_OK ? rpsx::blob_bytes(st.entries) : 0;
    };
    uint64_t sum = 0;
    int32_t status;
    uint32_t entries;
    for (uint32_t k = lo; k < hi; k++) sum += (size_of(k, &status, &entries) + 15) & ~(uint64_t)15;
    uint64_t at = block_scan_excl(sum, wsum);  // a barrier: `need` is zero for everyone
    unsigned long long end = 0;
    for (uint32_t k = lo; k < hi; k++) {
        const uint64_t bytes = size_of(k, &status, &entries);
        rpgpu_segidx_blob b;
        b.status = status, b.entries = entries, b.out_bytes = bytes, b.out_offset = at, b.reserved = 0;
        blobs[k] = b;
        if (status == RPGPU_SEGIDX_OK) end = at + bytes;
        at += (bytes + 15) & ~(uint64_t)15;
    }
    if (end) atomicMax(&need, end);
    __syncthreads();
    if (threadIdx.x == 0) totals[0] = need;
}

// a planned blob the run writes: OK or NO_ROOM rows, decided again by every run
__device__ __forceinline__ bool blob_fits(const rpgpu_segidx_blob& b, uint64_t out_cap) {
    return b.out_offset <= out_cap && b.out_bytes <= out_cap - b.out_offset;
}

// serde::to_iobuf(index_state) per state, all but the CRC
__global__ __launch_bounds__(256) void segidx_emit_kernel(const rpgpu_segidx_state* __restrict__ states,
                                                          uint32_t nstates,
                                                          const rpgpu_index_entry* __restrict__ entries,
                                                          uint64_t nentries, rpgpu_segidx_blob* __restrict__ blobs,
                                                          uint8_t* __restrict__ out, uint64_t out_cap) {
    const uint32_t si = wave_item();
    if (si >= nstates) return;
    const uint32_t l = lane_id();
    const rpgpu_segidx_blob b = blobs[si];
    if (b.status != RPGPU_SEGIDX_OK && b.status != RPGPU_SEGIDX_NO_ROOM) return;
    const rpgpu_segidx_state st = states[si];
    // the plan's row and the state still agree, and the slot lies in the array
    const bool fits = blob_fits(b, out_cap) && rpsx::slot_ok(st, nentries) && !rpsx::too_big(st.entries) &&
                      b.entries == st.entries && b.out_bytes == rpsx::blob_bytes(st.entries);
    if (l == 0) blobs[si].status = fits ? RPGPU_SEGIDX_OK : RPGPU_SEGIDX_NO_ROOM;
    if (!fits) return;
    const uint64_t n = st.entries;
    uint8_t* o = out + b.out_offset;
    uint8_t* t = o + rpsx::kTmpAt;
    if (l == 0) {
        o[0] = 5, o[1] = 4;
    } else if (l == 1) {
        rpsx::st<uint32_t>(o + 2, (uint32_t)(b.out_bytes - 6));
    } else if (l == 2) {
        rpsx::st<uint32_t>(o + 6, (uint32_t)rpsx::tmp_bytes(n));
    } else if (l == 3) {
        rpsx::st<uint32_t>(t, st.bitflags);
    } else if (l < 8) {
        rpsx::st<int64_t>(t + rpsx::scalar_at(l - 4), rpsx::scalar(st, l - 4));
    } else if (l < 11) {
        rpsx::st<uint32_t>(t + rpsx::count_at(l - 8, n), (uint32_t)n);
    } else if (l == 11) {
        uint8_t* f = t + rpsx::flags_at(n);
        f[0] = st.monotonic, f[1] = st.with_offset, f[2] = st.non_data_timestamps;
    }
    const uint8_t* e = reinterpret_cast<const uint8_t*>(entries + st.entry_first);
    uint8_t* c0 = t + rpsx::column_at(0, n);
    uint8_t* c1 = t + rpsx::column_at(1, n);
    uint8_t* c2 = t + rpsx::column_at(2, n);
    for (uint64_t i = l; i < n; i += 64) {
        const u32x4 x = ld16(e + 16 * i);
        rpsx::st<uint32_t>(c0 + 4 * i, x.x);
        rpsx::st<uint32_t>(c1 + 4 * i, x.y);
        rpsx::st<u32x2>(c2 + 8 * i, (u32x2){x.z, x.w});
    }
}

// the CRC of every blob the emit kernel wrote
__global__ __launch_bounds__(kValidateThreads) void segidx_crc_kernel(const rpgpu_segidx_blob* __restrict__ blobs,
                                                                      uint32_t nstates, uint8_t* out,
                                                                      const uint32_t* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kTableWords];
    load_tables(sT, tables);
    const uint32_t si = wave_item();
    if (si >= nstates) return;
    const uint32_t l = lane_id();
    const rpgpu_segidx_blob b = blobs[si];
    if (b.status != RPGPU_SEGIDX_OK) return;
    uint8_t* t = out + b.out_offset + rpsx::kTmpAt;
    const int64_t L = (int64_t)rpsx::tmp_bytes(b.entries);
    const uint32_t crc = crc_range_wave(sT, t, L, ~0u, l);
    if (l == 0) rpsx::st<uint32_t>(t + L, crc);
}

// materialize_index_from_file per file
__global__ __launch_bounds__(kValidateThreads) void segidx_hydrate_kernel(
    const uint8_t* __restrict__ files, uint64_t files_bytes, const rpgpu_segidx_file* __restrict__ rows, uint32_t nfiles,
    rpgpu_segidx_state* __restrict__ states, rpgpu_index_entry* __restrict__ entries, uint64_t nentries,
    rpgpu_segidx_hydrated* __restrict__ hydrated, const uint32_t* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kTableWords];
    load_tables(sT, tables);
    const uint32_t fi = wave_item();
    if (fi >= nfiles) return;
    const uint32_t l = lane_id();
    const rpgpu_segidx_file row = rows[fi];
    rpgpu_segidx_state st = states[fi];
    rpsx::View v;
    const bool row_ok = row.blob_offset <= files_bytes && row.blob_bytes <= files_bytes - row.blob_offset &&
                        (uint64_t)st.entry_first + st.entry_cap <= nentries;
    const uint8_t* p = files + row.blob_offset;
    if (!row_ok) {
        v = rpsx::View{};
        rpsx::view_fail(&v, RPGPU_SEGIDX_BAD_STATE, RPGPU_SEGIDX_R_BAD_ROW);
    } else if (rpsx::parse_head(p, row.blob_bytes, &v)) {  // wave-uniform
        uint64_t sum;
        if (v.legacy) {
            // the hashed length is 40 + 16 n: xxh_ok holds (rpgpu_segidx.h asserts it)
            const uint64_t mine = l < 4 ? rpsx::xxh_lane(p + v.sum_at, v.sum_len, l) : 0;
            const uint64_t acc[4] = {shfl64(mine, 0), shfl64(mine, 1), shfl64(mine, 2), shfl64(mine, 3)};
            sum = rpsx::xxh_finish(acc, p + v.sum_at, v.sum_len);
        } else {
            sum = crc_range_wave(sT, p + v.sum_at, (int64_t)v.sum_len, ~0u, l);
        }
        rpsx::parse_body(p, &v, sum);
        if (v.status == RPGPU_SEGIDX_OK && v.entries > st.entry_cap)
            rpsx::view_fail(&v, RPGPU_SEGIDX_NO_ROOM, RPGPU_SEGIDX_R_ENTRY_CAP);
    }
    if (v.status == RPGPU_SEGIDX_OK) {
        rpgpu_index_entry* e = entries + st.entry_first;
        for (uint64_t i = l; i < v.entries; i += 64) e[i] = rpsx::view_entry(p, v, i);
        if (l == 0) {
            rpsx::view_state(v, &st);
            states[fi] = st;
        }
    }
    if (l == 0) {
        rpgpu_segidx_hydrated h;
        h.status = v.status, h.reason = v.reason, h.version = v.version, h.entries = v.entries;
        hydrated[fi] = h;
    }
}

__global__ __launch_bounds__(256) void segidx_find_kernel(const rpgpu_segidx_state* __restrict__ states,
                                                          uint32_t nstates,
                                                          const rpgpu_index_entry* __restrict__ entries,
                                                          uint64_t nentries,
                                                          const rpgpu_segidx_query* __restrict__ queries, uint32_t nq,
                                                          rpgpu_segidx_found* __restrict__ found) {
    const uint32_t qi = blockIdx.x * blockDim.x + threadIdx.x;
    if (qi >= nq) return;
    const rpgpu_segidx_query q = queries[qi];
    rpgpu_segidx_found o;
    o.status = RPGPU_SEGIDX_BAD_QUERY, o.ix = 0, o.offset = 0, o.timestamp = 0, o.filepos = 0;
    if (q.state < nstates) {
        const rpgpu_segidx_state st = states[q.state];
        if (rpsx::slot_ok(st, nentries)) rpsx::find(st, entries + st.entry_first, q.kind, q.key, &o);
    }
    found[qi] = o;
}

}  // namespace

hipError_t launch_segidx_track(const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res, uint32_t n,
                               const rpgpu_segment* d_segs, uint32_t nsegs, rpgpu_segidx_state* d_states,
                               rpgpu_index_entry* d_entries, uint64_t nentries, rpgpu_segidx_tracked* d_tracked,
                               hipStream_t s) {
    if (nsegs == 0) return hipSuccess;
    segidx_track_kernel<<<(nsegs + 255) / 256, 256, 0, s>>>(d_descs, d_res, n, d_segs, nsegs, d_states, d_entries,
                                                           nentries, d_tracked);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_segidx_write_plan(const rpgpu_segidx_state* d_states, uint32_t nstates, uint64_t nentries,
                                    rpgpu_segidx_blob* d_blobs, uint64_t* d_totals, hipStream_t s) {
    segidx_place_kernel<<<1, kScanBlock, 0, s>>>(d_states, nstates, nentries, d_blobs, d_totals);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_segidx_write_run(const rpgpu_segidx_state* d_states, uint32_t nstates,
                                   const rpgpu_index_entry* d_entries, uint64_t nentries, rpgpu_segidx_blob* d_blobs,
                                   uint8_t* d_out, uint64_t out_cap, const uint32_t* d_tables, hipStream_t s) {
    if (nstates == 0) return hipSuccess;
    segidx_emit_kernel<<<wave_grid(nstates), 256, 0, s>>>(d_states, nstates, d_entries, nentries, d_blobs, d_out,
                                                          out_cap);
    RPGPU_LAUNCH_CHECK();
    segidx_crc_kernel<<<wave_grid(nstates), kValidateThreads, 0, s>>>(d_blobs, nstates, d_out, d_tables);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_segidx_hydrate(const uint8_t* d_files, uint64_t files_bytes, const rpgpu_segidx_file* d_rows,
                                 uint32_t nfiles, rpgpu_segidx_state* d_states, rpgpu_index_entry* d_entries,
                                 uint64_t nentries, rpgpu_segidx_hydrated* d_hydrated, const uint32_t* d_tables,
                                 hipStream_t s) {
    if (nfiles == 0) return hipSuccess;
    segidx_hydrate_kernel<<<wave_grid(nfiles), kValidateThreads, 0, s>>>(d_files, files_bytes, d_rows, nfiles, d_states,
                                                                         d_entries, nentries, d_hydrated, d_tables);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

hipError_t launch_segidx_find(const rpgpu_segidx_state* d_states, uint32_t nstates, const rpgpu_index_entry* d_entries,
                              uint64_t nentries, const rpgpu_segidx_query* d_queries, uint32_t nq,
                              rpgpu_segidx_found* d_found, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    segidx_find_kernel<<<(nq + 255) / 256, 256, 0, s>>>(d_states, nstates, d_entries, nentries, d_queries, nq, d_found);
    RPGPU_LAUNCH_CHECK();
    return hipSuccess;
}

}  // namespace rpgpu
