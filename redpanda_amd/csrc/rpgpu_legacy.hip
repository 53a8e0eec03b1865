// rpgpu_legacy.hip — legacy (magic 0 / 1) MessageSets to v2 batches on the
// device: kafka_batch_adapter::adapt_with_version for produce versions below 3
// (kafka/protocol/kafka_batch_adapter.cc:215-301).  The walk, the verdicts and
// the record encoder are the host/device functions of rpgpu_legacy.h.
//
//   legacy_scan_kernel    one lane per set: the message chain is serial (the
//                         next message starts where the value ended), sets are
//                         independent.  Plan: message count, body size, T and
//                         the first non-CRC event.  Run: the same walk again,
//                         now filling the message table in d_out.
//   legacy_offsets_kernel exclusive scans of the output slots and of the
//                         table slices, totals for the caller (one workgroup).
//   legacy_crc_lane_kernel  CRC32 of every tabled message of the arena in
//                         parallel, 64 messages per wave: a range of at most
//                         lane_max bytes on its lane (16 bytes per step through
//                         the block nibble tables); longer ones go on a work
//                         list.  A mismatch is an atomicMin on the set's key.
//   legacy_crc_wave_kernel  the listed ranges, a wave each (crc_range_wave, the
//                         strided rows of crc_ranges_kernel).
//   legacy_finish_kernel  one lane per set: the verdict of the smallest key,
//                         the result row, the rewritten descriptor and the
//                         header with zero CRCs.
//   legacy_emit_kernel    the records of the converted sets, 64 messages per
//                         wave: varints by the message's lane, short keys and
//                         values in 16-byte pieces; long ones are listed.
//   legacy_copy_wave_kernel the listed keys and values, a wave each, 16 bytes
//                         per lane.  (The record writer of both is
//                         rpgpu_emit.h, shared with rpgpu_produce.hip.)
//   then the RECRC validation of the rewritten batches (launch_plan /
//   launch_run) and recrc_patch_kernel, which stores both CRCs
//   (launch_revalidate, rpgpu_rewrite.h).
#include "rpgpu_device.h"
#include "rpgpu_rewrite.h"
#include "rpgpu_scan.h"
#include "rpgpu_legacy.h"
#include "rpgpu_emit.h"

namespace rpgpu {

namespace {

using rplegacy::Msg;
using rplegacy::Scan;

// scratch: totals (64 B) | Scan[n] | slot_sz[n] | slot_off[n] | msg_cnt[n] |
//          msg_first[n] | recs[n] (u64 each) | ev_key[n] u32 | validation scratch
struct Parts {
    uint64_t* totals;  // 0 slots, 1 messages, 2 records; per run: 3 long CRC ranges, 4 long copies
    Scan* info;
    uint64_t *slot_sz, *slot_off, *msg_cnt, *msg_first, *recs;
    uint32_t* ev_key;
    void* vscratch;
};
size_t vscratch_offset(uint32_t n) {
    return (64 + (size_t)n * (sizeof(Scan) + 5 * 8 + 4) + 255) & ~(size_t)255;
}
Parts parts(void* d_scratch, uint32_t n) {
    uint8_t* sc = static_cast<uint8_t*>(d_scratch);
    Parts p;
    p.totals = reinterpret_cast<uint64_t*>(sc);
    p.info = reinterpret_cast<Scan*>(sc + 64);
    p.slot_sz = reinterpret_cast<uint64_t*>(sc + 64 + (size_t)n * sizeof(Scan));
    p.slot_off = p.slot_sz + n;
    p.msg_cnt = p.slot_off + n;
    p.msg_first = p.msg_cnt + n;
    p.recs = p.msg_first + n;
    p.ev_key = reinterpret_cast<uint32_t*>(p.recs + n);
    p.vscratch = sc + vscratch_offset(n);
    return p;
}
static_assert(sizeof(Scan) % 8 == 0, "scratch arrays stay 8-byte aligned");

// d_out behind the slots (256-byte aligned): the message table, then the work
// list of the wave kernels, two 8-byte items per message (the long CRC ranges,
// then, once those are done, the long key / value copies)
constexpr uint64_t kMsgBytes = sizeof(Msg) + 16;
__device__ __forceinline__ uint64_t table_offset(uint64_t slots_total) { return (slots_total + 255) & ~(uint64_t)255; }
// table and list fit behind the slots (nothing to fit without messages)
__device__ __forceinline__ bool table_fits(const uint64_t* totals, uint64_t out_cap) {
    return totals[1] == 0 || table_offset(totals[0]) + totals[1] * kMsgBytes <= out_cap;
}
__device__ __forceinline__ uint64_t* work_list(uint8_t* out, const uint64_t* totals) {
    return reinterpret_cast<uint64_t*>(out + table_offset(totals[0]) + totals[1] * sizeof(Msg));
}
__global__ __launch_bounds__(256) void legacy_scan_kernel(const rpgpu_batch_desc* __restrict__ sets, uint32_t n,
                                                          const uint8_t* __restrict__ data, Parts p, uint8_t* out,
                                                          uint64_t out_cap, int run) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rpgpu_batch_desc d = sets[i];
    if (run) {
        // the table slice of the set, then the checksums' starting point
        const Scan s = p.info[i];
        if (s.ntab && table_fits(p.totals, out_cap)) {
            Msg* table = reinterpret_cast<Msg*>(out + table_offset(p.totals[0])) + p.msg_first[i];
            (void)rplegacy::scan_set(data + d.offset, d.length, d.offset, i, table, s.ntab);
        }
        p.ev_key[i] = s.key;
        return;
    }
    Scan s;
    if (d.flags & RPGPU_DESC_NULL_RECORDS) {
        s = Scan{0, 0, 0, rplegacy::kNoEvent, RPGPU_V_NULL_RECORDS, 0, 0, 0, 0};
    } else {
        s = rplegacy::scan_set(data + d.offset, d.length, d.offset, i, nullptr, 0);
    }
    p.info[i] = s;
    const bool cand = s.verdict == RPGPU_V_OK;  // converted unless a checksum fails
    p.slot_sz[i] = cand ? ((uint64_t)kHeaderSize + s.body + 63) & ~(uint64_t)63 : 0;
    p.msg_cnt[i] = s.ntab;
    p.recs[i] = cand ? s.nmsg : 0;
}

__global__ __launch_bounds__(kScanBlock) void legacy_offsets_kernel(Parts p, uint32_t n, uint64_t* out_bytes,
                                                                    uint64_t* records_total) {
    __shared__ uint64_t part[kScanBlock];
    const uint64_t slots = array_scan_excl(p.slot_sz, p.slot_off, n, part);
    const uint64_t msgs = array_scan_excl(p.msg_cnt, p.msg_first, n, part);
    const uint64_t recs = array_scan_excl<uint64_t>(p.recs, nullptr, n, part);
    if (threadIdx.x == 0) {
        p.totals[0] = slots;
        p.totals[1] = msgs;
        p.totals[2] = recs;
        if (out_bytes) *out_bytes = msgs ? table_offset(slots) + msgs * kMsgBytes : slots;
        if (records_total) *records_total = recs;
    }
}

// zlib crc32(0, p, len) on one lane: 16 bytes per step, the state folded into
// the block's first four bytes (32 conflict-free lookups in the block tables
// B), then the tail a byte at a time through the byte table's nibble halves L1
__device__ __forceinline__ uint32_t crc32_lane(const uint32_t* __restrict__ sB, const uint8_t* p, uint32_t len) {
    uint32_t c = ~0u;
    uint32_t k = 0;
    for (; k + 16 <= len; k += 16) {
        u32x4 x = ld16(p + k);
        x.x ^= c;
        c = crc_block(sB, x);
    }
    const uint32_t* sL1 = sB + (kOffL1 - kOffB);
    for (; k < len; k++) {
        c ^= p[k];
        c = (c >> 8) ^ sL1[c & 15u] ^ sL1[16 + ((c >> 4) & 15u)];
    }
    return ~c;
}

// short ranges: a lane each; the others go on the work list
__global__ __launch_bounds__(256) void legacy_crc_lane_kernel(const uint8_t* __restrict__ data, uint8_t* out, Parts p,
                                                              uint64_t out_cap, uint32_t lane_max,
                                                              const uint32_t* __restrict__ tables) {
    constexpr int kWords = kTableWords32 - kOffB;  // B and L1
    __shared__ __attribute__((aligned(16))) uint32_t sB[kWords];
    for (int i = threadIdx.x; i < kWords / 4; i += blockDim.x)
        reinterpret_cast<u32x4*>(sB)[i] = reinterpret_cast<const u32x4*>(tables + kOffB)[i];
    __syncthreads();
    if (!table_fits(p.totals, out_cap)) return;
    const uint64_t total = p.totals[1];
    const Msg* table = reinterpret_cast<const Msg*>(out + table_offset(p.totals[0]));
    uint64_t* list = work_list(out, p.totals);
    const uint32_t l = lane_id();
    const uint64_t gw = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t base = gw * 64; base < total; base += nw * 64) {
        const uint64_t m = base + l;
        const bool valid = m < total;
        bool lng = false;
        if (valid) {
            const Msg& e = table[m];
            const uint32_t len = e.crc_len;
            lng = len > lane_max;
            if (!lng && crc32_lane(sB, data + e.crc_off, len) != e.crc_expect)
                atomicMin(&p.ev_key[e.set], (e.index << 2) | rplegacy::kStageCrc);
        }
        list_append(list, p.totals + 3, lng, m, l);
    }
}

// the listed ranges: a wave each (crc_range_wave, the strided rows of
// crc_ranges_kernel), so a few long messages still spread over the device
__global__ __launch_bounds__(kValidateThreads) void legacy_crc_wave_kernel(const uint8_t* __restrict__ data,
                                                                           uint8_t* out, Parts p, uint64_t out_cap,
                                                                           const uint32_t* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kTableWords];
    for (int i = threadIdx.x; i < kTableWords / 4; i += blockDim.x)
        reinterpret_cast<u32x4*>(sT)[i] = reinterpret_cast<const u32x4*>(tables)[i];
    __syncthreads();
    if (!table_fits(p.totals, out_cap)) return;
    const uint64_t count = p.totals[3];
    const Msg* table = reinterpret_cast<const Msg*>(out + table_offset(p.totals[0]));
    const uint64_t* list = work_list(out, p.totals);
    const uint32_t l = lane_id();
    const uint64_t gw = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * kWavesPerBlock;
    for (uint64_t i = gw; i < count; i += nw) {
        const Msg& e = table[list[i]];
        const uint64_t off = uniform64(e.crc_off);
        const uint32_t len = uniform32(e.crc_len);
        const uint32_t crc = crc_range_wave(sT, data + off, (int64_t)len, ~0u, l);
        if (l == 0 && crc != e.crc_expect) atomicMin(&p.ev_key[e.set], (e.index << 2) | rplegacy::kStageCrc);
    }
}

__global__ __launch_bounds__(256) void legacy_finish_kernel(const rpgpu_batch_desc* __restrict__ sets, uint32_t n,
                                                            Parts p, int64_t now_ms, rpgpu_legacy_result* lres,
                                                            uint8_t* out, uint64_t out_cap,
                                                            rpgpu_batch_desc* out_descs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const rpgpu_batch_desc d = sets[i];
    const Scan s = p.info[i];
    const uint32_t key = p.ev_key[i];
    rpgpu_legacy_result r;
    r.verdict = RPGPU_V_NULL_RECORDS;
    r.record_count = 0;
    r.event_message = -1;
    r.codec = 0;
    r.timestamp = 0;
    r.out_offset = 0;
    r.out_len = 0;
    r.out_cap = 0;
    if (!(d.flags & RPGPU_DESC_NULL_RECORDS)) {
        if (!table_fits(p.totals, out_cap)) {
            r.verdict = RPGPU_V_DECOMP_OVERFLOW;  // no checksum was checked
        } else {
            r.verdict = rplegacy::verdict_of(s, key);
            if (key != rplegacy::kNoEvent) r.event_message = (int32_t)(key >> 2);
            if (r.verdict == RPGPU_V_LEGACY_COMPRESSED) r.codec = s.codec;
        }
    }
    if (r.verdict == RPGPU_V_OK) {
        const uint64_t off = p.slot_off[i], sz = p.slot_sz[i];
        if (off + sz > out_cap) {
            r.verdict = RPGPU_V_DECOMP_OVERFLOW;
            r.out_len = (uint64_t)kHeaderSize + s.body;
            r.out_cap = sz;
        } else {
            r.record_count = (int32_t)s.nmsg;
            r.timestamp = s.has_ts ? s.ts : now_ms;
            r.out_offset = off;
            r.out_len = (uint64_t)kHeaderSize + s.body;
            r.out_cap = sz;
            rplegacy::put_header(out + off, s.body, s.nmsg, r.timestamp);
        }
    }
    lres[i] = r;
    const bool ok = r.verdict == RPGPU_V_OK;
    rpgpu_batch_desc od;
    od.offset = r.out_offset;
    od.length = ok ? (uint32_t)r.out_len : 0u;
    od.partition = d.partition;
    od.format = RPGPU_FMT_RP_DISK;
    od.ops = ok ? (uint8_t)(RPGPU_OP_CRC | RPGPU_OP_HDRCRC | RPGPU_OP_RECRC | (d.ops & (RPGPU_OP_PARSE | RPGPU_OP_INDEX)))
                : (uint8_t)0;
    od.flags = 0;
    od.reserved = 0;
    out_descs[i] = od;
}

// where record m's key and value go
__device__ __forceinline__ RecordPlace place(const Msg& e, const rpgpu_batch_desc* __restrict__ sets,
                                             const uint8_t* __restrict__ data, const rpgpu_legacy_result& r,
                                             uint8_t* out) {
    const uint8_t* src = data + sets[e.set].offset;
    return place_record(out + r.out_offset + kHeaderSize + e.rec_off, src + e.key_off, src + e.val_off, e.rec_len,
                        e.index, e.key_len, e.val_len);
}

// the records of the converted sets, 64 messages per wave: the varints and
// the short keys / values by the message's lane, the long ones listed
__global__ __launch_bounds__(256) void legacy_emit_kernel(const rpgpu_batch_desc* __restrict__ sets,
                                                          const uint8_t* __restrict__ data, Parts p,
                                                          const rpgpu_legacy_result* __restrict__ lres, uint8_t* out,
                                                          uint64_t out_cap) {
    if (!table_fits(p.totals, out_cap)) return;
    const uint64_t total = p.totals[1];
    const Msg* table = reinterpret_cast<const Msg*>(out + table_offset(p.totals[0]));
    uint64_t* list = work_list(out, p.totals);
    const uint32_t l = lane_id();
    const uint64_t gw = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t base = gw * 64; base < total; base += nw * 64) {
        const uint64_t m = base + l;
        bool klong = false, vlong = false;
        if (m < total) {
            const Msg e = table[m];
            const rpgpu_legacy_result& r = lres[e.set];
            if (r.verdict == RPGPU_V_OK) {
                const RecordPlace q = place(e, sets, data, r, out);
                emit_record_lane(q, e.rec_len, e.index, e.key_len, e.val_len, klong, vlong);
            }
        }
        list_append(list, p.totals + 4, klong, m << 1, l);
        list_append(list, p.totals + 4, vlong, (m << 1) | 1, l);
    }
}

// the listed keys and values: a wave each
__global__ __launch_bounds__(256) void legacy_copy_wave_kernel(const rpgpu_batch_desc* __restrict__ sets,
                                                               const uint8_t* __restrict__ data, Parts p,
                                                               const rpgpu_legacy_result* __restrict__ lres,
                                                               uint8_t* out, uint64_t out_cap) {
    if (!table_fits(p.totals, out_cap)) return;
    const uint64_t count = p.totals[4];
    const Msg* table = reinterpret_cast<const Msg*>(out + table_offset(p.totals[0]));
    const uint64_t* list = work_list(out, p.totals);
    const uint32_t l = lane_id();
    const uint64_t gw = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t i = gw; i < count; i += nw) {
        const uint64_t item = list[i];
        const Msg e = table[item >> 1];
        const RecordPlace q = place(e, sets, data, lres[e.set], out);
        copy_listed(q, (item & 1) != 0, l);
    }
}

}  // namespace

size_t legacy_scratch_bytes(uint32_t n) { return vscratch_offset(n) + validate_scratch_bytes(n); }

hipError_t launch_legacy_plan(const rpgpu_batch_desc* d_sets, uint32_t n, const uint8_t* d_data,
                              uint64_t* d_out_bytes, uint64_t* d_records_total, void* d_scratch, hipStream_t s) {
    if (n == 0) {
        hipError_t e = d_out_bytes ? hipMemsetAsync(d_out_bytes, 0, sizeof(uint64_t), s) : hipSuccess;
        if (e == hipSuccess && d_records_total) e = hipMemsetAsync(d_records_total, 0, sizeof(uint64_t), s);
        return e;
    }
    const Parts p = parts(d_scratch, n);
    legacy_scan_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_sets, n, d_data, p, nullptr, 0, 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    legacy_offsets_kernel<<<1, kScanBlock, 0, s>>>(p, n, d_out_bytes, d_records_total);
    return hipGetLastError();
}

hipError_t launch_legacy_run(const rpgpu_batch_desc* d_sets, uint32_t n, const uint8_t* d_data, int64_t now_ms,
                             rpgpu_legacy_result* d_lres, uint8_t* d_out, uint64_t out_cap,
                             rpgpu_batch_desc* d_out_descs, rpgpu_batch_result* d_vres2, rpgpu_record_index* d_index,
                             uint64_t index_cap, uint64_t* d_index_used, void* d_scratch, const uint32_t* d_tables,
                             const uint32_t* d_tables32, int grid, uint32_t lane_max, hipStream_t s) {
    if (n == 0) return d_index_used ? hipMemsetAsync(d_index_used, 0, sizeof(uint64_t), s) : hipSuccess;
    const Parts p = parts(d_scratch, n);
    const uint32_t nblk = (n + 255) / 256;
    hipError_t e;
    legacy_scan_kernel<<<nblk, 256, 0, s>>>(d_sets, n, d_data, p, d_out, out_cap, 1);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemsetAsync(p.totals + 3, 0, 2 * sizeof(uint64_t), s)) != hipSuccess) return e;
    legacy_crc_lane_kernel<<<grid, 256, 0, s>>>(d_data, d_out, p, out_cap, lane_max, d_tables32);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    legacy_crc_wave_kernel<<<grid, kValidateThreads, 0, s>>>(d_data, d_out, p, out_cap, d_tables32);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    legacy_finish_kernel<<<nblk, 256, 0, s>>>(d_sets, n, p, now_ms, d_lres, d_out, out_cap, d_out_descs);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    legacy_emit_kernel<<<grid, 256, 0, s>>>(d_sets, d_data, p, d_lres, d_out, out_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    legacy_copy_wave_kernel<<<grid, 256, 0, s>>>(d_sets, d_data, p, d_lres, d_out, out_cap);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return launch_revalidate(d_out_descs, n, d_out, d_lres, d_vres2, d_index, index_cap, d_index_used, p.vscratch,
                             d_tables, grid, s);
}

}  // namespace rpgpu
