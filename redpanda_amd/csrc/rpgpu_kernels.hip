// rpgpu_kernels.hip — CDNA4 (gfx950) kernels of the record-batch engine.
//
// validate_kernel: one wavefront owns one batch at a time (grid-stride over
// the arena; 8 workgroups of 4 waves per CU, i.e. 8 waves per SIMD, which the
// kernel fits only within 64 VGPRs and without scratch memory:
// tests/test_kernel_resources.py).  32 of those registers are the rows in
// flight, so the per-batch section keeps nothing wide: the parsed header
// lives as one little-endian image from which the result fields, the header
// CRC window and the body-CRC image are read, and the batch's result is
// assembled one dword per lane and stored once.  Two passes over the arena:
//
// (1) CRC32C, all 64 lanes on one batch ("strided rows").  The Kafka CRC
// covers batch bytes [21, n) (kafka_batch_adapter.cc:99-134).  The region is
// cut into 1 KiB rows aligned to its END (the last row ends at n, so nothing
// past the batch is hashed and the tail needs no masking); row t is one
// coalesced 1 KiB load, 16 B per lane, lane l owning block 64t + l.  Each
// lane keeps its own CRC state over the blocks it owns; they are 1008 bytes
// apart, so the tables are pre-multiplied by x^(8*1008) and a lane advances
// with 32 nibble lookups per 16 bytes (16-entry tables: no LDS bank
// conflicts).  Rows are processed in straight-line chunks of kRowsPerChunk;
// the all-zero phantom rows that round a batch up to whole chunks shift
// every lane by 1 KiB each and are undone at the end (tables U).  A 6-step
// butterfly folds the 64 lane states (tables W).  Bytes [0, 61) of rows 0
// and 1 are replaced by an "image" built from the parsed header: zeros
// before 21, big-endian fields in [21, 61) as crc_record_batch_header
// hashes them (record_utils.cc:68-80), the CRC init folded into [21, 25),
// so one loop serves wire and on-disk batches.  The next chunk's (or next
// batch's) rows are loaded into the registers each row frees as it is
// checksummed, so 8 KiB per wave stay in flight.
//
// (2) Record walk (rpgpu_walk.h): walk_kernel, a separate launch with one
// lane per batch over the whole arena.  The walk is a chain of dependent
// reads; spread over a lane per batch it is hidden by occupancy instead of
// stalling the checksum stream of the wave that owns the batch.
//
// RPGPU_OP_RECRC (the rewritten batches of rpgpu_decomp_run_device): the
// header CRC is not checked but computed after the Kafka CRC, over a header
// that carries the computed crc (parser_utils.cc:122-128).
#include "rpgpu_device.h"
#include "rpgpu_launch.h"
#include "rpgpu_scan.h"
#include "rpgpu_walk.h"

namespace rpgpu {

// Diagnostics build only (scripts/diag_build.sh STAMPS): per-phase wave
// cycles from s_memtime, summed over all waves into g_stamps.
#ifdef RPGPU_DIAG_STAMPS
__device__ unsigned long long g_stamps[8];
struct Stamps {
    uint64_t st[8];
    uint64_t prev;
};
#define DIAG_PARAM , Stamps& sp
#define DIAG_PASS , sp
#define STAMP(i)                                          \
    do {                                                  \
        const uint64_t _t = __builtin_amdgcn_s_memtime(); \
        sp.st[i] += _t - sp.prev;                         \
        sp.prev = _t;                                     \
    } while (0)
#else
#define DIAG_PARAM
#define DIAG_PASS
#define STAMP(i) \
    do {         \
    } while (0)
#endif

// v with lane i < 16 holding dword i of the wave-uniform image
__device__ __forceinline__ uint32_t lanes16(const Img64& I) {
    uint32_t v = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) v = writelane(v, I.w[i], i);
    return v;
}

// A batch's rpgpu_batch_result is assembled one dword per lane (lanes 0..15
// of one VGPR) and leaves as a single 64-byte store: sixteen wave-uniform
// values held until the end of the batch would cost the row loop sixteen
// registers.
enum : int {
    kResVerdict = 0,
    kResCrc = 1,
    kResCrcExpected = 2,
    kResHeaderCrc = 3,
    kResSizeBytes = 4,
    kResRecordCount = 5,
    kResBaseOffset = 6,  // and 7
    kResLastOffsetDelta = 8,
    kResAttrsCodecType = 9,
    kResFirstTs = 10,  // and 11
    kResMaxTs = 12,    // and 13
    kResIndexFirst = 14,
    kResIndexCount = 15,
};
__device__ __forceinline__ void store_result(rpgpu_batch_result* out, uint32_t rv) {
    static_assert(sizeof(rpgpu_batch_result) == 64, "result layout");
    const uint32_t l = lane_id();
    if (l < 16) reinterpret_cast<uint32_t*>(out)[l] = rv;
}

// header CRC over image D[4..61) (internal_header_only_crc,
// record_utils.cc:34-55), D given one dword per lane (lanes 0..15 of dv):
// the 64-byte right-aligned window [7 zero bytes | D[4..61)], init folded
// into D[4..8), one byte per lane through the lane-minor tables HB (2
// conflict-free lookups), then an XOR reduction over the wave.
__device__ __forceinline__ uint32_t header_crc_lanes(const uint32_t* sT, uint32_t dv) {
    const uint32_t l = lane_id();
    // lane l hashes window byte l = D byte l - 3 (lanes 0..6: the zero bytes)
    const int32_t k = (int32_t)l - 3;
    const uint32_t w = __builtin_amdgcn_ds_bpermute((k >> 2) << 2, dv);
    uint32_t byte = (w >> (8 * (k & 3))) & 255u;
    byte = l < 7 ? 0u : (l < 11 ? byte ^ 255u : byte);
    const uint32_t* hb = sT + kOffHB + l;
    uint32_t c = hb[(byte & 15u) * 64] ^ hb[(16u + (byte >> 4)) * 64];
    c ^= row_shl<1>(c);
    c ^= row_shl<2>(c);
    c ^= row_shl<4>(c);
    c ^= row_shl<8>(c);
    return ~(rdl(c, 0) ^ rdl(c, 16) ^ rdl(c, 32) ^ rdl(c, 48));
}
__device__ __forceinline__ uint32_t header_crc_vec(const uint32_t* sT, const Img64& D) {
    return header_crc_lanes(sT, lanes16(D));
}

// Row geometry of the CRC region [21, n) of a batch: 1 KiB rows aligned to
// the region's END (row k covers batch bytes [g0 + 1024 k, +1024), the last
// row ends exactly at n), so no byte past the batch is ever hashed.  Rows
// are processed in chunks of kRowsPerChunk; the rows that round niter up to
// whole chunks are "phantom" rows past the end that read as zeros and
// advance every lane state by 1 KiB (undone with tables U).  Batches are
// shorter than 2^31 bytes (Kafka's batch_length is an int32), so 32-bit
// scalar arithmetic suffices (64-bit compares would run on the VALU).
struct Geom {
    int32_t niter, g0;
};
__device__ __forceinline__ Geom geometry(int32_t n) {
    const int32_t niter = (n - 21 + 1023) >> 10;
    return Geom{niter, n - (niter << 10)};
}
__device__ __forceinline__ int32_t chunk_rows(int32_t niter) {
    return (niter + kRowsPerChunk - 1) & ~(kRowsPerChunk - 1);
}

// One batch's first chunk of rows and its 64-byte header window, loaded
// ahead of time with the geometry implied by the descriptor length (the
// batch is re-loaded in the rare case its header trims it shorter).
struct Prefetch {
    u32x4 x[kRowsPerChunk];
    uint32_t hv;
    Geom gm;
};

// Rows are read through a buffer resource based at the batch start: lanes
// whose 16 bytes start before the batch (negative offset, out of range as
// an unsigned offset) and phantom rows (offset 2^31) read zeros without
// touching memory.  The load is always issued, so the number of loads per
// batch is fixed and the compiler waits for one row with a counted vmcnt
// instead of draining every row in flight.
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t batch_rsrc(const uint8_t* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(p), 0, 0x7ffffff0, 0x00020000);
}
#ifndef RPGPU_ROW_AUX
#define RPGPU_ROW_AUX 2  // row loads non-temporal (nt): C2 4.44 -> 4.18 ms per launch vs the default policy
#endif
__device__ __forceinline__ u32x4 load_row(__amdgpu_buffer_rsrc_t rs, const Geom& gm, int32_t row, uint32_t l) {
    const int32_t rb = row < gm.niter ? gm.g0 + (row << 10) : (int32_t)0x80000000;
    const i32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, rb + (int32_t)(16 * l), 0, RPGPU_ROW_AUX);
    return (u32x4){(uint32_t)v.x, (uint32_t)v.y, (uint32_t)v.z, (uint32_t)v.w};
}

__device__ __forceinline__ void load_rows(u32x4 (&x)[kRowsPerChunk], __amdgpu_buffer_rsrc_t rs, const Geom& gm,
                                          int32_t cb, uint32_t l) {
#pragma unroll
    for (int k = 0; k < kRowsPerChunk; k++) x[k] = load_row(rs, gm, cb + k, l);
}

__device__ __forceinline__ Geom desc_geometry(const rpgpu_batch_desc& d) {
    return (d.length >= (uint32_t)kHeaderSize && !(d.flags & RPGPU_DESC_NULL_RECORDS)) ? geometry((int32_t)d.length)
                                                                                      : Geom{0, 0};
}

// Row block at batch offset ro0 + 16*lane with bytes [0, 61) replaced by the
// header image (zero below 21, big-endian fields in [21, 61), CRC init folded
// into [21, 25)); rows starting at or after 61 pass through.  Whatever the
// load returned for bytes before the batch start is masked away.
__device__ __forceinline__ u32x4 merge_header(u32x4 y, int32_t ro0, uint32_t v_img, uint32_t l) {
    if (ro0 >= kHeaderSize) return y;
    const int32_t ro = ro0 + 16 * (int32_t)l;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int32_t o4 = ro + 4 * q;
        const uint32_t im = img_dword(v_img, o4);
        uint32_t keep;  // raw bytes at offsets >= 61
        if (o4 >= kHeaderSize)
            keep = 0xffffffffu;
        else if (o4 + 4 <= kHeaderSize)
            keep = 0;
        else
            keep = 0xffffffffu << (8 * (uint32_t)(kHeaderSize - o4));
        const uint32_t raw = q == 0 ? y.x : q == 1 ? y.y : q == 2 ? y.z : y.w;
        const uint32_t v = (raw & keep) | (o4 >= kHeaderSize ? 0u : im);
        if (q == 0) y.x = v;
        if (q == 1) y.y = v;
        if (q == 2) y.z = v;
        if (q == 3) y.w = v;
    }
    return y;
}

// Checksums one batch whose header window and first rows are in `pf` and,
// as the rows free their registers, loads the next batch's rows into them.
// A batch that needs a record walk is left at verdict OK / index_count 0
// for walk_kernel.
__device__ __forceinline__ void process_batch(const uint32_t* __restrict__ sT, const rpgpu_batch_desc& d,
                                              uint32_t b, const uint8_t* __restrict__ data,
                                              rpgpu_batch_result* __restrict__ res, Prefetch& pf,
                                              const rpgpu_batch_desc& nd, bool has_next DIAG_PARAM) {
    const uint32_t l = lane_id();
    const uint8_t* p = data + d.offset;
    const uint32_t len = d.length;
    int32_t verdict = RPGPU_V_OK;

    // ---- 64-byte header window; the next batch's goes in flight at once
    const uint32_t hv = pf.hv;
    Img64 H;
#pragma unroll
    for (int i = 0; i < 16; i++) H.w[i] = rdl(hv, i);
    Geom ngm{0, 0};
    // always issued (lanes 16..63 repeat the window): a fixed load count
    // keeps the compiler's vmcnt bookkeeping exact
    const __amdgpu_buffer_rsrc_t nrs = batch_rsrc(data + (has_next ? nd.offset : 0));
    pf.hv = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(nrs, (int32_t)(4 * (l & 15)), 0, 0);
    if (has_next) ngm = desc_geometry(nd);

    // The parse leaves one thing behind, the little-endian disk header image
    // D (storage's layout, model/record.h:356-440; all zero unless the header
    // is accepted): the result's fields, the header CRC and the body-CRC
    // image are all read out of it, so no parsed field outlives this section.
    Img64 D;
    D.clear();
    int64_t n;  // end of the Kafka-CRC region (trimmed batch length)
    bool body_trunc = false;
    bool fail = false;
    if (d.flags & RPGPU_DESC_NULL_RECORDS) {
        // produce.cc:440-449: the records field was null; nothing to read
        n = 0;
        verdict = RPGPU_V_NULL_RECORDS;
        fail = true;
    } else if (d.format == RPGPU_FMT_KAFKA_WIRE) {
        // kafka_batch_adapter::adapt / read_header (kafka_batch_adapter.cc:32-198)
        const int32_t bl = (int32_t)H.get_be(8, 4);
        const uint64_t blen = (uint64_t)(int64_t)bl + 12u;
        if (blen <= (uint64_t)len) {
            n = (int64_t)blen;
        } else {
            n = len;
            body_trunc = true;
        }
        if (len < 12) {
            verdict = RPGPU_V_TOO_SMALL;
            fail = true;
        } else if (n < 17) {
            verdict = RPGPU_V_HDR_TRUNC_THROW;
            fail = true;
        } else if ((int8_t)H.byte(16) != 2) {
            verdict = RPGPU_V_BAD_MAGIC;
            fail = true;
        } else if (n < kHeaderSize) {
            verdict = RPGPU_V_HDR_TRUNC_THROW;
            fail = true;
        } else {
            D.put_le(4, (uint32_t)bl + 12u, 4);                // size_bytes
            D.put_le(8, (uint32_t)H.get_be(4, 4), 4);          // base_offset
            D.put_le(12, (uint32_t)H.get_be(0, 4), 4);
            D.put_le(16, 1, 1);                                // record_batch_type::raft_data
            D.put_le(17, (uint32_t)H.get_be(17, 4), 4);        // crc
            D.put_le(21, (uint32_t)H.get_be(21, 2), 2);        // attrs
            D.put_le(23, (uint32_t)H.get_be(23, 4), 4);        // last_offset_delta
            D.put_le(27, (uint32_t)H.get_be(31, 4), 4);        // first_timestamp
            D.put_le(31, (uint32_t)H.get_be(27, 4), 4);
            D.put_le(35, (uint32_t)H.get_be(39, 4), 4);        // max_timestamp
            D.put_le(39, (uint32_t)H.get_be(35, 4), 4);
            D.put_le(43, (uint32_t)H.get_be(47, 4), 4);        // producer_id
            D.put_le(47, (uint32_t)H.get_be(43, 4), 4);
            D.put_le(51, (uint32_t)H.get_be(51, 2), 2);        // producer_epoch
            D.put_le(53, (uint32_t)H.get_be(53, 4), 4);        // base_sequence
            D.put_le(57, (uint32_t)H.get_be(57, 4), 4);        // record_count
        }
    } else {
        // storage::continuous_batch_parser read_header_impl (parser.cc:155-216)
        n = 0;
        if (len < kHeaderSize) {
            verdict = RPGPU_V_STREAM_SHORT;
            fail = true;
        } else {
            uint32_t any = 0;
#pragma unroll
            for (int i = 0; i < 15; i++) any |= H.w[i];
            any |= H.w[15] & 0xffu;  // byte 60 only (61..63 are past the header)
            if (any == 0) {
                verdict = RPGPU_V_FALLOCATED_ZERO;
                fail = true;
            } else {
#pragma unroll
                for (int i = 0; i < 16; i++) D.w[i] = H.w[i];
                D.w[15] &= 0xffu;
                n = (int64_t)(int32_t)D.w[1];  // size_bytes
            }
        }
    }
    const bool is_disk = d.format != RPGPU_FMT_KAFKA_WIRE;
    const bool recrc = is_disk && (d.ops & RPGPU_OP_RECRC);
    const int32_t size_bytes = (int32_t)D.w[1];
    const uint32_t attrs = (uint32_t)D.get_le(21, 2);
    uint32_t crc_expected = (uint32_t)D.get_le(17, 4);
    uint32_t rv = 0;  // the result, dword i in lane i (index_first / index_count: 0, the walk's)
    rv = writelane(rv, (uint32_t)size_bytes, kResSizeBytes);
    rv = writelane(rv, (uint32_t)D.get_le(57, 4), kResRecordCount);
    rv = writelane(rv, D.w[2], kResBaseOffset);
    rv = writelane(rv, D.w[3], kResBaseOffset + 1);
    rv = writelane(rv, (uint32_t)D.get_le(23, 4), kResLastOffsetDelta);
    rv = writelane(rv, attrs | ((attrs & 7u) << 16) | (D.byte(16) << 24), kResAttrsCodecType);
    rv = writelane(rv, (uint32_t)D.get_le(27, 4), kResFirstTs);
    rv = writelane(rv, (uint32_t)D.get_le(31, 4), kResFirstTs + 1);
    rv = writelane(rv, (uint32_t)D.get_le(35, 4), kResMaxTs);
    rv = writelane(rv, (uint32_t)D.get_le(39, 4), kResMaxTs + 1);
    rv = writelane(rv, crc_expected, kResCrcExpected);
    uint32_t dv = 0;  // D, dword i in lane i (kept for the re-checksummed header)
    if (!fail) {
        dv = lanes16(D);
        uint32_t header_crc = 0;
        if (!recrc && ((d.ops & RPGPU_OP_HDRCRC) || is_disk)) header_crc = header_crc_lanes(sT, dv);
        rv = writelane(rv, header_crc, kResHeaderCrc);
        if (is_disk) {
            if (!recrc && header_crc != H.w[0]) {
                verdict = RPGPU_V_HDR_CRC_MISMATCH;
                fail = true;
            } else if (size_bytes < kHeaderSize || (int64_t)size_bytes > (int64_t)len) {
                verdict = RPGPU_V_STREAM_SHORT;
                fail = true;
            }
        }
    }
    if (fail) {
        // nothing of this batch is checksummed: just move the next one's rows
        load_rows(pf.x, nrs, ngm, 0, l);
        pf.gm = ngm;
        rv = writelane(rv, (uint32_t)verdict, kResVerdict);
        store_result(res + b, rv);
        return;
    }

    // ---- body-CRC image: bytes [21, 61) big-endian (record_utils.cc:68-80),
    //      bytes < 21 zero, init 0xFFFFFFFF folded into [21, 25); dword i in
    //      lane i of v_img
    uint32_t v_img;
    {
        Img64 B;
        B.clear();
        B.put_be(21, attrs, 2);
        B.put_be(23, (uint32_t)D.get_le(23, 4), 4);  // last_offset_delta
        B.put_be(27, (uint32_t)D.get_le(31, 4), 4);  // first_timestamp
        B.put_be(31, (uint32_t)D.get_le(27, 4), 4);
        B.put_be(35, (uint32_t)D.get_le(39, 4), 4);  // max_timestamp
        B.put_be(39, (uint32_t)D.get_le(35, 4), 4);
        B.put_be(43, (uint32_t)D.get_le(47, 4), 4);  // producer_id
        B.put_be(47, (uint32_t)D.get_le(43, 4), 4);
        B.put_be(51, (uint32_t)D.get_le(51, 2), 2);  // producer_epoch
        B.put_be(53, (uint32_t)D.get_le(53, 4), 4);  // base_sequence
        B.put_be(57, (uint32_t)D.get_le(57, 4), 4);  // record_count
        B.w[5] ^= 0xffffff00u;  // bytes 21..23
        B.w[6] ^= 0x000000ffu;  // byte 24
        v_img = lanes16(B);
    }

    // ---- rows over the CRC region [21, n)
    const Geom gm = geometry((int32_t)n);
    const int32_t nrows = chunk_rows(gm.niter);  // real + phantom rows
    const bool pf_ok = pf.gm.niter == gm.niter && pf.gm.g0 == gm.g0;  // prefetch geometry matches
    const uint32_t* sN = sT + kOffN;
    const __amdgpu_buffer_rsrc_t rs = batch_rsrc(p);
    const __amdgpu_buffer_rsrc_t nrs_rows = batch_rsrc(data + (has_next ? nd.offset : 0));
    uint32_t c = 0;
    STAMP(0);
    if (!pf_ok) load_rows(pf.x, rs, gm, 0, l);
    // the header bytes lie in rows 0 and 1
    pf.x[0] = merge_header(pf.x[0], gm.g0, v_img, l);
    pf.x[1] = merge_header(pf.x[1], gm.g0 + 1024, v_img, l);
    for (int32_t cb = 0; cb < nrows; cb += kRowsPerChunk) {
        // each row's registers take row k of the next chunk once the row is
        // checksummed, or row k of the next batch during the last chunk
        const bool last_chunk = cb + kRowsPerChunk >= nrows;
        const __amdgpu_buffer_rsrc_t lrs = last_chunk ? nrs_rows : rs;
        const Geom lg = last_chunk ? ngm : gm;
        const int32_t lrow = last_chunk ? 0 : cb + kRowsPerChunk;
        // one straight-line block: the lookups of row k+1 that do not
        // depend on the lane state overlap row k's
#pragma unroll
        for (int k = 0; k < kRowsPerChunk; k++) {
            u32x4 y = pf.x[k];
            y.x ^= c;
            c = crc_block(sN, y);
            pf.x[k] = load_row(lrs, lg, lrow + k, l);
        }
    }
    pf.gm = ngm;
    STAMP(1);
#ifndef RPGPU_DIAG_NO_COMBINE
    c = combine64(sT + kOffW, c);
    if (nrows != gm.niter) c = apply8(sT + kOffU + (nrows - gm.niter) * 128, c);
#endif
    uint32_t crc = ~rdl(c, 0);
#if defined(RPGPU_DIAG_NO_COMBINE) || defined(RPGPU_DIAG_NO_LOOKUP)  // keep verdicts OK
    asm volatile("" ::"v"(c));  // keep the row loads (the CRC is discarded)
    crc = crc_expected;
#endif
    rv = writelane(rv, crc, kResCrc);
    if (recrc) {
        // reset_size_checksum_metadata: crc first, then the header CRC over a
        // header that carries it (D bytes [17, 21))
        crc_expected = crc;
        dv = writelane(dv, (rdl(dv, 4) & 0x000000ffu) | (crc << 8), 4);
        dv = writelane(dv, (rdl(dv, 5) & 0xffffff00u) | (crc >> 24), 5);
        rv = writelane(rv, crc_expected, kResCrcExpected);
        rv = writelane(rv, header_crc_lanes(sT, dv), kResHeaderCrc);
    }
    STAMP(2);

    // ---- verdict precedence (kafka_batch_adapter.cc:169-193)
    if (crc != crc_expected) {
        verdict = RPGPU_V_CRC_MISMATCH;
    } else if (body_trunc) {
        verdict = RPGPU_V_BODY_TRUNC_THROW;
    } else if ((attrs & 7u) > 4) {
        verdict = RPGPU_V_BAD_CODEC_THROW;
    }
    rv = writelane(rv, (uint32_t)verdict, kResVerdict);
    store_result(res + b, rv);
    STAMP(3);
}

// One wave per batch, grid-stride: header, both CRCs and the verdict.  The
// record walk and each batch's index_first are walk_kernel's /
// walk_wave_kernel's (the plan's local_first / block_base are theirs too).
__global__ __launch_bounds__(kValidateThreads, 8) void validate_kernel(
    const rpgpu_batch_desc* __restrict__ descs, uint32_t b0, uint32_t n, const uint8_t* __restrict__ data,
    rpgpu_batch_result* __restrict__ res, rpgpu_record_index* __restrict__ index,
    const uint32_t* __restrict__ local_first, const uint32_t* __restrict__ caps,
    const uint64_t* __restrict__ block_base, uint64_t index_cap, const uint32_t* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kTableWords];
    load_tables(sT, tables);
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + wave);
    const uint32_t nw = gridDim.x * kWavesPerBlock;
#ifdef RPGPU_DIAG_STAMPS
    Stamps sp{};
    sp.prev = __builtin_amdgcn_s_memtime();
#endif
    Prefetch pf;
    pf.gm = Geom{0, 0};
    if (b0 + gw < n) {
        const rpgpu_batch_desc d0 = sload_desc(descs + b0 + gw);
        const uint8_t* p0 = data + d0.offset;
        const __amdgpu_buffer_rsrc_t rs0 = batch_rsrc(p0);
        pf.hv = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs0, (int32_t)(4 * (lane_id() & 15)), 0, 0);
        pf.gm = desc_geometry(d0);
        load_rows(pf.x, rs0, pf.gm, 0, lane_id());
    }
    for (uint32_t b = b0 + gw; b < n; b += nw) {
        const rpgpu_batch_desc d = sload_desc(descs + b);
        const bool has_next = b + nw < n;
        // always loaded (the batch's own descriptor when there is no next
        // one; has_next masks its use): a conditionally initialised struct
        // is lowered to scratch memory
        const rpgpu_batch_desc nd = sload_desc(descs + (has_next ? b + nw : b));
        // index_first is the walk's to write (walk_kernel): the checksums do not
        // wait for the plan
        process_batch(sT, d, b, data, res, pf, nd, has_next DIAG_PASS);
        STAMP(5);
    }
#ifdef RPGPU_DIAG_STAMPS
    if (lane_id() == 0)
        for (int i = 0; i < 6; i++) atomicAdd(&g_stamps[i], (unsigned long long)sp.st[i]);
#endif
}

// One lane per batch: the record walk of every batch that needs one and
// passed validation (verdict OK, uncompressed).  Writes the batch's verdict
// and index_count; the index slice is the plan's (index_cap clamps it to
// the caller's buffer, as in rpgpu_validate_device).
__global__ __launch_bounds__(256) void walk_kernel(const rpgpu_batch_desc* __restrict__ descs, uint32_t b0,
                                                   uint32_t n,
                                                   const uint8_t* __restrict__ data,
                                                   rpgpu_batch_result* __restrict__ res,
                                                   rpgpu_record_index* __restrict__ index,
                                                   const uint32_t* __restrict__ local_first,
                                                   const uint32_t* __restrict__ caps,
                                                   const uint64_t* __restrict__ block_base, uint64_t index_cap,
                                                   uint32_t* __restrict__ wave_list, uint32_t* __restrict__ wave_count) {
    const uint32_t b = b0 + blockIdx.x * blockDim.x + threadIdx.x;
    WalkJob J;
    J.flags = 0;
    J.body = 0;
    J.base_offset = J.first_ts = 0;
    J.n = J.first = J.cap = J.b = 0;
    J.rc = 0;
    uint32_t first_all = 0;  // every batch's index_first (validate_kernel leaves it 0)
    if (b < n) {
        const rpgpu_batch_desc d = descs[b];
        const rpgpu_batch_result& r = res[b];
        const uint64_t first = block_base[b / kScanBlock] + local_first[b];
        first_all = (uint32_t)first;
        if ((d.ops & (RPGPU_OP_PARSE | RPGPU_OP_INDEX)) && r.verdict == RPGPU_V_OK && r.codec == 0) {
            uint64_t cap = caps[b];
            if (first >= index_cap) cap = 0;
            else if (first + cap > index_cap) cap = index_cap - first;
            J.body = d.offset + kHeaderSize;
            J.base_offset = r.base_offset;
            J.first_ts = r.first_timestamp;
            J.n = (uint32_t)r.size_bytes - kHeaderSize;  // verdict OK: the trimmed batch length
            J.rc = r.record_count;
            J.first = (uint32_t)first;
            J.cap = (uint32_t)cap;
            J.b = b;
            J.flags = kJobLive | ((d.ops & RPGPU_OP_INDEX) ? kJobIndex : 0u);
            if (J.rc > kWaveWalkMin) {  // many records: walk_wave_kernel's
                wave_list[atomicAdd(wave_count, 1u)] = b;
                J.flags = 0;
            }
        }
    }
    walk_lanes(data, J, index, res);
    if (b < n && !(J.flags & kJobLive)) reinterpret_cast<uint32_t*>(res + b)[14] = first_all;  // .index_first
}

// The batches walk_kernel listed (more than kWaveWalkMin records): one
// wavefront each, taken from an atomic queue (rpgpu_walk.h wave_walk_batch).
__global__ __launch_bounds__(256) void walk_wave_kernel(const rpgpu_batch_desc* __restrict__ descs,
                                                        const uint8_t* __restrict__ data,
                                                        rpgpu_batch_result* __restrict__ res,
                                                        rpgpu_record_index* __restrict__ index,
                                                        const uint32_t* __restrict__ local_first,
                                                        const uint32_t* __restrict__ caps,
                                                        const uint64_t* __restrict__ block_base, uint64_t index_cap,
                                                        const uint32_t* __restrict__ wave_list,
                                                        const uint32_t* __restrict__ wave_count,
                                                        uint32_t* __restrict__ head) {
    const uint32_t cnt = *wave_count;
    for (;;) {
        uint32_t k = 0;
        if (lane_id() == 0) k = atomicAdd(head, 1u);
        k = __builtin_amdgcn_readfirstlane(k);
        if (k >= cnt) break;
        const uint32_t b = wave_list[k];
        const rpgpu_batch_desc d = descs[b];
        const rpgpu_batch_result& r = res[b];
        const uint64_t first = block_base[b / kScanBlock] + local_first[b];
        uint64_t cap = caps[b];
        if (first >= index_cap) cap = 0;
        else if (first + cap > index_cap) cap = index_cap - first;
        WalkJob J;
        J.body = d.offset + kHeaderSize;
        J.base_offset = r.base_offset;
        J.first_ts = r.first_timestamp;
        J.n = (uint32_t)r.size_bytes - kHeaderSize;
        J.rc = r.record_count;
        J.first = (uint32_t)first;
        J.cap = (uint32_t)cap;
        J.b = b;
        J.flags = kJobLive | ((d.ops & RPGPU_OP_INDEX) ? kJobIndex : 0u);
        int32_t verdict;
        uint32_t count;
        wave_walk_batch(data, J, index, verdict, count);
        if (lane_id() == 0) {
            uint32_t* o = reinterpret_cast<uint32_t*>(res + b);
            o[0] = (uint32_t)verdict;
            o[15] = count;
        }
    }
}

// ------------------------------------------------------- index-cap prepass
// Same rule as oracle/batch.c orc_index_cap.
__device__ __forceinline__ uint32_t index_cap(const rpgpu_batch_desc& d, const uint8_t* data) {
    if (!(d.ops & (RPGPU_OP_PARSE | RPGPU_OP_INDEX)) || (d.flags & RPGPU_DESC_NULL_RECORDS)) return 0;
    const uint8_t* p = data + d.offset;
    const uint64_t len = d.length;
    if (len < (uint64_t)kHeaderSize) return 0;
    uint64_t n;
    int32_t rc;
    uint32_t attrs;
    if (d.format == RPGPU_FMT_KAFKA_WIRE) {
        const int32_t bl = (int32_t)bswap32(ld4(p + 8));
        const uint64_t blen = (uint64_t)(int64_t)bl + 12u;
        if (blen > len) return 0;
        n = blen;
        if (n < (uint64_t)kHeaderSize || p[16] != 2) return 0;
        attrs = ((uint32_t)p[21] << 8) | p[22];
        rc = (int32_t)bswap32(ld4(p + 57));
    } else {
        const int32_t sz = (int32_t)ld4(p + 4);
        if (sz < kHeaderSize || (uint64_t)sz > len) return 0;
        n = (uint64_t)sz;
        attrs = ((uint32_t)p[22] << 8) | p[21];
        rc = (int32_t)ld4(p + 57);
    }
    if ((attrs & 7u) != 0 || rc <= 0) return 0;
    uint64_t cap = (n - kHeaderSize) / 2;
    if ((uint64_t)rc < cap) cap = (uint64_t)rc;
    return (uint32_t)cap;
}

// per-batch cap + exclusive scan within blocks of kScanBlock batches
__global__ __launch_bounds__(kScanBlock) void caps_kernel(const rpgpu_batch_desc* __restrict__ descs,
                                                          uint32_t n, const uint8_t* __restrict__ data,
                                                          uint32_t* __restrict__ caps,
                                                          uint32_t* __restrict__ local_first,
                                                          uint64_t* __restrict__ block_sum) {
    __shared__ uint32_t wsum[kScanBlock / 64];
    const uint32_t i = blockIdx.x * kScanBlock + threadIdx.x;
    uint32_t cap = 0;
    if (i < n) cap = index_cap(descs[i], data);
    const uint32_t first = block_scan_excl(cap, wsum, block_sum);
    if (i < n) {
        caps[i] = cap;
        local_first[i] = first;
    }
}

// exclusive scan of block sums (single workgroup), total into *total_out
__global__ __launch_bounds__(kScanBlock) void block_scan_kernel(uint64_t* block_sum, uint32_t nb,
                                                                uint64_t* __restrict__ total_out) {
    __shared__ uint64_t part[kScanBlock];
    const uint64_t total = array_scan_excl(block_sum, block_sum, nb, part);
    if (threadIdx.x == kScanBlock - 1 && total_out) *total_out = total;
}

// ---------------------------------------------- generic CRC32C over ranges
// crc_out[i] = crc32c::Extend(seed[i], data + off[i], len[i])
// (hashing/crc32c.h:21-43).  Same strided-row scheme; init ~seed folded into
// the first four bytes, bytes before the range zeroed.
__global__ __launch_bounds__(kValidateThreads) void crc_ranges_kernel(
    const uint8_t* __restrict__ data, const uint64_t* __restrict__ offs, const uint32_t* __restrict__ lens,
    const uint32_t* __restrict__ seeds, uint32_t n, uint32_t* __restrict__ out,
    const uint32_t* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kTableWords];
    load_tables(sT, tables);
    const uint32_t l = lane_id();
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + wave);
    const uint32_t nw = gridDim.x * kWavesPerBlock;
    for (uint32_t i = gw; i < n; i += nw) {
        const uint8_t* base = data + offs[i];
        const int64_t len = lens[i];
        const uint32_t init = ~(seeds ? seeds[i] : 0u);
        const uint32_t crc = crc_range_wave(sT, base, len, init, l);
        if (l == 0) out[i] = crc;
    }
}

// ------------------------------------------------ stream-level storage parser
// storage::continuous_batch_parser::consume (storage/parser.cc:113-299) over
// one segment region per wavefront, with log_replayer's checksumming consumer
// (accept all) or log_reader's skipping_consumer (storage/log_reader.cc:
// 28-121).  The walk follows the size_bytes chain, so it is serial per
// segment: each step is one 64-byte header load (16 lanes x 4 B), the header
// CRC on all 64 lanes (header_crc_vec) and a wave-uniform decision.  Many
// segments (partitions) run side by side; the bodies are not read here --
// rpgpu_run_device checks them over the emitted descriptors.
__device__ __forceinline__ bool header_all_zero(const Img64& H) {
    uint32_t any = 0;
#pragma unroll
    for (int i = 0; i < 15; i++) any |= H.w[i];
    any |= H.w[15] & 0xffu;  // byte 60 only
    return any == 0;
}

__global__ __launch_bounds__(kValidateThreads) void segment_parse_kernel(
    const uint8_t* __restrict__ data, const rpgpu_segment_read* __restrict__ reads, uint32_t nreads,
    rpgpu_segment_parse_result* __restrict__ results, rpgpu_batch_desc* __restrict__ descs,
    const uint32_t* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kTableWords];
    load_tables(sT, tables);
    const uint32_t l = lane_id();
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * kWavesPerBlock;
    for (uint32_t s = gw; s < nreads; s += nw) {
        const rpgpu_segment_read rd = reads[s];
        const uint8_t* seg = data + rd.offset;
        const uint64_t len = rd.length;
        const bool reader = rd.mode == RPGPU_PARSE_READER;
        const uint64_t max_buffer = rd.max_buffer ? rd.max_buffer : 32u * 1024u;
        uint64_t pos = 0, bytes_consumed = 0, phys = 0, buffer = 0;
        int32_t err = RPGPU_V_OK;
        bool exception = false, stopped = false, over_budget = false;
        bool codec_throw = false;
        uint32_t accepted = 0, skipped = 0;
        int64_t start_offset = rd.start_offset, expected = rd.expected_next_batch;
        uint64_t cfg_bytes = rd.bytes_consumed;
        for (;;) {
            const uint64_t rem = len - pos;
            if (rem == 0) {
                err = RPGPU_V_END_OF_STREAM;
                break;
            }
            if (rem < (uint64_t)kHeaderSize) {
                err = RPGPU_V_STREAM_SHORT;
                break;
            }
            // the 64-byte header window at pos: pos is wave-uniform and 64-bit,
            // so the resource is rebuilt at seg + pos (a read may be any length;
            // the arena's tail pad covers the 3 bytes past 61)
            const __amdgpu_buffer_rsrc_t rs = batch_rsrc(seg + pos);
            const uint32_t hv = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int32_t)(4 * (l & 15)), 0, 0);
            Img64 H;
#pragma unroll
            for (int i = 0; i < 16; i++) H.w[i] = rdl(hv, i);
            if (header_all_zero(H)) {
                err = RPGPU_V_FALLOCATED_ZERO;
                break;
            }
            Img64 D;
#pragma unroll
            for (int i = 0; i < 16; i++) D.w[i] = H.w[i];
            D.w[15] &= 0xffu;
            if (header_crc_vec(sT, D) != H.w[0]) {
                err = RPGPU_V_HDR_CRC_MISMATCH;
                break;
            }
            const int32_t size_bytes = (int32_t)H.get_le(4, 4);
            const int64_t base_offset = (int64_t)H.get_le(8, 8);
            const int8_t type = (int8_t)H.byte(16);
            const int32_t lod = (int32_t)H.get_le(23, 4);
            const int64_t max_ts = (int64_t)H.get_le(35, 8);
            const int64_t last = base_offset + lod;
            const uint64_t sz = (uint64_t)(int64_t)size_bytes;
            int decision = 0;  // 0 accept, 1 skip, 2 stop
            if (reader) {
                if (base_offset < expected) {
                    exception = true;
                    break;
                }
                if (base_offset > rd.max_offset) {
                    decision = 2;
                } else if ((rd.strict_max_bytes || cfg_bytes) && cfg_bytes + sz > rd.max_bytes) {
                    over_budget = true;
                    decision = 2;
                } else if (last < start_offset) {
                    decision = 1;
                } else if (rd.has_type_filter && rd.type_filter != type) {
                    start_offset = last + 1;
                    decision = 1;
                } else if (rd.has_first_timestamp && rd.first_timestamp > max_ts) {
                    start_offset = last + 1;
                    decision = 1;
                }
            }
            if (decision == 2) {
                stopped = true;
                break;
            }
            const uint64_t body = (uint64_t)((int64_t)size_bytes - kHeaderSize);
            const uint64_t avail = len - pos - kHeaderSize;
            if (decision == 1) {
                expected = last + 1;
                phys += sz;
                if (body > avail) {
                    err = RPGPU_V_STREAM_SHORT;
                    break;
                }
                pos += kHeaderSize + body;
                bytes_consumed += sz;
                skipped++;
                continue;
            }
            if (reader) expected = last + 1;
            phys += sz;
            // consume_batch_end's record_batch(tag_ctor_ng) throws for codec
            // 5..7 (model/record.h:283-300,582-585): that batch is never
            // produced, so it gets no descriptor (as in remote_parse_kernel)
            const bool throws = reader && (H.byte(21) & 7u) > 4u && body <= avail;
            if (!throws && accepted < rd.desc_cap && l == 0) {
                rpgpu_batch_desc d;
                d.offset = rd.offset + pos;
                d.length = (uint32_t)(body > avail ? avail + kHeaderSize : body + kHeaderSize);
                d.partition = rd.partition;
                d.format = RPGPU_FMT_RP_DISK;
                d.ops = rd.ops;
                d.flags = 0;
                d.reserved = 0;
                descs[rd.desc_first + accepted] = d;
            }
            if (!throws) accepted++;
            bytes_consumed += sz;
            if (body > avail) {
                err = RPGPU_V_STREAM_SHORT;
                break;
            }
            pos += kHeaderSize + body;
            if (throws) {
                codec_throw = true;
                break;
            }
            if (reader) {
                start_offset = last + 1;
                cfg_bytes += sz;
                buffer += sz;
                if (last >= rd.stable_offset || last >= rd.max_offset ||
                    (rd.has_next_cached && rd.next_cached_batch == last + 1) || cfg_bytes >= rd.max_bytes ||
                    buffer >= max_buffer) {
                    stopped = true;
                    break;
                }
            }
        }
        if (l == 0) {
            rpgpu_segment_parse_result r;
            r.last_error = (exception || codec_throw) ? RPGPU_V_OK : err;
            const bool benign = err == RPGPU_V_OK || err == RPGPU_V_END_OF_STREAM || err == RPGPU_V_FALLOCATED_ZERO;
            r.status = exception     ? RPGPU_V_READ_OFFSET_REGRESSION
                       : codec_throw ? RPGPU_V_BAD_CODEC_THROW
                                     : ((bytes_consumed || benign) ? RPGPU_V_OK : err);
            r.accepted = accepted < rd.desc_cap ? accepted : rd.desc_cap;
            r.skipped = skipped;
            r.bytes_consumed = bytes_consumed;
            r.physical_offset = phys;
            r.start_offset = start_offset;
            r.cfg_bytes_consumed = cfg_bytes;
            r.expected_next_batch = expected;
            r.over_budget = over_budget;
            r.stopped = stopped;
            r.reserved0 = 0;
            r.reserved1 = 0;
            results[s] = r;
        }
    }
}

// ---------------------------------------- remote (tiered storage) segment reader
// continuous_batch_parser::consume driving cloud_storage's
// remote_segment_batch_consumer (cloud_storage/remote_segment.cc:788-975), one
// wavefront per read (one read_some call), same header step as
// segment_parse_kernel; the consumer's decisions are wave-uniform.
constexpr uint64_t kMaxConsumeSize = 128u * 1024u;  // remote_segment.cc:61
constexpr int8_t kTypeRaftData = 1, kTypeRaftConfiguration = 2, kTypeArchivalMetadata = 19;

__global__ __launch_bounds__(kValidateThreads) void remote_parse_kernel(
    const uint8_t* __restrict__ data, const rpgpu_remote_read* __restrict__ reads, uint32_t nreads,
    rpgpu_remote_parse_result* __restrict__ results, rpgpu_batch_desc* __restrict__ descs,
    int64_t* __restrict__ kafka_base, int64_t* __restrict__ gaps, const uint32_t* __restrict__ tables) {
    __shared__ __attribute__((aligned(16))) uint32_t sT[kTableWords];
    load_tables(sT, tables);
    const uint32_t l = lane_id();
    const uint32_t gw = __builtin_amdgcn_readfirstlane(blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6));
    const uint32_t nw = gridDim.x * kWavesPerBlock;
    for (uint32_t s = gw; s < nreads; s += nw) {
        const rpgpu_remote_read rd = reads[s];
        const uint8_t* seg = data + rd.offset;
        const uint64_t len = rd.length;
        uint64_t pos = 0, bytes_consumed = 0, produced = 0;
        int32_t err = RPGPU_V_OK, thrown = RPGPU_V_OK;
        bool stopped = false, over_budget = rd.over_budget != 0;
        uint32_t accepted = 0, skipped = 0, ngaps = 0;
        int64_t start_offset = rd.start_offset, delta = rd.cur_delta, cur_rp = rd.cur_rp_offset;
        uint64_t cfg_bytes = rd.bytes_consumed;
        for (;;) {
            const uint64_t rem = len - pos;
            if (rem == 0) {
                err = RPGPU_V_END_OF_STREAM;
                break;
            }
            if (rem < (uint64_t)kHeaderSize) {
                err = RPGPU_V_STREAM_SHORT;
                break;
            }
            const __amdgpu_buffer_rsrc_t rs = batch_rsrc(seg + pos);  // as in segment_parse_kernel
            const uint32_t hv = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int32_t)(4 * (l & 15)), 0, 0);
            Img64 H;
#pragma unroll
            for (int i = 0; i < 16; i++) H.w[i] = rdl(hv, i);
            if (header_all_zero(H)) {
                err = RPGPU_V_FALLOCATED_ZERO;
                break;
            }
            Img64 D;
#pragma unroll
            for (int i = 0; i < 16; i++) D.w[i] = H.w[i];
            D.w[15] &= 0xffu;
            if (header_crc_vec(sT, D) != H.w[0]) {
                err = RPGPU_V_HDR_CRC_MISMATCH;
                break;
            }
            const int32_t size_bytes = (int32_t)H.get_le(4, 4);
            const int64_t base_offset = (int64_t)H.get_le(8, 8);
            const int8_t type = (int8_t)H.byte(16);
            const uint32_t codec = H.byte(21) & 7u;
            const int32_t lod = (int32_t)H.get_le(23, 4);
            const int64_t max_ts = (int64_t)H.get_le(35, 8);
            const int64_t last = base_offset + lod;
            const uint64_t sz = (uint64_t)(int64_t)size_bytes;
            // accept_batch_start (remote_segment.cc:846-900); rp_to_kafka
            // vasserts its argument is not below the delta (:808-815)
            int decision = 0;  // 0 accept, 1 skip, 2 stop
            if (base_offset < delta) {
                thrown = RPGPU_V_REMOTE_DELTA_ASSERT;
                break;
            }
            if (base_offset - delta > rd.max_offset) {
                decision = 2;
            } else if (type != kTypeRaftData) {
                decision = 1;
            } else if (last < delta) {
                thrown = RPGPU_V_REMOTE_DELTA_ASSERT;
                break;
            } else if (last - delta < start_offset) {
                decision = 1;
            } else if ((rd.strict_max_bytes || cfg_bytes) && cfg_bytes + sz > rd.max_bytes) {
                over_budget = true;
                decision = 2;
            } else if (rd.has_first_timestamp && rd.first_timestamp > max_ts) {
                decision = 1;
            }
            if (decision == 2) {
                stopped = true;
                break;
            }
            const uint64_t body = (uint64_t)((int64_t)size_bytes - kHeaderSize);
            const uint64_t avail = len - pos - kHeaderSize;
            if (decision == 1) {
                // skip_batch_start (:916-946): advance_config_offsets, then the
                // offset-translation gap of a configuration / archival batch
                cur_rp = last + 1;
                if (type == kTypeRaftData && last - delta + 1 > start_offset) start_offset = last - delta + 1;
                if (type == kTypeRaftConfiguration || type == kTypeArchivalMetadata) {
                    if (ngaps < rd.gap_cap && l == 0) {
                        gaps[2 * ((uint64_t)rd.gap_first + ngaps)] = base_offset;
                        gaps[2 * ((uint64_t)rd.gap_first + ngaps) + 1] = last;
                    }
                    ngaps++;
                    delta += (int64_t)lod + 1;
                }
                if (body > avail) {
                    err = RPGPU_V_STREAM_SHORT;
                    break;
                }
                pos += kHeaderSize + body;
                bytes_consumed += sz;
                skipped++;
                continue;
            }
            bytes_consumed += sz;
            if (body > avail) {
                err = RPGPU_V_STREAM_SHORT;
                break;
            }
            const uint64_t bpos = pos;
            pos += kHeaderSize + body;
            // consume_batch_end (:951-975)
            if (codec > 4u) {  // record_batch(tag_ctor_ng) throws (model/record.h:582-585)
                thrown = RPGPU_V_BAD_CODEC_THROW;
                break;
            }
            cfg_bytes += sz;
            cur_rp = last + 1;
            if (last - delta + 1 > start_offset) start_offset = last - delta + 1;
            if (accepted < rd.desc_cap && l == 0) {
                rpgpu_batch_desc d;
                d.offset = rd.offset + bpos;
                d.length = (uint32_t)(body + kHeaderSize);
                d.partition = rd.partition;
                d.format = RPGPU_FMT_RP_DISK;
                d.ops = rd.ops;
                d.flags = 0;
                d.reserved = 0;
                descs[rd.desc_first + accepted] = d;
                kafka_base[rd.desc_first + accepted] = base_offset - delta;
            }
            accepted++;
            produced += sz;  // remote_segment_batch_reader::produce (:1073-1079)
            if (over_budget || produced > kMaxConsumeSize) {
                stopped = true;
                break;
            }
        }
        if (l == 0) {
            rpgpu_remote_parse_result r;
            const bool benign = err == RPGPU_V_OK || err == RPGPU_V_END_OF_STREAM || err == RPGPU_V_FALLOCATED_ZERO;
            r.last_error = thrown != RPGPU_V_OK ? RPGPU_V_OK : err;
            r.status = thrown != RPGPU_V_OK ? thrown : ((bytes_consumed || benign) ? RPGPU_V_OK : err);
            r.accepted = accepted < rd.desc_cap ? accepted : rd.desc_cap;
            r.skipped = skipped;
            r.bytes_consumed = bytes_consumed;
            r.start_offset = start_offset;
            r.cfg_bytes_consumed = cfg_bytes;
            r.cur_delta = delta;
            r.cur_rp_offset = cur_rp;
            r.produced_bytes = produced;
            r.gaps = ngaps;
            r.over_budget = over_budget;
            r.stopped = stopped;
            r.reserved = 0;
            results[s] = r;
        }
    }
}

hipError_t launch_remote_parse(const uint8_t* d_data, const rpgpu_remote_read* d_reads, uint32_t n,
                               rpgpu_remote_parse_result* d_res, rpgpu_batch_desc* d_descs, int64_t* d_kafka_base,
                               int64_t* d_gaps, const uint32_t* d_tables, int grid, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t need = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    const uint32_t g = (uint32_t)grid < need ? (uint32_t)grid : need;
    remote_parse_kernel<<<g, kValidateThreads, 0, s>>>(d_data, d_reads, n, d_res, d_descs, d_kafka_base, d_gaps,
                                                       d_tables);
    return hipGetLastError();
}

hipError_t launch_segment_parse(const uint8_t* d_data, const rpgpu_segment_read* d_reads, uint32_t n,
                                rpgpu_segment_parse_result* d_res, rpgpu_batch_desc* d_descs,
                                const uint32_t* d_tables, int grid, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t need = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    const uint32_t g = (uint32_t)grid < need ? (uint32_t)grid : need;
    segment_parse_kernel<<<g, kValidateThreads, 0, s>>>(d_data, d_reads, n, d_res, d_descs, d_tables);
    return hipGetLastError();
}

// produce-handler error codes (rpgpu_kafka_error_codes_device)
__global__ __launch_bounds__(256) void kafka_codes_kernel(const rpgpu_batch_result* __restrict__ res, uint32_t n,
                                                          uint32_t batch_max_bytes, int32_t* __restrict__ codes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) codes[i] = kafka_error_code(res[i].verdict, res[i].size_bytes, batch_max_bytes);
}

hipError_t launch_kafka_codes(const rpgpu_batch_result* d_res, uint32_t n, uint32_t batch_max_bytes,
                              int32_t* d_codes, hipStream_t s) {
    if (n == 0) return hipSuccess;
    kafka_codes_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_res, n, batch_max_bytes, d_codes);
    return hipGetLastError();
}

// ------------------------------------------------------------ launchers
// scratch layout: caps[n] u32 | local_first[n] u32 | block_sum[nb] u64 |
//                 wave counters (count, head; 64 B) | wave_list[n] u32
struct WaveWalk {
    uint32_t *list, *count;  // count[0]: batches listed, count[1]: queue head
};
static void scratch_parts(void* d_scratch, uint32_t n, uint32_t** caps, uint32_t** local_first,
                          uint64_t** block_sum, WaveWalk* ww = nullptr) {
    uint8_t* sc = static_cast<uint8_t*>(d_scratch);
    *caps = reinterpret_cast<uint32_t*>(sc);
    *local_first = *caps + n;
    const size_t o_bs = ((size_t)n * 8 + 15) & ~(size_t)15;
    *block_sum = reinterpret_cast<uint64_t*>(sc + o_bs);
    const size_t nb = (n + kScanBlock - 1) / kScanBlock;
    const size_t o_ww = (o_bs + nb * 8 + 63) & ~(size_t)63;
    if (ww) {
        ww->count = reinterpret_cast<uint32_t*>(sc + o_ww);
        ww->list = ww->count + 16;
    }
}

hipError_t launch_plan(const rpgpu_batch_desc* d_descs, uint32_t n, const uint8_t* d_data,
                       uint64_t* d_index_used, void* d_scratch, hipStream_t s) {
    if (n == 0) {
        if (d_index_used) return hipMemsetAsync(d_index_used, 0, sizeof(uint64_t), s);
        return hipSuccess;
    }
    const uint32_t nb = (n + kScanBlock - 1) / kScanBlock;
    uint32_t *caps, *local_first;
    uint64_t* block_sum;
    scratch_parts(d_scratch, n, &caps, &local_first, &block_sum);
    caps_kernel<<<nb, kScanBlock, 0, s>>>(d_descs, n, d_data, caps, local_first, block_sum);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_block_scan(block_sum, nb, d_index_used, s);
}

hipError_t launch_block_scan(uint64_t* block_sum, uint32_t nb, uint64_t* total, hipStream_t s) {
    block_scan_kernel<<<1, kScanBlock, 0, s>>>(block_sum, nb, total);
    return hipGetLastError();
}

// Overlap (RPGPU_OPT_WALK_OVERLAP): the arena is checksummed in ov->chunks
// launches and each chunk's walk runs on the overlap stream while the next
// chunk is checksummed.  The walk is latency-bound, the checksum
// bandwidth-bound; they share the CUs.  (Checksums and walks side by side in
// one launch each were measured slower and removed: profiles/r4/NOTES.md r4b.)
hipError_t launch_run(const rpgpu_batch_desc* d_descs, uint32_t n, const uint8_t* d_data,
                      rpgpu_batch_result* d_res, rpgpu_record_index* d_index, uint64_t index_cap,
                      const void* d_scratch, const uint32_t* d_tables, int grid, hipStream_t s,
                      const Overlap* ov) {
    if (n == 0) return hipSuccess;
    uint32_t *caps, *local_first;
    uint64_t* block_sum;
    WaveWalk ww;
    scratch_parts(const_cast<void*>(d_scratch), n, &caps, &local_first, &block_sum, &ww);
    hipError_t e = hipSuccess;
    const uint32_t chunks = (ov && n >= kRunChunkMin) ? (uint32_t)ov->chunks : 1u;
    if ((e = hipMemsetAsync(ww.count, 0, 2 * sizeof(uint32_t), s)) != hipSuccess) return e;
    hipStream_t ws = s;  // the walks' stream
    for (uint32_t k = 0; k < chunks; k++) {
        const uint32_t lo = (uint32_t)((uint64_t)n * k / chunks), hi = (uint32_t)((uint64_t)n * (k + 1) / chunks);
        const uint32_t need = (hi - lo + kWavesPerBlock - 1) / kWavesPerBlock;
        const uint32_t g = (uint32_t)grid < need ? (uint32_t)grid : need;
        validate_kernel<<<g, kValidateThreads, 0, s>>>(d_descs, lo, hi, d_data, d_res, d_index, local_first, caps,
                                                        block_sum, index_cap, d_tables);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if (chunks > 1) {
            if ((e = hipEventRecord(ov->ev[k], s)) != hipSuccess) return e;
            if ((e = hipStreamWaitEvent(ov->aux, ov->ev[k], 0)) != hipSuccess) return e;
            ws = ov->aux;
        }
        walk_kernel<<<(hi - lo + 255) / 256, 256, 0, ws>>>(d_descs, lo, hi, d_data, d_res, d_index, local_first,
                                                           caps, block_sum, index_cap, ww.list, ww.count);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    // batches of many records, a wavefront each, after the lane walks
    {
        // 1,024 waves from the queue (C5 lists ~7,600 batches of 65..1,024 records:
        // 1.75 ms at 512 waves); an empty list costs each wave one load
        const uint32_t wg = (n < 1024u ? (n + 3) / 4 : 256u);
        walk_wave_kernel<<<wg, 256, 0, ws>>>(d_descs, d_data, d_res, d_index, local_first, caps, block_sum, index_cap,
                                             ww.list, ww.count, ww.count + 1);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (chunks > 1) {  // the caller's stream sees the last walk
        if ((e = hipEventRecord(ov->ev[chunks], ov->aux)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(s, ov->ev[chunks], 0)) != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_validate(const rpgpu_batch_desc* d_descs, uint32_t n, const uint8_t* d_data,
                           rpgpu_batch_result* d_res, rpgpu_record_index* d_index, uint64_t index_cap,
                           uint64_t* d_index_used, void* d_scratch, const uint32_t* d_tables, int grid,
                           hipStream_t s, const Overlap* ov) {
    hipError_t e;
    if (ov && n >= kRunChunkMin) {
        // the plan (index slices) on the walks' stream: only the walks read it,
        // so the first checksums start at once (launch_run's closing join makes
        // d_index_used visible on s with the walks)
        if ((e = hipEventRecord(ov->ev[ov->chunks], s)) != hipSuccess) return e;
        if ((e = hipStreamWaitEvent(ov->aux, ov->ev[ov->chunks], 0)) != hipSuccess) return e;
        if ((e = launch_plan(d_descs, n, d_data, d_index_used, d_scratch, ov->aux)) != hipSuccess) return e;
    } else if ((e = launch_plan(d_descs, n, d_data, d_index_used, d_scratch, s)) != hipSuccess) {
        return e;
    }
    return launch_run(d_descs, n, d_data, d_res, d_index, index_cap, d_scratch, d_tables, grid, s, ov);
}

hipError_t launch_crc_ranges(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len,
                             const uint32_t* d_seed, uint32_t n, uint32_t* d_out, const uint32_t* d_tables,
                             int grid, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint32_t need = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    const uint32_t g = (uint32_t)grid < need ? (uint32_t)grid : need;
    crc_ranges_kernel<<<g, kValidateThreads, 0, s>>>(d_data, d_off, d_len, d_seed, n, d_out, d_tables);
    return hipGetLastError();
}

hipError_t validate_occupancy(int* blocks_per_cu) {
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(blocks_per_cu, validate_kernel, kValidateThreads, 0);
}

size_t validate_scratch_bytes(uint32_t n) {
    const size_t nb = (n + kScanBlock - 1) / kScanBlock;
    return (((((size_t)n * 8 + 15) & ~(size_t)15) + nb * 8 + 63) & ~(size_t)63) + 64 + (size_t)n * 4 + 64;
}

}  // namespace rpgpu

#ifdef RPGPU_DIAG_STAMPS
// diagnostics build: read and clear the per-phase cycle sums
extern "C" int rpgpu_diag_stamps(unsigned long long* out) {
    unsigned long long z[8] = {};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(rpgpu::g_stamps), sizeof(z)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(rpgpu::g_stamps), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
