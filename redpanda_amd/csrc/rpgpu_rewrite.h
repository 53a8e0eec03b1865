// rpgpu_rewrite.h — what the kernels that emit new on-disk batches share
// (decompression, compression, compaction rewrite, legacy conversion, produce).
//
// A rewriter stores the new body and a header whose two CRC fields are zero,
// and one output descriptor per batch with RPGPU_OP_RECRC.  launch_revalidate
// then runs the validation over those descriptors -- the Kafka CRC of the new
// body, then the header CRC over a header carrying it
// (reset_size_checksum_metadata, storage/parser_utils.cc:122-128), the record
// walk and the index -- and recrc_patch_kernel stores both CRCs into the
// headers.
#ifndef RPGPU_REWRITE_H
#define RPGPU_REWRITE_H

#include "rpgpu_device.h"
#include "rpgpu_launch.h"

namespace rpgpu {

// header field of the input batch: big-endian on the wire, little-endian on disk
__device__ __forceinline__ uint64_t hdr_field(const uint8_t* p, int off, int nb, bool be) {
    uint64_t v = 0;
    for (int k = 0; k < nb; k++) v = be ? (v << 8) | p[off + k] : v | ((uint64_t)p[off + k] << (8 * k));
    return v;
}
__device__ __forceinline__ void put_le(uint8_t* o, int off, uint64_t v, int nb) {
    for (int k = 0; k < nb; k++) o[off + k] = (uint8_t)(v >> (8 * k));
}

// The on-disk header (storage/parser.cc:40-80) at o of a batch rewritten from
// the input batch at p (wire: be): size_bytes as given, the attributes' codec
// bits replaced by codec, both CRCs zero, raft_data for a produced batch,
// every other field the input's.
// A macro, not a function: as a function (always inlined) the compiler merges
// the byte accesses differently and compress_lane_kernel<4> needs 131 VGPRs
// instead of 127, which costs it the fourth wave per SIMD.
#define RPGPU_WRITE_DISK_HEADER_FROM(o, p, be, codec, size_bytes)                       \
    do {                                                                                \
        put_le(o, 0, 0, 4);                                                             \
        put_le(o, 4, size_bytes, 4);                                                    \
        put_le(o, 8, (be) ? hdr_field(p, 0, 8, true) : hdr_field(p, 8, 8, false), 8);   \
        (o)[16] = (be) ? (uint8_t)1 : (p)[16];                                          \
        put_le(o, 17, 0, 4);                                                            \
        put_le(o, 21, (hdr_field(p, 21, 2, be) & ~(uint64_t)7) | (codec), 2);           \
        put_le(o, 23, hdr_field(p, 23, 4, be), 4);                                      \
        put_le(o, 27, hdr_field(p, 27, 8, be), 8);                                      \
        put_le(o, 35, hdr_field(p, 35, 8, be), 8);                                      \
        put_le(o, 43, hdr_field(p, 43, 8, be), 8);                                      \
        put_le(o, 51, hdr_field(p, 51, 2, be), 2);                                      \
        put_le(o, 53, hdr_field(p, 53, 4, be), 4);                                      \
        put_le(o, 57, hdr_field(p, 57, 4, be), 4);                                      \
    } while (0)

// descriptor of an output batch (ops 0: none was emitted)
__device__ __forceinline__ rpgpu_batch_desc out_desc(uint64_t off, uint32_t length, uint32_t partition, uint8_t ops) {
    rpgpu_batch_desc od;
    od.offset = off;
    od.length = length;
    od.partition = partition;
    od.format = RPGPU_FMT_RP_DISK;
    od.ops = ops;
    od.flags = 0;
    od.reserved = 0;
    return od;
}

// did the rewriter emit a batch for this result row?
__device__ __forceinline__ bool rewritten(const rpgpu_decomp_result& r) { return r.verdict == RPGPU_V_OK; }
__device__ __forceinline__ bool rewritten(const rpgpu_legacy_result& r) { return r.verdict == RPGPU_V_OK; }
__device__ __forceinline__ bool rewritten(const rpgpu_compact_result& r) { return r.out_len != 0; }
__device__ __forceinline__ bool rewritten(const rpgpu_produce_batch& r) { return r.out_len != 0; }

// stores the CRCs the validation of the rewritten batches computed
template <class R>
__global__ __launch_bounds__(256) void recrc_patch_kernel(const R* __restrict__ rres,
                                                          const rpgpu_batch_result* __restrict__ vres2, uint32_t n,
                                                          uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !rewritten(rres[i])) return;
    uint8_t* o = out + rres[i].out_offset;
    put_le(o, 0, vres2[i].header_crc, 4);
    put_le(o, 17, vres2[i].crc, 4);
}

// The tail of every rewriter's run: plan, validate and walk the rewritten
// batches in one launch (no chunked overlap: 16 chunks measured slower on the
// rewritten arena, 103 vs 95 ms per C3 step), then patch the headers.
template <class R>
hipError_t launch_revalidate(const rpgpu_batch_desc* d_out_descs, uint32_t n, uint8_t* d_out, const R* d_rres,
                             rpgpu_batch_result* d_vres2, rpgpu_record_index* d_index, uint64_t index_cap,
                             uint64_t* d_index_used, void* d_vscratch, const uint32_t* d_tables, int grid,
                             hipStream_t s) {
    hipError_t e;
    if ((e = launch_plan(d_out_descs, n, d_out, d_index_used, d_vscratch, s)) != hipSuccess) return e;
    if ((e = launch_run(d_out_descs, n, d_out, d_vres2, d_index, index_cap, d_vscratch, d_tables, grid, s, nullptr)) !=
        hipSuccess)
        return e;
    recrc_patch_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_rres, d_vres2, n, d_out);
    return hipGetLastError();
}

}  // namespace rpgpu
#endif
