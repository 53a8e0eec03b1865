// rpgpu_summary.hip — per-partition summaries of validated batches, the data
// each GPU contributes to the final gather of a partition-sharded run
// (redpanda_amd/shard.py does the all-gather).
//
// Per partition p in [part_lo, part_lo + nparts): batches, OK batches, index
// entries, bytes of OK batches (size_bytes), sum of the computed CRCs, and
// the last offset (max base_offset + last_offset_delta over OK batches, -1 if
// none) -- the state produce / recovery would hand to the partition's owner
// (storage/offset_assignment.h:25-28: next offset = last_offset + 1).
//
// Up to 4096 partitions (summary_lds_kernel): per-workgroup tables in LDS,
// added up by summary_reduce_kernel.  More partitions: one thread per batch,
// 64-bit atomics into the partition's row; a wave whose lanes all hit one
// partition reduces in registers first and issues one atomic per column.
#include "rpgpu_device.h"
#include "rpgpu_launch.h"

namespace rpgpu {

constexpr int kSumCols = 6;

__global__ __launch_bounds__(256) void summary_init_kernel(int64_t* __restrict__ out, uint32_t nparts) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nparts) return;
    int64_t* o = out + (size_t)i * kSumCols;
    o[0] = o[1] = o[2] = o[3] = o[4] = 0;
    o[5] = -1;
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}
__device__ __forceinline__ int64_t wave_max(int64_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int64_t o = __shfl_xor(v, s, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void summary_kernel(const rpgpu_batch_desc* __restrict__ descs,
                                                      const rpgpu_batch_result* __restrict__ res, uint32_t n,
                                                      uint32_t part_lo, uint32_t nparts, int64_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = i < n;
    uint32_t part = 0;
    int64_t v[kSumCols] = {0, 0, 0, 0, 0, -1};
    bool in_range = false;
    if (live) {
        part = descs[i].partition - part_lo;
        in_range = part < nparts;
        const rpgpu_batch_result& r = res[i];
        const bool ok = r.verdict == RPGPU_V_OK;
        v[0] = 1;
        v[1] = ok;
        v[2] = r.index_count;
        v[3] = ok ? (int64_t)r.size_bytes : 0;
        v[4] = r.crc;
        v[5] = ok ? r.base_offset + r.last_offset_delta : -1;
    }
    // one partition across the whole (full) wave: reduce, one atomic per column
    const uint32_t p0 = __builtin_amdgcn_readfirstlane(part);
    const bool uniform = __ballot(live && in_range && part == p0) == __ballot(1);
    if (uniform && __ballot(live) == __ballot(1)) {
        int64_t s[kSumCols];
#pragma unroll
        for (int c = 0; c < 5; c++) s[c] = wave_sum(v[c]);
        s[5] = wave_max(v[5]);
        if (lane_id() == 0) {
            int64_t* o = out + (size_t)p0 * kSumCols;
#pragma unroll
            for (int c = 0; c < 5; c++) atomicAdd(reinterpret_cast<unsigned long long*>(o + c), (unsigned long long)s[c]);
            atomicMax(reinterpret_cast<long long*>(o + 5), (long long)s[5]);
        }
        return;
    }
    if (!live || !in_range) return;
    int64_t* o = out + (size_t)part * kSumCols;
#pragma unroll
    for (int c = 0; c < 5; c++)
        if (v[c]) atomicAdd(reinterpret_cast<unsigned long long*>(o + c), (unsigned long long)v[c]);
    if (v[5] >= 0) atomicMax(reinterpret_cast<long long*>(o + 5), (long long)v[5]);
}

// Up to kLdsParts partitions: privatised tables instead of global atomics.
// Arenas interleave partitions at least as often as not (C2: batch i belongs
// to partition i mod 4096), so a wave's 64 batches hit 64 rows and the atomic
// path above costs one 64-bit atomic per batch and column (0.22 ms for C2).
// Here each workgroup owns a contiguous range of batches and accumulates into
// an LDS table (160 KiB for 4096 partitions: LDS atomics), writes the table
// out with plain stores, and summary_reduce_kernel adds the G tables up.
constexpr uint32_t kLdsParts = 4096;
constexpr uint32_t kSumThreads = 1024;

__global__ __launch_bounds__(kSumThreads) void summary_lds_kernel(const rpgpu_batch_desc* __restrict__ descs,
                                                                  const rpgpu_batch_result* __restrict__ res,
                                                                  uint32_t n, uint32_t part_lo, uint32_t nparts,
                                                                  int64_t* __restrict__ partial) {
    __shared__ uint32_t s_cnt[kLdsParts], s_ok[kLdsParts];
    __shared__ unsigned long long s_idx[kLdsParts], s_bytes[kLdsParts], s_crc[kLdsParts];
    __shared__ long long s_last[kLdsParts];
    for (uint32_t p = threadIdx.x; p < nparts; p += kSumThreads) {
        s_cnt[p] = s_ok[p] = 0;
        s_idx[p] = s_bytes[p] = s_crc[p] = 0;
        s_last[p] = -1;
    }
    __syncthreads();
    const uint32_t lo = (uint32_t)((uint64_t)n * blockIdx.x / gridDim.x);
    const uint32_t hi = (uint32_t)((uint64_t)n * (blockIdx.x + 1) / gridDim.x);
    for (uint32_t i = lo + threadIdx.x; i < hi; i += kSumThreads) {
        const uint32_t part = descs[i].partition - part_lo;
        if (part >= nparts) continue;
        const rpgpu_batch_result& r = res[i];
        const bool ok = r.verdict == RPGPU_V_OK;
        atomicAdd(&s_cnt[part], 1u);
        if (r.index_count) atomicAdd(&s_idx[part], (unsigned long long)r.index_count);
        if (r.crc) atomicAdd(&s_crc[part], (unsigned long long)r.crc);
        if (ok) {
            atomicAdd(&s_ok[part], 1u);
            atomicAdd(&s_bytes[part], (unsigned long long)(int64_t)r.size_bytes);
            atomicMax(&s_last[part], (long long)(r.base_offset + r.last_offset_delta));
        }
    }
    __syncthreads();
    int64_t* o = partial + (size_t)blockIdx.x * nparts * kSumCols;
    for (uint32_t q = threadIdx.x; q < nparts * kSumCols; q += kSumThreads) {
        const uint32_t p = q / kSumCols, c = q % kSumCols;
        o[q] = c == 0   ? (int64_t)s_cnt[p]
               : c == 1 ? (int64_t)s_ok[p]
               : c == 2 ? (int64_t)s_idx[p]
               : c == 3 ? (int64_t)s_bytes[p]
               : c == 4 ? (int64_t)s_crc[p]
                        : (int64_t)s_last[p];
    }
}

__global__ __launch_bounds__(256) void summary_reduce_kernel(const int64_t* __restrict__ partial, uint32_t groups,
                                                             uint32_t nparts, int64_t* __restrict__ out) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nparts * kSumCols) return;
    const bool is_max = q % kSumCols == 5;
    int64_t v = is_max ? -1 : 0;
    for (uint32_t g = 0; g < groups; g++) {
        const int64_t x = partial[(size_t)g * nparts * kSumCols + q];
        v = is_max ? (x > v ? x : v) : v + x;
    }
    out[q] = v;
}

uint32_t summary_groups(int cu_count) { return cu_count > 0 ? (uint32_t)cu_count : 256u; }
size_t summary_scratch_bytes(int cu_count) { return (size_t)summary_groups(cu_count) * kLdsParts * kSumCols * 8; }

hipError_t launch_summaries(const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res, uint32_t n,
                            uint32_t part_lo, uint32_t nparts, int64_t* d_out, hipStream_t s, int64_t* d_partial,
                            int cu_count) {
    if (nparts == 0) return hipSuccess;
    if (d_partial && nparts <= kLdsParts && n > 0) {
        // enough batches per workgroup to amortise its table (>= 4 per partition)
#ifndef RPGPU_SUM_PER_PART
#define RPGPU_SUM_PER_PART 4
#endif
        uint32_t g = (uint32_t)(((uint64_t)n + (uint64_t)RPGPU_SUM_PER_PART * nparts - 1) /
                                ((uint64_t)RPGPU_SUM_PER_PART * nparts));
        if (g > summary_groups(cu_count)) g = summary_groups(cu_count);
        if (g < 1) g = 1;
        summary_lds_kernel<<<g, kSumThreads, 0, s>>>(d_descs, d_res, n, part_lo, nparts, d_partial);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        summary_reduce_kernel<<<(nparts * kSumCols + 255) / 256, 256, 0, s>>>(d_partial, g, nparts, d_out);
        return hipGetLastError();
    }
    summary_init_kernel<<<(nparts + 255) / 256, 256, 0, s>>>(d_out, nparts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n == 0) return e;
    summary_kernel<<<(n + 255) / 256, 256, 0, s>>>(d_descs, d_res, n, part_lo, nparts, d_out);
    return hipGetLastError();
}

}  // namespace rpgpu
