// rpgpu_sort.h — the stable LSD radix sort of item numbers on a 32-bit key
// (device only; include after rpgpu_device.h and rpgpu_scan.h, inside a
// translation unit that launches it: the kernels have internal linkage).
//
// 8-bit digits.  Per pass: a digit histogram per block of kSortBlock items
// (radix_hist_kernel), an exclusive scan of the digits x blocks table,
// digit-major (radix_scan_kernel over the table), a stable scatter
// (radix_scatter_kernel).  The rank inside a wave is a ballot match
// (popc(same-digit lanes below)), the waves of a block are combined in LDS in
// wave order: no atomic ticket, so equal keys keep their input order.
//
//   key    the key of item i, for every i < n (never permuted)
//   in     the pass's input order (null for pass 0: the items' own order)
//   table  sort_blocks(n) * 256 words of scratch
// rpgpu_append.hip sorts batches by log; rpgpu_txfilter.hip abort markers by producer;
// rpgpu_produce.hip rows by partition, then by request.
#ifndef RPGPU_SORT_H
#define RPGPU_SORT_H

#include "rpgpu_device.h"
#include "rpgpu_scan.h"

namespace rpgpu {
namespace {

constexpr uint32_t kSortBlock = 1024;  // items per sort block (16 waves, one item per lane)
constexpr uint32_t kSortWaves = kSortBlock / 64;

inline uint32_t sort_blocks(uint32_t n) { return (uint32_t)(((uint64_t)n + kSortBlock - 1) / kSortBlock); }
// digits of the largest key
inline uint32_t sort_passes(uint32_t max_key) {
    uint32_t bits = 1;
    while (bits < 32 && (max_key >> bits)) bits++;
    return (bits + 7) / 8;
}

// in-place exclusive scan of a[0, len) by one workgroup
__global__ __launch_bounds__(kScanBlock) void radix_scan_kernel(uint32_t* a, uint32_t len) {
    __shared__ uint32_t part[kScanBlock];
    (void)array_scan_excl(a, a, len, part);
}

// item i of a pass's input order (pass 0: the items' own order)
__device__ __forceinline__ uint32_t sort_item(const uint32_t* __restrict__ in, uint32_t i) { return in ? in[i] : i; }

__global__ __launch_bounds__(kSortBlock) void radix_hist_kernel(const uint32_t* __restrict__ key,
                                                                const uint32_t* __restrict__ in, uint32_t n,
                                                                uint32_t shift, uint32_t nblocks,
                                                                uint32_t* __restrict__ table) {
    __shared__ uint32_t h[256];
    if (threadIdx.x < 256) h[threadIdx.x] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x;
    if (i < n) atomicAdd(&h[(key[sort_item(in, (uint32_t)i)] >> shift) & 255u], 1u);
    __syncthreads();
    if (threadIdx.x < 256) table[(size_t)threadIdx.x * nblocks + blockIdx.x] = h[threadIdx.x];
}

__global__ __launch_bounds__(kSortBlock) void radix_scatter_kernel(const uint32_t* __restrict__ key,
                                                                   const uint32_t* __restrict__ in, uint32_t n,
                                                                   uint32_t shift, uint32_t nblocks,
                                                                   const uint32_t* __restrict__ table,
                                                                   uint32_t* __restrict__ out) {
    __shared__ uint32_t wc[kSortWaves][256];  // per wave and digit: count, then the count of the waves before
    for (uint32_t q = threadIdx.x; q < kSortWaves * 256; q += kSortBlock) (&wc[0][0])[q] = 0;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * kSortBlock + threadIdx.x;
    const bool live = i < n;
    const uint32_t item = live ? sort_item(in, (uint32_t)i) : 0u;
    const uint32_t dg = live ? (key[item] >> shift) & 255u : 0u;
    // lanes of this wave with the same digit
    uint64_t m = __ballot(live);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (dg >> b) & 1u;
        const uint64_t bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t below = m & ((1ull << lane) - 1);
    if (live && below == 0) wc[w][dg] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x < 256) {
        uint32_t run = 0;
        for (uint32_t k = 0; k < kSortWaves; k++) {
            const uint32_t v = wc[k][threadIdx.x];
            wc[k][threadIdx.x] = run;
            run += v;
        }
    }
    __syncthreads();
    if (live) {
        const uint64_t at = (uint64_t)table[(size_t)dg * nblocks + blockIdx.x] + wc[w][dg] + (uint32_t)__popcll(below);
        if (at < n) out[at] = item;
    }
}

// Sorts the items 0..n-1 on key (keys <= max_key), ping-ponging between idx_a
// and idx_b; *sorted is the array that holds the result (null when n == 0).
// in0: the order the first pass reads (null: the items' own), so a sort on a
// second key chains behind one on a first; in0 must not be idx_a.
inline hipError_t radix_sort_items(const uint32_t* key, uint32_t n, uint32_t max_key, uint32_t* idx_a,
                                   uint32_t* idx_b, uint32_t* table, const uint32_t** sorted, hipStream_t s,
                                   const uint32_t* in0 = nullptr) {
    const uint32_t passes = sort_passes(max_key), nb = sort_blocks(n);
    const uint32_t* in = in0;
    for (uint32_t k = 0; n && k < passes; k++) {
        uint32_t* out = (k & 1) ? idx_b : idx_a;
        radix_hist_kernel<<<nb, kSortBlock, 0, s>>>(key, in, n, 8 * k, nb, table);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        radix_scan_kernel<<<1, kScanBlock, 0, s>>>(table, nb * 256);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        radix_scatter_kernel<<<nb, kSortBlock, 0, s>>>(key, in, n, 8 * k, nb, table, out);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        in = out;
    }
    *sorted = in;
    return hipSuccess;
}

}  // namespace
}  // namespace rpgpu
#endif
