// rpgpu_scan.h — the prefix sums of the planners (device only; include after
// rpgpu_device.h).
//
// A planner gives every item (batch, record set) a span of an output array: a
// slot of bytes, a slice of descriptors.  The item's position is the sum of the
// spans in front of it, computed in two levels:
//
//   block_scan_excl   in the planner, one thread per item and kScanBlock items
//                     per workgroup: the item's offset within its workgroup
//                     (stored as local[i]) and the workgroup's total
//                     (block_sum[blockIdx.x]);
//   array_scan_excl   one workgroup turns block_sum into the exclusive scan of
//                     itself and returns the grand total;
//   slot_offset       what every later kernel reads: block_base[i / kScanBlock]
//                     + local[i].
#ifndef RPGPU_SCAN_H
#define RPGPU_SCAN_H

#include "rpgpu_device.h"

namespace rpgpu {

// lane l receives lane l - s (its own value below s)
__device__ __forceinline__ uint32_t shfl_up(uint32_t x, int s) { return __shfl_up(x, s, 64); }
__device__ __forceinline__ uint64_t shfl_up(uint64_t x, int s) {
    const uint32_t lo = __shfl_up((uint32_t)x, s, 64), hi = __shfl_up((uint32_t)(x >> 32), s, 64);
    return ((uint64_t)hi << 32) | lo;
}
// every lane receives lane src's value
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src) {
    const uint32_t lo = __shfl((uint32_t)v, src, 64), hi = __shfl((uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

// inclusive scan over the wave's lanes (wrapping).  T: uint32_t, uint64_t, or
// a type with operator+ and a shfl_up of its own.
template <class T>
__device__ __forceinline__ T wave_scan_incl(T x, uint32_t lane) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const T y = shfl_up(x, s);
        if (lane >= (uint32_t)s) x = x + y;
    }
    return x;
}

// Exclusive scan of v over a workgroup of kScanBlock threads (one barrier).
// wsum: kScanBlock / 64 values in LDS, afterwards the sums of the waves.
template <class T>
__device__ __forceinline__ T block_scan_excl(T v, T* wsum) {
    const uint32_t l = lane_id();
    const T x = wave_scan_incl(v, l);
    const uint32_t wv = threadIdx.x >> 6;
    if (l == 63) wsum[wv] = x;
    __syncthreads();
    T wbase = T();
    for (uint32_t k = 0; k < wv; k++) wbase = wbase + wsum[k];
    return wbase + x - v;
}
// the same; the last thread stores the workgroup's total to block_sum[blockIdx.x]
template <class T>
__device__ __forceinline__ T block_scan_excl(T v, T* wsum, uint64_t* block_sum) {
    const T e = block_scan_excl(v, wsum);
    if (threadIdx.x == kScanBlock - 1) {
        uint64_t tot = 0;
        for (uint32_t k = 0; k < kScanBlock / 64; k++) tot += wsum[k];
        block_sum[blockIdx.x] = tot;
    }
    return e;
}

// item i's position: its workgroup's base (the scanned block_sum) + local[i]
template <class T>
__device__ __forceinline__ uint64_t slot_offset(const uint64_t* block_base, const T* local, uint32_t i) {
    return block_base[i / kScanBlock] + local[i];
}

// Exclusive scan of in[0, n) into out by one workgroup of kScanBlock threads,
// a contiguous chunk per thread; out may be in, or null (only the total is
// wanted).  part: kScanBlock values in LDS, free again on return.  Returns the
// total, in every thread.
template <class T>
__device__ __forceinline__ T array_scan_excl(const T* in, T* out, uint64_t n, T* part) {
    const uint32_t t = threadIdx.x;
    const uint64_t per = (n + kScanBlock - 1) / kScanBlock;
    const uint64_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    T s = 0;
    for (uint64_t k = lo; k < hi; k++) s += in[k];
    part[t] = s;
    __syncthreads();
    for (uint32_t off = 1; off < kScanBlock; off <<= 1) {
        const T v = t >= off ? part[t - off] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    if (out) {
        T run = part[t] - s;
        for (uint64_t k = lo; k < hi; k++) {
            const T v = in[k];
            out[k] = run;
            run += v;
        }
    }
    const T total = part[kScanBlock - 1];
    __syncthreads();
    return total;
}

}  // namespace rpgpu
#endif
