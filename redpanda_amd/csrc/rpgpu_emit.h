// rpgpu_emit.h — the one v2 record writer of the kernels that build batches
// from keys and values: the legacy conversion (rpgpu_legacy.hip) and the
// produce path (rpgpu_produce.hip).  Device only; include after rpgpu_device.h
// and rpgpu_legacy.h (the varint writer and put_record_head live there, shared
// with the host programs).
//
// 64 records per wave: the varints and the keys / values of at most
// kLaneCopyMax bytes by the record's lane, in 16-byte pieces; longer ones go
// on a work list (list_append, one atomic per wave) that a second kernel
// copies a wave each (copy_wave, 16 bytes per lane).
#ifndef RPGPU_EMIT_H
#define RPGPU_EMIT_H

#include "rpgpu_device.h"
#include "rpgpu_legacy.h"

namespace rpgpu {

constexpr uint32_t kLaneCopyMax = 128;  // longer keys / values are copied by the whole wave

// a value every lane holds, as a wave-uniform one
__device__ __forceinline__ uint32_t uniform32(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
    return ((uint64_t)uniform32((uint32_t)(v >> 32)) << 32) | uniform32((uint32_t)v);
}

// the lanes with `want` append `item` to the list: one atomic per wave
__device__ __forceinline__ void list_append(uint64_t* list, uint64_t* count, bool want, uint64_t item, uint32_t l) {
    const uint64_t mask = __ballot(want);
    if (!mask) return;
    const int first = __builtin_ctzll(mask);
    uint64_t base = 0;
    if ((int)l == first) base = atomicAdd(reinterpret_cast<unsigned long long*>(count), (unsigned long long)__builtin_popcountll(mask));
    base = ((uint64_t)__shfl((uint32_t)(base >> 32), first, 64) << 32) | __shfl((uint32_t)base, first, 64);
    if (want) list[base + __builtin_popcountll(mask & ((1ull << l) - 1))] = item;
}

// 16-byte pieces; the last one ends at the range's end and overlaps the one
// before it (the same bytes twice), so nothing past either range is touched
__device__ __forceinline__ void copy_lane(uint8_t* dst, const uint8_t* src, uint32_t len) {
    if (len < 16) {
        for (uint32_t k = 0; k < len; k++) dst[k] = src[k];
        return;
    }
    for (uint32_t k = 0; k + 16 <= len; k += 16) {
        const u32x4 v = ld16(src + k);
        __builtin_memcpy(dst + k, &v, 16);
    }
    if (len & 15u) {
        const u32x4 v = ld16(src + len - 16);
        __builtin_memcpy(dst + len - 16, &v, 16);
    }
}
__device__ __forceinline__ void copy_wave(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t l) {
    for (uint64_t o = 16ull * l; o + 16 <= len; o += 1024) {
        const u32x4 v = ld16(src + o);
        __builtin_memcpy(dst + o, &v, 16);
    }
    if ((len & 15u) && l == 0) {
        const u32x4 v = ld16(src + len - 16);
        __builtin_memcpy(dst + len - 16, &v, 16);
    }
}

// where a record's key and value go
struct RecordPlace {
    const uint8_t *ksrc, *vsrc;
    uint8_t *head, *kdst, *vlen_at, *vdst;
    uint32_t klen, vlen;
};
// the record at head: length field rec_len, offset delta index, key_len / val_len as encoded (-1 null)
__device__ __forceinline__ RecordPlace place_record(uint8_t* head, const uint8_t* ksrc, const uint8_t* vsrc,
                                                    uint32_t rec_len, uint32_t index, int32_t key_len,
                                                    int32_t val_len) {
    RecordPlace q;
    q.head = head;
    q.klen = key_len > 0 ? (uint32_t)key_len : 0u;
    q.vlen = val_len > 0 ? (uint32_t)val_len : 0u;
    q.ksrc = ksrc;
    q.vsrc = vsrc;
    q.kdst = q.head + rplegacy::vint_size(rec_len) + 2 + rplegacy::vint_size(index) + rplegacy::vint_size(key_len);
    q.vlen_at = q.kdst + q.klen;
    q.vdst = q.vlen_at + rplegacy::vint_size(val_len);
    return q;
}

// the record's lane: the varints, the empty header count and the short key /
// value; klong / vlong: the key / value is left to copy_wave
__device__ __forceinline__ void emit_record_lane(const RecordPlace& q, uint32_t rec_len, uint32_t index,
                                                 int32_t key_len, int32_t val_len, bool& klong, bool& vlong) {
    (void)rplegacy::put_record_head(q.head, rec_len, index, key_len);
    (void)rplegacy::put_vint(q.vlen_at, val_len);
    q.vdst[q.vlen] = 0;  // no headers
    klong = q.klen > kLaneCopyMax;
    vlong = q.vlen > kLaneCopyMax;
    if (!klong) copy_lane(q.kdst, q.ksrc, q.klen);
    if (!vlong) copy_lane(q.vdst, q.vsrc, q.vlen);
}

// a listed key (value: is_val) of the record at q, by the whole wave
__device__ __forceinline__ void copy_listed(const RecordPlace& q, bool is_val, uint32_t l) {
    if (is_val) copy_wave((uint8_t*)uniform64((uint64_t)q.vdst), (const uint8_t*)uniform64((uint64_t)q.vsrc), uniform32(q.vlen), l);
    else copy_wave((uint8_t*)uniform64((uint64_t)q.kdst), (const uint8_t*)uniform64((uint64_t)q.ksrc), uniform32(q.klen), l);
}

}  // namespace rpgpu
#endif
