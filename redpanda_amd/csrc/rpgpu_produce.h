// rpgpu_produce.h — the per-row logic of building produce batches from records
// (include/rpgpu.h, "produce batches from records"), as host/device functions:
// the kernels of rpgpu_produce.hip and the host program
// tests/native/produce_host.cpp compile the same code.
//
// Reference (paths relative to src/v/):
//   client::produce_records                    kafka/client/client.cc:231-271
//     (absent key -> iobuf{}: 257-260; topic_error -> partition 0: 240-246)
//   default / identity / murmur2 / roundrobin  kafka/client/partitioners.cc:25-109
//   murmur2, seed 0x9747b28c                   hashing/murmur.cc:384-432, hashing/murmur.h:38-44
//   record_batch_builder::add_raw_kw / build   storage/record_batch_builder.cc:29-102
//
// A row's partition is the first rule that answers: (1) its own id, unchecked;
// (2) a non-empty key: murmur2(key) % partition_count on the unsigned hash;
// (3) (rr_initial + k) % partition_count, k = the earlier rule-3 rows of the
// request.  partition_count 0 (topic not cached): partition 0 for every row
// without an id, and the round-robin counter stays.
#ifndef RPGPU_PRODUCE_H
#define RPGPU_PRODUCE_H

#include <stdint.h>

#include "rpgpu.h"
#include "rpgpu_legacy.h"

#ifdef __HIPCC__
#define RPR_HD __host__ __device__ __forceinline__
#else
#define RPR_HD static inline
#endif

namespace rpproduce {

constexpr uint32_t kMurmurSeed = 0x9747b28cu;
constexpr uint32_t kNone = 0xffffffffu;
constexpr uint32_t kRuleId = 1, kRuleHash = 2, kRuleRoundRobin = 3, kRuleUncached = 4;

struct Mur {
    uint32_t h;
    uint64_t buf;   // bytes not mixed yet, the oldest lowest
    uint32_t have;  // how many: 0..3 between feeds
};
RPR_HD void mur_word(Mur& s) {
    const uint32_t m = 0x5bd1e995u;
    uint32_t k = (uint32_t)s.buf;
    k *= m;
    k ^= k >> 24;
    k *= m;
    s.h *= m;
    s.h ^= k;
    s.buf >>= 32;
    s.have -= 4;
}
RPR_HD void mur_byte(Mur& s, uint8_t b) {
    s.buf |= (uint64_t)b << (8 * s.have);
    if (++s.have == 4) mur_word(s);
}
RPR_HD void mur_u32(Mur& s, uint32_t w) {
    s.buf |= (uint64_t)w << (8 * s.have);
    s.have += 4;
    mur_word(s);
}

// murmur2 (hashing/murmur.cc:384-432) of p[0, len).  The reference reads the
// key in unaligned 4-byte little-endian words; here the bytes up to the first
// 16-byte boundary and behind the last one are read one by one, everything
// between in aligned 16-byte loads, and the words are put together by shifts.
// No byte outside [p, p + len) is read.
RPR_HD uint32_t murmur2(const uint8_t* p, uint32_t len, uint32_t seed) {
    const uint32_t m = 0x5bd1e995u;
    Mur s;
    s.h = seed ^ len;
    s.buf = 0;
    s.have = 0;
    uint32_t i = 0;
    const uint32_t lead = (uint32_t)((16u - ((uintptr_t)p & 15u)) & 15u);
    for (; i < len && i < lead; i++) mur_byte(s, p[i]);
    for (; i + 16 <= len; i += 16) {
        uint32_t w[4];
        __builtin_memcpy(w, __builtin_assume_aligned(p + i, 16), 16);
        mur_u32(s, w[0]);
        mur_u32(s, w[1]);
        mur_u32(s, w[2]);
        mur_u32(s, w[3]);
    }
    for (; i < len; i++) mur_byte(s, p[i]);
    // the tail: case 3 / 2 / 1 with fall-through is the xor of the bytes left, in place
    if (s.have) {
        s.h ^= (uint32_t)s.buf;
        s.h *= m;
    }
    s.h ^= s.h >> 13;
    s.h *= m;
    s.h ^= s.h >> 15;
    return s.h;
}

// engine guard rail (unpinned): a length below -1, or a range outside the data
RPR_HD bool row_ok(const rpgpu_produce_row& r, uint64_t data_bytes) {
    if (r.key_len < -1 || r.val_len < -1) return false;
    if (r.key_len > 0 && (r.key_off > data_bytes || data_bytes - r.key_off < (uint64_t)r.key_len)) return false;
    if (r.val_len > 0 && (r.val_off > data_bytes || data_bytes - r.val_off < (uint64_t)r.val_len)) return false;
    return true;
}

// engine guard rails on the request itself (unpinned: the reference's inputs are typed)
RPR_HD bool request_ok(const rpgpu_produce_request& q) {
    return q.partition_count <= 0x7fffffffu && q.rr_initial >= 0;
}

// default_partitioner's first two rules; *partition is set unless rule 3 answers
RPR_HD uint32_t row_rule(const rpgpu_produce_row& r, const uint8_t* data, uint32_t partition_count,
                         int32_t* partition) {
    if (r.flags & RPGPU_PRODUCE_HAS_PARTITION) {
        *partition = r.partition;
        return kRuleId;
    }
    if (partition_count == 0) {  // partition_for throws topic_error: partition 0
        *partition = 0;
        return kRuleUncached;
    }
    if (r.key_len > 0) {
        *partition = (int32_t)(murmur2(data + r.key_off, (uint32_t)r.key_len, kMurmurSeed) % partition_count);
        return kRuleHash;
    }
    return kRuleRoundRobin;
}
// rule 3 for the request's k-th round-robin row
RPR_HD int32_t round_robin(int32_t rr_initial, uint32_t k, uint32_t partition_count) {
    return (int32_t)(((uint64_t)(uint32_t)rr_initial + k) % partition_count);
}

// the stable sort's first key: signed partition ids in unsigned order
RPR_HD uint32_t partition_key(int32_t partition) { return (uint32_t)partition ^ 0x80000000u; }

// produce_records passes key.value_or(iobuf{}): an absent key is an empty one
RPR_HD int32_t encoded_key_len(int32_t key_len) { return key_len < 0 ? 0 : key_len; }
// the record's length field, and its bytes in the body
// (rplegacy::record_len in 64 bits: two lengths near 2^31 pass 32; such a
// record makes its batch TOO_LARGE, and only records of emitted batches are
// encoded, where the length fits the encoder's 32 bits)
RPR_HD uint64_t record_len(uint32_t delta, const rpgpu_produce_row& r) {
    const int32_t kl = encoded_key_len(r.key_len);
    return 2ull + rplegacy::vint_size(delta) + rplegacy::vint_size(kl) + (uint64_t)kl +
           rplegacy::vint_size(r.val_len) + (r.val_len > 0 ? (uint64_t)r.val_len : 0ull) + 1;
}
RPR_HD uint64_t record_bytes(uint32_t delta, const rpgpu_produce_row& r) {
    const uint64_t n = record_len(delta, r);
    return rplegacy::vint_size((int64_t)n) + n;
}
// engine guard rail: size_bytes is an int32
RPR_HD bool body_fits(uint64_t body) { return body <= 0x7fffffffull - RPGPU_HEADER_SIZE; }

}  // namespace rpproduce
#endif
