// rpgpu_segidx.h — the segment index's life cycle as host/device functions: the
// kernels of rpgpu_segidx.hip and the host program tests/native/segidx_host.cpp
// compile the same code (include/rpgpu.h, "segment index life cycle").
//
// Reference (paths relative to src/v/):
//   offset_time_index                      storage/index_state.h:36-70
//   index_state::maybe_index               storage/index_state.cc:38-109
//   segment_index::maybe_track             storage/segment_index.cc:98-120
//   index_state::serde_write / read_nested storage/index_state.cc:124-219
//   legacy version 3                       storage/index_state_serde_compat.h:23-101
//   serde envelope, scalars, vectors       serde/serde.h:515-565, 592-647, 725-742, 824-830
//   find_nearest, find_highest_...         storage/segment_index.cc:32-41, 122-163, 306-323
//   find_entry                             storage/index_state.h:166-190
//
// The primitives (time_index_raw, track_step, the layout functions, parse_head /
// parse_body, xxh_*, find) are what the kernels call; blob_put, crc32c_bytes and
// xxh64_mult8 are the same work on one thread, which the host program runs.
#ifndef RPGPU_SEGIDX_H
#define RPGPU_SEGIDX_H

#include <stdint.h>

#include "rpgpu.h"

#ifdef __HIPCC__
#define RSX_HD __host__ __device__ __forceinline__
#else
#define RSX_HD static inline
#endif

namespace rpsx {

template <class T>
RSX_HD T ld(const uint8_t* p) {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}
template <class T>
RSX_HD void st(uint8_t* p, T v) {
    __builtin_memcpy(p, &v, sizeof(T));
}

// ------------------------------------------------------- offset_time_index
// the stored time delta (index_state.h:41-53)
RSX_HD uint32_t time_index_raw(int64_t ts, bool with_offset) {
    const int64_t off = 2147483648ll;
    if (with_offset) {
        const int64_t c = ts < -off ? -off : (ts > off - 1 ? off - 1 : ts);
        return (uint32_t)(c + off);
    }
    const int64_t c = ts < 0 ? 0 : (ts > 4294967295ll ? 4294967295ll : ts);
    return (uint32_t)c;
}
// operator() (index_state.h:55-61): a uint32, so a negative delta reads back large
RSX_HD uint32_t offset_time(uint32_t raw, bool with_offset) { return with_offset ? raw - 2147483648u : raw; }

// a state's slot lies inside the entry array and holds its entries
RSX_HD bool slot_ok(const rpgpu_segidx_state& s, uint64_t nentries) {
    return s.entries <= s.entry_cap && (uint64_t)s.entry_first + s.entry_cap <= nentries;
}

// ------------------------------------------------------------------- track
struct Batch {  // what maybe_track reads of a header, and the file position
    int64_t base_offset, first_timestamp, max_timestamp;
    int32_t size_bytes, last_offset_delta;
    bool user_data;  // path().is_internal_topic() || type == raft_data
    uint64_t position;
};
// One batch into the state (e: the state's slot).  RPGPU_V_OK, or the verdict
// that stops tracking in front of this batch: the state is then unchanged.
RSX_HD int32_t track_step(rpgpu_segidx_state* s, rpgpu_index_entry* e, uint32_t step, const Batch& b) {
    if (b.base_offset < s->base_offset) return RPGPU_V_INDEX_OFFSET_BELOW_BASE;  // vassert, index_state.cc:48
    const bool rewrite = b.user_data && s->non_data_timestamps;
    if (rewrite && s->entries != 1) return RPGPU_V_INDEX_NON_DATA_ASSERT;  // vassert, index_state.cc:61
    const uint64_t acc = s->acc + (uint64_t)(int64_t)b.size_bytes;  // _acc += hdr.size_bytes
    const bool first = s->entries == 0;
    const bool indexed = (acc >= step && b.user_data) || first;
    if (indexed && s->entries >= s->entry_cap) return RPGPU_V_INDEX_NO_ROOM;
    s->monotonic = s->monotonic && b.max_timestamp >= s->last_batch_max_timestamp;
    s->last_batch_max_timestamp = b.first_timestamp > b.max_timestamp ? b.first_timestamp : b.max_timestamp;
    int64_t last_ts = b.max_timestamp;
    if (rewrite) {  // first data batch after a configuration batch indexed first
        e[0].relative_time = time_index_raw(last_ts, s->with_offset);
        s->base_timestamp = b.first_timestamp;
        s->max_timestamp = b.first_timestamp;
        s->non_data_timestamps = 0;
    }
    if (first) {
        s->non_data_timestamps = !b.user_data;
        s->base_timestamp = b.first_timestamp;
        s->max_timestamp = b.first_timestamp;
    }
    s->max_offset = (int64_t)((uint64_t)b.base_offset + (uint64_t)(int64_t)b.last_offset_delta);
    if (b.user_data) {
        last_ts = b.first_timestamp > last_ts ? b.first_timestamp : last_ts;
        s->max_timestamp = s->max_timestamp > last_ts ? s->max_timestamp : last_ts;
    }
    s->acc = acc;
    if (indexed) {
        rpgpu_index_entry x;
        x.relative_offset = (uint32_t)((uint64_t)b.base_offset - (uint64_t)s->base_offset);
        x.relative_time = time_index_raw((int64_t)((uint64_t)last_ts - (uint64_t)s->base_timestamp), s->with_offset);
        x.position = b.position;
        e[s->entries++] = x;
        s->acc = 0;
    }
    return RPGPU_V_OK;
}

// -------------------------------------------------------------------- blob
constexpr uint32_t kTmpAt = 10;      // version, compat version, u32 size, u32 L
constexpr uint32_t kTmpFixed = 51;   // bitflags, four int64, three counts, three flags
constexpr uint32_t kBlobFixed = 65;  // ... and the CRC
constexpr uint32_t kV3Fixed = 53;    // version 3: everything in front of the columns
constexpr uint32_t kV3HashAt = 13;   // ... of which [13, 53) and the columns are hashed
RSX_HD uint64_t tmp_bytes(uint64_t n) { return kTmpFixed + 16 * n; }
RSX_HD uint64_t blob_bytes(uint64_t n) { return kBlobFixed + 16 * n; }
// "envelope too big" (serde.h:539-541): what follows the size field
RSX_HD bool too_big(uint64_t n) { return blob_bytes(n) - 6 > 0xFFFFFFFFull; }
// in tmp: count c in front of column c, the columns, the flags
RSX_HD uint64_t count_at(uint32_t c, uint64_t n) { return 36 + (4 + 4 * n) * c; }
RSX_HD uint64_t column_at(uint32_t c, uint64_t n) { return count_at(c, n) + 4; }
RSX_HD uint64_t flags_at(uint64_t n) { return 48 + 16 * n; }
// int64 field f of tmp: base_offset, max_offset, base_timestamp, max_timestamp
RSX_HD uint32_t scalar_at(uint32_t f) { return 4 + 8 * f; }
RSX_HD int64_t scalar(const rpgpu_segidx_state& s, uint32_t f) {
    return f == 0 ? s.base_offset : (f == 1 ? s.max_offset : (f == 2 ? s.base_timestamp : s.max_timestamp));
}

// crc::crc32c over [p, p + n), one byte at a time
RSX_HD uint32_t crc32c_bytes(const uint8_t* p, uint64_t n) {
    uint32_t c = ~0u;
    for (uint64_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0x82F63B78u & (0u - (c & 1u)));
    }
    return ~c;
}

// serde::to_iobuf(index_state) on one thread; out: blob_bytes(s.entries) bytes
RSX_HD void blob_put(const rpgpu_segidx_state& s, const rpgpu_index_entry* e, uint8_t* out) {
    const uint64_t n = s.entries, L = tmp_bytes(n);
    out[0] = 5, out[1] = 4;
    st<uint32_t>(out + 2, (uint32_t)(blob_bytes(n) - 6));
    st<uint32_t>(out + 6, (uint32_t)L);
    uint8_t* t = out + kTmpAt;
    st<uint32_t>(t, s.bitflags);
    for (uint32_t f = 0; f < 4; f++) st<int64_t>(t + scalar_at(f), scalar(s, f));
    for (uint32_t c = 0; c < 3; c++) st<uint32_t>(t + count_at(c, n), (uint32_t)n);
    for (uint64_t i = 0; i < n; i++) {
        st<uint32_t>(t + column_at(0, n) + 4 * i, e[i].relative_offset);
        st<uint32_t>(t + column_at(1, n) + 4 * i, e[i].relative_time);
        st<uint64_t>(t + column_at(2, n) + 8 * i, e[i].position);
    }
    t[flags_at(n)] = s.monotonic, t[flags_at(n) + 1] = s.with_offset, t[flags_at(n) + 2] = s.non_data_timestamps;
    st<uint32_t>(t + L, crc32c_bytes(t, L));
}

// ------------------------------------------------------------------- XXH64
// A legacy blob hashes 40 + 16 n bytes: a multiple of 8 and at least 40.  So
// only the 32-byte stripe loop, the merge and the 8-byte tail steps exist here;
// xxh_ok states the precondition and every caller checks it.
constexpr uint64_t kXxhP1 = 0x9E3779B185EBCA87ull, kXxhP2 = 0xC2B2AE3D27D4EB4Full, kXxhP3 = 0x165667B19E3779F9ull,
                   kXxhP4 = 0x85EBCA77C2B2AE63ull;
RSX_HD bool xxh_ok(uint64_t len) { return len >= 32 && (len & 7) == 0; }
static_assert(kV3Fixed - kV3HashAt >= 32 && (kV3Fixed - kV3HashAt) % 8 == 0,
              "a legacy blob's hashed length 40 + 16 n takes the stripe loop and 8-byte tail steps only");
RSX_HD uint64_t xxh_rotl(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
RSX_HD uint64_t xxh_round(uint64_t acc, uint64_t in) { return xxh_rotl(acc + in * kXxhP2, 31) * kXxhP1; }
// accumulator a of 4 at seed 0
RSX_HD uint64_t xxh_init(uint32_t a) { return a == 0 ? kXxhP1 + kXxhP2 : (a == 1 ? kXxhP2 : (a == 2 ? 0 : 0 - kXxhP1)); }
// accumulator a over the len / 32 stripes of p
RSX_HD uint64_t xxh_lane(const uint8_t* p, uint64_t len, uint32_t a) {
    uint64_t v = xxh_init(a);
    for (uint64_t s = 0; s + 32 <= len; s += 32) v = xxh_round(v, ld<uint64_t>(p + s + 8 * a));
    return v;
}
// the merge, the 8-byte tail steps behind the last stripe, the avalanche
RSX_HD uint64_t xxh_finish(const uint64_t v[4], const uint8_t* p, uint64_t len) {
    uint64_t h = xxh_rotl(v[0], 1) + xxh_rotl(v[1], 7) + xxh_rotl(v[2], 12) + xxh_rotl(v[3], 18);
    for (uint32_t a = 0; a < 4; a++) h = (h ^ xxh_round(0, v[a])) * kXxhP1 + kXxhP4;
    h += len;
    for (uint64_t at = len & ~(uint64_t)31; at < len; at += 8)
        h = xxh_rotl(h ^ xxh_round(0, ld<uint64_t>(p + at)), 27) * kXxhP1 + kXxhP4;
    h ^= h >> 33, h *= kXxhP2;
    h ^= h >> 29, h *= kXxhP3;
    return h ^ (h >> 32);
}
RSX_HD uint64_t xxh64_mult8(const uint8_t* p, uint64_t len) {  // xxh_ok(len)
    uint64_t v[4];
    for (uint32_t a = 0; a < 4; a++) v[a] = xxh_lane(p, len, a);
    return xxh_finish(v, p, len);
}

// ----------------------------------------------------------------- hydrate
struct View {
    int32_t status, reason;
    uint32_t version, entries;
    bool legacy;
    uint64_t sum_at, sum_len;  // the checksummed bytes: tmp, or the hashed part of a legacy blob
    uint64_t expect;           // the stored CRC32C or XXH64
    uint64_t after;            // bytes behind the CRC (behind the columns of a legacy blob)
    uint32_t n[3];
    uint64_t col[3];           // the columns in the blob
    uint32_t bitflags;
    int64_t scalars[4];
    uint8_t monotonic, with_offset, non_data;
};
RSX_HD bool view_fail(View* v, int32_t status, int32_t reason) {
    v->status = status, v->reason = reason;
    return false;
}
// Everything in front of the checksum comparison, in the reference's order.
// true: the caller checksums [sum_at, sum_at + sum_len) and calls parse_body.
// Reads inside [p, p + bytes).
RSX_HD bool parse_head(const uint8_t* p, uint64_t bytes, View* v) {
    *v = View{};
    if (bytes == 0) return view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_EMPTY_FILE);  // segment_index.cc:215
    v->version = p[0];
    if (v->version < 3) return view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_UNSUPPORTED_VERSION);
    if (v->version == 3) {  // adl<> reads: consume_type throws std::out_of_range (io_iterator_consumer.h:72-92)
        v->legacy = true;
        if (bytes < 5) return view_fail(v, RPGPU_SEGIDX_THROW, RPGPU_SEGIDX_R_V3_SHORT);
        if (bytes - 5 != ld<uint32_t>(p + 1)) return view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_V3_SIZE_MISMATCH);
        if (bytes < kV3Fixed) return view_fail(v, RPGPU_SEGIDX_THROW, RPGPU_SEGIDX_R_V3_SHORT);
        const uint64_t n = ld<uint32_t>(p + 49);
        v->entries = (uint32_t)n;
        if (bytes - kV3Fixed < 16 * n) return view_fail(v, RPGPU_SEGIDX_THROW, RPGPU_SEGIDX_R_V3_SHORT);
        v->expect = ld<uint64_t>(p + 5);
        v->sum_at = kV3HashAt, v->sum_len = kV3Fixed - kV3HashAt + 16 * n;
        v->after = bytes - kV3Fixed - 16 * n;
        v->bitflags = ld<uint32_t>(p + 13);
        for (uint32_t f = 0; f < 4; f++) v->scalars[f] = ld<int64_t>(p + 17 + 8 * f);
        for (uint32_t c = 0; c < 3; c++) v->n[c] = (uint32_t)n;
        v->col[0] = kV3Fixed, v->col[1] = kV3Fixed + 4 * n, v->col[2] = kV3Fixed + 8 * n;
        return true;
    }
    // read_header (serde.h:592-647): three scalars, each checked before it is read
    if (bytes < 6) return view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_HEADER_SHORT);
    uint64_t left = bytes - 6;
    if (left < ld<uint32_t>(p + 2)) return view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_SIZE_BEYOND);
    if (p[1] > 5) return view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_COMPAT_VERSION);
    if (left < 4) return view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_TMP_LEN_SHORT);
    const uint64_t L = ld<uint32_t>(p + 6);
    left -= 4;
    if (L > left) return view_fail(v, RPGPU_SEGIDX_THROW, RPGPU_SEGIDX_R_TMP_BEYOND);  // share clamps, skip throws
    left -= L;
    if (left < 4) return view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_CRC_SHORT);
    v->expect = ld<uint32_t>(p + kTmpAt + L);
    v->sum_at = kTmpAt, v->sum_len = L;
    v->after = left - 4;
    return true;
}
// The comparison and what follows it.  sum: the checksum of the bytes parse_head named.
RSX_HD void parse_body(const uint8_t* p, View* v, uint64_t sum) {
    if (v->legacy) {
        if (sum != v->expect) return (void)view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_V3_CHECKSUM);
        if (v->after) return (void)view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_TRAILING);
        return;
    }
    if (sum != v->expect) return (void)view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_CRC_MISMATCH);
    const uint8_t* t = p + kTmpAt;
    const uint64_t L = v->sum_len;
    uint64_t at = 0;
    if (L - at < 4) return (void)view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_FIELD_SHORT);
    v->bitflags = ld<uint32_t>(t + at), at += 4;
    for (uint32_t f = 0; f < 4; f++) {
        if (L - at < 8) return (void)view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_FIELD_SHORT);
        v->scalars[f] = ld<int64_t>(t + at), at += 8;
    }
    for (uint32_t c = 0; c < 3; c++) {
        if (L - at < 4) return (void)view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_FIELD_SHORT);
        v->n[c] = ld<uint32_t>(t + at), at += 4;
        if (c == 0) v->entries = v->n[0];
        const uint64_t need = (uint64_t)v->n[c] * (c == 2 ? 8 : 4);
        if (L - at < need) return (void)view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_FIELD_SHORT);
        v->col[c] = kTmpAt + at, at += need;
    }
    if (v->version >= 5) {  // monotonic_timestamps_version; version 4 keeps the three at false
        if (L - at < 3) return (void)view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_FIELD_SHORT);
        v->monotonic = t[at] != 0, v->with_offset = t[at + 1] != 0, v->non_data = t[at + 2] != 0;
    }
    if (v->after) return (void)view_fail(v, RPGPU_SEGIDX_REBUILD, RPGPU_SEGIDX_R_TRAILING);
    if (v->n[1] != v->n[0] || v->n[2] != v->n[0])
        return (void)view_fail(v, RPGPU_SEGIDX_COLUMNS_DIFFER, RPGPU_SEGIDX_R_COLUMNS_DIFFER);
}
// the state of an accepted blob; entry_first and entry_cap stay the row's
RSX_HD void view_state(const View& v, rpgpu_segidx_state* s) {
    s->base_offset = v.scalars[0], s->max_offset = v.scalars[1];
    s->base_timestamp = v.scalars[2], s->max_timestamp = v.scalars[3];
    s->bitflags = v.bitflags, s->entries = v.entries;
    s->acc = 0, s->last_batch_max_timestamp = -1;
    s->monotonic = v.monotonic, s->with_offset = v.with_offset, s->non_data_timestamps = v.non_data;
    s->reserved0 = 0, s->reserved1 = 0, s->reserved2 = 0;
}
RSX_HD rpgpu_index_entry view_entry(const uint8_t* p, const View& v, uint64_t i) {
    rpgpu_index_entry x;
    x.relative_offset = ld<uint32_t>(p + v.col[0] + 4 * i);
    x.relative_time = ld<uint32_t>(p + v.col[1] + 4 * i);
    x.position = ld<uint64_t>(p + v.col[2] + 8 * i);
    return x;
}

// -------------------------------------------------------------------- find
// std::lower_bound's loop over one column of the slot, restated
RSX_HD uint32_t lower_bound(const rpgpu_index_entry* e, uint32_t n, bool time, uint32_t v) {
    uint32_t first = 0, len = n;
    while (len > 0) {
        const uint32_t half = len >> 1, mid = first + half;
        if ((time ? e[mid].relative_time : e[mid].relative_offset) < v) {
            first = mid + 1;
            len -= half + 1;
        } else {
            len = half;
        }
    }
    return first;
}
// translate_index_entry (segment_index.cc:32-41)
RSX_HD void found_entry(const rpgpu_segidx_state& s, const rpgpu_index_entry* e, uint32_t i, rpgpu_segidx_found* o) {
    o->status = RPGPU_SEGIDX_FOUND, o->ix = i;
    o->offset = (int64_t)((uint64_t)e[i].relative_offset + (uint64_t)s.base_offset);
    o->timestamp = (int64_t)((uint64_t)offset_time(e[i].relative_time, s.with_offset) + (uint64_t)s.base_timestamp);
    o->filepos = e[i].position;
}
RSX_HD void find(const rpgpu_segidx_state& s, const rpgpu_index_entry* e, uint32_t kind, int64_t key,
                 rpgpu_segidx_found* o) {
    o->status = RPGPU_SEGIDX_NONE, o->ix = 0, o->offset = 0, o->timestamp = 0, o->filepos = 0;
    const uint32_t n = s.entries;
    if (kind == RPGPU_SEGIDX_BY_OFFSET) {
        if (key < s.base_offset || n == 0) return;
        const uint32_t needle = (uint32_t)((uint64_t)key - (uint64_t)s.base_offset);
        uint32_t it = lower_bound(e, n, false, needle);
        if (it == n) it = n - 1;
        for (int64_t i = it; i >= 0; i--)
            if (e[i].relative_offset <= needle) return found_entry(s, e, (uint32_t)i, o);
    } else if (kind == RPGPU_SEGIDX_BY_TIME) {
        if (key < s.base_timestamp || n == 0) return;
        const uint32_t raw = time_index_raw((int64_t)((uint64_t)key - (uint64_t)s.base_timestamp), s.with_offset);
        const uint32_t dist = lower_bound(e, n, true, raw);
        found_entry(s, e, dist > 0 ? dist - 1 : 0, o);
    } else if (kind == RPGPU_SEGIDX_TIME_BEFORE) {
        if (s.base_timestamp > key || n == 0) return;
        const int64_t rel = (int64_t)((uint64_t)key - (uint64_t)s.base_timestamp);
        for (int64_t i = (int64_t)n - 1; i >= 0; i--) {
            const uint32_t ot = offset_time(e[i].relative_time, s.with_offset);
            if ((int64_t)ot < rel) {
                o->status = RPGPU_SEGIDX_FOUND, o->ix = (uint32_t)i;
                o->timestamp = (int64_t)((uint64_t)s.base_timestamp + ot);
                return;
            }
        }
    } else {
        o->status = RPGPU_SEGIDX_BAD_QUERY;
    }
}

}  // namespace rpsx
#endif
