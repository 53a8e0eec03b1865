// rpgpu_pp.h — the REST proxy's fetch reply as host/device functions: the
// kernels of rpgpu_pp.hip and the host program tests/native/pp_host.cpp
// compile the same code.
//
// Reference (paths relative to src/v/):
//   rjson_serialize_impl<kafka::fetch_response>  pandaproxy/json/requests/fetch.h:94-154
//   rjson_serialize_impl<model::record>          pandaproxy/json/requests/fetch.h:46-82
//   rjson_serialize_impl<iobuf> (base64 path)    pandaproxy/json/iobuf.h:70-89
//   iobuf_to_base64 (libbase64, flags 0)         utils/base64.cc:74-112
//   model::validate_kafka_topic_name             model/validation.cc:20-38
//   the expected string                          pandaproxy/json/requests/test/fetch.cc:77,95-96
//
// An object is
//   {"topic":"<name>","key":K,"value":V,"partition":<int32>,"offset":<int64>}
// and owns the byte in front of it: '[' in front of the response's first
// object, ',' in front of every other one.  A response is its objects and a
// closing ']' ("[]" without objects), so an object's place follows from sums
// of (1 + object size) alone.
#ifndef RPGPU_PP_H
#define RPGPU_PP_H

#include <stdint.h>

#include "rpgpu.h"

#ifdef __HIPCC__
#define RPP_HD __host__ __device__ __forceinline__
#else
#define RPP_HD static inline
#endif

namespace rppp {

constexpr uint32_t kNone = 0xffffffffu;
constexpr uint64_t kNoEvent = ~0ull;
// {"topic":"  ","key":  ,"value":  ,"partition":  ,"offset":  }
constexpr uint32_t kSkeleton = 10 + 8 + 9 + 13 + 10 + 1;

// ---------------------------------------------------------------- decimals
// |v| without the overflow of -INT64_MIN
RPP_HD uint64_t dec_mag(int64_t v) { return v < 0 ? 0 - (uint64_t)v : (uint64_t)v; }
RPP_HD uint32_t dec_len(int64_t v) {
    const auto m = dec_mag(v);
    uint32_t n = 1;
    uint64_t p = 10;
    while (n < 20 && m >= p) {  // 10^19 fits, 20 digits is the most
        p *= 10;
        n++;
    }
    return n + (v < 0 ? 1u : 0u);
}
// writes v in decimal at p (dec_len(v) bytes), returns the byte behind it
RPP_HD uint8_t* put_dec(uint8_t* p, int64_t v) {
    const uint32_t n = dec_len(v);
    auto m = dec_mag(v);
    if (v < 0) p[0] = '-';
    uint32_t k = n;
    while (m > 0xffffffffull) {  // 64-bit steps only while they are needed
        p[--k] = (uint8_t)('0' + (uint32_t)(m % 10));
        m /= 10;
    }
    uint32_t w = (uint32_t)m;
    do {
        p[--k] = (uint8_t)('0' + w % 10);
        w /= 10;
    } while (w);
    return p + n;
}

// ------------------------------------------------------------------ base64
RPP_HD uint64_t b64_len(uint32_t n) { return 4ull * ((n + 2ull) / 3); }
// four 6-bit values, one per byte -> their characters (the standard alphabet
// by arithmetic: A-Z, a-z +6, 0-9 -75, '+' -15, '/' +3; the comparisons are
// the carries into bit 7 of v + (128 - bound), which never leave the byte)
RPP_HD uint32_t b64_chars(uint32_t x) {
    const uint32_t ge26 = ((x + 0x66666666u) >> 7) & 0x01010101u;
    const uint32_t ge52 = ((x + 0x4c4c4c4cu) >> 7) & 0x01010101u;
    const uint32_t ge62 = ((x + 0x42424242u) >> 7) & 0x01010101u;
    const uint32_t ge63 = ((x + 0x41414141u) >> 7) & 0x01010101u;
    return x + 0x41414141u + ge26 * 6u - ge52 * 75u - ge62 * 15u + ge63 * 3u;
}
// three bytes -> four characters, the first in the low byte
RPP_HD uint32_t b64_group(uint32_t b0, uint32_t b1, uint32_t b2) {
    const uint32_t n = (b0 << 16) | (b1 << 8) | b2;
    return b64_chars((n >> 18) | (((n >> 12) & 63u) << 8) | (((n >> 6) & 63u) << 16) | ((n & 63u) << 24));
}
RPP_HD void b64_put_group(uint8_t* dst, const uint8_t* src) {
    const uint32_t c = b64_group(src[0], src[1], src[2]);
    __builtin_memcpy(dst, &c, 4);
}
// twelve bytes -> sixteen characters, one 16-byte store
RPP_HD void b64_put_piece(uint8_t* dst, const uint8_t* src) {
    uint32_t w[3], c[4];
    __builtin_memcpy(w, src, 12);
    c[0] = b64_group(w[0] & 255u, (w[0] >> 8) & 255u, (w[0] >> 16) & 255u);
    c[1] = b64_group(w[0] >> 24, w[1] & 255u, (w[1] >> 8) & 255u);
    c[2] = b64_group((w[1] >> 16) & 255u, w[1] >> 24, w[2] & 255u);
    c[3] = b64_group((w[2] >> 8) & 255u, (w[2] >> 16) & 255u, w[2] >> 24);
    __builtin_memcpy(dst, c, 16);
}
// the last one or two bytes: two or three characters, then '=' up to four
RPP_HD void b64_put_tail(uint8_t* dst, const uint8_t* src, uint32_t rem) {
    const uint32_t pad = 3 - rem;
    uint32_t c = b64_group(src[0], rem == 2 ? src[1] : 0u, 0u);
    c = pad == 2 ? (c & 0x0000ffffu) | 0x3d3d0000u : (c & 0x00ffffffu) | 0x3d000000u;
    __builtin_memcpy(dst, &c, 4);
}
// a whole field by one lane: b64_len(len) bytes at dst, nothing else
RPP_HD void b64_encode_lane(uint8_t* dst, const uint8_t* src, uint32_t len) {
    uint32_t k = 0;
    for (; k + 12 <= len; k += 12, dst += 16) b64_put_piece(dst, src + k);
    for (; k + 3 <= len; k += 3, dst += 4) b64_put_group(dst, src + k);
    if (k < len) b64_put_tail(dst, src + k, len - k);
}
// lane l's share of a field the 64 lanes of a wavefront encode together.
// Whole groups in front bring a 4-byte aligned destination to a 16-byte
// boundary (the head), the interior leaves as 16-character pieces, a piece
// per lane and step, the groups behind them and the padded tail go to one
// lane each.  Every store lies inside the field's b64_len(len) bytes.
RPP_HD void b64_encode_wave(uint8_t* dst, const uint8_t* src, uint32_t len, uint32_t l) {
    const uint32_t groups = len / 3, rem = len - 3 * groups;
    const uint32_t mis = (uint32_t)((uintptr_t)dst & 15u);
    uint32_t head = (mis & 3u) ? 0u : ((16u - mis) & 15u) >> 2;
    if (head > groups) head = groups;
    const uint32_t pieces = (groups - head) >> 2, tail = (groups - head) & 3u;
    if (l < head) b64_put_group(dst + 4 * l, src + 3 * l);
    for (uint32_t i = l; i < pieces; i += 64)
        b64_put_piece(dst + 4 * head + 16ull * i, src + 3 * head + 12ull * i);
    const uint32_t g0 = head + 4 * pieces;  // the first group behind the pieces
    if (l < tail) b64_put_group(dst + 4ull * (g0 + l), src + 3ull * (g0 + l));
    if (rem && l == 63) b64_put_tail(dst + 4ull * groups, src + 3ull * groups, rem);
}

// -------------------------------------------------------------------- sizes
// null for an absent or empty field, else the quoted base64
RPP_HD uint64_t field_size(int32_t len) { return len <= 0 ? 4 : 2 + b64_len((uint32_t)len); }
// what of an object's size the range decides
RPP_HD uint32_t object_fixed(uint32_t topic_len, int32_t partition) {
    return kSkeleton + topic_len + dec_len(partition);
}
// and what the record's index entry decides
RPP_HD uint64_t object_var(const rpgpu_record_index& e) {
    return field_size(e.key_len) + field_size(e.val_len) + dec_len(e.offset);
}
// a field of at most lane_max bytes is encoded by the record's lane
RPP_HD bool on_lane(int32_t len, uint32_t lane_max) { return len <= 0 || (uint32_t)len <= lane_max; }
// the byte in front of an object that starts off_in_range bytes into a range
// that starts range_off bytes into the response
RPP_HD uint8_t lead_byte(uint64_t range_off, uint64_t off_in_range) {
    return (range_off | off_in_range) == 0 ? '[' : ',';
}

// ------------------------------------------------------------------ objects
RPP_HD uint8_t* put_lit(uint8_t* p, const char* s, uint32_t n) {
    for (uint32_t k = 0; k < n; k++) p[k] = (uint8_t)s[k];
    return p + n;
}
// a key or value at p: null, or the quotes and, for a field on the lane's
// path, the characters between them.  Returns the byte behind the field.
RPP_HD uint8_t* put_field(uint8_t* p, const uint8_t* src, int32_t len, uint32_t lane_max) {
    if (len <= 0) return put_lit(p, "null", 4);
    const uint64_t n = b64_len((uint32_t)len);
    p[0] = '"';
    p[1 + n] = '"';
    if (on_lane(len, lane_max)) b64_encode_lane(p + 1, src, (uint32_t)len);
    return p + 2 + n;
}
// where the characters of an object's long key and value go (null: the
// field is on the lane's path); obj: the object's lead byte
struct Fields {
    uint8_t *kdst, *vdst;
};
RPP_HD Fields locate_fields(uint8_t* obj, uint32_t topic_len, const rpgpu_record_index& e, uint32_t lane_max) {
    uint8_t* k = obj + 1 + 10 + topic_len + 8;
    uint8_t* v = k + field_size(e.key_len) + 9;
    Fields f;
    f.kdst = on_lane(e.key_len, lane_max) ? nullptr : k + 1;
    f.vdst = on_lane(e.val_len, lane_max) ? nullptr : v + 1;
    return f;
}
// the lead byte and one object at p; batch: the batch's first byte (key_off
// and val_off count from there).  Returns the byte behind the object.
RPP_HD uint8_t* put_object(uint8_t* p, uint8_t lead, const uint8_t* topic, uint32_t topic_len, int32_t partition,
                           const rpgpu_record_index& e, const uint8_t* batch, uint32_t lane_max) {
    *p++ = lead;
    p = put_lit(p, "{\"topic\":\"", 10);
    for (uint32_t k = 0; k < topic_len; k++) p[k] = topic[k];
    p = put_lit(p + topic_len, "\",\"key\":", 8);
    p = put_field(p, batch + e.key_off, e.key_len, lane_max);
    p = put_lit(p, ",\"value\":", 9);
    p = put_field(p, batch + e.val_off, e.val_len, lane_max);
    p = put_lit(p, ",\"partition\":", 13);
    p = put_dec(p, partition);
    p = put_lit(p, ",\"offset\":", 10);
    p = put_dec(p, e.offset);
    *p++ = '}';
    return p;
}

// ------------------------------------------------------------------ verdicts
// model::validate_kafka_topic_name: 1..249 bytes of [A-Za-z0-9._-], not "." or ".."
RPP_HD bool topic_ok(const uint8_t* t, uint32_t len) {
    if (len == 0 || len > 249) return false;
    if (t[0] == '.' && (len == 1 || (len == 2 && t[1] == '.'))) return false;
    for (uint32_t k = 0; k < len; k++) {
        const uint8_t c = t[k];
        const bool ok = (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '.' ||
                        c == '_' || c == '-';
        if (!ok) return false;
    }
    return true;
}
// a range's own defect: the topic first, then the bounds
RPP_HD int32_t range_status(const rpgpu_pp_range& g, const uint8_t* topics, uint32_t topics_len, uint32_t n) {
    if ((uint64_t)g.topic_off + g.topic_len > topics_len || !topic_ok(topics + g.topic_off, g.topic_len))
        return RPGPU_PP_BAD_TOPIC;
    if ((uint64_t)g.first + g.count > n) return RPGPU_PP_BAD_RANGE;
    return RPGPU_PP_OK;
}
// what a batch does to its response (fetch.h:114-131); *records: the objects it renders
RPP_HD int32_t batch_status(const rpgpu_batch_result& r, uint32_t* records) {
    *records = 0;
    if (r.verdict != RPGPU_V_OK) return RPGPU_PP_BAD_BATCH;
    if (r.attrs & 0x20) return RPGPU_PP_OK;  // control: skipped, whatever its codec
    if (r.codec != 0) return RPGPU_PP_COMPRESSED;
    if (r.record_count < 0 || (uint32_t)r.record_count != r.index_count) return RPGPU_PP_NOT_INDEXED;
    *records = r.index_count;
    return RPGPU_PP_OK;
}
// a response's first offender is its smallest key: the range's position in
// the response, then 0 for the range itself or 1 + the batch's position in it
RPP_HD uint64_t event_key(uint32_t range_pos, uint32_t batch_pos_plus1) {
    return ((uint64_t)range_pos << 32) | batch_pos_plus1;
}
// bytes of a response with `body` bytes of objects and lead bytes
RPP_HD uint64_t response_len(uint64_t body) { return body ? body + 1 : 2; }
RPP_HD uint64_t slot_size(uint64_t out_len) { return (out_len + 15) & ~(uint64_t)15; }

}  // namespace rppp
#endif
