// rpgpu_legacy.h — the legacy (magic 0 / 1) MessageSet walk, its verdicts and
// the v2 record encoder, as host/device functions: the kernels of
// rpgpu_legacy.hip and the host program tests/native/legacy_host.cpp compile
// the same code.
//
// Reference (paths relative to src/v/):
//   kafka_batch_adapter::convert_message_set   kafka/protocol/kafka_batch_adapter.cc:215-274
//   decode_legacy_batch                        kafka/protocol/legacy_message.h
//   iobuf_parser consume_* (out_of_range)      bytes/details/io_iterator_consumer.h:63-83
//   iobuf::share (clamps, never throws)        bytes/iobuf.cc:162-185
//   crc::crc32 (zlib polynomial)               hashing/crc32.h:18-33
//   record_batch_builder::build                storage/record_batch_builder.cc
//
// A set's outcome is its first "event" in message order; within a message the
// order is: header reads (truncation, magic) -> CRC -> key / value reads ->
// codec checks.  An event is a key (message index << 2 | stage), so the
// checksums can run apart from the walk: the walk stops at its first non-CRC
// event, every message it reached is checksummed in parallel, and the set's
// verdict is that of the smallest key.
#ifndef RPGPU_LEGACY_H
#define RPGPU_LEGACY_H

#include <stdint.h>

#include "rpgpu.h"

#ifdef __HIPCC__
#define RPL_HD __host__ __device__ __forceinline__
#else
#define RPL_HD static inline
#endif

namespace rplegacy {

constexpr uint32_t kStagePre = 0;   // before the CRC check: header truncation, magic
constexpr uint32_t kStageCrc = 1;   // the CRC32 comparison
constexpr uint32_t kStagePost = 2;  // after it: key / value reads, codec checks
constexpr uint32_t kNoEvent = 0xffffffffu;
constexpr uint32_t kMaxFraming = 23;  // v2 framing of one record (the legacy framing is >= 26)

// One message the walk reached the CRC check of (48 bytes).
struct Msg {
    uint64_t crc_off;     // arena offset of the CRC range
    uint32_t crc_len;     // share_no_consume(batch_length - 4), clamped to the set
    uint32_t crc_expect;  // the message's crc field
    uint32_t set;         // the set it belongs to
    uint32_t index;       // its index in the set = the record's offset delta
    uint32_t key_off;     // key bytes, relative to the set's start
    int32_t key_len;      // -1: null
    uint32_t val_off;
    int32_t val_len;
    uint32_t rec_off;     // the record's offset in the batch body
    uint32_t rec_len;     // the record's length field (bytes after its own varint)
};
static_assert(sizeof(Msg) == 48, "message table entry");

// What the walk knows of a set without the checksums.
struct Scan {
    uint32_t nmsg;    // messages accepted as records
    uint32_t ntab;    // messages whose CRC is to be checked (table entries)
    uint32_t body;    // bytes of the v2 records body of the accepted messages
    uint32_t key;     // first non-CRC event, or kNoEvent
    int32_t verdict;  // its verdict (RPGPU_V_OK without one)
    uint32_t codec;   // attributes & 7 of the event message (COMPRESSED)
    int64_t ts;       // the last magic-1 timestamp
    uint32_t has_ts;
    uint32_t pad;
};

RPL_HD uint32_t be32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return __builtin_bswap32(v);
}
RPL_HD uint64_t be64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return __builtin_bswap64(v);
}

// zigzag varint (utils/vint.h:133-161)
RPL_HD uint64_t zigzag(int64_t v) { return ((uint64_t)v << 1) ^ (uint64_t)(v >> 63); }
RPL_HD uint32_t vint_size(int64_t v) {
    uint64_t z = zigzag(v);
    uint32_t n = 1;
    while (z >= 0x80) {
        z >>= 7;
        n++;
    }
    return n;
}
RPL_HD uint32_t put_vint(uint8_t* o, int64_t v) {
    uint64_t z = zigzag(v);
    uint32_t n = 0;
    while (z >= 0x80) {
        o[n++] = (uint8_t)(z | 0x80);
        z >>= 7;
    }
    o[n++] = (uint8_t)z;
    return n;
}

// record i of the batch: vint(len) 00 vint(0) vint(i) vint(klen|-1) key
// vint(vlen|-1) value vint(0) (model/record_utils.cc:183-225 as add_raw_kv
// fills it: attributes 0, timestamp delta 0, offset delta i, no headers)
RPL_HD uint32_t record_len(uint32_t i, int32_t klen, int32_t vlen) {
    return 2 + vint_size(i) + vint_size(klen) + (klen > 0 ? (uint32_t)klen : 0u) + vint_size(vlen) +
           (vlen > 0 ? (uint32_t)vlen : 0u) + 1;
}
// the bytes before the key; returns their count
RPL_HD uint32_t put_record_head(uint8_t* o, uint32_t rec_len, uint32_t i, int32_t klen) {
    uint32_t n = put_vint(o, rec_len);
    o[n++] = 0;
    o[n++] = 0;
    n += put_vint(o + n, i);
    n += put_vint(o + n, klen);
    return n;
}

// The 61-byte little-endian on-disk header record_batch_builder::build leaves
// (raft_data, base offset 0, no producer), crc and header_crc zero: they are
// stamped by reset_size_checksum_metadata (storage/parser_utils.cc:122-128).
RPL_HD void put_le(uint8_t* o, uint64_t v, int nb) {
    for (int k = 0; k < nb; k++) o[k] = (uint8_t)(v >> (8 * k));
}
RPL_HD void put_header(uint8_t* o, uint32_t body, uint32_t n, int64_t ts) {
    put_le(o + 0, 0, 4);                                   // header_crc
    put_le(o + 4, (uint64_t)RPGPU_HEADER_SIZE + body, 4);  // size_bytes
    put_le(o + 8, 0, 8);                                   // base_offset
    o[16] = 1;                                             // raft_data
    put_le(o + 17, 0, 4);                                  // crc
    put_le(o + 21, 0, 2);                                  // attrs
    put_le(o + 23, (uint64_t)(int64_t)((int32_t)n - 1), 4);  // last_offset_delta (-1: empty)
    put_le(o + 27, (uint64_t)ts, 8);
    put_le(o + 35, (uint64_t)ts, 8);
    put_le(o + 43, ~0ull, 8);  // producer_id -1
    put_le(o + 51, ~0ull, 2);  // producer_epoch -1
    put_le(o + 53, ~0ull, 4);  // base_sequence -1
    put_le(o + 57, n, 4);
}

// The walk over one set of n bytes at p (arena offset abs).  Fills at most
// table_cap entries of table (may be null: count only).
RPL_HD Scan scan_set(const uint8_t* p, uint32_t n, uint64_t abs, uint32_t set, Msg* table, uint64_t table_cap) {
    Scan s;
    s.nmsg = 0;
    s.ntab = 0;
    s.body = 0;
    s.key = kNoEvent;
    s.verdict = RPGPU_V_OK;
    s.codec = 0;
    s.ts = 0;
    s.has_ts = 0;
    s.pad = 0;
    uint32_t pos = 0, i = 0;
    auto event = [&](uint32_t stage, int32_t verdict) {
        s.key = (i << 2) | stage;
        s.verdict = verdict;
    };
    while (pos < n) {  // parser.bytes_left()
        // offset, batch_length, crc: each consume throws when bytes lack
        if (n - pos < 16) {
            event(kStagePre, RPGPU_V_LEGACY_TRUNC_THROW);
            break;
        }
        const int32_t bl = (int32_t)be32(p + pos + 8);
        const uint32_t crc = be32(p + pos + 12);
        uint32_t q = pos + 16;
        // share_no_consume((size_t)batch_length - 4): batch_length < 4 wraps to a
        // huge size and the share clamps to what is left
        const uint32_t left = n - q;
        const uint32_t crc_len = (bl >= 4 && (uint32_t)(bl - 4) < left) ? (uint32_t)(bl - 4) : left;
        if (n - q < 1) {
            event(kStagePre, RPGPU_V_LEGACY_TRUNC_THROW);
            break;
        }
        const uint32_t magic = p[q++];
        if (magic > 1) {
            event(kStagePre, RPGPU_V_LEGACY_MAGIC);
            break;
        }
        if (n - q < 1) {
            event(kStagePre, RPGPU_V_LEGACY_TRUNC_THROW);
            break;
        }
        const uint32_t attrs = p[q++];
        int64_t ts = 0;
        if (magic == 1) {
            if (n - q < 8) {
                event(kStagePre, RPGPU_V_LEGACY_TRUNC_THROW);
                break;
            }
            ts = (int64_t)be64(p + q);
            q += 8;
        }
        // the CRC check happens here: from now on the message is in the table
        Msg m;
        m.crc_off = abs + pos + 16;
        m.crc_len = crc_len;
        m.crc_expect = crc;
        m.set = set;
        m.index = i;
        m.key_off = 0;
        m.key_len = -1;
        m.val_off = 0;
        m.val_len = -1;
        m.rec_off = s.body;
        m.rec_len = 0;
        s.ntab = i + 1;
        int32_t post = RPGPU_V_OK;
        // key, then value: int32 size, -1 null, else share(size) + skip
        for (int f = 0; f < 2 && post == RPGPU_V_OK; f++) {
            if (n - q < 4) {
                post = RPGPU_V_LEGACY_TRUNC_THROW;
                break;
            }
            const int32_t sz = (int32_t)be32(p + q);
            q += 4;
            if (sz != -1) {
                if (sz < 0 || (uint32_t)sz > n - q) {
                    post = RPGPU_V_LEGACY_TRUNC_THROW;
                    break;
                }
                if (f == 0) {
                    m.key_off = q;
                    m.key_len = sz;
                } else {
                    m.val_off = q;
                    m.val_len = sz;
                }
                q += (uint32_t)sz;
            }
        }
        if (post == RPGPU_V_OK) {
            // convert_message_set: timestamp, compression(), the codec checks
            const uint32_t codec = attrs & 7u;
            if (codec >= 4) post = RPGPU_V_LEGACY_BAD_CODEC_THROW;
            else if (codec != 0) {
                if (magic == 0 && codec == 3) post = RPGPU_V_LEGACY_LZ4_MAGIC0;
                else if (m.val_len < 0) post = RPGPU_V_LEGACY_NULL_COMPRESSED;
                else {
                    post = RPGPU_V_LEGACY_COMPRESSED;
                    s.codec = codec;
                }
            }
        }
        if (post == RPGPU_V_OK) {
            m.rec_len = record_len(i, m.key_len, m.val_len);
            s.body += vint_size(m.rec_len) + m.rec_len;
            s.nmsg = i + 1;
            if (magic == 1) {
                s.ts = ts;
                s.has_ts = 1;
            }
        }
        if (table && i < table_cap) table[i] = m;
        if (post != RPGPU_V_OK) {
            event(kStagePost, post);
            break;
        }
        pos = q;  // the next message starts where the value ended
        i++;
    }
    return s;
}

// the set's verdict from the smallest event key
RPL_HD int32_t verdict_of(const Scan& s, uint32_t key) {
    if (key == kNoEvent) return RPGPU_V_OK;
    if ((key & 3u) == kStageCrc) return RPGPU_V_LEGACY_CRC_MISMATCH;
    return s.verdict;
}

// one record, serially (the kernels copy long keys and values by the wave)
RPL_HD void put_record(uint8_t* o, const Msg& m, const uint8_t* set_base) {
    uint32_t n = put_record_head(o, m.rec_len, m.index, m.key_len);
    for (int32_t k = 0; k < m.key_len; k++) o[n + k] = set_base[m.key_off + k];
    n += m.key_len > 0 ? (uint32_t)m.key_len : 0u;
    n += put_vint(o + n, m.val_len);
    for (int32_t k = 0; k < m.val_len; k++) o[n + k] = set_base[m.val_off + k];
    n += m.val_len > 0 ? (uint32_t)m.val_len : 0u;
    o[n] = 0;
}

// crc::crc32 (hashing/crc32.h:18-33): zlib's crc32, polynomial 0xEDB88320,
// a nibble at a time (the serial host path; the kernels use the LDS tables)
RPL_HD uint32_t crc32_extend(uint32_t crc, const uint8_t* p, uint64_t n) {
    uint32_t t[16];
    for (uint32_t v = 0; v < 16; v++) {
        uint32_t c = v;
        for (int k = 0; k < 4; k++) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : (c >> 1);
        t[v] = c;
    }
    crc = ~crc;
    for (uint64_t i = 0; i < n; i++) {
        crc ^= p[i];
        crc = (crc >> 4) ^ t[crc & 15u];
        crc = (crc >> 4) ^ t[crc & 15u];
    }
    return ~crc;
}

}  // namespace rplegacy
#endif
