// rpgpu_dfor.h — the tiered-storage offset index as host/device functions: the
// kernels of rpgpu_rsindex.hip and the host program tests/native/rsindex_host.cpp
// compile the same code.
//
// Reference (paths relative to src/v/):
//   remote_segment_index_builder          cloud_storage/remote_segment_index.cc:307-349
//   offset_index::add / find / to_iobuf   cloud_storage/remote_segment_index.cc:37-305
//   delta_xor, delta_delta                utils/delta_for.h:29-119
//   deltafor_encoder::add / pack          utils/delta_for.h:276-284, 515-764
//   deltafor_decoder::read / unpack       utils/delta_for.h:799-809
//   serde envelope, vector, iobuf         serde/serde.h:515-565
//
// A row is 16 values.  Its bytes are one byte nbits, then the values' low
// bits section by section: 32 bits of each value (if nbits >= 32), 16 bits (if
// what is left >= 16), 8 bits (if what is left >= 8), each section 16
// little-endian fields, value-major; then the remaining r = 1..7 bits of each
// value as one little-endian bit string of 2r bytes, value i at bit i * r.
// nbits == 64 is 16 little-endian uint64.  A row takes 1 + 2 * nbits bytes.
//
// The primitives (width, elem_put, rem_byte, elem_get, field_offset,
// blob_parse) are what the kernels call, one value per lane; the serial
// functions below them (row_put, row_get, Index, Builder, blob_put, find) are
// the same index on one thread, which the host program runs.
#ifndef RPGPU_DFOR_H
#define RPGPU_DFOR_H

#include <stdint.h>

#include "rpgpu.h"

#ifdef __HIPCC__
#define RDF_HD __host__ __device__ __forceinline__
#else
#define RDF_HD static inline
#endif

namespace rpdf {

constexpr uint32_t kRow = 16;         // details::FOR_buffer_depth
constexpr uint32_t kStreams = 3;      // rp, Kafka, file
constexpr uint32_t kHeaderEnd = 466;  // envelope, eight int64, three write buffers
constexpr uint32_t kMinBlob = 478;    // ... and three empty streams
constexpr uint32_t kFields = 8 + kStreams * kRow;  // the int64 fields in front of the streams

template <class T>
RDF_HD T ld(const uint8_t* p) {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}
template <class T>
RDF_HD void st(uint8_t* p, T v) {
    __builtin_memcpy(p, &v, sizeof(T));
}

// ------------------------------------------------------------------ the row
// std::bit_width of the OR of a row's deltas
RDF_HD uint32_t width(uint64_t agg) { return agg ? 64u - (uint32_t)__builtin_clzll(agg) : 0u; }
RDF_HD uint32_t row_bytes(uint32_t nbits) { return 1 + 2 * nbits; }
// the bits below the 32 / 16 / 8-bit sections, and where their bit string starts in the row's body
RDF_HD uint32_t rem_bits(uint32_t nbits) { return nbits == 64 ? 0u : (nbits & 7u); }
RDF_HD uint32_t rem_offset(uint32_t nbits) { return 2 * (nbits - rem_bits(nbits)); }

RDF_HD uint64_t delta_xor(uint64_t v, uint64_t prev) { return v ^ prev; }
RDF_HD uint64_t delta_delta(uint64_t v, uint64_t prev, uint64_t step) { return v - prev - step; }
// the two vasserts of delta_delta::encode (delta_for.h:86-96)
RDF_HD bool delta_ok(int64_t v, int64_t prev, int64_t step) {
    return v >= prev && (int64_t)((uint64_t)v - (uint64_t)prev) >= step;
}

// value e's pieces of the 64 / 32 / 16 / 8-bit sections into the row's body b
// (the bytes behind nbits); returns what is left for the remainder bit string
RDF_HD uint64_t elem_put(uint8_t* b, uint32_t nbits, uint32_t e, uint64_t v) {
    if (nbits == 64) {
        st<uint64_t>(b + 8 * e, v);
        return 0;
    }
    uint32_t left = nbits;
    if (left >= 32) {
        st<uint32_t>(b + 4 * e, (uint32_t)v);
        b += 64, v >>= 32, left -= 32;
    }
    if (left >= 16) {
        st<uint16_t>(b + 2 * e, (uint16_t)v);
        b += 32, v >>= 16, left -= 16;
    }
    if (left >= 8) {
        b[e] = (uint8_t)v;
        v >>= 8;
    }
    return v;
}

// byte j of the bit string of 16 r-bit fields (r in 1..7, j < 2r); get(i) is
// value i's remainder.  Always eight calls of get, values past 15 clamped, so
// a wave can back it with a cross-lane read.
template <class Get>
RDF_HD uint32_t rem_byte(uint32_t r, uint32_t j, Get get) {
    const uint32_t mask = (1u << r) - 1, i0 = 8 * j / r;
    uint32_t out = 0;
    for (uint32_t k = 0; k < 8; k++) {
        const uint32_t i = i0 + k;
        const uint32_t v = (uint32_t)get(i < kRow ? i : kRow - 1) & mask;
        const int sh = (int)(i * r) - (int)(8 * j);
        if (i < kRow && sh < 8) out |= sh >= 0 ? v << sh : v >> -sh;
    }
    return out & 255u;
}

// value e of the row whose body is b
RDF_HD uint64_t elem_get(const uint8_t* b, uint32_t nbits, uint32_t e) {
    if (nbits == 64) return ld<uint64_t>(b + 8 * e);
    uint64_t v = 0;
    uint32_t left = nbits, shift = 0;
    if (left >= 32) {
        v |= ld<uint32_t>(b + 4 * e);
        b += 64, shift += 32, left -= 32;
    }
    if (left >= 16) {
        v |= (uint64_t)ld<uint16_t>(b + 2 * e) << shift;
        b += 32, shift += 16, left -= 16;
    }
    if (left >= 8) {
        v |= (uint64_t)b[e] << shift;
        b += 16, shift += 8, left -= 8;
    }
    if (left) {
        const uint32_t bit = e * left, at = bit >> 3, sh = bit & 7u;
        uint32_t w = b[at];
        if (sh + left > 8) w |= (uint32_t)b[at + 1] << 8;
        v |= (uint64_t)((w >> sh) & ((1u << left) - 1)) << shift;
    }
    return v;
}

// ---------------------------------------------------------------- the blob
// int64 field f of the serialized header: 0 min_file_pos_step, 1 num_elements,
// 2 base_rp, 3 last_rp, 4 base_kaf, 5 last_kaf, 6 base_file, 7 last_file, then
// the three write buffers, each behind its u32 count
RDF_HD uint32_t field_offset(uint32_t f) {
    return f < 8 ? 6 + 8 * f : 70 + 132 * ((f - 8) / kRow) + 4 + 8 * ((f - 8) % kRow);
}
RDF_HD uint32_t count_offset(uint32_t s) { return 70 + 132 * s; }
// the sample a write-buffer slot holds when `samples` were added (the buffers
// are never cleared: the last sample whose index is j mod 16); false: still zero
RDF_HD bool slot_sample(uint64_t samples, uint32_t j, uint64_t* idx) {
    if (samples <= j) return false;
    *idx = ((samples - 1 - j) / kRow) * kRow + j;
    return true;
}

struct View {
    int64_t step;
    uint64_t elements;
    int64_t base[kStreams], last[kStreams];
    const uint8_t* wb[kStreams];      // 16 unaligned int64 each
    const uint8_t* stream[kStreams];
    uint32_t len[kStreams];
};
// from_iobuf (remote_segment_index.cc:260-287) over exactly the layout of
// to_iobuf; false: RPGPU_RSINDEX_BAD_BLOB.  Reads inside [blob, blob + bytes).
RDF_HD bool blob_parse(const uint8_t* blob, uint64_t bytes, View* v) {
    if (bytes < kMinBlob || blob[0] != 1 || blob[1] != 1) return false;
    if ((uint64_t)ld<uint32_t>(blob + 2) + 6 != bytes) return false;
    v->step = ld<int64_t>(blob + field_offset(0));
    v->elements = ld<uint64_t>(blob + field_offset(1));
    for (uint32_t s = 0; s < kStreams; s++) {
        v->base[s] = ld<int64_t>(blob + field_offset(2 + 2 * s));
        v->last[s] = ld<int64_t>(blob + field_offset(3 + 2 * s));
        if (ld<uint32_t>(blob + count_offset(s)) != kRow) return false;
        v->wb[s] = blob + count_offset(s) + 4;
    }
    uint64_t at = kHeaderEnd;
    for (uint32_t s = 0; s < kStreams; s++) {
        if (at + 4 > bytes) return false;
        v->len[s] = ld<uint32_t>(blob + at);
        at += 4;
        if (at + v->len[s] > bytes) return false;
        v->stream[s] = blob + at;
        at += v->len[s];
    }
    return at == bytes;
}

// -------------------------------------------------- the index on one thread
RDF_HD uint32_t row_put(uint8_t* out, const uint64_t* buf, uint32_t nbits) {
    out[0] = (uint8_t)nbits;
    uint64_t rem[kRow];
    for (uint32_t e = 0; e < kRow; e++) rem[e] = elem_put(out + 1, nbits, e, buf[e]);
    const uint32_t r = rem_bits(nbits);
    for (uint32_t j = 0; j < 2 * r; j++)
        out[1 + rem_offset(nbits) + j] = (uint8_t)rem_byte(r, j, [&](uint32_t i) { return rem[i]; });
    return row_bytes(nbits);
}

// a row chain of `rows` rows inside stream[0, len)
RDF_HD bool chain_ok(const uint8_t* stream, uint32_t len, uint64_t rows) {
    uint64_t p = 0;
    for (uint64_t r = 0; r < rows; r++) {
        if (p >= len) return false;
        const uint32_t nbits = stream[p];
        if (nbits > 64 || p + row_bytes(nbits) > len) return false;
        p += row_bytes(nbits);
    }
    return true;
}

struct Encoder {  // deltafor_encoder<int64_t>
    uint8_t* data;
    uint64_t len;
    int64_t last;
    uint32_t rows;
};

struct Index {  // offset_index
    int64_t wb[kStreams][kRow];
    uint64_t pos;
    int64_t base[kStreams];
    int64_t step;
    Encoder enc[kStreams];
    int32_t status;
};
// streams: room for (samples / 16) * 129 bytes each
RDF_HD void index_init(Index* x, int64_t base_rp, int64_t base_kaf, int64_t step, uint8_t* rp, uint8_t* kaf,
                       uint8_t* file) {
    for (uint32_t s = 0; s < kStreams; s++)
        for (uint32_t e = 0; e < kRow; e++) x->wb[s][e] = 0;
    x->pos = 0;
    x->base[0] = base_rp, x->base[1] = base_kaf, x->base[2] = 0;
    x->step = step;
    uint8_t* d[kStreams] = {rp, kaf, file};
    for (uint32_t s = 0; s < kStreams; s++) x->enc[s] = Encoder{d[s], 0, x->base[s], 0};
    x->status = RPGPU_RSINDEX_OK;
}
// offset_index::add (:37-63)
RDF_HD void index_add(Index* x, int64_t rp, int64_t kaf, int64_t fpos) {
    const uint32_t slot = (uint32_t)(x->pos++ & (kRow - 1));
    x->wb[0][slot] = rp, x->wb[1][slot] = kaf, x->wb[2][slot] = fpos;
    if ((x->pos & (kRow - 1)) != 0) return;
    for (uint32_t s = 0; s < kStreams; s++) {
        Encoder& en = x->enc[s];
        uint64_t buf[kRow], agg = 0;
        int64_t p = en.last;
        for (uint32_t e = 0; e < kRow; e++) {
            const int64_t v = x->wb[s][e];
            if (s == 2 && !delta_ok(v, p, x->step)) x->status = RPGPU_RSINDEX_DELTA_ASSERT;
            buf[e] = s == 2 ? delta_delta((uint64_t)v, (uint64_t)p, (uint64_t)x->step) : delta_xor((uint64_t)v, (uint64_t)p);
            agg |= buf[e];
            p = v;
        }
        en.len += row_put(en.data + en.len, buf, width(agg));
        en.last = x->wb[s][kRow - 1];
        en.rows++;
    }
}

RDF_HD bool is_config(int type) { return type == 2 || type == 19; }  // raft_configuration, archival_metadata
RDF_HD bool window_full(uint64_t window, uint64_t sampling_step) { return window >= sampling_step; }

struct Builder {  // remote_segment_index_builder + the parser's running position
    int64_t delta;
    uint64_t window, pos, sampling_step;
    uint32_t config;
};
RDF_HD void builder_init(Builder* b, int64_t initial_delta, uint64_t sampling_step) {
    b->delta = initial_delta, b->window = 0, b->pos = 0, b->sampling_step = sampling_step, b->config = 0;
}
// consume_batch_start (:319-337)
RDF_HD void builder_step(Builder* b, Index* x, int type, int32_t last_offset_delta, int32_t size_bytes,
                         int64_t base_offset) {
    if (is_config(type)) {
        b->delta = (int64_t)((uint64_t)b->delta + (uint64_t)((int64_t)last_offset_delta + 1));
        b->config++;
    } else if (window_full(b->window, b->sampling_step)) {
        index_add(x, base_offset, (int64_t)((uint64_t)base_offset - (uint64_t)b->delta), (int64_t)b->pos);
        b->window = 0;
    }
    b->window += (uint64_t)size_bytes;
    b->pos += (uint64_t)size_bytes;
}

RDF_HD uint64_t blob_bytes(const Index& x) { return kMinBlob + x.enc[0].len + x.enc[1].len + x.enc[2].len; }
// to_iobuf (:237-258)
RDF_HD uint64_t blob_put(const Index& x, uint8_t* out) {
    const uint64_t total = blob_bytes(x);
    out[0] = 1, out[1] = 1;
    st<uint32_t>(out + 2, (uint32_t)(total - 6));
    st<int64_t>(out + field_offset(0), x.step);
    st<uint64_t>(out + field_offset(1), x.pos);
    for (uint32_t s = 0; s < kStreams; s++) {
        st<int64_t>(out + field_offset(2 + 2 * s), x.base[s]);
        st<int64_t>(out + field_offset(3 + 2 * s), x.enc[s].last);
        st<uint32_t>(out + count_offset(s), kRow);
        for (uint32_t e = 0; e < kRow; e++) st<int64_t>(out + field_offset(8 + kRow * s + e), x.wb[s][e]);
    }
    uint64_t at = kHeaderEnd;
    for (uint32_t s = 0; s < kStreams; s++) {
        st<uint32_t>(out + at, (uint32_t)x.enc[s].len);
        at += 4;
        for (uint64_t k = 0; k < x.enc[s].len; k++) out[at + k] = x.enc[s].data[k];
        at += x.enc[s].len;
    }
    return at;
}

// one row of a deserialized stream (deltafor_decoder::read), prev carried
RDF_HD uint64_t row_get(const uint8_t* row, bool file, int64_t step, int64_t* prev, int64_t* vals) {
    const uint32_t nbits = row[0];
    for (uint32_t e = 0; e < kRow; e++) {
        const uint64_t d = elem_get(row + 1, nbits, e);
        *prev = file ? (int64_t)(d + (uint64_t)*prev + (uint64_t)step) : (int64_t)(d ^ (uint64_t)*prev);
        vals[e] = *prev;
    }
    return row_bytes(nbits);
}
// _fetch_ix (remote_segment_index.h:122-135); ix < 16 * rows
RDF_HD int64_t fetch_ix(const View& v, uint32_t s, uint64_t ix) {
    int64_t prev = v.base[s], vals[kRow];
    uint64_t p = 0;
    for (uint64_t r = 0;; r++) {
        p += row_get(v.stream[s] + p, s == 2, v.step, &prev, vals);
        if (r == ix / kRow) return vals[ix % kRow];
    }
}
// find_rp_offset / find_kaf_offset (:105-174) with maybe_find_offset (:65-103)
// and _find_under (:289-305)
RDF_HD void find(const uint8_t* blob, uint64_t bytes, bool by_rp, int64_t upper_bound, rpgpu_rsindex_found* out) {
    *out = rpgpu_rsindex_found{};
    out->status = RPGPU_RSINDEX_BAD_BLOB;
    View v;
    if (!blob_parse(blob, bytes, &v)) return;
    const uint64_t rows = v.elements / kRow;
    for (uint32_t s = 0; s < kStreams; s++)
        if (!chain_ok(v.stream[s], v.len[s], rows)) return;
    const uint32_t q = by_rp ? 0 : 1;
    bool have = false;
    uint64_t ix = 0, p = 0;
    int64_t value = 0, prev = v.base[q], vals[kRow];
    for (uint64_t r = 0, stop = 0; r < rows && !stop; r++) {
        p += row_get(v.stream[q] + p, false, 0, &prev, vals);
        for (uint32_t e = 0; e < kRow; e++) {
            if (vals[e] >= upper_bound) {
                stop = 1;
                break;
            }
            have = true, ix = r * kRow + e, value = vals[e];
        }
    }
    if (!have || ix == rows * kRow - 1) {
        const uint32_t end = (uint32_t)(v.elements & (kRow - 1));
        bool hit = false;
        uint32_t slot = 0;
        for (uint32_t i = 0; i < end; i++) {
            if (ld<int64_t>(v.wb[q] + 8 * i) < upper_bound) hit = true, slot = i;
            else break;
        }
        if (hit) {
            out->status = RPGPU_RSINDEX_FOUND, out->from_write_buffer = 1, out->ix = slot;
            out->rp_offset = ld<int64_t>(v.wb[0] + 8 * slot);
            out->kaf_offset = ld<int64_t>(v.wb[1] + 8 * slot);
            out->file_pos = ld<int64_t>(v.wb[2] + 8 * slot);
            return;
        }
        if (!have) {
            out->status = RPGPU_RSINDEX_NONE;
            return;
        }
    }
    out->status = RPGPU_RSINDEX_FOUND, out->ix = ix;
    out->rp_offset = by_rp ? value : fetch_ix(v, 0, ix);
    out->kaf_offset = by_rp ? fetch_ix(v, 1, ix) : value;
    out->file_pos = fetch_ix(v, 2, ix);
}

}  // namespace rpdf
#endif
