// rpgpu_txfilter.h — storage::internal::tx_reducer as host/device functions: the
// kernels of rpgpu_txfilter.hip and the host program tests/native/txfilter_host.cpp
// compile the same code (include/rpgpu.h, "aborted transactions ahead of
// compaction"; DESIGN.md §3 has the argument).
//
// Reference (paths relative to src/v/):
//   tx_reducer                          storage/compaction_reducers.cc:322-428, .h:150-256
//   parse_control_batch                 cluster/rm_stm.cc:258-279
//   filter_intersecting                 cluster/rm_stm.cc:1948-1962
//   consume_type (short iobuf throws)   bytes/details/io_iterator_consumer.h:88-97
//
// The serial state machine -- a min-heap of ranges on `first`, a map pid ->
// range, one batch after another -- is evaluated in closed form.  With
// L_i = base_offset + last_offset_delta and M_i = max_{k <= i} L_k:
//   * range r is consumed at c(r) = min{i : M_i >= r.first} (consume_pos, a
//     binary search on the non-decreasing M; MaxOp is M's scan operator);
//   * data batch i of pid p is discarded iff some range r of p has
//     a < c(r) <= i, a being p's last abort marker in front of i (or -1).
// The abort markers of one pid cut the scope into intervals; a range and a data
// batch meet iff they fall into the same interval (interval_of, a binary search
// over the pid's markers) and the range comes first, so each interval keeps
// one number, the smallest c(r) that fell into it (a min: order-free).
#ifndef RPGPU_TXFILTER_H
#define RPGPU_TXFILTER_H

#include <stdint.h>

#include "rpgpu.h"

#ifdef __HIPCC__
#define RTX_HD __host__ __device__ __forceinline__
#else
#define RTX_HD static inline
#endif

namespace rptx {

constexpr int16_t kAttrTx = 0x10, kAttrControl = 0x20;  // model/record.h attrs bits
constexpr uint8_t kRaftData = 1, kTxPrepare = 9, kTxFence = 10;
constexpr uint32_t kNone = 0xffffffffu;

// what a batch is to the later passes
enum Kind : uint8_t { kKindNone = 0, kKindData = 1, kKindAbort = 2 };

struct Class {
    int32_t stop;     // enum rpgpu_tx_status; RPGPU_TX_OK: the batch does not stop its scope
    uint8_t flag;     // RPGPU_TX_DELEGATED / MARKER / PREPARE (a data batch: DELEGATED until decided)
    uint8_t kind;     // enum Kind
    int16_t epoch;    // producer identity of a kKindData / kKindAbort batch
    int64_t pid;
};

template <class T>
RTX_HD T ld(const uint8_t* p) {
    T v;
    __builtin_memcpy(&v, p, sizeof(T));
    return v;
}

// producer_id and producer_epoch: header bytes [43, 51) and [51, 53) of both layouts
RTX_HD void read_pid(const uint8_t* hdr, uint8_t format, int64_t* pid, int16_t* epoch) {
    uint64_t p = ld<uint64_t>(hdr + 43);
    uint16_t e = ld<uint16_t>(hdr + 51);
    if (format == RPGPU_FMT_KAFKA_WIRE) {
        p = __builtin_bswap64(p);
        e = __builtin_bswap16(e);
    }
    *pid = (int64_t)p;
    *epoch = (int16_t)e;
}

// parse_control_batch's two read_int16 over the key: RPGPU_TX_OK and *type, or the status
RTX_HD int32_t control_type(const uint8_t* key, int32_t key_len, int32_t* type) {
    if (key_len < 2) return RPGPU_TX_KEY_SHORT_THROW;  // a null key is an empty iobuf
    if (key[0] != 0 || key[1] != 0) return RPGPU_TX_ASSERT;  // "unknown control record version"
    if (key_len < 4) return RPGPU_TX_KEY_SHORT_THROW;
    *type = (int16_t)(uint16_t)(((uint32_t)key[2] << 8) | key[3]);
    return RPGPU_TX_OK;
}

// tx_reducer::operator() on one batch, all of it that does not depend on the
// batches in front.  batch: the batch's bytes (desc.offset), its header first.
RTX_HD Class classify(const rpgpu_batch_result& r, const rpgpu_batch_desc& d, const uint8_t* batch,
                      const rpgpu_record_index* index, uint64_t index_cap, bool non_transactional) {
    Class c;
    c.stop = RPGPU_TX_OK, c.flag = RPGPU_TX_DELEGATED, c.kind = kKindNone, c.epoch = 0, c.pid = 0;
    if (r.verdict != RPGPU_V_OK) {
        c.stop = RPGPU_TX_BAD_BATCH;
        return c;
    }
    if (non_transactional) return c;
    const bool is_tx = (r.attrs & kAttrTx) != 0, is_control = (r.attrs & kAttrControl) != 0;
    const bool is_data = r.type == kRaftData;
    if (is_tx && is_control) {
        if (!is_data || r.record_count != 1) {
            c.stop = RPGPU_TX_ASSERT;
            return c;
        }
        if (r.index_count < 1 || r.index_first >= index_cap) {
            c.stop = RPGPU_TX_NOT_INDEXED;
            return c;
        }
        const rpgpu_record_index e = index[r.index_first];
        const int32_t len = e.key_len < 0 ? 0 : e.key_len;
        // the key lies inside the batch (an index entry of the validator's always does)
        if ((uint64_t)e.key_off + (uint32_t)(len < 4 ? len : 4) > d.length) {
            c.stop = RPGPU_TX_NOT_INDEXED;
            return c;
        }
        int32_t type = -1;
        c.stop = control_type(batch + e.key_off, len, &type);
        if (c.stop != RPGPU_TX_OK) return c;
        if (type == 0 || type == 1) c.flag = RPGPU_TX_MARKER;  // tx_abort, tx_commit
        if (type == 0) {
            c.kind = kKindAbort;
            read_pid(batch, d.format, &c.pid, &c.epoch);
        }
    } else if (is_tx && is_data) {
        c.kind = kKindData;
        read_pid(batch, d.format, &c.pid, &c.epoch);
    } else if (!is_tx && is_control && !is_data) {
        if (r.type != kTxPrepare && r.type != kTxFence) {
            c.stop = RPGPU_TX_ASSERT;
            return c;
        }
        if (r.type == kTxPrepare) c.flag = RPGPU_TX_PREPARE;
    }
    return c;
}

RTX_HD int64_t last_offset(const rpgpu_batch_result& r) {
    return (int64_t)((uint64_t)r.base_offset + (uint64_t)(int64_t)r.last_offset_delta);  // wrapping, as model::offset
}

// M's scan: the running maximum of last_offset(); closed under composition, identity INT64_MIN
struct MaxOp {
    int64_t v;
};
RTX_HD MaxOp max_identity() { return MaxOp{INT64_MIN}; }
RTX_HD MaxOp max_combine(MaxOp a, MaxOp b) { return MaxOp{a.v > b.v ? a.v : b.v}; }

// does the range take part in the scope (the heap's initial contents)
RTX_HD bool takes_part(const rpgpu_tx_range& r, const rpgpu_tx_scope& s) {
    return !(s.flags & RPGPU_TX_FILTER_RANGES) || (r.last >= s.from && r.first <= s.to);
}

// c(r): the first of the m processed batches with M[i] >= first; m: never consumed
RTX_HD uint32_t consume_pos(const int64_t* M, uint32_t m, int64_t first) {
    uint32_t lo = 0, hi = m;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (M[mid] >= first) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// the abort markers of one pid: ascending batch numbers sorted[lo, hi).  The
// last one below x, as an index into sorted, or kNone (x lies in the pid's
// first interval).  A range consumed at x sits in front of batch x, so a marker
// at x itself erases it: the same "below" serves ranges and data batches.
RTX_HD uint32_t interval_of(const uint32_t* sorted, uint32_t lo, uint32_t hi, uint32_t x) {
    const uint32_t lo0 = lo;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (sorted[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo == lo0 ? kNone : lo - 1;
}

// data batch i is discarded iff the smallest consume position of its interval is at or in front of it
RTX_HD bool aborted(uint32_t interval_min, uint32_t i) { return interval_min <= i; }

// producer table hash; restated by tests/tx_compaction.py (mix64 / pid_hash): change both
RTX_HD uint64_t mix64(uint64_t h) {  // splitmix64 finaliser
    h ^= h >> 30;
    h *= 0xbf58476d1ce4e5b9ull;
    h ^= h >> 27;
    h *= 0x94d049bb133111ebull;
    h ^= h >> 31;
    return h;
}
RTX_HD uint64_t pid_hash(uint32_t scope, int64_t pid, int16_t epoch) {
    return mix64(mix64((uint64_t)pid ^ 0x9e3779b97f4a7c15ull) ^ ((uint64_t)scope << 16) ^ (uint16_t)epoch);
}

}  // namespace rptx
#endif
