/*
 * rpgpu.h — C ABI of the MI355X record-batch validation / decode engine.
 *
 * This is the drop-in boundary for Redpanda's record-batch hot path
 * (SURVEY.md §8b).  Every entry point is `extern "C"`, takes plain pointers
 * and sizes, never throws and reports errors through an int32 status.
 * The reference interfaces each entry point replaces are cited beside it
 * (paths relative to the reference tree's src/v/).
 *
 * Layouts used throughout
 *   - Kafka v2 wire batch, big-endian 61-byte header
 *       (kafka/protocol/kafka_batch_adapter.h:26-38, kafka/protocol/wire.h:645-681)
 *   - Redpanda on-disk batch, little-endian 61-byte header
 *       (storage/parser.cc:40-80, storage/segment_appender_utils.cc:28-51)
 *
 * An "arena" is one device (or pinned host) buffer holding many batches back
 * to back plus an array of rpgpu_batch_desc, one per batch.  The data buffer
 * must stay readable for RPGPU_ARENA_TAIL_PAD bytes past the last batch: the
 * kernels read headers as whole 64-byte windows and mask what lies beyond.
 */
#ifndef RPGPU_H
#define RPGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPGPU_ABI_VERSION 6
#define RPGPU_ARENA_TAIL_PAD 64
#define RPGPU_HEADER_SIZE 61 /* model/record.h:527-540 */

/* ---- status codes (return values) ------------------------------------- */
enum rpgpu_status {
    RPGPU_OK = 0,
    RPGPU_PENDING = 1,
    RPGPU_EINVAL = -1,
    RPGPU_ENOMEM = -2,
    RPGPU_EDEVICE = -3, /* HIP runtime error; see rpgpu_last_error() */
    RPGPU_ECAPACITY = -4, /* an output buffer is too small */
};

/* ---- batch formats and operations ------------------------------------- */
enum rpgpu_format {
    RPGPU_FMT_KAFKA_WIRE = 0, /* produce path: kafka_batch_adapter::adapt */
    RPGPU_FMT_RP_DISK = 1,    /* storage path: continuous_batch_parser     */
};

enum rpgpu_op {
    RPGPU_OP_CRC = 1u << 0,    /* Kafka CRC32C over the batch body        */
    RPGPU_OP_HDRCRC = 1u << 1, /* internal_header_only_crc                */
    RPGPU_OP_PARSE = 1u << 2,  /* record field walk (uncompressed batches)*/
    RPGPU_OP_INDEX = 1u << 3,  /* emit per-record index entries           */
    RPGPU_OP_DECOMP = 1u << 4, /* decompress compressed bodies            */
    /* on-disk batches only: compute crc and header_crc instead of checking
     * them (reset_size_checksum_metadata, storage/parser_utils.cc:122-128);
     * used for the rewritten batches of rpgpu_decomp_run_device */
    RPGPU_OP_RECRC = 1u << 5,
    /* LogAppendTime topics: rpgpu_set_max_timestamp_device re-stamps the
     * batch (model::record_batch::set_max_timestamp, model/record.h:651-661,
     * as produce_topic_partition calls it, kafka/server/handlers/produce.cc:
     * 278-281); ignored by the validation kernels */
    RPGPU_OP_APPEND_TIME = 1u << 6,
};
#define RPGPU_OPS_PRODUCE (RPGPU_OP_CRC | RPGPU_OP_HDRCRC | RPGPU_OP_PARSE | RPGPU_OP_INDEX)

/* ---- per-batch verdicts ------------------------------------------------
 * Produce path, built from kafka_batch_adapter.cc:136-198,
 * model/record.h:283-300,668-691, model/record_utils.cc:93-176 and
 * kafka/server/handlers/produce.cc:440-489.  SURVEY.md §8a verdict table.
 */
enum rpgpu_verdict {
    RPGPU_V_OK = 0,
    RPGPU_V_NULL_RECORDS = 1,      /* records field null (produce.cc:440-449)      */
    RPGPU_V_TOO_SMALL = 2,         /* < 12 bytes: adapter flags indeterminate     */
    RPGPU_V_HDR_TRUNC_THROW = 3,   /* out_of_range escapes read_header            */
    RPGPU_V_BAD_MAGIC = 4,         /* magic != 2 -> !v2_format                     */
    RPGPU_V_CRC_MISMATCH = 5,      /* !valid_crc -> corrupt_message                */
    RPGPU_V_BAD_CODEC_THROW = 6,   /* attrs codec 5..7: runtime_error escapes      */
    RPGPU_V_BODY_TRUNC_THROW = 7,  /* parser.share(size-61) skip throws            */
    RPGPU_V_REC_ATTR_EOF = 8,      /* record attrs consume_type at end of body    */
    RPGPU_V_REC_TRAILING = 9,      /* "Record iteration stopped with N bytes ..."  */
    RPGPU_V_REC_HCOUNT_NEG = 10,   /* headers.reserve(negative) -> length_error    */
    RPGPU_V_REC_UNDEFINED = 11,    /* reference UB / allocation-dependent */
    /* storage path (parser_errc, storage/parser_errc.h:18-25) */
    RPGPU_V_HDR_CRC_MISMATCH = 20, /* parser_errc::header_only_crc_missmatch       */
    RPGPU_V_STREAM_SHORT = 21,     /* parser_errc::input_stream_not_enough_bytes   */
    RPGPU_V_FALLOCATED_ZERO = 22,  /* parser_errc::fallocated_file_read_zero_bytes_for_header */
    /* decompression (compression/compression.cc:35-55 and the codec wrappers) */
    RPGPU_V_DECOMP_ERROR = 30,     /* codec library error -> runtime_error         */
    /* 31 is reserved (RPGPU_V_DECOMP_BAD_ALLOC in ABI v1, never produced): the
     * reference's zstd bad_alloc branch is dead code (stream_zstd.cc:29-36
     * compares the size_t return with the error enum), so a frame window the
     * 8 MiB workspace cannot hold is RPGPU_V_DECOMP_ERROR like every other
     * zstd error. */
    RPGPU_V_LZ4_TRAILING = 32,     /* unconsumed input after LZ4 frame end        */
    RPGPU_V_DECOMP_UNSUPPORTED = 33,/* reserved: every codec 1..4 is decoded     */
    RPGPU_V_DECOMP_OVERFLOW = 34,  /* decompressed size exceeds the output slot, or
                                      its bound exceeds opts.max_decoded_batch */
    /* multi-batch record sets (kafka/protocol/batch_reader.cc:50-58) */
    RPGPU_V_SET_HEADER_SHORT = 36, /* < 61 bytes left for the next batch header:
                                      corrupt_message "Invalid kafka header parsing" */
    /* stream parser (storage/parser.cc:223-299, parser_errc) */
    RPGPU_V_END_OF_STREAM = 23,    /* parser_errc::end_of_stream (benign)         */
    RPGPU_V_READ_OFFSET_REGRESSION = 24, /* skipping_consumer throws: batch base
                                      offset below the expected next one
                                      (storage/log_reader.cc:30-38)             */
    /* segment index (storage/index_state.cc:48-54) */
    RPGPU_V_INDEX_OFFSET_BELOW_BASE = 37, /* vassert: batch base offset below the segment's */
    /* remote segment reader (cloud_storage/remote_segment.cc:808-815) */
    RPGPU_V_REMOTE_DELTA_ASSERT = 38, /* vassert in rp_to_kafka: a batch's Redpanda
                                      offset below the offset-translation delta */
    /* 39, 41 and 42 appear only in rpgpu_segidx_tracked.status
     * (rpgpu_segidx_track_device), never in an rpgpu_batch_result */
    RPGPU_V_INDEX_NON_DATA_ASSERT = 39, /* vassert in maybe_index (index_state.cc:61): a
                                     user-data batch while non_data_timestamps is set
                                     and the index does not hold exactly one entry
                                     (only from a hostile hydrated state)         */
    RPGPU_V_SKIPPED = 40,          /* not decompressed: no RPGPU_OP_DECOMP, not
                                      validated OK, or not compressed        */
    RPGPU_V_INDEX_NO_ROOM = 41,    /* the next entry would pass the state's entry_cap */
    RPGPU_V_INDEX_BAD_STATE = 42,  /* the state's slot or the segment's batches lie
                                     outside the arrays                          */
    /* legacy MessageSets, produce versions below 3 (rpgpu_legacy_*; kafka/protocol/
     * kafka_batch_adapter.cc:215-301, kafka/protocol/legacy_message.h) */
    RPGPU_V_LEGACY_MAGIC = 50,           /* magic not 0 or 1: legacy_error            */
    RPGPU_V_LEGACY_CRC_MISMATCH = 51,    /* CRC32 mismatch: legacy_error              */
    RPGPU_V_LEGACY_LZ4_MAGIC0 = 52,      /* magic 0 with lz4: legacy_error            */
    RPGPU_V_LEGACY_NULL_COMPRESSED = 53, /* compressed message, null value: legacy_error */
    RPGPU_V_LEGACY_TRUNC_THROW = 54,     /* out_of_range escapes the message decoder  */
    RPGPU_V_LEGACY_BAD_CODEC_THROW = 55, /* attributes & 7 in 4..7: runtime_error     */
    RPGPU_V_LEGACY_COMPRESSED = 56,      /* a compressed wrapper message that passed its
                                            own checks: the set is NOT converted, the
                                            caller routes it to the reference path   */
};

/* Kafka error codes of the produce path (kafka/protocol/errors.h:22,29,47,227). */
#define RPGPU_KAFKA_ERR_UNKNOWN_SERVER_ERROR (-1)
#define RPGPU_KAFKA_ERR_NONE 0
#define RPGPU_KAFKA_ERR_CORRUPT_MESSAGE 2
#define RPGPU_KAFKA_ERR_MESSAGE_TOO_LARGE 10
#define RPGPU_KAFKA_ERR_INVALID_RECORD 87

/* rpgpu_batch_desc.flags */
enum rpgpu_desc_flag {
    /* the partition's records field was null on the wire (decoder::
     * read_nullable_iobuf, kafka/protocol/wire.h:152-159): no bytes are read,
     * the verdict is RPGPU_V_NULL_RECORDS (produce.cc:440-449) */
    RPGPU_DESC_NULL_RECORDS = 1u << 0,
};

/* ---- descriptors and results ------------------------------------------ */
typedef struct rpgpu_batch_desc {
    uint64_t offset;    /* byte offset of the batch in the arena data buffer */
    uint32_t length;    /* bytes of record data handed over for this batch   */
    uint32_t partition; /* topic-partition id (sharding key)                 */
    uint8_t format;     /* enum rpgpu_format                                 */
    uint8_t ops;        /* enum rpgpu_op bitmask                             */
    uint16_t flags;     /* enum rpgpu_desc_flag bitmask                      */
    uint32_t reserved;  /* reserved, 0                                       */
} rpgpu_batch_desc;     /* 24 bytes */

typedef struct rpgpu_batch_result {
    int32_t verdict;           /* enum rpgpu_verdict                            */
    uint32_t crc;              /* computed Kafka CRC32C (record_utils.cc:82-87) */
    uint32_t crc_expected;     /* header crc field                               */
    uint32_t header_crc;       /* internal_header_only_crc (record_utils.cc:34-55) */
    int32_t size_bytes;        /* RP size_bytes = batch_length + 12             */
    int32_t record_count;
    int64_t base_offset;
    int32_t last_offset_delta;
    int16_t attrs;
    uint8_t codec;             /* attrs & 7                                     */
    uint8_t type;              /* record_batch_type (raft_data=1 on produce)   */
    int64_t first_timestamp;
    int64_t max_timestamp;
    uint32_t index_first;      /* first entry of this batch in the record index */
    uint32_t index_count;      /* records fully parsed                          */
} rpgpu_batch_result;          /* 64 bytes */

typedef struct rpgpu_record_index {
    int64_t offset;    /* base_offset + (int32)offset_delta                   */
    int64_t timestamp; /* first_timestamp + timestamp_delta                   */
    uint32_t key_off;  /* byte offset of the key within the batch             */
    int32_t key_len;   /* (int32) decoded key length; <= 0: no key bytes      */
    uint32_t val_off;
    int32_t val_len;
} rpgpu_record_index;  /* 32 bytes */

/* Little-endian record_batch_header image as the reference hashes it
 * (model/record_utils.cc:34-55).  Packed: 61 bytes, same as disk. */
#pragma pack(push, 1)
typedef struct rpgpu_rp_header {
    uint32_t header_crc;
    int32_t size_bytes;
    int64_t base_offset;
    int8_t type;
    int32_t crc;
    int16_t attrs;
    int32_t last_offset_delta;
    int64_t first_timestamp;
    int64_t max_timestamp;
    int64_t producer_id;
    int16_t producer_epoch;
    int32_t base_sequence;
    int32_t record_count;
} rpgpu_rp_header;
#pragma pack(pop)

/* rpgpu_opts.flags */
/* The record walk overlaps the checksums (the default since ABI 4): arenas of
 * at least 16,384 batches are checksummed in rpgpu_opts.walk_chunks chunks and
 * each chunk's records are walked on a second stream beside the next chunk's
 * checksums (C2 4.33 vs 4.76 ms per 1M batches).  Batches of more than 64
 * records are walked by a wavefront each after the chunks, so a chunk's walk
 * is never a long serial chain (C5 435 vs 431 ms without the overlap, 491
 * before the wave walk).  RPGPU_OPT_WALK_OVERLAP states the default;
 * RPGPU_OPT_NO_WALK_OVERLAP checksums the whole arena, then walks it. */
#define RPGPU_OPT_WALK_OVERLAP 1u
#define RPGPU_OPT_NO_WALK_OVERLAP 2u
/* RPGPU_OPT_ZSTD_SPLIT / RPGPU_OPT_ZSTD_FUSED (ABI 4): the split zstd decoder
 * for lane-sized frames, measured slower than the one-lane decoder and removed
 * in ABI 5; the flags are accepted and ignored (every lane-sized zstd frame
 * takes the one-lane decoder, whose sequences are write-combined since ABI 5). */
#define RPGPU_OPT_ZSTD_SPLIT 4u
#define RPGPU_OPT_ZSTD_FUSED 8u
/* RPGPU_OPT_ZSTD_WAVE_ONLY: zstd frames above the lane decoders' slots all go
 * to the one-wave-per-frame decoder.  By default a large frame that is one
 * complete frame without checksum or dictionary, of known content size that
 * the decoder's ring holds whole, is decoded block-parallel (rpgpu_zblk.h:
 * every block's literals and sequences at once, then the frame's repeat
 * offsets resolved and its sequences executed by one wave).  Same verdicts
 * and bytes either way. */
#define RPGPU_OPT_ZSTD_WAVE_ONLY 16u

typedef struct rpgpu_opts {
    uint32_t flags;        /* RPGPU_OPT_* */
    uint32_t max_batches;  /* per-submission capacity hint (0 = default)   */
    uint64_t max_arena;    /* per-submission arena bytes hint (0 = default) */
    /* decompression: ceiling on one batch's output slot (61-byte header +
     * the decoded-size bound read off its frame + slack).  A batch above it
     * gets RPGPU_V_DECOMP_OVERFLOW and no slot, so one hostile frame (e.g. a
     * 1 MiB body of RLE blocks bounding 32 GB) cannot inflate the shared
     * output plan.  0 = RPGPU_DEFAULT_MAX_DECODED_BATCH.  Not a reference
     * limit: there the outcome depends on the broker's free memory. */
    uint64_t max_decoded_batch;
    /* decompression: ceiling on the zstd / gzip decoder lanes, each with a
     * workspace (zstd ~19 KB, after the output slots, one per zstd batch up
     * to the ceiling; gzip 2 KB, in the scratch: rpgpu_decomp_scratch_bytes_ctx).
     * 0 = 131072 zstd / 32768 gzip lanes (the C4 tuning); a smaller value
     * (minimum 256) bounds the memory: the batches still decode, each lane
     * taking more of them. */
    uint32_t decomp_ws_lanes;
    /* the walk overlap: the arena checksummed in k chunks, each chunk's walk
     * beside the next chunk's checksums (0 = 16; at most 256; 1 = one
     * checksum launch, then the walk). */
    uint16_t walk_chunks;
    /* validate_kernel workgroups per CU of the persistent grid (0 = 8,
     * capped by occupancy; at most 32). */
    uint16_t blocks_per_cu;
} rpgpu_opts;
#define RPGPU_DEFAULT_MAX_DECODED_BATCH (64ull << 20)

typedef struct rpgpu_ctx rpgpu_ctx;
typedef uint64_t rpgpu_ticket;

/* ---- context ----------------------------------------------------------- */
/* One context per (Seastar shard x GPU); not thread-safe per context, which
 * matches shard-per-core ownership. */
rpgpu_ctx* rpgpu_open(int device, const rpgpu_opts* opts);
void rpgpu_close(rpgpu_ctx* ctx);
const char* rpgpu_last_error(const rpgpu_ctx* ctx);
int32_t rpgpu_abi_version(void);
/* CU count of the device and the persistent grid (workgroups) used. */
int32_t rpgpu_device_info(const rpgpu_ctx* ctx, int32_t* cu_count, int32_t* grid);

/* ---- pinned host arenas ------------------------------------------------ */
void* rpgpu_arena_alloc(rpgpu_ctx* ctx, size_t bytes);
void rpgpu_arena_free(rpgpu_ctx* ctx, void* p);

/* ---- batch validation (produce path / storage path) ---------------------
 * Replaces, per batch:
 *   kafka::kafka_batch_adapter::adapt        kafka/protocol/kafka_batch_adapter.cc:136-198
 *   model::record_batch::for_each_record     model/record.h:668-691
 *   model::crc_record_batch                  model/record_utils.cc:82-91
 *   model::internal_header_only_crc          model/record_utils.cc:34-55
 * and for RPGPU_FMT_RP_DISK batches the per-batch checks of
 *   storage::continuous_batch_parser          storage/parser.cc:155-216
 *   storage log_replayer checksumming_consumer storage/log_replayer.cc:26-92
 *
 * Host-memory submission: copies descriptors + data to the device, runs the
 * kernels and copies results back, asynchronously on the context's stream.
 * `index_cap` is the capacity of out_index in entries; entries are laid out
 * per batch in descriptor order (index_first of result i).
 */
int32_t rpgpu_submit(rpgpu_ctx* ctx, const rpgpu_batch_desc* descs, uint32_t n,
                     const void* data, size_t data_len,
                     rpgpu_batch_result* out_results,
                     rpgpu_record_index* out_index, uint64_t index_cap,
                     uint64_t* out_index_used, rpgpu_ticket* ticket);
/* 0 = done, 1 = still running, <0 = error. Never blocks. */
int32_t rpgpu_poll(rpgpu_ctx* ctx, rpgpu_ticket ticket);
/* Blocks until the ticket completes. */
int32_t rpgpu_wait(rpgpu_ctx* ctx, rpgpu_ticket ticket);
/* Blocks until every *_device call issued on the context's own stream
 * (hip_stream == NULL) has completed: the C caller's join point for device
 * calls when it does not drive HIP streams itself.  A reactor thread must not
 * call it (use rpgpu_submit + rpgpu_eventfd there). */
int32_t rpgpu_sync(rpgpu_ctx* ctx);
/* A non-blocking eventfd (EFD_NONBLOCK | EFD_CLOEXEC) owned by the context:
 * it becomes readable whenever a stage of a submission completes, so a
 * Seastar reactor awaits it with a readable() future on the fd (the
 * ssx::thread_worker pattern, ssx/thread_worker.h:97-174) instead of
 * blocking in rpgpu_wait; on readiness it reads the counter and calls
 * rpgpu_poll.  -1 if the context has none. */
int rpgpu_eventfd(rpgpu_ctx* ctx);

/* ---- produce-handler glue ---------------------------------------------------
 * The per-partition error code produce_handler would answer for a batch with
 * this validation result (kafka/server/handlers/produce.cc:440-489, and the
 * batch_max_bytes check of produce_topic_partition, produce.cc:317-324;
 * batch_max_bytes 0 = no limit).  Verdicts whose reference behaviour is an
 * exception escaping the request decoder (HDR_TRUNC_THROW, BAD_CODEC_THROW,
 * BODY_TRUNC_THROW) map to RPGPU_KAFKA_ERR_UNKNOWN_SERVER_ERROR; TOO_SMALL
 * and BAD_MAGIC, whose reference flags are uninitialised (kafka_batch_adapter.h:65-66),
 * map to RPGPU_KAFKA_ERR_INVALID_RECORD.  Pure host function. */
int32_t rpgpu_kafka_error_code(const rpgpu_batch_result* r, uint32_t batch_max_bytes);
/* The same over a device result array: d_codes[i] (int32) for d_results[i]. */
int32_t rpgpu_kafka_error_codes_device(rpgpu_ctx* ctx, const rpgpu_batch_result* d_results, uint32_t n,
                                       uint32_t batch_max_bytes, int32_t* d_codes, void* hip_stream);

/* Device-resident entry point: every pointer is device memory, the work is
 * enqueued on `hip_stream` (a hipStream_t; NULL = the context stream, a blocking
 * stream ordered after the legacy default stream) and the
 * call returns without synchronising.  `d_scratch` must hold
 * rpgpu_validate_scratch_bytes(n) bytes.  *d_index_used receives the total
 * number of index entries reserved. */
size_t rpgpu_validate_scratch_bytes(uint32_t n);
int32_t rpgpu_validate_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs,
                              uint32_t n, const uint8_t* d_data,
                              rpgpu_batch_result* d_results,
                              rpgpu_record_index* d_index, uint64_t index_cap,
                              uint64_t* d_index_used, void* d_scratch,
                              void* hip_stream);

/* The two halves of rpgpu_validate_device, for callers that reuse a plan or
 * time the validation kernel on its own:
 *   plan: per-batch index capacity + exclusive scan into d_scratch, total
 *         into *d_index_used;
 *   run:  the fused validate / parse / index kernel (needs the plan). */
int32_t rpgpu_plan_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs, uint32_t n,
                          const uint8_t* d_data, uint64_t* d_index_used, void* d_scratch,
                          void* hip_stream);
int32_t rpgpu_run_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs, uint32_t n,
                         const uint8_t* d_data, rpgpu_batch_result* d_results,
                         rpgpu_record_index* d_index, uint64_t index_cap,
                         const void* d_scratch, void* hip_stream);

/* ---- append-time re-stamp (produce path) ---------------------------------
 * model::record_batch::set_max_timestamp(ts_type, ts) (model/record.h:651-661)
 * for every batch of a validated arena (d_results of rpgpu_validate_device /
 * rpgpu_run_device over the same descriptors) whose descriptor has
 * RPGPU_OP_APPEND_TIME and whose verdict is RPGPU_V_OK -- what
 * produce_topic_partition does for a LogAppendTime topic with ts =
 * model::timestamp::now() (kafka/server/handlers/produce.cc:278-281):
 *   - timestamp type (attrs bit 3) already ts_type and max_timestamp == ts:
 *     nothing changes (record.h:652-656);
 *   - otherwise attrs bit 3 := ts_type, max_timestamp := ts, crc :=
 *     crc_record_batch, header_crc := internal_header_only_crc: the batch's
 *     bytes are rewritten in place (attrs, max_timestamp, crc; on-disk batches
 *     also header_crc) and its result row takes the new attrs, max_timestamp,
 *     crc, crc_expected and header_crc (the verdict stays OK).
 * ts_type: 0 = create_time, 1 = append_time (model/timestamp.h).  The new crc
 * is derived from the validated one without re-reading the body (CRC32C is
 * affine: only the 22 bytes [21, 43) change).  d_changed (optional, one
 * uint32 the caller zeroes) counts the batches that changed. */
int32_t rpgpu_set_max_timestamp_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs, uint32_t n,
                                       uint8_t* d_data, rpgpu_batch_result* d_results, int32_t ts_type,
                                       int64_t ts, uint32_t* d_changed, void* hip_stream);

/* ---- generic CRC32C over many byte ranges (device) ----------------------
 * crc_out[i] = crc32c::Extend(seed[i] (or 0), data + off[i], len[i]) —
 * the semantics of crc::crc32c::extend (hashing/crc32c.h:21-43). */
int32_t rpgpu_crc32c_ranges_device(rpgpu_ctx* ctx, const uint8_t* d_data,
                                   const uint64_t* d_off, const uint32_t* d_len,
                                   const uint32_t* d_seed, uint32_t n,
                                   uint32_t* d_crc_out, void* hip_stream);

/* ---- synchronous scalar mirrors (run on the GPU, host pointers) ---------
 *   crc::crc32c::extend                 hashing/crc32c.h:21-43
 *   model::internal_header_only_crc     model/record_utils.cc:34-55
 *   model::crc_record_batch             model/record_utils.cc:82-87
 * Status return (RPGPU_OK or < 0); the value goes to *out. */
int32_t rpgpu_crc32c_extend(rpgpu_ctx* ctx, uint32_t crc, const void* p, size_t n, uint32_t* out);
int32_t rpgpu_internal_header_only_crc(rpgpu_ctx* ctx, const rpgpu_rp_header* h, uint32_t* out);
int32_t rpgpu_crc_record_batch(rpgpu_ctx* ctx, const rpgpu_rp_header* h,
                               const void* body, size_t n, int32_t* out);
/*   model::record_batch::set_max_timestamp  model/record.h:651-661
 * on a header image and its records body: unchanged (RPGPU_OK, nothing
 * written) when the timestamp type and max_timestamp already match, else
 * attrs bit 3, max_timestamp, crc and header_crc updated in *h. */
int32_t rpgpu_set_max_timestamp(rpgpu_ctx* ctx, rpgpu_rp_header* h, const void* body, size_t n,
                                int32_t ts_type, int64_t ts);

/* ---- decompression (storage read path) ---------------------------------
 * Replaces, per compressed batch,
 *   compression::compressor::uncompress            compression/compression.cc:35-55
 *     lz4_frame_compressor::uncompress             compression/internal/lz4_frame_compressor.cc:160-278
 *     stream_zstd::do_uncompress                   compression/stream_zstd.cc:198-223
 *     snappy_java_compressor::uncompress           compression/internal/snappy_java_compressor.cc:76-110
 *     gzip_compressor::uncompress                  compression/internal/gzip_compressor.cc:177-229
 *   storage::internal::maybe_decompress_batch_sync storage/parser_utils.cc:52-68,122-128
 * and walks / indexes the records of the decompressed batch
 * (model/record.h:668-691).  Every codec is decoded for one contiguous
 * (single-fragment) body; see DESIGN.md §4 for the fragmented-iobuf case.
 *
 * A batch is decompressed when its descriptor has RPGPU_OP_DECOMP, its
 * validation verdict (d_results of rpgpu_run_device / rpgpu_validate_device
 * over the same arena) is RPGPU_V_OK and its codec is not none; every other
 * batch reports RPGPU_V_SKIPPED.  For each decompressed batch the output
 * buffer receives the rewritten on-disk batch (little-endian 61-byte header +
 * body) at out_offset: codec bits removed, size_bytes = 61 + out_len,
 * crc = crc_record_batch over the decompressed body, header_crc =
 * internal_header_only_crc.  A truncated frame yields the partial output with
 * RPGPU_V_OK, as the reference does. */
typedef struct rpgpu_decomp_result {
    int32_t verdict;     /* OK, DECOMP_ERROR, LZ4_TRAILING,
                            DECOMP_OVERFLOW, REC_UNDEFINED (snappy-java chunk
                            length with bit 31 set), SKIPPED                  */
    uint32_t codec;      /* attrs & 7 of the input batch                      */
    uint64_t out_offset; /* rewritten batch in the output buffer              */
    uint64_t out_len;    /* decompressed body bytes (verdict OK; unspecified
                            after an error, where the reference throws and
                            keeps nothing)                                    */
    uint64_t out_cap;    /* bytes reserved for the batch (header + bound of
                            the decoded size + slack)                         */
} rpgpu_decomp_result;   /* 32 bytes */

/* Scratch of the decompress path: the plan's slots, lists and scans, the
 * validation scratch of the rewritten batches, the wave decoders' literal
 * buffers, one 2 KB gzip workspace per gzip lane (min(n, 32768), fewer with
 * rpgpu_opts.decomp_ws_lanes, see rpgpu_decomp_scratch_bytes_ctx), the part
 * list of split bodies (36 B per part, n + 4096 parts) and the block-parallel
 * zstd plan (48 B per frame for min(n, 16384) frames, 68 B per block for
 * min(64 n, 65536) blocks).  The zstd lane workspaces (~19 KB each) are not in
 * it: the plan counts the arena's zstd batches and puts one workspace per batch
 * (at most 131,072, or decomp_ws_lanes) after the output slots, so an arena
 * without zstd batches reserves none (ABI 4); nor are the block-parallel
 * decoder's literal, record and entropy-workspace regions, which follow them
 * when the plan takes frames. */
size_t rpgpu_decomp_scratch_bytes(uint32_t n);
/* The same for a context's rpgpu_opts.decomp_ws_lanes (never more than
 * rpgpu_decomp_scratch_bytes(n)); the scratch of a context's decompress calls
 * must hold at least this. */
size_t rpgpu_decomp_scratch_bytes_ctx(const rpgpu_ctx* ctx, uint32_t n);
/* Plan: per-batch output slots and their exclusive scan into d_scratch;
 * *d_out_bytes = output bytes needed: the slots, then (256-byte aligned) the
 * zstd lane workspaces, then, when large zstd frames are planned block by
 * block, their literal and sequence-record regions and one 2,864-byte entropy
 * workspace per task.  The output buffer must hold *d_out_bytes +
 * RPGPU_ARENA_TAIL_PAD bytes; with less, batches whose slot does not fit get
 * RPGPU_V_DECOMP_OVERFLOW, and so do the zstd lane batches when the
 * workspaces do not fit. */
int32_t rpgpu_decomp_plan_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs, uint32_t n,
                                 const uint8_t* d_data, const rpgpu_batch_result* d_results,
                                 uint64_t* d_out_bytes, void* d_scratch, void* hip_stream);
/* Run (needs the plan, same d_scratch): decode, rewrite, then validate, walk
 * and index the rewritten batches.  The decoders fork from hip_stream onto the
 * context's own streams and join back: issue a context's
 * runs on one stream (or order them with events), never on two at once.
 * d_out_descs[i] / d_out_results[i]
 * describe rewritten batch i (length 0, ops 0, verdict STREAM_SHORT where
 * nothing was decompressed); index entries are laid out as by
 * rpgpu_run_device over d_out_descs; *d_index_used = entries reserved. */
int32_t rpgpu_decomp_run_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs, uint32_t n,
                                const uint8_t* d_data, const rpgpu_batch_result* d_results,
                                rpgpu_decomp_result* d_dres, uint8_t* d_out, uint64_t out_cap,
                                rpgpu_batch_desc* d_out_descs, rpgpu_batch_result* d_out_results,
                                rpgpu_record_index* d_index, uint64_t index_cap,
                                uint64_t* d_index_used, void* d_scratch, void* hip_stream);

/* ---- compression (the encode side) -------------------------
 * storage::internal::compress_batch (storage/parser_utils.cc:89-119) for every
 * batch of a validated arena that is OK and uncompressed: the records bytes
 * through compression::compressor::compress (compression/compression.cc:
 * 19-35) -- codec 3, LZ4 frame (lz4_frame_compressor.cc:68-158), and codec 2,
 * snappy-java (snappy_java_compressor.cc:58-75), byte-identical to liblz4
 * 1.9.3 / snappy 1.1.8 through the reference's loops (a body is one iobuf
 * fragment per 128 KiB) -- and a rewritten on-disk batch: attrs |= codec,
 * size_bytes = 61 + payload, fresh crc and header_crc
 * (reset_size_checksum_metadata, :122-128).  Same two-call shape as the
 * decompress path: plan (output slot per batch = header + the codec's bound,
 * total in *d_out_bytes), then run.  d_cres[i] (an rpgpu_decomp_result):
 * verdict OK / SKIPPED (not OK or already compressed) / DECOMP_OVERFLOW
 * (out_cap below the plan), out_offset, out_len (payload bytes), out_cap;
 * d_out_descs / d_out_results: the compressed batches and their validation
 * (crc, header_crc).  Codec 1 (gzip, gzip_compressor.cc:106-172) and 4
 * (zstd, stream_zstd.cc:89-151) produce valid streams that decode to the
 * records bytes with zlib / libzstd and with this engine, but not the
 * libraries' own bytes (fixed-Huffman deflate; raw literals with predefined
 * FSE sequences).  Codec 0 or > 4: RPGPU_EINVAL. */
size_t rpgpu_compress_scratch_bytes(uint32_t n);
int32_t rpgpu_compress_plan_device(rpgpu_ctx* ctx, const rpgpu_batch_result* d_results, uint32_t n, int32_t codec,
                                   uint64_t* d_out_bytes, void* d_scratch, void* hip_stream);
int32_t rpgpu_compress_run_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs, uint32_t n,
                                  const uint8_t* d_data, const rpgpu_batch_result* d_results, int32_t codec,
                                  rpgpu_decomp_result* d_cres, uint8_t* d_out, uint64_t out_cap,
                                  rpgpu_batch_desc* d_out_descs, rpgpu_batch_result* d_out_results,
                                  void* d_scratch, void* hip_stream);
/* Synchronous scalar mirror of compression::compressor::uncompress(buf, codec)
 * on the GPU, host buffers.  Returns the verdict (>= 0) or a negative status;
 * *out_len = decompressed bytes (the size needed when the verdict is
 * RPGPU_V_DECOMP_OVERFLOW; `out` then holds the first `cap` bytes).  The
 * per-batch ceiling (opts.max_decoded_batch) applies only when `cap` is
 * smaller than the frame's decoded-size bound: a caller that supplies the
 * capacity gets the decode (the retry of a DECOMP_OVERFLOW batch). */
int32_t rpgpu_uncompress(rpgpu_ctx* ctx, int32_t codec, const void* in, size_t n, void* out,
                         size_t cap, size_t* out_len);

/* Retry path of the arena decompressor: a batch that
 * validated OK but got RPGPU_V_DECOMP_OVERFLOW from rpgpu_decomp_run_device
 * (its decoded-size bound is above opts.max_decoded_batch; dres.out_len holds
 * the bound) is decompressed alone, as storage::internal::
 * maybe_decompress_batch_sync does (storage/parser_utils.cc:52-68,122-128):
 * `out` receives the rewritten on-disk batch -- the 61-byte little-endian
 * header with the codec bits removed, size_bytes = 61 + body, fresh crc and
 * header_crc -- followed by the body.  Size `cap` as 61 + dres.out_len.
 * Returns the verdict (RPGPU_V_OK, a decompress error, or
 * RPGPU_V_DECOMP_OVERFLOW with *out_len = the capacity needed) or a negative
 * status (RPGPU_EINVAL: not a compressed batch of the given format). */
int32_t rpgpu_decompress_batch(rpgpu_ctx* ctx, const void* batch, size_t len, int32_t format, void* out, size_t cap,
                               size_t* out_len);

/* ---- multi-batch record sets ---------------------------------------------
 * Replaces kafka::batch_reader (kafka/protocol/batch_reader.cc:50-161) over
 * the record data of many produce partitions at once.  d_sets[i] (a
 * rpgpu_batch_desc: offset, length, partition, ops; format must be
 * RPGPU_FMT_KAFKA_WIRE) is one record set: Kafka v2 batches back to back.
 * Each is split as read_record_batch_info / consume_batch do (size =
 * batch_length + 12, shares clamped to the bytes left), every batch is
 * validated (rpgpu_run_device semantics) and the set's outcome is the first
 * batch that is not accepted, in order (do_load_slice: corrupt_message), or
 * RPGPU_V_SET_HEADER_SHORT when < 61 bytes remain after accepted batches. */
typedef struct rpgpu_record_set_result {
    int32_t verdict;       /* OK, the failing batch's verdict, or SET_HEADER_SHORT */
    uint32_t batch_count;  /* batches the set's header chain yields             */
    uint32_t first_batch;  /* its first batch in the batch arrays               */
    uint32_t failed_batch; /* index within the set of the first failing batch
                              (= batch_count when none failed)                  */
} rpgpu_record_set_result; /* 16 bytes */

size_t rpgpu_record_sets_scratch_bytes(uint32_t nsets);
/* Plan: *d_nbatches = total batches of all sets (size the batch arrays and
 * a second scratch of rpgpu_validate_scratch_bytes(*d_nbatches) from it). */
int32_t rpgpu_record_sets_plan_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_sets, uint32_t nsets,
                                      const uint8_t* d_data, uint64_t* d_nbatches, void* d_scratch,
                                      void* hip_stream);
int32_t rpgpu_record_sets_run_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_sets, uint32_t nsets,
                                     const uint8_t* d_data, rpgpu_record_set_result* d_set_results,
                                     rpgpu_batch_desc* d_batch_descs, uint32_t nbatches,
                                     rpgpu_batch_result* d_batch_results, rpgpu_record_index* d_index,
                                     uint64_t index_cap, uint64_t* d_index_used, void* d_scratch,
                                     void* d_batch_scratch, void* hip_stream);

/* ---- legacy MessageSets (produce versions 0..2) ------------------------------
 * Replaces kafka_batch_adapter::adapt_with_version for version < 3
 * (kafka/protocol/kafka_batch_adapter.cc:215-301): convert_message_set over
 * decode_legacy_batch (kafka/protocol/legacy_message.h), record_batch_builder::
 * add_raw_kv / build and reset_size_checksum_metadata
 * (storage/parser_utils.cc:122-128).  d_sets[i] (an rpgpu_batch_desc, format
 * RPGPU_FMT_KAFKA_WIRE, length < 2^31: the caller's duty, only
 * rpgpu_convert_message_set checks it) is the record data of one produce
 * partition: magic-0 / magic-1 messages back to back in one fragment.  A
 * descriptor with RPGPU_DESC_NULL_RECORDS reads no bytes: RPGPU_V_NULL_RECORDS.
 *
 * The walk, per message, while bytes are left: int64 offset, int32
 * batch_length, int32 crc (big-endian; a consume that lacks bytes throws,
 * bytes/details/io_iterator_consumer.h:63-83: LEGACY_TRUNC_THROW, so 1..15
 * trailing bytes throw); the CRC range is share_no_consume((size_t)
 * batch_length - 4) right after the crc field, and iobuf::share clamps to the
 * bytes left (bytes/iobuf.cc:162-185): batch_length < 4 covers everything
 * left, a batch_length beyond the message covers the following ones, 4 is the
 * CRC of nothing; int8 magic (not 0 / 1: LEGACY_MAGIC, before any CRC check);
 * int8 attributes; magic 1: int64 timestamp; zlib CRC32 of the range
 * (hashing/crc32.h:18-33) against crc (LEGACY_CRC_MISMATCH); int32 key size
 * and key, int32 value size and value (-1 null; any other negative size or one
 * past the set's end throws); the next message starts where the value ended
 * (batch_length does not delimit it).  Then attributes & 7: 4..7
 * LEGACY_BAD_CODEC_THROW; 0 the record is added; 1..3: magic 0 with lz4
 * LEGACY_LZ4_MAGIC0, else a null value LEGACY_NULL_COMPRESSED, else
 * LEGACY_COMPRESSED.  The first event in this order decides the set.
 *
 * RPGPU_V_LEGACY_COMPRESSED: the reference decompresses the wrapper's value and
 * recurses; this engine does not (out of scope, as is fragmented input: DESIGN.md
 * §3 and §7), so the set is not converted and the caller sends it down the reference's
 * CPU path, as for a compaction scope over the key budget.
 *
 * A converted set is one on-disk batch: size_bytes 61 + body, base_offset 0,
 * type raft_data, attrs 0, last_offset_delta n - 1 (-1 for an empty set, which
 * converts to an empty batch), first_timestamp = max_timestamp = T (the last
 * magic-1 timestamp, else now_ms, the caller's model::timestamp::now()),
 * producer id / epoch / base sequence -1, record_count n, crc =
 * crc_record_batch, header_crc = internal_header_only_crc; record i is
 * vint(len) 00 vint(0) vint(i) vint(klen|-1) key vint(vlen|-1) value vint(0).
 * Hand vector: message A (magic 1, ts 1600000000000, key "k", value "v")
 *   0000000000000000 00000018 5eaf63dc 01 00 00000174876e8000 00000001 6b 00000001 76
 * then B (magic 0, null key, value "hi", offset 1)
 *   0000000000000001 00000010 fd6ebddb 00 00 ffffffff 00000002 6869
 * give the body 10 00 00 00 02 6b 02 76 00 10 00 00 02 01 04 68 69 00, T =
 * 1600000000000, n = 2.  A record's v2 framing is at most 23 bytes, the legacy
 * framing at least 26, so the body never exceeds the set's length. */
typedef struct rpgpu_legacy_result {
    int32_t verdict;       /* OK, NULL_RECORDS, LEGACY_*, DECOMP_OVERFLOW         */
    int32_t record_count;  /* records of the batch                               */
    int32_t event_message; /* index of the deciding message; -1: OK, NULL_RECORDS,
                              DECOMP_OVERFLOW                                    */
    uint32_t codec;        /* attributes & 7 of that message (LEGACY_COMPRESSED), else 0 */
    int64_t timestamp;     /* T                                                  */
    uint64_t out_offset;   /* the batch in d_out                                 */
    uint64_t out_len;      /* its bytes (61 + body)                              */
    uint64_t out_cap;      /* bytes reserved for it                              */
} rpgpu_legacy_result;     /* 48 bytes; a verdict other than OK specifies only
                              verdict, event_message and codec */

/* The same two-call shape and stream rules as rpgpu_decomp_*: plan, then run
 * with the same d_scratch, a context's calls on one stream (or ordered with
 * events).  Plan: *d_out_bytes = the output slots, then (256-byte aligned) the
 * message table and work list the run keeps in d_out (64 bytes per message the walk
 * reaches);
 * the output buffer must hold *d_out_bytes + RPGPU_ARENA_TAIL_PAD bytes and
 * be 16-byte aligned (RPGPU_EINVAL otherwise).
 * *d_records_total = the index capacity the run needs.  Run: d_lres[i], the
 * batches in d_out, and d_out_descs / d_out_results / d_index / *d_index_used
 * exactly as rpgpu_decomp_run_device writes them (length 0, ops 0, verdict
 * STREAM_SHORT where nothing was converted), so the output feeds
 * rpgpu_run_device, fetch, compaction and compress unchanged.  A set whose slot
 * does not fit out_cap gets RPGPU_V_DECOMP_OVERFLOW (reused: the output slot is
 * too small), and so does every non-null set when the message table does not
 * fit, because no checksum can then be checked. */
size_t rpgpu_legacy_scratch_bytes(uint32_t nsets);
int32_t rpgpu_legacy_plan_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_sets, uint32_t nsets,
                                 const uint8_t* d_data, uint64_t* d_out_bytes, uint64_t* d_records_total,
                                 void* d_scratch, void* hip_stream);
int32_t rpgpu_legacy_run_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_sets, uint32_t nsets,
                                const uint8_t* d_data, int64_t now_ms, rpgpu_legacy_result* d_lres,
                                uint8_t* d_out, uint64_t out_cap, rpgpu_batch_desc* d_out_descs,
                                rpgpu_batch_result* d_out_results, rpgpu_record_index* d_index,
                                uint64_t index_cap, uint64_t* d_index_used, void* d_scratch, void* hip_stream);
/* Synchronous scalar mirror (runs on the GPU, host buffers), shaped like
 * rpgpu_decompress_batch: returns the verdict (>= 0) or a negative status;
 * verdict OK: `out` holds the on-disk batch, *out_len its bytes;
 * RPGPU_V_DECOMP_OVERFLOW: *out_len = the capacity needed. */
int32_t rpgpu_convert_message_set(rpgpu_ctx* ctx, const void* in, size_t n, int64_t now_ms, void* out,
                                  size_t cap, size_t* out_len);
/* The error code produce_handler answers for the partition (produce.cc:440-489):
 * NULL_RECORDS and the legacy_error verdicts (LEGACY_MAGIC, _CRC_MISMATCH,
 * _LZ4_MAGIC0, _NULL_COMPRESSED) invalid_record; the *_THROW verdicts
 * unknown_server_error; OK the batch_max_bytes rule of rpgpu_kafka_error_code
 * on out->size_bytes (out: the set's row of d_out_results; may be NULL when
 * batch_max_bytes is 0); LEGACY_COMPRESSED the sentinel below, outside the
 * int16 range of Kafka error codes: the reference's answer depends on the
 * nested set.  Any other verdict: unknown_server_error.  Pure host function. */
#define RPGPU_LEGACY_ROUTE_TO_REFERENCE 0x10000
int32_t rpgpu_legacy_kafka_error_code(const rpgpu_legacy_result* r, const rpgpu_batch_result* out,
                                      uint32_t batch_max_bytes);

/* ---- generic CRC32 (zlib polynomial) over many byte ranges ----------------
 * The twins of rpgpu_crc32c_ranges_device / rpgpu_crc32c_extend with the
 * semantics of crc::crc32 (hashing/crc32.h:18-33; zlib's crc32(seed, p, n)). */
int32_t rpgpu_crc32_ranges_device(rpgpu_ctx* ctx, const uint8_t* d_data, const uint64_t* d_off,
                                  const uint32_t* d_len, const uint32_t* d_seed, uint32_t n,
                                  uint32_t* d_crc_out, void* hip_stream);
int32_t rpgpu_crc32_extend(rpgpu_ctx* ctx, uint32_t crc, const void* p, size_t n, uint32_t* out);

/* ---- segment offset/time index --------------------------------------------
 * Replaces segment_index::maybe_track (storage/segment_index.cc:98-120) +
 * index_state::maybe_index (storage/index_state.cc:38-109) over recovered
 * on-disk batches, as log_replayer feeds them (storage/log_replayer.cc:26-92).
 * Segment s covers descriptors [first_batch, first_batch + batch_count) of
 * a validated arena (d_results of rpgpu_run_device); its batches are tracked
 * in order up to the first one whose verdict is not OK.  Entries of segment
 * s are written from d_entries + first_batch (at most one per batch). */
typedef struct rpgpu_segment {
    uint32_t first_batch, batch_count;
    int64_t base_offset;    /* index_state base_offset (the segment's)       */
    uint64_t file_base;     /* arena offset of file position 0               */
    uint32_t step;          /* segment_index step (default 4096 * 8)         */
    uint8_t internal_topic; /* path().is_internal_topic()                     */
    uint8_t with_offset;    /* offset_delta_time (index_state.h:28-70)       */
    uint16_t reserved;
} rpgpu_segment;            /* 32 bytes */

typedef struct rpgpu_segment_state {
    int32_t status;         /* OK or RPGPU_V_INDEX_OFFSET_BELOW_BASE          */
    uint32_t entries;       /* index entries written                          */
    uint32_t tracked;       /* batches tracked                                */
    uint8_t monotonic;      /* batch_timestamps_are_monotonic                 */
    uint8_t non_data_timestamps;
    uint16_t reserved;
    int64_t max_offset, base_timestamp, max_timestamp;
    uint64_t acc;           /* segment_index _acc after the last batch       */
} rpgpu_segment_state;      /* 48 bytes */

typedef struct rpgpu_index_entry {
    uint32_t relative_offset; /* batch base offset - segment base offset     */
    uint32_t relative_time;   /* offset_time_index raw value                  */
    uint64_t position;        /* file position of the batch                   */
} rpgpu_index_entry;          /* 16 bytes */

int32_t rpgpu_segment_index_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs,
                                   const rpgpu_batch_result* d_results, const rpgpu_segment* d_segs,
                                   uint32_t nsegs, rpgpu_segment_state* d_states,
                                   rpgpu_index_entry* d_entries, void* hip_stream);

/* ---- stream-level storage parser -------------------------------------------
 * Replaces storage::continuous_batch_parser::consume (storage/parser.cc:
 * 113-299) over one segment file region per rpgpu_segment_read, driving one of
 * the reference's consumers (storage/parser.h:33-91):
 *   RPGPU_PARSE_RECOVERY  log_replayer's checksumming_consumer
 *                         (storage/log_replayer.cc:26-92): every batch whose
 *                         header parses is accepted; its body CRC and the stop
 *                         at the first bad one are left to rpgpu_run_device +
 *                         rpgpu_segment_index_device over the emitted batches;
 *   RPGPU_PARSE_READER    log_segment_batch_reader's skipping_consumer
 *                         (storage/log_reader.cc:28-121): accept / skip / stop
 *                         by offset range, batch type, timestamp, byte budget,
 *                         stable offset, next cached batch and the 32 KiB
 *                         reader buffer, as one read_some call does
 *                         (log_reader.cc:164-215).
 * The parser follows the size_bytes chain: per batch it reads the 61-byte
 * little-endian header (an empty read ends the stream, a short one is
 * input_stream_not_enough_bytes, all zeros is a fallocated tail), checks the
 * header CRC, asks the consumer, then reads (accept) or skips the body; the
 * result is the bytes consumed, or the error when nothing was consumed.
 * Each accepted batch becomes an on-disk rpgpu_batch_desc at
 * d_descs[desc_first + k] (k < desc_cap) for rpgpu_run_device. */
enum rpgpu_parse_mode {
    RPGPU_PARSE_RECOVERY = 0,
    RPGPU_PARSE_READER = 1,
};

typedef struct rpgpu_segment_read {
    uint64_t offset;          /* the segment's bytes in the arena             */
    uint64_t length;          /* bytes the input stream yields: any value, the
                                 parser's positions are 64-bit (a batch's own
                                 size_bytes is an int32)                      */
    uint32_t desc_first;      /* first output descriptor slot                 */
    uint32_t desc_cap;        /* slots available                              */
    uint32_t partition;       /* copied into the emitted descriptors          */
    uint8_t mode;             /* enum rpgpu_parse_mode                        */
    uint8_t ops;              /* rpgpu_op mask of the emitted descriptors     */
    uint8_t has_type_filter;  /* log_reader_config::type_filter set           */
    int8_t type_filter;
    /* log_reader_config (storage/types.h:270-300), READER mode */
    uint8_t has_first_timestamp;
    uint8_t strict_max_bytes;
    uint8_t has_next_cached;  /* skipping_consumer::_next_cached_batch set    */
    uint8_t reserved0;
    uint32_t reserved1;
    int64_t start_offset, max_offset, first_timestamp;
    int64_t stable_offset;    /* segment offsets().stable_offset              */
    int64_t next_cached_batch;
    int64_t expected_next_batch; /* skipping_consumer::_expected_next_batch
                                    (model::offset{} = INT64_MIN)             */
    uint64_t max_bytes, bytes_consumed;
    uint64_t max_buffer;      /* reader buffer limit; 0 = 32 KiB (log_reader.h:91) */
} rpgpu_segment_read;         /* 112 bytes */

typedef struct rpgpu_segment_parse_result {
    int32_t status;        /* RPGPU_OK when consume() returned a byte count;
                              else the parser_errc verdict, or
                              RPGPU_V_READ_OFFSET_REGRESSION (an exception)     */
    int32_t last_error;    /* the parser's _err: OK, END_OF_STREAM,
                              FALLOCATED_ZERO, STREAM_SHORT, HDR_CRC_MISMATCH   */
    uint32_t accepted;     /* batches accepted (descriptors emitted, up to cap) */
    uint32_t skipped;      /* batches skipped                                  */
    uint64_t bytes_consumed;   /* the parser's _bytes_consumed                  */
    uint64_t physical_offset;  /* _physical_base_offset when the parser stopped */
    int64_t start_offset;      /* READER: log_reader_config::start_offset after */
    uint64_t cfg_bytes_consumed; /* READER: log_reader_config::bytes_consumed   */
    int64_t expected_next_batch; /* READER: skipping_consumer state after      */
    uint8_t over_budget;       /* READER: log_reader_config::over_budget        */
    uint8_t stopped;           /* the consumer stopped the parser               */
    uint16_t reserved0;
    uint32_t reserved1;
} rpgpu_segment_parse_result;  /* 64 bytes */

int32_t rpgpu_segment_parse_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_segment_read* d_reads,
                                   uint32_t nreads, rpgpu_segment_parse_result* d_results,
                                   rpgpu_batch_desc* d_descs, void* hip_stream);

/* ---- remote (tiered storage) segment reader ---------------------------------
 * Replaces continuous_batch_parser::consume driving cloud_storage's
 * remote_segment_batch_consumer (cloud_storage/remote_segment.cc:788-975): one
 * remote_segment_batch_reader::read_some call (:1007-1050) per read.  The
 * config's offsets are Kafka offsets, the segment's batches carry Redpanda
 * offsets; rp_to_kafka(o) = o - cur_delta (:808-815).  Per batch:
 * accept_batch_start (:846-900) stops past max_offset or over the byte budget,
 * skips every batch that is not raft_data, and raft_data batches below
 * start_offset or older than first_timestamp; skip_batch_start (:916-946)
 * advances the config and, for raft_configuration / archival_metadata batches,
 * records an offset-translation gap [base, last] and grows cur_delta by
 * last_offset_delta + 1; consume_batch_end (:951-975) advances the config,
 * produces the batch with its base offset rewritten to the Kafka offset and
 * stops once the produced bytes pass max_consume_size (128 KiB, :61) or the
 * budget is spent.  Produced batch k becomes an on-disk descriptor at
 * d_descs[desc_first + k] with its Kafka base offset at
 * d_kafka_base[desc_first + k] (k < desc_cap); gap g is d_gaps[2 * (gap_first
 * + g)] = base, [.. + 1] = last (g < gap_cap).  Parser errors and statuses as
 * rpgpu_segment_parse_device; an exception status is RPGPU_V_BAD_CODEC_THROW
 * (the record_batch constructor of a codec 5..7 batch, model/record.h:582-585)
 * or RPGPU_V_REMOTE_DELTA_ASSERT. */
typedef struct rpgpu_remote_read {
    uint64_t offset;          /* the stream's bytes in the arena              */
    uint64_t length;          /* bytes the input stream yields: any value, as
                                 rpgpu_segment_read.length                    */
    uint32_t desc_first, desc_cap;
    uint32_t gap_first, gap_cap;
    uint32_t partition;       /* copied into the emitted descriptors          */
    uint8_t ops;              /* rpgpu_op mask of the emitted descriptors     */
    uint8_t has_first_timestamp;
    uint8_t strict_max_bytes;
    uint8_t over_budget;      /* log_reader_config::over_budget on entry      */
    int64_t start_offset;     /* log_reader_config (Kafka offsets)            */
    int64_t max_offset;
    int64_t first_timestamp;
    int64_t cur_delta;        /* remote_segment_batch_reader::_cur_delta      */
    int64_t cur_rp_offset;    /* remote_segment_batch_reader::_cur_rp_offset  */
    uint64_t max_bytes, bytes_consumed;
} rpgpu_remote_read;          /* 96 bytes */

typedef struct rpgpu_remote_parse_result {
    int32_t status;           /* as rpgpu_segment_parse_result.status (above) */
    int32_t last_error;       /* the parser's _err                            */
    uint32_t accepted;        /* batches produced (descriptors, up to cap)    */
    uint32_t skipped;
    uint64_t bytes_consumed;  /* the parser's _bytes_consumed                 */
    int64_t start_offset;     /* log_reader_config::start_offset after (Kafka) */
    uint64_t cfg_bytes_consumed;
    int64_t cur_delta;        /* after the read                               */
    int64_t cur_rp_offset;    /* after the read                               */
    uint64_t produced_bytes;  /* remote_segment_batch_reader::_total_size     */
    uint32_t gaps;            /* gaps recorded (all of them, even past gap_cap) */
    uint8_t over_budget;
    uint8_t stopped;          /* the consumer stopped the parser              */
    uint16_t reserved;
} rpgpu_remote_parse_result;  /* 72 bytes */

int32_t rpgpu_remote_segment_parse_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_remote_read* d_reads,
                                          uint32_t nreads, rpgpu_remote_parse_result* d_results,
                                          rpgpu_batch_desc* d_descs, int64_t* d_kafka_base, int64_t* d_gaps,
                                          void* hip_stream);

/* ---- partition summaries (multi-GPU gather) -------------------------------
 * Per partition p of [part_lo, part_lo + nparts), over the batches of
 * d_descs / d_results (a validation's output; batches of other partitions
 * are ignored), six int64 columns at d_out[p * 6]: batches, OK batches,
 * index entries, bytes of OK batches (size_bytes), sum of the computed CRCs,
 * and the last offset (max base_offset + last_offset_delta over OK batches,
 * -1 if none; storage/offset_assignment.h:25-28).  A partition-sharded run
 * (one GPU per partition range) gathers these to one rank.
 * The calls of one context share its per-workgroup partial table: issue them
 * on one stream (or order them with events), never on two streams at once. */
int32_t rpgpu_partition_summaries_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs,
                                         const rpgpu_batch_result* d_results, uint32_t n, uint32_t part_lo,
                                         uint32_t nparts, int64_t* d_out, void* hip_stream);

/* ---- compaction keys -------------------------------------
 * Which records survive self-compaction of a segment:
 * segment::compaction_index_batch (storage/segment.cc:456-483) indexes every
 * record of a compactible batch (not raft_configuration, archival_metadata or
 * version_fence: segment_utils.h:198-203) under its key prefixed with the
 * batch type (compacted_index.h:33-44; a null key is an empty one), keeping
 * the latest offset per key (spill_key_index.cc:154-176);
 * compaction_key_reducer / compacted_offset_list_reducer
 * (compaction_reducers.cc:35-113) turn that into the set of offsets to keep,
 * and copy_data_segment_reducer::filter keeps a record iff its offset is in
 * the set (should_keep, compaction_reducers.h:130-133; a non-compactible batch
 * whole, compaction_reducers.cc:117-123).
 * Input: a validated and indexed arena (rpgpu_validate_device / submit, or the
 * rewritten batches of the decompress path).  Batches with the same
 * desc.partition form one compaction scope (a segment).  keep[j] for each of
 * the index_cap index entries: 1 keep, 0 superseded by a later record with the
 * same key, 2 not a record of an OK batch (slack between batch slices, failed
 * batches).  *d_nkeys = distinct keys over all scopes.  The key map here is
 * unbounded: parity with the reference holds only while its maps stay under
 * their memory budgets (spill_key_index.cc:99-138; compaction_key_reducer,
 * compaction_reducers.cc:49-67).  Past them the reference evicts entries in
 * its hash map's iteration order and keeps the evicted keys' records as well,
 * which this engine does not reproduce (it can only keep fewer records).  That
 * order is not a function of the input: the map is an absl::node_hash_map, and
 * absl's SwissTable starts each probe at H1 = (hash >> 7) ^ PerTableSalt(ctrl),
 * a salt taken from the address of the table's control bytes, so which entry
 * is "first" depends on where the heap put the table.  A caller wanting the
 * reference's bytes sends a scope whose distinct keys (*d_nkeys for a one-scope
 * call) would exceed the budget (5 MiB: ~60 B of map per key plus its bytes)
 * to the reference's CPU path.
 * d_scratch: rpgpu_compaction_scratch_bytes(index_cap) bytes. */
size_t rpgpu_compaction_scratch_bytes(uint64_t index_cap);
int32_t rpgpu_compaction_keep_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                     const rpgpu_batch_result* d_results, uint32_t n,
                                     const rpgpu_record_index* d_index, uint64_t index_cap, uint8_t* d_keep,
                                     uint64_t* d_nkeys, void* d_scratch, void* hip_stream);

/* ---- compaction rewrite ----------------------------------
 * copy_data_segment_reducer::filter (storage/compaction_reducers.cc:117-251)
 * over the batches whose records rpgpu_compaction_keep_device classified:
 *   - a batch that did not validate OK, or whose index slice does not hold
 *     all its records, is not rewritten (SKIPPED, no output);
 *   - a raft_configuration / archival_metadata / version_fence batch is kept
 *     whole (NOT_COMPACTIBLE, :119-123);
 *   - a transactional, non-control batch loses its transactional bit (:125-143);
 *   - no record kept: the batch is dropped (DROPPED, std::nullopt :155-158);
 *   - every record kept: the batch as it is (KEPT; TX_CLEARED when its bit was
 *     cleared, with fresh CRCs, :160-167);
 *   - otherwise the kept records are re-encoded (model::append_record_to_buffer,
 *     model/record_utils.cc:183-225: canonical varints of the parsed fields --
 *     record size, 32-bit offset delta, key / value / header sizes -- the
 *     bytes the parser copied, every header of the record's count), first_ts =
 *     first_ts + the first kept record's ts delta, max_ts (create-time batches)
 *     = that new first_ts + the last kept record's ts delta, record_count = the
 *     kept records, then reset_size_checksum_metadata (FILTERED, :169-251).
 * Every output is an on-disk (little-endian) batch at out_offset with fresh
 * crc / header_crc, walked and indexed (d_out_results, d_out_index) like the
 * rewritten batches of rpgpu_decomp_run_device.  Recompressing an originally
 * compressed batch (do_compaction's compress_batch, :253-284) is
 * rpgpu_compress_plan_device / run_device over the output.
 * Plan, then run, on the same stream: the plan sizes the output
 * (*d_out_bytes); keep is rpgpu_compaction_keep_device's d_keep.  The
 * reference keeps a record when its offset_delta is among the deltas of the
 * records should_keep() accepted (std::count, :174-178); a record is kept here
 * by its own keep flag.  The two agree because rpgpu_compaction_keep_device's
 * flags are a function of the record's offset, as should_keep is: records
 * sharing an offset_delta share one flag (tests/test_compaction.py,
 * duplicate-delta case).  A caller passing its own flags must keep that
 * property. */
enum rpgpu_compact_action {
    RPGPU_COMPACT_SKIPPED = 0,
    RPGPU_COMPACT_DROPPED = 1,
    RPGPU_COMPACT_KEPT = 2,
    RPGPU_COMPACT_TX_CLEARED = 3,
    RPGPU_COMPACT_FILTERED = 4,
    RPGPU_COMPACT_NOT_COMPACTIBLE = 5,
};

typedef struct rpgpu_compact_result {
    int32_t action;        /* enum rpgpu_compact_action                       */
    int32_t record_count;  /* records of the output batch                     */
    uint64_t out_offset;   /* output batch in d_out                           */
    uint64_t out_len;      /* its bytes (61 + body); 0 without an output      */
    uint32_t removed;      /* records dropped from the batch                  */
    uint32_t reserved;
} rpgpu_compact_result;    /* 32 bytes */

size_t rpgpu_compaction_rewrite_scratch_bytes(uint32_t n);
int32_t rpgpu_compaction_rewrite_plan_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                             const rpgpu_batch_result* d_results, uint32_t n,
                                             const rpgpu_record_index* d_index, uint64_t index_cap,
                                             const uint8_t* d_keep, uint64_t* d_out_bytes, void* d_scratch,
                                             void* hip_stream);
int32_t rpgpu_compaction_rewrite_run_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                            const rpgpu_batch_result* d_results, uint32_t n,
                                            const rpgpu_record_index* d_index, uint64_t index_cap,
                                            const uint8_t* d_keep, rpgpu_compact_result* d_cres, uint8_t* d_out,
                                            uint64_t out_cap, rpgpu_batch_desc* d_out_descs,
                                            rpgpu_batch_result* d_out_results, rpgpu_record_index* d_out_index,
                                            uint64_t out_index_cap, uint64_t* d_out_index_used, void* d_scratch,
                                            void* hip_stream);

/* ---- fetch serialization ----------------------------------
 * kafka_batch_serializer (kafka/protocol/batch_consumer.h:26-101) over batches a
 * reader returns: each on-disk batch becomes a Kafka v2 wire batch,
 * writer_serialize_batch (kafka/protocol/wire.h:645-681) -- big-endian
 * header, batch_length = size_bytes - 12, partition leader epoch =
 * leader_epoch_from_term(term) (kafka/types.h:117-124: -1 when the term does
 * not fit int32), magic 2, the stored Kafka crc, then the records bytes
 * unchanged.  A wire batch is exactly as long as the on-disk one, so batch i
 * is written at d_out + d_descs[i].offset: d_out mirrors the arena and a
 * contiguous run of batches stays contiguous (d_out must not overlap
 * d_data).  d_terms: the term of each
 * batch (record_batch::term(), set by the reader from its segment), or NULL
 * for term 0.  The header is read from the batch bytes (format must be
 * RPGPU_FMT_RP_DISK; size_bytes < 61 or > desc.length writes nothing and
 * counts as an error in the range's status).
 * Optional per-range summaries (the serializer's result, :29-40, built by
 * operator() and end_of_stream, :54-77): for the
 * batches [first, first + count) of d_descs, in order: record_count (uint32
 * sum), base_offset (of the batch at which the running record count was 0),
 * last_offset, first_tx_batch_offset (INT64_MIN with has_first_tx = 0 when
 * no batch is transactional), output bytes.  Empty range: offsets INT64_MIN
 * (a default model::offset). */
typedef struct rpgpu_fetch_range {
    uint32_t first;
    uint32_t count;
} rpgpu_fetch_range;      /* 8 bytes */
typedef struct rpgpu_fetch_summary {
    int64_t base_offset;
    int64_t last_offset;
    int64_t first_tx_batch_offset;
    uint64_t bytes;
    uint32_t record_count;
    uint8_t has_first_tx;
    uint8_t reserved0;
    uint16_t reserved1;
    int32_t status;       /* 0, or the number of batches with a bad size */
    uint32_t reserved2;
} rpgpu_fetch_summary;    /* 48 bytes */
int32_t rpgpu_kafka_serialize_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                     const int64_t* d_terms, uint32_t n, uint8_t* d_out,
                                     const rpgpu_fetch_range* d_ranges, uint32_t nranges,
                                     rpgpu_fetch_summary* d_summaries, void* hip_stream);

/* ---- batch timequery --------------------------------------
 * storage::batch_timequery (storage/log_reader.cc:381-407) for batch `batch` of
 * a validated and indexed arena: (base_offset, first_timestamp), or, when
 * first_timestamp < time and the batch is uncompressed, the first record with
 * first_timestamp + timestamp_delta >= time.  The batch is the first one a
 * log_reader with first_timestamp = time returns (disk_log_impl.cc:1299-1319):
 * rpgpu_segment_parse_device in reader mode with has_first_timestamp finds it.
 * status: the batch's verdict (RPGPU_V_OK = result valid), -1 out of range. */
typedef struct rpgpu_timequery {
    uint32_t batch;
    uint32_t reserved;
    int64_t time;
} rpgpu_timequery;        /* 16 bytes */
typedef struct rpgpu_timequery_result {
    int64_t offset;
    int64_t time;
    int32_t status;
    uint32_t reserved;
} rpgpu_timequery_result; /* 24 bytes */
int32_t rpgpu_batch_timequery_device(rpgpu_ctx* ctx, const rpgpu_batch_result* d_results, uint32_t n,
                                     const rpgpu_record_index* d_index, const rpgpu_timequery* d_queries,
                                     uint32_t nq, rpgpu_timequery_result* d_out, void* hip_stream);

/* ---- REST proxy fetch rendering ---------------------------
 * rjson_serialize_impl<kafka::fetch_response> (pandaproxy/json/requests/fetch.h:94-154)
 * over validated and indexed batches: the body of the proxy's fetch reply,
 * one JSON array per response.
 *   A response (rpgpu_pp_response) is an ordered run of ranges of d_ranges and
 *   stands for one kafka::fetch_response; a range (rpgpu_pp_range) is one
 *   partition_response: the batches [first, first + count) of d_descs, a topic
 *   name (topic_len bytes at topic_off of d_topics) and a partition.  Ranges
 *   must not overlap: a batch belongs to at most one range and a range to at
 *   most one response (the scratch holds one output offset per batch).
 * Output per response: '[' + objects joined by ',' + ']' without whitespace,
 * "[]" when no record is rendered (test/fetch.cc:77).  Per batch, in order
 * (fetch.h:114-131):
 *   - a verdict other than RPGPU_V_OK fails the response (consume_batch
 *     throws, no body exists): RPGPU_PP_BAD_BATCH;
 *   - a control batch (attrs & 0x20) contributes nothing, whatever its codec;
 *   - codec != 0: RPGPU_PP_COMPRESSED.  The reference decompresses here
 *     (maybe_decompress_batch_sync); a caller renders such batches from the
 *     output of rpgpu_decomp_run_device (its d_out, descriptors, results and
 *     index).  A response mixing both kinds needs two arenas: the caller
 *     splits it;
 *   - index_count != record_count (validated without RPGPU_OP_INDEX, or the
 *     index was cut): RPGPU_PP_NOT_INDEXED.
 * Per record (fetch.h:46-82, test/fetch.cc:95-96), keys in this order:
 *   {"topic":"<name>","key":K,"value":V,"partition":<int32>,"offset":<int64>}
 * offset is the index entry's offset (base_offset + offset_delta as the engine
 * wrapped it) in decimal, K and V are null when the length is <= 0 (a null
 * and an empty field are both an empty iobuf, pandaproxy/json/iobuf.h:84-86),
 * else '"' + base64 + '"' (iobuf.h:83-89, utils/base64.cc:74-112: the
 * standard alphabet, '=' padding, no line breaks).  Record headers are not
 * rendered.  format: serialization_format::none (0) and binary_v2 (3) both
 * take this path (iobuf.h:70-73); any other value returns RPGPU_EINVAL
 * (json_v2 re-parses every value, iobuf.h:91-101: not on the device).
 * Topic names must pass model::validate_kafka_topic_name
 * (model/validation.cc:20-38: 1..249 bytes of [A-Za-z0-9._-], not "." or
 * ".."), so they need no JSON escaping; anything else, or a name outside
 * d_topics, is RPGPU_PP_BAD_TOPIC.  A range running past n, or a response
 * running past nranges, is RPGPU_PP_BAD_RANGE.
 * A response's status is that of its first offending item in range order,
 * then batch order; a range's own defects (topic, then bounds) come before
 * its batches'.  bad_batch: the offending batch's index in d_descs
 * (BAD_BATCH, COMPRESSED, NOT_INDEXED), the offending range's index in
 * d_ranges (BAD_TOPIC, BAD_RANGE; nranges for a response past nranges), else
 * 0.  A failed response has out_len 0 and writes nothing.
 * Plan, then run, on the same stream and scratch.  The plan fills every
 * result row (status, records, the exact out_len, out_off: an exclusive scan
 * of the lengths, every slot on a 16-byte boundary) and *d_out_bytes.  The
 * run writes exactly out_len bytes at out_off of every OK response, nothing
 * between the slots and nothing at or past out_cap; a response whose slot
 * ends past out_cap becomes RPGPU_PP_NO_ROOM (out_off and out_len kept: what
 * it needs) and writes nothing.  A plan may be run any number of times; every
 * run rewrites all result rows.  Wire and on-disk arenas are both accepted
 * (key / value offsets are relative to the batch start in both); d_out must
 * not overlap d_data. */
enum rpgpu_pp_format { RPGPU_PP_FMT_NONE = 0, RPGPU_PP_FMT_BINARY_V2 = 3 };
enum rpgpu_pp_status {
    RPGPU_PP_OK = 0,
    RPGPU_PP_BAD_BATCH,
    RPGPU_PP_COMPRESSED,
    RPGPU_PP_NOT_INDEXED,
    RPGPU_PP_BAD_TOPIC,
    RPGPU_PP_BAD_RANGE,
    RPGPU_PP_NO_ROOM,
};
typedef struct rpgpu_pp_range {
    uint32_t first;      /* first batch of the partition_response in d_descs */
    uint32_t count;
    uint32_t topic_off;  /* the topic name in d_topics                        */
    uint16_t topic_len;
    uint16_t reserved0;
    int32_t partition;
    uint32_t reserved1;
} rpgpu_pp_range;        /* 24 bytes */
typedef struct rpgpu_pp_response {
    uint32_t first_range;
    uint32_t range_count;
} rpgpu_pp_response;     /* 8 bytes */
typedef struct rpgpu_pp_result {
    uint64_t out_off;    /* the response's JSON in d_out                      */
    uint64_t out_len;
    uint32_t records;    /* objects in the array                              */
    int32_t status;      /* enum rpgpu_pp_status                              */
    uint32_t bad_batch;
    uint32_t reserved;
} rpgpu_pp_result;       /* 32 bytes */
/* The longest key or value a record's own lane encodes; a longer one is
 * encoded by a whole wavefront.  On 512 MiB arenas the lane path measured
 * faster at 16, 64 and 128-byte values, the wave path at 256 and 1,024
 * bytes. */
#define RPGPU_PP_LANE_FIELD_MAX 128

size_t rpgpu_pp_fetch_scratch_bytes(uint32_t n, uint32_t nranges, uint32_t nresponses);
int32_t rpgpu_pp_fetch_plan_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs,
                                   const rpgpu_batch_result* d_results, uint32_t n,
                                   const rpgpu_record_index* d_index, const uint8_t* d_topics, uint32_t topics_len,
                                   const rpgpu_pp_range* d_ranges, uint32_t nranges,
                                   const rpgpu_pp_response* d_responses, uint32_t nresponses, int32_t format,
                                   rpgpu_pp_result* d_out_results, uint64_t* d_out_bytes, void* d_scratch,
                                   void* hip_stream);
int32_t rpgpu_pp_fetch_run_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                  const rpgpu_batch_result* d_results, uint32_t n,
                                  const rpgpu_record_index* d_index, const uint8_t* d_topics,
                                  const rpgpu_pp_range* d_ranges, uint32_t nranges,
                                  const rpgpu_pp_response* d_responses, uint32_t nresponses, uint8_t* d_out,
                                  uint64_t out_cap, rpgpu_pp_result* d_out_results, void* d_scratch,
                                  void* hip_stream);

/* ---- log append (the end of the produce call stack) -----------
 * disk_log_appender::operator() (storage/disk_log_appender.cc:71-135) and
 * storage::write -> disk_header_to_iobuf (storage/segment_appender_utils.cc:
 * 28-61) over a validated arena: the batches the produce handler accepted
 * leave the device as the bytes each partition's segment files receive.
 * Call order on the produce path: validate -> rpgpu_set_max_timestamp_device
 * -> rpgpu_kafka_error_codes_device -> append.
 *
 * The caller supplies a dense range of logs (rpgpu_append_log, nlogs rows):
 * the batch of descriptor i belongs to log desc.partition - part_lo, the
 * sharding convention of rpgpu_partition_summaries_device.  A batch is
 * eligible when its verdict is RPGPU_V_OK, its partition lies in [part_lo,
 * part_lo + nlogs) and d_codes is NULL or d_codes[i] == 0 (d_codes: the
 * output of rpgpu_kafka_error_codes_device, so a batch over batch_max_bytes
 * is not appended, produce.cc:317-324).  Every other batch is skipped: the
 * handler answers it with an error and never appends it.  (RPGPU_V_OK implies
 * 61 <= size_bytes <= desc.length; a result row that breaks this is skipped.)
 *
 * Per log, the eligible batches in descriptor order go through the appender:
 *   idx = log.next_offset; last = INT64_MIN (model::offset{}); byte_size = 0
 *   left = ROLL_FIRST ? 0 : (max_segment_size > file_offset
 *                            ? max_segment_size - file_offset : 0)
 *   pos  = file_offset
 *   for each eligible batch b:
 *       base = idx                                  (disk_log_appender.cc:73)
 *       if left == 0:                 (needs_to_roll_log, :61 and :80-97)
 *           new segment {base_offset = idx, file position 0, ROLLED}; pos = 0
 *           left = max_segment_size   (initialize() -> bytes_left_before_roll())
 *       if b.type == ghost_batch (7):               (:111-117, on-disk input)
 *           last = base + lod; idx = last + 1; continue   (GHOST, no bytes)
 *       write the 61-byte header + body at pos      (segment.cc:507-531)
 *       pos += size_bytes; byte_size += size_bytes
 *       left -= min(left, size_bytes)               (:119-132)
 *       last = base + lod; idx = last + 1
 * RPGPU_APPEND_ROLL_FIRST is the caller's statement that the log has no
 * segment or appender, or that the batches' term differs from the log's
 * (needs_to_roll_log); the term is neither serialized nor part of the header
 * CRC, so nothing else of it is needed.  max_segment_size == 0 makes the
 * reference's do_until spin forever: such a log gets RPGPU_APPEND_BAD_CONFIG
 * and appends nothing (its batches are RPGPU_APPEND_SKIPPED).  Offsets wrap in
 * 64-bit arithmetic as in rpgpu_segment_index_device; the precondition is
 * next_offset + sum(lod + 1) <= INT64_MAX (signed overflow of model::offset
 * is undefined in the reference).
 *
 * The written header (disk_header_to_iobuf, little-endian): size_bytes is
 * batch_length + 12 for wire input and the stored value for on-disk input;
 * base_offset is `base`; type is 1 (raft_data, as read_header sets it) for
 * wire input and the stored type for on-disk input; crc, attrs,
 * last_offset_delta, both timestamps, producer id and epoch, base sequence
 * and record count are taken from the batch bytes, so a batch re-stamped by
 * rpgpu_set_max_timestamp_device is appended as stamped; header_crc is
 * internal_header_only_crc of the above (CRC32C of bytes [4, 61)).  The body
 * is the size_bytes - 61 bytes after the input header: trailing bytes of a
 * wire descriptor past batch_length + 12 are not copied, compressed batches
 * are appended as they are.
 *
 * Output.  Log l's bytes form one region at out_offset (an exclusive scan of
 * the logs' byte_size, every region start on a 16-byte boundary); its
 * segments lie back to back inside it: exactly the bytes appended to its
 * files, in order.  Output rows (d_out_descs, d_out_results) are log-major, in
 * descriptor order within a log, so a segment is a contiguous run of rows.
 * d_out_descs are RPGPU_FMT_RP_DISK descriptors into d_out (ops = RPGPU_OP_CRC |
 * RPGPU_OP_HDRCRC, the log's partition, length = size_bytes); d_out_results[r]
 * is the input row with base_offset, header_crc, type and size_bytes as
 * written.  index_first / index_count are unchanged: they still name the
 * input index, whose offset column holds the produce-time offsets.  The
 * output feeds rpgpu_run_device, rpgpu_kafka_serialize_device and, for ROLLED
 * segments, rpgpu_segment_index_device without conversion; a continuing
 * segment's index goes on from its state with rpgpu_segidx_track_device.
 * A segment row (rpgpu_append_segment) is opened at each roll, and for the
 * continuing segment when the first eligible batch reaches it with left > 0.
 * A ghost batch's file_pos is the position the next written batch takes.
 *
 * Plan, then run, on the same stream and scratch
 * (rpgpu_append_scratch_bytes(n, nlogs) bytes).  The plan reads descriptors,
 * result rows, codes and logs, never d_data; it fills every batch row, every
 * log row and d_totals: [0] the smallest out_cap that holds every log, [1]
 * the output rows, [2] the segment rows.  A log is written whole or not at
 * all: if its bytes end past out_cap, its rows past rows_cap or its segment
 * rows past seg_cap, the run sets its status to RPGPU_APPEND_NO_ROOM (a log
 * without bytes, rows or segments needs no room for them); every other field
 * is kept, they say what it needs, and nothing of such a log is written.  The
 * run writes nothing outside the regions of OK logs and nothing at or past
 * out_cap; d_out must not overlap d_data.  A plan may be run any number of
 * times; every run sets the status of every log again.
 *
 * Hand vector: one log {next_offset 42, file_offset 0, max_segment_size 64},
 * two wire batches (71 and 78 bytes; the first exhausts the segment, the
 * second rolls):
 *   in  00000000000000000000003b0000000002d00832e900000000000000000000000003
 *       e800000000000003e800000000000000010002000000030000000112000000026b04
 *       763100
 *       0000000000000007000000420000000002d66127c600000000000100000000000007
 *       d000000000000007d1ffffffffffffffffffffffffffff0000000210000000010476
 *       32000e000202026b0100
 *   out af809a44470000002a0000000000000001e93208d0000000000000e8030000000000
 *       00e80300000000000001000000000000000200030000000100000012000000026b04
 *       763100
 *       8f4feff44e0000002b0000000000000001c62761d6000001000000d0070000000000
 *       00d107000000000000ffffffffffffffffffffffffffff0200000010000000010476
 *       32000e000202026b0100
 *   rows {APPENDED, 0, base 42, pos 0, segment 0}, {APPENDED, 1, 43, 0, 1};
 *   log {OK, 2 batches, 2 segments, last_offset 44, next_offset 45, 149 bytes};
 *   segments {flags 0, first 0, count 1, base 42, pos 0, out 0, 71 bytes},
 *            {ROLLED, first 1, count 1, base 43, pos 0, out 71, 78 bytes}. */
#define RPGPU_APPEND_ROLL_FIRST 1u /* rpgpu_append_log.flags */
typedef struct rpgpu_append_log {
    int64_t next_offset;       /* offset the next batch takes (_idx)             */
    uint64_t file_offset;      /* size of the active segment's file              */
    uint64_t max_segment_size;
    uint32_t flags;            /* RPGPU_APPEND_ROLL_FIRST                        */
    uint32_t reserved;
} rpgpu_append_log;            /* 32 bytes */

enum rpgpu_append_action { RPGPU_APPEND_SKIPPED = 0, RPGPU_APPEND_APPENDED = 1, RPGPU_APPEND_GHOST = 2 };
typedef struct rpgpu_append_batch { /* one per input descriptor */
    int32_t action;            /* enum rpgpu_append_action                       */
    uint32_t out_row;          /* row in d_out_descs / d_out_results; UINT32_MAX if none */
    int64_t base_offset;
    uint64_t file_pos;         /* start_physical_offset in its segment           */
    uint32_t segment;          /* row in the segment table                       */
    uint32_t reserved;
} rpgpu_append_batch;          /* 32 bytes */

enum rpgpu_append_status { RPGPU_APPEND_OK = 0, RPGPU_APPEND_NO_ROOM = 1, RPGPU_APPEND_BAD_CONFIG = 2 };
typedef struct rpgpu_append_log_result { /* append_result (end_of_stream) plus bookkeeping */
    int32_t status;            /* enum rpgpu_append_status                       */
    uint32_t batches;          /* batches written                                */
    uint32_t ghosts;
    uint32_t segments;         /* segment rows                                   */
    uint32_t first_row;        /* first output row                               */
    uint32_t first_segment;    /* first segment row                              */
    int64_t base_offset;       /* = rpgpu_append_log.next_offset                 */
    int64_t last_offset;       /* INT64_MIN when nothing was eligible            */
    int64_t next_offset;       /* _idx after the call                            */
    uint64_t byte_size;
    uint64_t out_offset;       /* the log's region in d_out                      */
} rpgpu_append_log_result;     /* 64 bytes */

#define RPGPU_APPEND_SEG_ROLLED 1u /* rpgpu_append_segment.flags: a new segment file */
typedef struct rpgpu_append_segment {
    uint32_t log;
    uint32_t flags;            /* RPGPU_APPEND_SEG_ROLLED                        */
    uint32_t first, count;     /* output rows; count 0: only ghosts reached it   */
    int64_t base_offset;       /* _idx when the row was opened (ROLLED: the new
                                  segment's base offset)                         */
    uint64_t file_pos;         /* 0 when ROLLED, else file_offset                */
    uint64_t out_offset;       /* its bytes in d_out                             */
    uint64_t bytes;
} rpgpu_append_segment;        /* 48 bytes */

size_t rpgpu_append_scratch_bytes(uint32_t n, uint32_t nlogs);
int32_t rpgpu_append_plan_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs,
                                 const rpgpu_batch_result* d_results, uint32_t n, const int32_t* d_codes,
                                 const rpgpu_append_log* d_logs, uint32_t part_lo, uint32_t nlogs,
                                 rpgpu_append_batch* d_batch_rows, rpgpu_append_log_result* d_log_results,
                                 uint64_t* d_totals, void* d_scratch, void* hip_stream);
int32_t rpgpu_append_run_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                const rpgpu_batch_result* d_results, uint32_t n, const rpgpu_append_log* d_logs,
                                uint32_t part_lo, uint32_t nlogs, const rpgpu_append_batch* d_batch_rows,
                                rpgpu_append_log_result* d_log_results, uint8_t* d_out, uint64_t out_cap,
                                rpgpu_batch_desc* d_out_descs, rpgpu_batch_result* d_out_results, uint32_t rows_cap,
                                rpgpu_append_segment* d_segments, uint32_t seg_cap, void* d_scratch,
                                void* hip_stream);

/* ---- tiered-storage offset index: build and seek ------------------------------
 * cloud_storage::offset_index (cloud_storage/remote_segment_index.{h,cc}): the
 * sampled (Redpanda offset, Kafka offset, file position) index that every
 * uploaded or hydrated segment gets (archival/ntp_archiver_service.cc:1139-1174,
 * cloud_storage/remote_segment.cc:281-300) and that every remote read seeks
 * with (find_kaf_offset, remote_segment.cc:257-275).  rpgpu_rsindex_plan_device
 * + rpgpu_rsindex_run_device are remote_segment_index_builder riding the
 * parser over a segment and offset_index::to_iobuf; rpgpu_rsindex_find_device
 * is from_iobuf + find_rp_offset / find_kaf_offset.  Integer-only: the blobs
 * are the reference's, byte for byte.
 *
 * Builder (remote_segment_index.cc:307-349), one segment = one stream of
 * RPGPU_FMT_RP_DISK descriptors in file order (on-disk header: size_bytes i32
 * at 4, base_offset i64 at 8, type i8 at 16, last_offset_delta i32 at 23):
 *   delta = initial_delta; window = 0; pos = 0
 *   for each batch:
 *       if type == 2 (raft_configuration) or type == 19 (archival_metadata):
 *           delta += last_offset_delta + 1
 *       else if window >= sampling_step:
 *           add(base_offset, base_offset - delta, pos); window = 0
 *       window += size_bytes; pos += size_bytes   (the parser's running sum,
 *                                                  storage/parser.cc:132-138)
 * Every other type is sampled like data (ghost batches and unknown types too);
 * a configuration batch that arrives when the window is full defers the sample
 * to the next other batch; sampling_step 0 samples the first such batch, 1
 * does not.  Only the 61-byte headers are read, no CRC is checked: the parser
 * that delivered the descriptors did that.
 *
 * offset_index::add (:37-63) fills three 16-entry write buffers cyclically and,
 * when the position wraps to 0 mod 16, appends them as one row to each of
 * three delta-FOR encoders (utils/delta_for.h).  The buffers are never
 * cleared: slots at and past (samples mod 16) keep the previous row's values
 * (zero before the first flush), and to_iobuf serializes all 16.
 *
 * Delta-FOR row (delta_for.h:276-284, 515-764): the rp and Kafka streams use
 * delta_xor (buf[i] = row[i] ^ prev), the file stream delta_delta
 * (buf[i] = row[i] - prev - file_pos_step); prev starts at the encoder's
 * initial value (base rp, base Kafka, 0) and carries across rows.  nbits =
 * bit_width(OR of buf); the row is one byte nbits, a 32-bit section if nbits
 * >= 32, a 16-bit section if what is left >= 16, an 8-bit section if what is
 * left >= 8 (each: the 16 values' next low bits, little-endian, value-major),
 * then the remaining r = 1..7 bits as 16 r-bit fields in one little-endian bit
 * string of 2r bytes, value i at bit i * r; nbits == 64 is 16 little-endian
 * uint64.  A row takes 1 + 2 * nbits bytes.  delta_delta::encode asserts
 * row[i] - prev >= file_pos_step when a row is flushed: such a segment gets
 * RPGPU_RSINDEX_DELTA_ASSERT (possible only with sampling_step <
 * file_pos_step); the same delta in the unflushed tail goes unnoticed, as in
 * the reference.
 *
 * Blob (to_iobuf :216-258 in a serde envelope, serde/serde.h:515-565; all
 * little-endian, nothing aligned):
 *     0, 1  version 1, compat version 1
 *     2     u32 payload size = blob size - 6
 *     6     min_file_pos_step i64        14  num_elements u64 (samples)
 *    22, 30 base_rp, last_rp             38, 46  base_kaf, last_kaf
 *    54, 62 base_file (0), last_file
 *    70     u32 16 + 16 x i64 rp write buffer; 202 the Kafka one; 334 the file one
 *   466     u32 length + rp stream, u32 length + Kafka stream, u32 length + file stream
 * last_* is the encoder's _last: the last value of the last flushed row, or the
 * initial value without rows.  Blob size = 478 + the three stream lengths.
 *
 * Plan (rpgpu_rsindex_scratch_bytes(n, nsegs) bytes of scratch, shared with the
 * run): reads d_segs, d_descs and the headers at desc.offset.  The segments'
 * descriptor ranges must not overlap.  It fills every field of every result
 * row; d_totals[0] is the smallest out_cap that holds every OK blob,
 * d_totals[1] the samples of the OK segments.  RPGPU_RSINDEX_BAD_BATCH: a
 * descriptor index >= n, a descriptor that is not RPGPU_FMT_RP_DISK or shorter
 * than 61 bytes, or a header whose size_bytes < 61; bad_batch is the index of
 * the first one in d_descs and samples, rows, config_batches, final_delta and
 * stream_bytes describe the batches in front of it (a segment that would also
 * assert is BAD_BATCH).  A BAD_BATCH or
 * DELTA_ASSERT segment has out_bytes 0 and the three stream sizes 0, and gets
 * no blob.  Blobs lie at out_offset, an exclusive scan of the OK segments'
 * out_bytes with every start on a 16-byte boundary.
 * Run: reads the plan's scratch and d_segs (the same rows), not d_data, and
 * writes each blob whole or not at all: one that ends past out_cap gets
 * RPGPU_RSINDEX_NO_ROOM, every other field is kept.  It writes nothing outside
 * the OK blobs and nothing at or past out_cap.  A plan may be run any number
 * of times; every run sets every status again.
 *
 * Find, one query per row: d_blobs + blob_offset is any blob to_iobuf could
 * have written.  RPGPU_RSINDEX_BAD_BLOB: blob_bytes < 478, version or compat
 * version not 1, size field + 6 != blob_bytes, a write-buffer count != 16,
 * stream lengths that do not end at blob_bytes, or, in any of the three
 * streams, a chain of num_elements / 16 rows with an nbits above 64 or a row
 * that ends past its stream.  Nothing outside [blob_offset, blob_offset +
 * blob_bytes) is read.  Lookup (maybe_find_offset :65-103, _find_under
 * :289-305) on the rp (by_rp != 0) or Kafka column:
 *   1. decode the searched stream; the candidate is the last element <
 *      upper_bound, stopping at the first element >= upper_bound;
 *   2. without a candidate, or if it is element 16 * rows - 1: scan write-buffer
 *      slots [0, num_elements & 15) of the searched column the same way; a hit
 *      answers with the three write-buffer values of that slot
 *      (from_write_buffer = 1, ix = the slot); no hit and no candidate is
 *      RPGPU_RSINDEX_NONE (every other field 0);
 *   3. otherwise the answer is the candidate's value and element ix of the
 *      other two decoded streams (the file stream decodes with the blob's
 *      min_file_pos_step and base_file).
 * The answer seeds rpgpu_remote_read (remote_segment.cc:237-254): offset +=
 * file_pos, cur_rp_offset = rp_offset, cur_delta = rp_offset - kaf_offset.
 *
 * Hand vector: 60 headers, batch k has type 2 and last_offset_delta 2 if k ==
 * 7, else type 1 and last_offset_delta 0; size_bytes = 100 + k % 3; base
 * offsets consecutive from 1000 (the configuration batch takes three).  Base rp
 * 1000, base Kafka 990, initial delta 10, both steps 150.  29 samples, one row
 * per stream, blob 527 bytes (payload size 09020000); last_rp 1034, last_kaf
 * 1021, last_file 3231; streams
 *   rp    0b0206021c06020e020602fe0206020e02000000c00100
 *   Kafka 06be6004822318822718822318
 *   file  06335dcf743dd3f54cd7335dcf
 * first samples (1002, 992, 201), (1004, 994, 403), (1006, 996, 606), (1010,
 * 997, 807); rp write-buffer slots 13..15 are the stale 1030, 1032, 1034.
 * find_kaf(1003) -> element 5 (1014, 1001, 1212); find_kaf(1022) -> element 15
 * (1034, 1021, 3231); find_kaf(1030) -> write-buffer slot 3 (1042, 1029, 4039);
 * find_kaf(992) -> none; find_rp(1036) -> element 15 (slot 0 holds 1036, not
 * below the bound); find_rp(99999) -> slot 12 (1060, 1047, 5857). */
typedef struct rpgpu_rsindex_segment { /* one stream = one offset_index */
    uint32_t first_batch, batch_count; /* its descriptors, in file order                   */
    int64_t base_rp_offset;            /* offset_index initial_rp                          */
    int64_t base_kafka_offset;         /* offset_index initial_kaf                         */
    int64_t initial_delta;             /* remote_segment_index_builder initial_delta       */
    int64_t file_pos_step;             /* offset_index file_pos_step (64 KiB at call sites) */
    uint64_t sampling_step;            /* builder's sampling_step (64 KiB at call sites)   */
} rpgpu_rsindex_segment;               /* 48 bytes */

enum rpgpu_rsindex_status {
    RPGPU_RSINDEX_OK = 0,
    RPGPU_RSINDEX_NO_ROOM = 1,
    RPGPU_RSINDEX_BAD_BATCH = 2,
    RPGPU_RSINDEX_DELTA_ASSERT = 3
};
typedef struct rpgpu_rsindex_result {
    int32_t status;          /* enum rpgpu_rsindex_status                     */
    uint32_t samples;        /* offset_index _pos (num_elements)              */
    uint32_t rows;           /* rows flushed to each encoder: samples / 16    */
    uint32_t config_batches; /* type 2 and type 19 batches                    */
    uint32_t bad_batch;      /* BAD_BATCH: the first offending descriptor     */
    uint32_t rp_bytes, kaf_bytes, file_bytes; /* the three streams            */
    uint32_t out_bytes;      /* 478 + the three; 0 without a blob             */
    uint32_t reserved;
    int64_t final_delta;     /* _running_delta after the stream               */
    uint64_t stream_bytes;   /* sum of size_bytes: the parser's position      */
    uint64_t out_offset;     /* the blob in d_out, 16-byte aligned            */
} rpgpu_rsindex_result;      /* 64 bytes */

size_t rpgpu_rsindex_scratch_bytes(uint32_t n, uint32_t nsegs);
int32_t rpgpu_rsindex_plan_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_batch_desc* d_descs, uint32_t n,
                                  const rpgpu_rsindex_segment* d_segs, uint32_t nsegs,
                                  rpgpu_rsindex_result* d_results, uint64_t* d_totals, void* d_scratch,
                                  void* hip_stream);
int32_t rpgpu_rsindex_run_device(rpgpu_ctx* ctx, const rpgpu_rsindex_segment* d_segs, uint32_t nsegs,
                                 rpgpu_rsindex_result* d_results, uint8_t* d_out, uint64_t out_cap, void* d_scratch,
                                 void* hip_stream);

typedef struct rpgpu_rsindex_query {
    uint64_t blob_offset;    /* the blob in d_blobs                           */
    uint32_t blob_bytes;
    uint32_t by_rp;          /* != 0: find_rp_offset, else find_kaf_offset    */
    int64_t upper_bound;
    uint64_t reserved;
} rpgpu_rsindex_query;       /* 32 bytes */

enum rpgpu_rsindex_find_status { RPGPU_RSINDEX_FOUND = 0, RPGPU_RSINDEX_NONE = 1, RPGPU_RSINDEX_BAD_BLOB = 2 };
typedef struct rpgpu_rsindex_found { /* offset_index::find_result */
    int32_t status;          /* enum rpgpu_rsindex_find_status                */
    uint32_t from_write_buffer;
    uint64_t ix;             /* element of the decoded streams, or the slot   */
    int64_t rp_offset, kaf_offset, file_pos;
    uint64_t reserved;
} rpgpu_rsindex_found;       /* 48 bytes */

int32_t rpgpu_rsindex_find_device(rpgpu_ctx* ctx, const uint8_t* d_blobs, const rpgpu_rsindex_query* d_queries,
                                  uint32_t nq, rpgpu_rsindex_found* d_found, void* hip_stream);

/* ---- segment index life cycle: track, write, hydrate, seek ---------------------
 * What the broker does with a segment's offset/time index after recovery built
 * it, on index_state rows that stay on the device:
 *   rpgpu_segidx_track_device       segment_index::maybe_track (storage/segment_index.cc:98-120)
 *                                   + index_state::maybe_index (storage/index_state.cc:38-109)
 *                                   continued from any state;
 *   rpgpu_segidx_write_plan_device, segment_index::flush -> serde::to_iobuf(index_state)
 *   rpgpu_segidx_write_run_device   (segment_index.cc:237-263, index_state.cc:124-147):
 *                                   the bytes of the .base_index file;
 *   rpgpu_segidx_hydrate_device     segment_index::materialize_index_from_file
 *                                   (segment_index.cc:205-229, index_state.cc:149-219,
 *                                   index_state_serde_compat.h:46-101);
 *   rpgpu_segidx_find_device        find_nearest(offset) (segment_index.cc:140-163),
 *                                   find_nearest(timestamp) (:122-138, index_state.h:166-190),
 *                                   find_highest_timestamp_before (:306-323).
 * Integer-only: blobs, states and answers are the reference's, byte for byte.
 *
 * State i is one index_state plus the two segment_index members tracking needs.
 * Its entries are rows [entry_first, entry_first + entries) of one shared
 * rpgpu_index_entry array of nentries rows; entry_cap is the size of its slot.
 * Every entry point checks entry_first + entry_cap <= nentries and entries <=
 * entry_cap before it touches the array (a row that fails is *_BAD_STATE).
 *
 * Track: segment row s (first_batch, batch_count, file_base, step,
 * internal_topic; its base_offset and with_offset are ignored, the state's
 * hold) continues state s.  The recurrence is rpgpu_segment_index_device's,
 * started from the state: a fresh state is base_offset, with_offset, monotonic
 * = 1, last_batch_max_timestamp = -1 (model::timestamp{}), everything else 0.
 * position = desc.offset - file_base in wrapping 64-bit arithmetic; when the
 * first user-data batch follows a configuration batch that was indexed first,
 * entry 0's relative_time is rewritten with the batch's absolute, clamped
 * max_timestamp (index_state.cc:62-63).  Tracking stops in front of the first
 * batch whose verdict is not OK (status OK), whose base offset lies below the
 * state's (RPGPU_V_INDEX_OFFSET_BELOW_BASE), that is user data while
 * non_data_timestamps is set and entries != 1 (RPGPU_V_INDEX_NON_DATA_ASSERT),
 * or whose entry would not fit entry_cap (RPGPU_V_INDEX_NO_ROOM); the state
 * then is the state in front of that batch, `tracked` says how many batches
 * went in, and tracking can go on from there.  Nothing is written past the cap.
 *
 * Blob (current format; all little-endian, nothing aligned), n = entries:
 *     0  u8 5, u8 4        version, compat version
 *     2  u32 size          = blob bytes - 6
 *     6  u32 L             = 51 + 16 n
 *    10  tmp: u32 bitflags, i64 base_offset, max_offset, base_timestamp, max_timestamp,
 *             u32 n + n x u32 relative_offset, u32 n + n x u32 relative_time (raw),
 *             u32 n + n x u64 position, u8 monotonic, u8 with_offset, u8 non_data_timestamps
 *  10+L  u32 CRC32C(tmp)   crc::crc32c, seed 0, as rpgpu_crc32c_extend
 * Blob size = 65 + 16 n.  Plan: every row gets status, out_bytes and out_offset
 * (an exclusive scan of the OK blobs with every start on a 16-byte boundary);
 * d_totals[0] is the smallest out_cap that holds every OK blob.  A state whose
 * envelope (59 + 16 n bytes) exceeds UINT32_MAX is RPGPU_SEGIDX_TOO_BIG
 * (serde.h:539-541) and gets no blob.  Run: each blob whole, or not at all
 * and RPGPU_SEGIDX_NO_ROOM; nothing outside the OK blobs and nothing at or past
 * out_cap is written; a plan may be run any number of times, every run sets
 * every OK / NO_ROOM status again.
 *
 * Hydrate, file i = bytes [blob_offset, blob_offset + blob_bytes) of d_files at
 * any alignment, nothing outside is read; state i supplies entry_first and
 * entry_cap ((blob_bytes - 53) / 16 always suffices) and, on OK only, receives
 * the state and the entries; acc = 0, last_batch_max_timestamp = -1.  status:
 * OK; REBUILD (materialize_index returns false: empty file or a
 * serde::serde_exception); THROW (another exception escapes); NO_ROOM (more
 * entries than entry_cap, `entries` = the need); COLUMNS_DIFFER (below).
 * `reason` is the first event in the reference's order:
 *   empty file                                     REBUILD  EMPTY_FILE
 *   byte 0 < 3                                     REBUILD  UNSUPPORTED_VERSION
 *   byte 0 == 3, legacy (index_state_serde_compat.h:46-101):
 *       0 u8 3; 1 u32 size; 5 u64 checksum; 13 u32 bitflags; 17 four i64; 49 u32 n; 53 columns
 *     fewer than 4 bytes for size (consume_type)   THROW    V3_SHORT
 *     size != bytes after it                       REBUILD  V3_SIZE_MISMATCH
 *     any later field or column short              THROW    V3_SHORT
 *     XXH64(seed 0) of [13, 53 + 16 n) != checksum REBUILD  V3_CHECKSUM
 *     bytes left after the columns                 REBUILD  TRAILING
 *     -> monotonic = 0, with_offset = 0, non_data_timestamps = 0
 *   otherwise the serde envelope (serde.h:592-647, index_state.cc:179-218):
 *     fewer than 6 bytes                           REBUILD  HEADER_SHORT
 *     bytes left < size (a smaller size is fine)   REBUILD  SIZE_BEYOND
 *     byte 1 > 5                                   REBUILD  COMPAT_VERSION
 *     fewer than 4 bytes for L                     REBUILD  TMP_LEN_SHORT
 *     L > bytes left (share clamps, skip throws)   THROW    TMP_BEYOND
 *     fewer than 4 bytes for the CRC               REBUILD  CRC_SHORT
 *     CRC32C(tmp) != CRC                           REBUILD  CRC_MISMATCH
 *     a field of tmp short (each column carries
 *       its own count; byte 0 == 4 has no flags;
 *       bytes of tmp behind the last field are
 *       ignored)                                   REBUILD  FIELD_SHORT
 *     bytes left after the CRC                     REBUILD  TRAILING
 *     the three column counts differ               COLUMNS_DIFFER: the reference
 *       accepts the blob and later indexes past the shorter columns (undefined
 *       behaviour); here the caller rebuilds.  `entries` = the first count.
 * The hashed length of a legacy blob is 40 + 16 n: a multiple of 8 and at least
 * 40, so XXH64 runs its 32-byte stripe loop, the merge and 8-byte tail steps only.
 *
 * Find, one query per lane, restating the reference's loops (a hostile blob's
 * columns need not be sorted); lower_bound is std::lower_bound's halving loop:
 *   kind 0 find_nearest(offset o): o < base_offset or no entries -> NONE; needle =
 *     (uint32)(o - base_offset) (truncating); it = lower_bound(relative_offset),
 *     the last element if at the end; walk down to the first rel[i] <= needle.
 *   kind 1 find_nearest(timestamp t): t < base_timestamp or no entries -> NONE;
 *     raw = offset_time_index{t - base_timestamp, with_offset} (clamped); dist =
 *     lower_bound(relative_time); the answer is entry max(dist - 1, 0), dist may
 *     be n.  (The reference's end test compares iterators of two different
 *     vectors and never holds: a non-empty index always answers.)  The caller
 *     checks `monotonic` first (disk_log_impl.cc:1229).
 *   kind 2 find_highest_timestamp_before(t): base_timestamp > t or no entries ->
 *     NONE; from the last entry down, the first (int64)(uint32)offset_time() <
 *     t - base_timestamp; timestamp = base_timestamp + offset_time(), ix; offset
 *     and filepos 0.
 *   offset = base_offset + relative_offset; timestamp = base_timestamp +
 *   (uint32)offset_time(), offset_time() = raw - 2^31 as a uint32 when with_offset
 *   (a negative stored delta comes back as a large positive one, as in the
 *   reference).  A kind-0 answer seeds rpgpu_segment_read.offset += filepos.
 *   Cost: on sorted columns kind 0 and kind 1 are the binary search plus at most
 *   one step; kind 2 is the reference's linear scan from the last entry, O(n) by
 *   design.  On a hostile state (unsorted or constant columns) the downward
 *   walk of kind 0 is O(n) too: one lookup on a 2^28-entry state then reads
 *   every entry on one lane, so bound entry_cap by what a segment can hold.
 *
 * Hand vectors.  State: base_offset 1000, max_offset 1159, base_timestamp T =
 * 1700000000000, max_timestamp T + 9, with_offset 1, monotonic 1, non_data 0,
 * entries (0, dt 0, 0), (48, dt 3, 49143), (96, dt 6, 98286).  Current format,
 * 113 bytes, CRC 0a040bb7:
 *   05046b0000006300000000000000e80300000000000087040000000000000068e5cf8b0100000968e5cf8b01
 *   00000300000000000000300000006000000003000000000000800300008006000080030000000000000000000000
 *   f7bf000000000000ee7f010000000000010100b70b040a
 * Version 3, the same columns with with_offset 0 (raw times 0, 3, 6), 101 bytes,
 * XXH64 fd40fabf14e63b1d:
 *   03600000001d3be614bffa40fd00000000e80300000000000087040000000000000068e5cf8b0100000968e5cf8b
 *   010000030000000000000030000000600000000000000003000000060000000000000000000000f7bf000000000000
 *   ee7f010000000000
 * XXH64, seed 0: "" ef46db3751d8e999, "abc" 44bc2cf5ad770999, bytes 0..99
 * 6ac1e58032166597.  Lookups on the first state: offset 1047 -> entry 0 (1000,
 * T, 0); 1048 -> entry 1 (1048, T + 3, 49143); 5000 -> entry 2; 999 -> NONE; time
 * T + 3 -> entry 0; T -> entry 0; T + 100 -> entry 2; T - 1 -> NONE; before(T + 6)
 * -> T + 3, ix 1; before(T) -> NONE. */
typedef struct rpgpu_segidx_state {
    int64_t base_offset, max_offset, base_timestamp, max_timestamp; /* index_state */
    uint32_t bitflags;       /* index_state bitflags (unused by the broker)   */
    uint32_t entries;        /* rows used at d_entries + entry_first          */
    uint32_t entry_first, entry_cap; /* the state's slot in d_entries         */
    uint64_t acc;            /* segment_index _acc                            */
    int64_t last_batch_max_timestamp; /* segment_index _last_batch_max_timestamp */
    uint8_t monotonic;       /* batch_timestamps_are_monotonic                */
    uint8_t with_offset;     /* offset_delta_time                             */
    uint8_t non_data_timestamps;
    uint8_t reserved0;
    uint32_t reserved1;
    uint64_t reserved2;
} rpgpu_segidx_state;        /* 80 bytes */

typedef struct rpgpu_segidx_tracked {
    int32_t status;          /* RPGPU_V_OK, RPGPU_V_INDEX_OFFSET_BELOW_BASE, _NON_DATA_ASSERT, _NO_ROOM, _BAD_STATE */
    uint32_t tracked;        /* batches that went into the state              */
    uint32_t added;          /* entries appended                              */
    uint32_t reserved;
} rpgpu_segidx_tracked;      /* 16 bytes */

int32_t rpgpu_segidx_track_device(rpgpu_ctx* ctx, const rpgpu_batch_desc* d_descs,
                                  const rpgpu_batch_result* d_results, uint32_t n, const rpgpu_segment* d_segs,
                                  uint32_t nsegs, rpgpu_segidx_state* d_states, rpgpu_index_entry* d_entries,
                                  uint64_t nentries, rpgpu_segidx_tracked* d_tracked, void* hip_stream);

enum rpgpu_segidx_status {
    RPGPU_SEGIDX_OK = 0,
    RPGPU_SEGIDX_NO_ROOM = 1,
    RPGPU_SEGIDX_TOO_BIG = 2,        /* write: "envelope too big"                  */
    RPGPU_SEGIDX_REBUILD = 3,        /* hydrate: materialize_index returns false   */
    RPGPU_SEGIDX_THROW = 4,          /* hydrate: std::out_of_range escapes         */
    RPGPU_SEGIDX_COLUMNS_DIFFER = 5, /* hydrate: engine-only, see above            */
    RPGPU_SEGIDX_BAD_STATE = 6       /* a slot or a file outside the arrays given  */
};
enum rpgpu_segidx_reason {
    RPGPU_SEGIDX_R_NONE = 0,
    RPGPU_SEGIDX_R_EMPTY_FILE = 1,
    RPGPU_SEGIDX_R_UNSUPPORTED_VERSION = 2,
    RPGPU_SEGIDX_R_HEADER_SHORT = 3,
    RPGPU_SEGIDX_R_SIZE_BEYOND = 4,
    RPGPU_SEGIDX_R_COMPAT_VERSION = 5,
    RPGPU_SEGIDX_R_TMP_LEN_SHORT = 6,
    RPGPU_SEGIDX_R_TMP_BEYOND = 7,
    RPGPU_SEGIDX_R_CRC_SHORT = 8,
    RPGPU_SEGIDX_R_CRC_MISMATCH = 9,
    RPGPU_SEGIDX_R_FIELD_SHORT = 10,
    RPGPU_SEGIDX_R_TRAILING = 11,
    RPGPU_SEGIDX_R_V3_SIZE_MISMATCH = 12,
    RPGPU_SEGIDX_R_V3_SHORT = 13,
    RPGPU_SEGIDX_R_V3_CHECKSUM = 14,
    RPGPU_SEGIDX_R_COLUMNS_DIFFER = 15,
    RPGPU_SEGIDX_R_ENTRY_CAP = 16,
    RPGPU_SEGIDX_R_BAD_ROW = 17
};

typedef struct rpgpu_segidx_blob {
    int32_t status;          /* OK, NO_ROOM (run), TOO_BIG, BAD_STATE         */
    uint32_t entries;        /* the state's entries when it was planned       */
    uint64_t out_bytes;      /* 65 + 16 entries (up to 2^32 + 1); 0 without a blob */
    uint64_t out_offset;     /* the blob in d_out, 16-byte aligned            */
    uint64_t reserved;
} rpgpu_segidx_blob;         /* 32 bytes */

int32_t rpgpu_segidx_write_plan_device(rpgpu_ctx* ctx, const rpgpu_segidx_state* d_states, uint32_t nstates,
                                       uint64_t nentries, rpgpu_segidx_blob* d_blobs, uint64_t* d_totals,
                                       void* hip_stream);
int32_t rpgpu_segidx_write_run_device(rpgpu_ctx* ctx, const rpgpu_segidx_state* d_states, uint32_t nstates,
                                      const rpgpu_index_entry* d_entries, uint64_t nentries,
                                      rpgpu_segidx_blob* d_blobs, uint8_t* d_out, uint64_t out_cap,
                                      void* hip_stream);

typedef struct rpgpu_segidx_file {
    uint64_t blob_offset;    /* the file's bytes in d_files                   */
    uint64_t blob_bytes;
} rpgpu_segidx_file;         /* 16 bytes */

typedef struct rpgpu_segidx_hydrated {
    int32_t status;          /* enum rpgpu_segidx_status                      */
    int32_t reason;          /* enum rpgpu_segidx_reason                      */
    uint32_t version;        /* byte 0 of the file (0 for an empty file)      */
    uint32_t entries;        /* the first column count, once it was read      */
} rpgpu_segidx_hydrated;     /* 16 bytes */

int32_t rpgpu_segidx_hydrate_device(rpgpu_ctx* ctx, const uint8_t* d_files, uint64_t files_bytes,
                                    const rpgpu_segidx_file* d_rows, uint32_t nfiles,
                                    rpgpu_segidx_state* d_states, rpgpu_index_entry* d_entries,
                                    uint64_t nentries, rpgpu_segidx_hydrated* d_hydrated, void* hip_stream);

enum rpgpu_segidx_kind {
    RPGPU_SEGIDX_BY_OFFSET = 0,      /* find_nearest(model::offset)               */
    RPGPU_SEGIDX_BY_TIME = 1,        /* find_nearest(model::timestamp)            */
    RPGPU_SEGIDX_TIME_BEFORE = 2     /* find_highest_timestamp_before             */
};
typedef struct rpgpu_segidx_query {
    uint32_t state;          /* row of d_states                               */
    uint32_t kind;           /* enum rpgpu_segidx_kind                        */
    int64_t key;             /* the offset or the timestamp                   */
} rpgpu_segidx_query;        /* 16 bytes */

enum rpgpu_segidx_find_status { RPGPU_SEGIDX_FOUND = 0, RPGPU_SEGIDX_NONE = 1, RPGPU_SEGIDX_BAD_QUERY = 2 };
typedef struct rpgpu_segidx_found { /* segment_index::entry */
    int32_t status;          /* enum rpgpu_segidx_find_status                 */
    uint32_t ix;             /* the entry                                     */
    int64_t offset, timestamp;
    uint64_t filepos;
} rpgpu_segidx_found;        /* 32 bytes */

int32_t rpgpu_segidx_find_device(rpgpu_ctx* ctx, const rpgpu_segidx_state* d_states, uint32_t nstates,
                                 const rpgpu_index_entry* d_entries, uint64_t nentries,
                                 const rpgpu_segidx_query* d_queries, uint32_t nq, rpgpu_segidx_found* d_found,
                                 void* hip_stream);

/* ---- aborted transactions ahead of compaction ------------------------------
 * storage::internal::tx_reducer (storage/compaction_reducers.cc:322-428,
 * compaction_reducers.h:150-256), which rebuild_compaction_index
 * (storage/segment_utils.cc:508-555, called from self_compact_segment
 * :597-620) puts in front of index_rebuilder_reducer: the data batches of
 * aborted transactions, the commit and abort markers and the tx_prepare
 * batches never reach the compaction index, so no offset of theirs is in the
 * keep list and copy_data_segment_reducer drops them.
 *
 * Per scope (one segment, its batches in file order) and per batch b, with
 * ranges = stm_manager::aborted_tx_ranges(base, stable) in a min-heap on first:
 *   consume_aborted_txs(b.last_offset()) (:322-328): ongoing[r.pid] = r for
 *     every range with r.first <= b.last_offset(); r.last is not read;
 *   transactional control batch (:330-362): parse_control_batch
 *     (cluster/rm_stm.cc:258-279) vasserts type == raft_data, record_count == 1
 *     and key version == 0 and reads the control type, the second big-endian
 *     int16 of the first record's key; tx_abort (0) erases ongoing[pid] and is
 *     discarded, tx_commit (1) is discarded, any other value is kept;
 *   transactional raft_data batch (:364-372): discarded iff ongoing holds its
 *     pid = (producer_id, producer_epoch), header bytes [43, 51) and [51, 53);
 *   control batch without the transactional bit and not raft_data (:374-391):
 *     vassert tx_prepare (9) or tx_fence (10); prepare is discarded;
 *   everything else is delegated (:393-428).
 * The device form is in DESIGN.md §3 ("aborted transactions"). */
typedef struct rpgpu_tx_range { /* model::tx_range */
    int64_t producer_id;
    int16_t producer_epoch;
    uint16_t reserved0;
    uint32_t reserved1;
    int64_t first;
    int64_t last;
} rpgpu_tx_range;               /* 32 bytes */

/* rpgpu_tx_scope.flags */
#define RPGPU_TX_NON_TRANSACTIONAL 1u /* !has_tx_stm(): every batch is delegated (compaction_reducers.cc:394-396) */
#define RPGPU_TX_FILTER_RANGES 2u     /* only ranges with last >= from && first <= to take part
                                         (filter_intersecting, cluster/rm_stm.cc:1948-1962): a caller passes a
                                         partition's aborted list once for all its segments */
typedef struct rpgpu_tx_scope {
    uint32_t first_batch, batch_count; /* its descriptors, in file order; scopes are disjoint      */
    uint32_t range_first, range_count; /* rows of d_ranges; several scopes may name the same rows  */
    int64_t from, to;                  /* RPGPU_TX_FILTER_RANGES                                   */
    uint32_t flags;
    uint32_t reserved;
} rpgpu_tx_scope;                      /* 40 bytes */

/* d_discard[b] */
enum rpgpu_tx_discard {
    RPGPU_TX_DELEGATED = 0,
    RPGPU_TX_ABORTED_DATA = 1,
    RPGPU_TX_MARKER = 2,      /* tx_commit or tx_abort                       */
    RPGPU_TX_PREPARE = 3,
    RPGPU_TX_NOT_REACHED = 4, /* behind the scope's stop, or in no scope     */
};

enum rpgpu_tx_status {
    RPGPU_TX_OK = 0,
    RPGPU_TX_BAD_BATCH = 1,       /* a verdict other than RPGPU_V_OK: the scope stops there, as a
                                     segment of rpgpu_segment_index_device does                    */
    RPGPU_TX_ASSERT = 2,          /* one of the vasserts above: the reference aborts               */
    RPGPU_TX_KEY_SHORT_THROW = 3, /* the control key is null or shorter than the int16 it is asked
                                     for: decoder::read_int16 -> iobuf_parser::consume_be_type ->
                                     io_iterator_consumer::consume_type throws std::out_of_range
                                     (bytes/details/io_iterator_consumer.h:88-97), which ends the
                                     consume ("Error rebuilding index", segment_utils.cc:528-533).
                                     A key of 2 or 3 bytes whose version is not 0 is the vassert. */
    RPGPU_TX_NOT_INDEXED = 4,     /* a control batch without its index entry                       */
    RPGPU_TX_BAD_SCOPE = 5,       /* rows outside the arrays: no flag of the scope is written      */
};

typedef struct rpgpu_tx_stats { /* tx_reducer::stats (compaction_reducers.h:201-224) */
    uint64_t tx_data_batches_discarded;
    uint64_t tx_control_batches_discarded;
    uint64_t non_tx_control_batches_discarded;
    uint64_t all_batches_discarded;
    uint64_t num_aborted_txes; /* after RPGPU_TX_FILTER_RANGES                    */
    uint64_t all_batches;      /* 0 under RPGPU_TX_NON_TRANSACTIONAL              */
    uint32_t processed;        /* batches in front of the stop                    */
    int32_t status;            /* enum rpgpu_tx_status                            */
    uint32_t bad_batch;        /* the batch that stopped the scope (index into d_descs), else UINT32_MAX */
    uint32_t reserved;
} rpgpu_tx_stats;              /* 64 bytes */

/* Input: a validated and indexed arena, as rpgpu_compaction_keep_device takes.
 * d_discard[n]: enum rpgpu_tx_discard per batch.  d_stats[nscopes].  Whether a
 * batch stops its scope depends on that batch alone; flags and counters are
 * those of the batches in front of it, the offender and everything behind it
 * get RPGPU_TX_NOT_REACHED.  Under RPGPU_TX_NON_TRANSACTIONAL only a verdict
 * stops the scope.  Every output byte is a function of the input.
 * d_scratch: rpgpu_compaction_tx_scratch_bytes(n, nranges) bytes. */
size_t rpgpu_compaction_tx_scratch_bytes(uint32_t n, uint32_t nranges);
int32_t rpgpu_compaction_tx_filter_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                          const rpgpu_batch_result* d_results, uint32_t n,
                                          const rpgpu_record_index* d_index, uint64_t index_cap,
                                          const rpgpu_tx_scope* d_scopes, uint32_t nscopes,
                                          const rpgpu_tx_range* d_ranges, uint32_t nranges, uint8_t* d_discard,
                                          rpgpu_tx_stats* d_stats, void* d_scratch, void* hip_stream);

/* rpgpu_compaction_keep_device behind the filter.  d_discard: the filter's
 * flags, or NULL for none.  The records of a batch flagged 1..3 are not
 * inserted into the key table (index_rebuilder_reducer never sees them); their
 * own flag is still "is (scope, offset) in the keep set", because
 * copy_data_segment_reducer decides by offset alone
 * (compaction_reducers.h:130-133): 0 in a well-formed segment, so the rewrite
 * reports RPGPU_COMPACT_DROPPED, and 1 for a hostile duplicate of a kept offset,
 * exactly as the reference keeps it. */
int32_t rpgpu_compaction_keep_tx_device(rpgpu_ctx* ctx, const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                        const rpgpu_batch_result* d_results, uint32_t n,
                                        const rpgpu_record_index* d_index, uint64_t index_cap,
                                        const uint8_t* d_discard, uint8_t* d_keep, uint64_t* d_nkeys,
                                        void* d_scratch, void* hip_stream);

/* ---- produce batches from records -------------------------------------------
 * Replaces kafka::client::client::produce_records (kafka/client/client.cc:231-271),
 * which is behind the REST proxy's POST /topics/{topic}
 * (pandaproxy/rest/handlers.cc:198-199): a partition per record
 * (kafka/client/partitioners.cc:25-109), one storage::record_batch_builder per
 * partition, add_raw_kw, build() (storage/record_batch_builder.cc:29-102).
 * The JSON parse and the base64 decode stay on the host: the
 * engine takes decoded rows.
 *
 * A call holds many independent requests; one request is one produce_records
 * call (one topic, one partitioner state) and owns the next `nrows` rows, the
 * record_essences in request order.  The partition of a row is
 * default_partitioner, the first rule that answers:
 *  1. RPGPU_PRODUCE_HAS_PARTITION: the row's id as it is (identity_partitioner
 *     checks nothing: a negative id or one >= partition_count gets a batch of
 *     its own; the broker rejects it later);
 *  2. a key that is present and not empty: murmur2(key, len, 0x9747b28c) %
 *     partition_count (hashing/murmur.cc:384-432, hashing/murmur.h:38-44):
 *     4-byte little-endian words, a tail of 3 / 2 / 1 bytes with fall-through,
 *     the modulus on the unsigned hash (Java clients mask the sign bit first;
 *     the reference does not, and neither does the engine);
 *  3. otherwise (rr_initial + k) % partition_count, k = the earlier rows of the
 *     request that reached this rule (roundrobin_partitioner, _next++).
 * rr_next = rr_initial + the rows that reached rule 3; the caller carries it
 * to the topic's next request.  partition_count 0 stands for a topic that is
 * not in the client's cache: partition_for throws topic_error and
 * produce_records assigns partition 0 (client.cc:240-246), so every row without
 * its own id goes to partition 0 and the counter does not advance.
 *
 * Rows of one request with the same partition form one batch, in request order
 * (offset delta = rank in the group).  The reference emits a request's
 * partitions in absl::node_hash_map iteration order, which is no function of
 * the input; the engine's order is ascending request, then ascending partition
 * id as a signed int32 (unpinned).
 *
 * The batch is record_batch_builder::build() with nothing set: on-disk layout,
 * size_bytes 61 + body, base_offset 0, type raft_data (1), attrs 0,
 * last_offset_delta n - 1, record_count n, first_timestamp = max_timestamp =
 * the request's now_ms (the caller's model::timestamp::now()), producer id /
 * epoch / base sequence -1, crc = crc_record_batch, header_crc =
 * internal_header_only_crc.  Record d is vint(len) 00 00 vint(d) vint(klen)
 * key vint(vlen | -1) value 00.  produce_records passes key.value_or(iobuf{})
 * (client.cc:257-260): an absent key is encoded as length 0, never -1; a null
 * value is -1.  Headers are always empty on this path (the proxy's handler
 * never sets them): the row format has none.
 *
 * Hand vectors.  murmur2: "21" c5f2f8ec, "foobar" d0e47bbe,
 * "a-little-bit-long-string" c53b1da0, "a-little-bit-longer-string" a768c9c3,
 * "lkjh234lh9fiuh90y23oiuhsafujhadof229phr9h19h89h8" fc7d49cd, "abc" 1c94221b,
 * "the key" c4c66957 (% 6 = 1), "k" a291e5e0 (% 6 = 4), "" 106e08d9.
 * One request, partition_count 6, rr_initial 5, rows r0 (id 4, no key, "v0"),
 * r1 (key "the key", null value), r2 (no key, "hi"), r3 (key of length 0,
 * value of length 0), r4 (key "k", value "v"): rr_next 7 and four batches,
 *   partition 0 (r3)      0c 00 00 00 00 00 00
 *   partition 1 (r1)      1a 00 00 00 0e 74 68 65 20 6b 65 79 01 00
 *   partition 4 (r0, r4)  10 00 00 00 00 04 76 30 00 10 00 00 02 02 6b 02 76 00
 *   partition 5 (r2)      10 00 00 00 00 04 68 69 00 */
#define RPGPU_PRODUCE_HAS_PARTITION 1u
typedef struct rpgpu_produce_row {
    uint64_t key_off, val_off; /* into d_data; ignored when the length is <= 0 */
    int32_t key_len;           /* -1 no key (encoded as an empty one)          */
    int32_t val_len;           /* -1 null value                                */
    int32_t partition;         /* used iff flags & RPGPU_PRODUCE_HAS_PARTITION */
    uint32_t flags;
} rpgpu_produce_row;           /* 32 bytes */
typedef struct rpgpu_produce_request { /* requests tile the rows in order */
    int64_t now_ms;
    uint32_t nrows;
    uint32_t partition_count; /* 0: topic not in the cache */
    int32_t rr_initial;
    uint32_t pad;
} rpgpu_produce_request;      /* 24 bytes */

/* The request statuses are the engine's own guard rails (the reference's inputs
 * are typed, so they are unpinned).  A request keeps the first that applies, in
 * this order; a request whose status is not OK emits no batch and the other
 * requests are unaffected. */
enum rpgpu_produce_status {
    RPGPU_PRODUCE_OK = 0,
    RPGPU_PRODUCE_BAD_REQUEST = 1, /* every request of the call: the requests' nrows do not sum to
                                      nrows.  One request: partition_count > INT32_MAX, rr_initial
                                      < 0 (both ahead of BAD_ROW), or rr_initial + its rule-3 rows
                                      pass INT32_MAX (behind BAD_ROW; signed overflow in the
                                      reference)                                                  */
    RPGPU_PRODUCE_BAD_ROW = 2,     /* a length below -1, or a key / value range outside data_bytes */
    RPGPU_PRODUCE_TOO_LARGE = 3,   /* a body that would make size_bytes pass INT32_MAX             */
    RPGPU_PRODUCE_OUT_OVERFLOW = 4 /* out_cap is too small for the request's batches               */
};
typedef struct rpgpu_produce_result { /* per request */
    int32_t status;
    int32_t rr_next;      /* OK: rr_initial + the rule-3 rows; else rr_initial                     */
    uint32_t first_batch; /* OK: the request's batches are rows [first_batch, first_batch + nbatches)
                             of d_batches; else 0                                                  */
    uint32_t nbatches;    /* 0 unless OK; a request with zero rows is OK with zero batches         */
} rpgpu_produce_result;   /* 16 bytes */
typedef struct rpgpu_produce_batch { /* per emitted batch */
    uint32_t request;     /* UINT32_MAX in the unused rows */
    int32_t partition;
    uint32_t record_count;
    uint32_t pad;
    uint64_t out_offset; /* the batch in d_out (64-byte aligned) */
    uint64_t out_len;    /* 61 + body; 0 in the unused rows      */
} rpgpu_produce_batch;   /* 32 bytes */

/* The stream and alignment rules of rpgpu_legacy_*: plan, then run with the
 * same d_scratch, on one stream; a plan may be run any number of times.  Plan:
 * *d_out_bytes = the output slots of the requests that are OK so far,
 * *d_nbatches = their batches (<= nrows, so a caller may size the per-batch
 * arrays by nrows without reading the plan back).  Run: d_out is 16-byte
 * aligned (RPGPU_EINVAL otherwise) and holds *d_out_bytes +
 * RPGPU_ARENA_TAIL_PAD bytes; out_cap is the buffer's size, pad included.  A
 * request whose last slot does not end RPGPU_ARENA_TAIL_PAD bytes in front of
 * out_cap (the validation reads that far past a batch) gets OUT_OVERFLOW; slots
 * ascend with the request, so those are the last ones, and nothing is written
 * past out_cap.  d_req_results[nrequests]; d_batches, d_out_descs and
 * d_out_results have nrows rows each and all of them are written: the emitted
 * batches first, in order, then unused rows (out_len 0; descriptor length 0
 * and ops 0; verdict STREAM_SHORT, as rpgpu_decomp_run_device leaves a batch
 * it did not rewrite).  d_row_batch[i] / d_row_delta[i]: the row of d_batches
 * and the offset delta row i received (produce_batcher::handle_response answers
 * per record), UINT32_MAX for the rows of a refused request.  d_out_descs (ops
 * CRC | HDRCRC | RECRC | PARSE | INDEX, the descriptor's partition = the batch's
 * partition id), d_out_results, d_index (capacity needed: nrows) and
 * *d_index_used are written exactly as rpgpu_legacy_run_device /
 * rpgpu_decomp_run_device write them, so the output feeds rpgpu_run_device,
 * rpgpu_kafka_serialize_device, rpgpu_compress_* and rpgpu_append_* unchanged.
 * nrows and nrequests are at most 2^30 (RPGPU_EINVAL).
 * d_scratch: rpgpu_produce_scratch_bytes(nrows, nrequests) bytes. */
size_t rpgpu_produce_scratch_bytes(uint32_t nrows, uint32_t nrequests);
int32_t rpgpu_produce_plan_device(rpgpu_ctx* ctx, const rpgpu_produce_row* d_rows, uint32_t nrows,
                                  const rpgpu_produce_request* d_requests, uint32_t nrequests,
                                  const uint8_t* d_data, uint64_t data_bytes, uint64_t* d_out_bytes,
                                  uint32_t* d_nbatches, void* d_scratch, void* hip_stream);
int32_t rpgpu_produce_run_device(rpgpu_ctx* ctx, const rpgpu_produce_row* d_rows, uint32_t nrows,
                                 const rpgpu_produce_request* d_requests, uint32_t nrequests,
                                 const uint8_t* d_data, uint64_t data_bytes, rpgpu_produce_result* d_req_results,
                                 rpgpu_produce_batch* d_batches, uint32_t* d_row_batch, uint32_t* d_row_delta,
                                 uint8_t* d_out, uint64_t out_cap, rpgpu_batch_desc* d_out_descs,
                                 rpgpu_batch_result* d_out_results, rpgpu_record_index* d_index,
                                 uint64_t index_cap, uint64_t* d_index_used, void* d_scratch, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* RPGPU_H */
