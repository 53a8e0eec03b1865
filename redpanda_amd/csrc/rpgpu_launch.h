// rpgpu_launch.h — every launcher and scratch-size function that one
// translation unit defines and another calls, declared once.  The defining
// .hip file includes this header too: a definition whose return type differs
// does not compile, and one whose parameters differ is a new overload that
// leaves the prototype here undefined, which the link of librpgpu.so rejects
// (-Wl,--no-undefined, redpanda_amd/_build.py).
#ifndef RPGPU_LAUNCH_H
#define RPGPU_LAUNCH_H

#include "rpgpu_internal.h"

// after a kernel launch, inside a launcher: return the launch's error, if any
#define RPGPU_LAUNCH_CHECK()                        \
    do {                                            \
        hipError_t e_ = hipGetLastError();          \
        if (e_ != hipSuccess) return e_;            \
    } while (0)

namespace rpgpu {

// workgroups of 256 threads for one wavefront per item (wave_item, rpgpu_device.h)
inline uint32_t wave_grid(uint32_t n) { return (uint32_t)(((uint64_t)n + 3) / 4); }

// ---- rpgpu_kernels.hip
hipError_t launch_validate(const rpgpu_batch_desc* d_descs, uint32_t n, const uint8_t* d_data,
                           rpgpu_batch_result* d_res, rpgpu_record_index* d_index, uint64_t index_cap,
                           uint64_t* d_index_used, void* d_scratch, const uint32_t* d_tables, int grid,
                           hipStream_t s, const Overlap* ov);
hipError_t launch_plan(const rpgpu_batch_desc* d_descs, uint32_t n, const uint8_t* d_data,
                       uint64_t* d_index_used, void* d_scratch, hipStream_t s);
hipError_t launch_run(const rpgpu_batch_desc* d_descs, uint32_t n, const uint8_t* d_data,
                      rpgpu_batch_result* d_res, rpgpu_record_index* d_index, uint64_t index_cap,
                      const void* d_scratch, const uint32_t* d_tables, int grid, hipStream_t s,
                      const Overlap* ov);
// block_sum[0, nb) becomes its exclusive scan (one workgroup); the total into *total unless null
hipError_t launch_block_scan(uint64_t* block_sum, uint32_t nb, uint64_t* total, hipStream_t s);
size_t validate_scratch_bytes(uint32_t n);
hipError_t validate_occupancy(int* blocks_per_cu);
hipError_t launch_crc_ranges(const uint8_t* d_data, const uint64_t* d_off, const uint32_t* d_len,
                             const uint32_t* d_seed, uint32_t n, uint32_t* d_out, const uint32_t* d_tables,
                             int grid, hipStream_t s);
hipError_t launch_kafka_codes(const rpgpu_batch_result* d_res, uint32_t n, uint32_t batch_max_bytes,
                              int32_t* d_codes, hipStream_t s);
hipError_t launch_segment_parse(const uint8_t* d_data, const rpgpu_segment_read* d_reads, uint32_t n,
                                rpgpu_segment_parse_result* d_res, rpgpu_batch_desc* d_descs,
                                const uint32_t* d_tables, int grid, hipStream_t s);
hipError_t launch_remote_parse(const uint8_t* d_data, const rpgpu_remote_read* d_reads, uint32_t n,
                               rpgpu_remote_parse_result* d_res, rpgpu_batch_desc* d_descs, int64_t* d_kafka_base,
                               int64_t* d_gaps, const uint32_t* d_tables, int grid, hipStream_t s);

// ---- rpgpu_index.hip, rpgpu_summary.hip, rpgpu_stamp.hip, rpgpu_fetch.hip
hipError_t launch_segment_index(const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res,
                                const rpgpu_segment* d_segs, uint32_t nsegs, rpgpu_segment_state* d_states,
                                rpgpu_index_entry* d_entries, hipStream_t s);
hipError_t launch_summaries(const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res, uint32_t n,
                            uint32_t part_lo, uint32_t nparts, int64_t* d_out, hipStream_t s, int64_t* d_partial,
                            int cu_count);
size_t summary_scratch_bytes(int cu_count);
hipError_t launch_set_max_timestamp(const rpgpu_batch_desc* d_descs, uint32_t n, uint8_t* d_data,
                                    rpgpu_batch_result* d_res, uint32_t ts_type, int64_t ts, uint32_t* d_changed,
                                    hipStream_t s);
hipError_t launch_kafka_serialize(const uint8_t* d_data, const rpgpu_batch_desc* d_descs, const int64_t* d_terms,
                                  uint32_t n, uint8_t* d_out, const rpgpu_fetch_range* d_ranges, uint32_t nranges,
                                  rpgpu_fetch_summary* d_sums, hipStream_t s);

// ---- rpgpu_sets.hip
size_t sets_scratch_bytes(uint32_t n);
hipError_t launch_sets_plan(const rpgpu_batch_desc* d_sets, uint32_t n, const uint8_t* d_data,
                            uint64_t* d_nbatches, void* d_scratch, hipStream_t s);
hipError_t launch_sets_run(const rpgpu_batch_desc* d_sets, uint32_t n, const uint8_t* d_data,
                           rpgpu_record_set_result* d_set_res, rpgpu_batch_desc* d_bdescs, uint32_t nbatches,
                           rpgpu_batch_result* d_bres, rpgpu_record_index* d_index, uint64_t index_cap,
                           uint64_t* d_index_used, void* d_scratch, void* d_vscratch, const uint32_t* d_tables,
                           int grid, hipStream_t s, const Overlap* ov);

// ---- rpgpu_decomp.hip
size_t decomp_scratch_bytes(uint32_t n, uint32_t ws_cap);
size_t decomp_counter_offset(uint32_t n, uint32_t ws_cap);
hipError_t launch_decomp_plan(const rpgpu_batch_desc* d_descs, uint32_t n, const uint8_t* d_data,
                              const rpgpu_batch_result* d_vres, uint64_t* d_out_bytes, void* d_scratch,
                              uint64_t max_decoded, uint32_t ws_cap, uint32_t zmode, hipStream_t s);
hipError_t launch_decomp_run(const rpgpu_batch_desc* d_descs, uint32_t n, const uint8_t* d_data,
                             const rpgpu_batch_result* d_vres, rpgpu_decomp_result* d_dres, uint8_t* d_out,
                             uint64_t out_cap, rpgpu_batch_desc* d_out_descs, rpgpu_batch_result* d_vres2,
                             rpgpu_record_index* d_index, uint64_t index_cap, uint64_t* d_index_used,
                             void* d_scratch, const uint32_t* d_tables, int grid, uint32_t ws_cap, uint32_t zmode,
                             hipStream_t s, const Overlap* ov, const DecompStreams* ds, const uint32_t* plan_counts);
hipError_t launch_uncompress_bound(uint32_t codec, const uint8_t* d_in, uint64_t n, uint64_t* d_res,
                                   hipStream_t s);
hipError_t launch_uncompress_one(uint32_t codec, const uint8_t* d_in, uint64_t n, uint8_t* d_out, uint64_t cap,
                                 uint64_t* d_res, uint8_t* d_lits, hipStream_t s);
size_t uncompress_scratch_bytes();

// ---- rpgpu_compress.hip
size_t compress_scratch_bytes(uint32_t n);
hipError_t launch_compress_plan(const rpgpu_batch_result* d_vres, uint32_t n, uint32_t codec, uint64_t* d_out_bytes,
                                void* d_scratch, hipStream_t s);
hipError_t launch_compress_run(const rpgpu_batch_desc* d_descs, uint32_t n, const uint8_t* d_data,
                               const rpgpu_batch_result* d_vres, uint32_t codec, rpgpu_decomp_result* d_cres,
                               uint8_t* d_out, uint64_t out_cap, rpgpu_batch_desc* d_out_descs,
                               rpgpu_batch_result* d_vres2, void* d_scratch, const uint32_t* d_tables, int grid,
                               hipStream_t s);

// ---- rpgpu_compact.hip, rpgpu_compact_rw.hip
size_t compaction_scratch_bytes(uint64_t index_cap);
hipError_t launch_compaction_keep(const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                  const rpgpu_batch_result* d_res, uint32_t n, const rpgpu_record_index* d_index,
                                  uint64_t index_cap, const uint8_t* d_discard, uint8_t* d_keep, uint64_t* d_nkeys,
                                  void* d_scratch, hipStream_t s);
hipError_t launch_timequery(const rpgpu_batch_result* d_res, uint32_t n, const rpgpu_record_index* d_index,
                            const rpgpu_timequery* d_q, uint32_t nq, rpgpu_timequery_result* d_out, hipStream_t s);
size_t compaction_rewrite_scratch_bytes(uint32_t n);
hipError_t launch_compact_rw_plan(const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                  const rpgpu_batch_result* d_res, uint32_t n, uint64_t index_cap,
                                  const uint8_t* d_keep, uint64_t* d_out_bytes, void* d_scratch, hipStream_t s);
hipError_t launch_compact_rw_run(const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                                 const rpgpu_batch_result* d_res, uint32_t n, const uint8_t* d_keep,
                                 rpgpu_compact_result* d_cres, uint8_t* d_out, uint64_t out_cap,
                                 rpgpu_batch_desc* d_out_descs, rpgpu_batch_result* d_out_res,
                                 rpgpu_record_index* d_out_index, uint64_t out_index_cap, uint64_t* d_out_index_used,
                                 void* d_scratch, const uint32_t* d_tables, int grid, hipStream_t s);

// ---- rpgpu_legacy.hip
size_t legacy_scratch_bytes(uint32_t n);
hipError_t launch_legacy_plan(const rpgpu_batch_desc* d_sets, uint32_t n, const uint8_t* d_data,
                              uint64_t* d_out_bytes, uint64_t* d_records_total, void* d_scratch, hipStream_t s);
hipError_t launch_legacy_run(const rpgpu_batch_desc* d_sets, uint32_t n, const uint8_t* d_data, int64_t now_ms,
                             rpgpu_legacy_result* d_lres, uint8_t* d_out, uint64_t out_cap,
                             rpgpu_batch_desc* d_out_descs, rpgpu_batch_result* d_vres2, rpgpu_record_index* d_index,
                             uint64_t index_cap, uint64_t* d_index_used, void* d_scratch, const uint32_t* d_tables,
                             const uint32_t* d_tables32, int grid, uint32_t lane_max, hipStream_t s);

// ---- rpgpu_pp.hip
size_t pp_fetch_scratch_bytes(uint32_t n, uint32_t nranges, uint32_t nresponses);
hipError_t launch_pp_fetch_plan(const rpgpu_batch_result* d_results, uint32_t n, const rpgpu_record_index* d_index,
                                const uint8_t* d_topics, uint32_t topics_len, const rpgpu_pp_range* d_ranges,
                                uint32_t nranges, const rpgpu_pp_response* d_responses, uint32_t nresponses,
                                rpgpu_pp_result* d_out_results, uint64_t* d_out_bytes, void* d_scratch,
                                hipStream_t s);
hipError_t launch_pp_fetch_run(const uint8_t* d_data, const rpgpu_batch_desc* d_descs,
                               const rpgpu_batch_result* d_results, uint32_t n, const rpgpu_record_index* d_index,
                               const uint8_t* d_topics, const rpgpu_pp_range* d_ranges, uint32_t nranges,
                               const rpgpu_pp_response* d_responses, uint32_t nresponses, uint8_t* d_out,
                               uint64_t out_cap, rpgpu_pp_result* d_out_results, void* d_scratch, uint32_t lane_max,
                               hipStream_t s);

// ---- rpgpu_append.hip
size_t append_scratch_bytes(uint32_t n, uint32_t nlogs);
hipError_t launch_append_plan(const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res, uint32_t n,
                              const int32_t* d_codes, const rpgpu_append_log* d_logs, uint32_t part_lo,
                              uint32_t nlogs, rpgpu_append_batch* d_rows, rpgpu_append_log_result* d_lres,
                              uint64_t* d_totals, void* d_scratch, hipStream_t s);
hipError_t launch_append_run(const uint8_t* d_data, const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res,
                             uint32_t n, uint32_t part_lo, uint32_t nlogs, const rpgpu_append_batch* d_rows,
                             rpgpu_append_log_result* d_lres, uint8_t* d_out, uint64_t out_cap,
                             rpgpu_batch_desc* d_out_descs, rpgpu_batch_result* d_out_res, uint32_t rows_cap,
                             rpgpu_append_segment* d_segments, uint32_t seg_cap, void* d_scratch,
                             const uint32_t* d_tables, hipStream_t s);

// ---- rpgpu_rsindex.hip
size_t rsindex_scratch_bytes(uint32_t n, uint32_t nsegs);
hipError_t launch_rsindex_plan(const uint8_t* d_data, const rpgpu_batch_desc* d_descs, uint32_t n,
                               const rpgpu_rsindex_segment* d_segs, uint32_t nsegs, rpgpu_rsindex_result* d_results,
                               uint64_t* d_totals, void* d_scratch, hipStream_t s);
hipError_t launch_rsindex_run(const rpgpu_rsindex_segment* d_segs, uint32_t nsegs, rpgpu_rsindex_result* d_results,
                              uint8_t* d_out, uint64_t out_cap, void* d_scratch, hipStream_t s);
hipError_t launch_rsindex_find(const uint8_t* d_blobs, const rpgpu_rsindex_query* d_queries, uint32_t nq,
                               rpgpu_rsindex_found* d_found, hipStream_t s);

// ---- rpgpu_segidx.hip
hipError_t launch_segidx_track(const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res, uint32_t n,
                               const rpgpu_segment* d_segs, uint32_t nsegs, rpgpu_segidx_state* d_states,
                               rpgpu_index_entry* d_entries, uint64_t nentries, rpgpu_segidx_tracked* d_tracked,
                               hipStream_t s);
hipError_t launch_segidx_write_plan(const rpgpu_segidx_state* d_states, uint32_t nstates, uint64_t nentries,
                                    rpgpu_segidx_blob* d_blobs, uint64_t* d_totals, hipStream_t s);
hipError_t launch_segidx_write_run(const rpgpu_segidx_state* d_states, uint32_t nstates,
                                   const rpgpu_index_entry* d_entries, uint64_t nentries, rpgpu_segidx_blob* d_blobs,
                                   uint8_t* d_out, uint64_t out_cap, const uint32_t* d_tables, hipStream_t s);
hipError_t launch_segidx_hydrate(const uint8_t* d_files, uint64_t files_bytes, const rpgpu_segidx_file* d_rows,
                                 uint32_t nfiles, rpgpu_segidx_state* d_states, rpgpu_index_entry* d_entries,
                                 uint64_t nentries, rpgpu_segidx_hydrated* d_hydrated, const uint32_t* d_tables,
                                 hipStream_t s);
hipError_t launch_segidx_find(const rpgpu_segidx_state* d_states, uint32_t nstates, const rpgpu_index_entry* d_entries,
                              uint64_t nentries, const rpgpu_segidx_query* d_queries, uint32_t nq,
                              rpgpu_segidx_found* d_found, hipStream_t s);

// ---- rpgpu_txfilter.hip
size_t compaction_tx_scratch_bytes(uint32_t n, uint32_t nranges);
hipError_t launch_tx_filter(const uint8_t* d_data, const rpgpu_batch_desc* d_descs, const rpgpu_batch_result* d_res,
                            uint32_t n, const rpgpu_record_index* d_index, uint64_t index_cap,
                            const rpgpu_tx_scope* d_scopes, uint32_t nscopes, const rpgpu_tx_range* d_ranges,
                            uint32_t nranges, uint8_t* d_discard, rpgpu_tx_stats* d_stats, void* d_scratch,
                            hipStream_t s);

// ---- rpgpu_produce.hip
size_t produce_scratch_bytes(uint32_t nrows, uint32_t nrequests);
hipError_t launch_produce_plan(const rpgpu_produce_row* d_rows, uint32_t n, const rpgpu_produce_request* d_requests,
                               uint32_t nreq, const uint8_t* d_data, uint64_t data_bytes, uint64_t* d_out_bytes,
                               uint32_t* d_nbatches, void* d_scratch, hipStream_t s);
hipError_t launch_produce_run(const rpgpu_produce_row* d_rows, uint32_t n, const rpgpu_produce_request* d_requests,
                              uint32_t nreq, const uint8_t* d_data, rpgpu_produce_result* d_req_results,
                              rpgpu_produce_batch* d_batches, uint32_t* d_row_batch, uint32_t* d_row_delta,
                              uint8_t* d_out, uint64_t out_cap, rpgpu_batch_desc* d_out_descs,
                              rpgpu_batch_result* d_vres2, rpgpu_record_index* d_index, uint64_t index_cap,
                              uint64_t* d_index_used, void* d_scratch, const uint32_t* d_tables, int grid,
                              hipStream_t s);

}  // namespace rpgpu
#endif
