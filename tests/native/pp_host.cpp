// pp_host.cpp — the shared core of the REST proxy fetch rendering
// (redpanda_amd/csrc/rpgpu_pp.h: sizes, verdicts, base64, decimals, the object
// writer) compiled for the host and run over an arena file, pass by pass as
// the kernels of rpgpu_pp.hip run it.  TEST INFRASTRUCTURE, built and run by
// tests/test_pandaproxy_fetch.py, plainly and with -fsanitize=address,undefined.
//
//   pp_host render IN OUT   every response: its rpgpu_pp_result row (32 bytes),
//                           then its out_len bytes.  Each response is written
//                           into a heap block of exactly out_len bytes, so a
//                           byte past it is an ASan finding.  stdout: the
//                           number of fields on the lane and on the wave path.
//   pp_host fields IN OUT   every non-empty key and value of the index, in
//                           index order, encoded alone into a block of exactly
//                           b64_len bytes by the lane path, and by the 64 lanes
//                           of the wave path at each of the 16 destination
//                           alignments (must equal the lane path's and leave
//                           the bytes in front alone).  OUT: the encodings.
//
// IN (little-endian): uint32 n, nindex, topics_len, nranges, nresponses,
// reserved; uint64 data_len; then data, descs[n], results[n], index[nindex],
// topics, ranges[nranges], responses[nresponses].
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rpgpu_pp.h"

namespace {

template <class T>
bool read_vec(FILE* f, std::vector<T>& v, size_t count) {
    v.resize(count);
    return count == 0 || fread(v.data(), sizeof(T), count, f) == count;
}

// a block of exactly `size` bytes, 16-byte aligned like the device's slots
uint8_t* exact_block(size_t size) {
    void* p = nullptr;
    if (posix_memalign(&p, 16, size ? size : 1) != 0) return nullptr;
    return static_cast<uint8_t*>(p);
}

void encode_by_wave(uint8_t* dst, const uint8_t* src, uint32_t len) {
    for (uint32_t l = 0; l < 64; l++) rppp::b64_encode_wave(dst, src, len, l);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const bool fields = strcmp(argv[1], "fields") == 0;
    if (!fields && strcmp(argv[1], "render") != 0) return 2;
    FILE* f = fopen(argv[2], "rb");
    if (!f) return 2;
    uint32_t h[6];
    uint64_t data_len = 0;
    if (fread(h, 4, 6, f) != 6 || fread(&data_len, 8, 1, f) != 1) return 2;
    const uint32_t n = h[0], nindex = h[1], topics_len = h[2], nranges = h[3], nresponses = h[4];
    std::vector<uint8_t> data, topics;
    std::vector<rpgpu_batch_desc> descs;
    std::vector<rpgpu_batch_result> results;
    std::vector<rpgpu_record_index> index;
    std::vector<rpgpu_pp_range> ranges;
    std::vector<rpgpu_pp_response> responses;
    if (!read_vec(f, data, data_len) || !read_vec(f, descs, n) || !read_vec(f, results, n) ||
        !read_vec(f, index, nindex) || !read_vec(f, topics, topics_len) || !read_vec(f, ranges, nranges) ||
        !read_vec(f, responses, nresponses))
        return 2;
    fclose(f);
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 2;

    if (fields) {
        for (uint32_t b = 0; b < n; b++) {
            uint32_t recs;
            if (rppp::batch_status(results[b], &recs) != RPGPU_PP_OK) continue;
            for (uint32_t i = 0; i < recs; i++) {
                const rpgpu_record_index& e = index[results[b].index_first + i];
                for (int kv = 0; kv < 2; kv++) {
                    const int32_t len = kv ? e.val_len : e.key_len;
                    if (len <= 0) continue;
                    // the source alone on the heap as well: a read past the field is a finding
                    uint8_t* src = exact_block((size_t)len);
                    memcpy(src, data.data() + descs[b].offset + (kv ? e.val_off : e.key_off), (size_t)len);
                    const size_t m = (size_t)rppp::b64_len((uint32_t)len);
                    uint8_t* lane = exact_block(m);
                    rppp::b64_encode_lane(lane, src, (uint32_t)len);
                    for (size_t r = 0; r < 16; r++) {
                        uint8_t* wave = exact_block(r + m);
                        memset(wave, 0xA5, r + m);
                        encode_by_wave(wave + r, src, (uint32_t)len);
                        for (size_t k = 0; k < r; k++)
                            if (wave[k] != 0xA5) return 8;
                        if (memcmp(wave + r, lane, m) != 0) return 9;
                        free(wave);
                    }
                    if (fwrite(lane, 1, m, out) != m) return 2;
                    free(lane);
                    free(src);
                }
            }
        }
        fclose(out);
        return 0;
    }

    // ---- plan: pp_ranges_kernel
    std::vector<uint64_t> key(nresponses, rppp::kNoEvent), b_off(n), r_off(nranges);
    std::vector<uint32_t> r_resp(nranges, rppp::kNone), r_stat(nranges), r_recs(nranges), b_recs(n), b_stat(n),
        b_range(n, rppp::kNone);
    auto event = [&](uint32_t r, uint64_t k) {
        if (k < key[r]) key[r] = k;
    };
    for (uint32_t r = 0; r < nresponses; r++) {
        const rpgpu_pp_response R = responses[r];
        if ((uint64_t)R.first_range + R.range_count > nranges) continue;
        for (uint32_t pos = 0; pos < R.range_count; pos++) {
            const uint32_t g = R.first_range + pos;
            const int32_t st = rppp::range_status(ranges[g], topics.data(), topics_len, n);
            r_resp[g] = r;
            r_stat[g] = (uint32_t)st;
            if (st != RPGPU_PP_OK) event(r, rppp::event_key(pos, 0));
        }
    }
    // ---- pp_batch_kernel
    for (uint32_t b = 0; b < n; b++) {
        uint32_t recs;
        b_stat[b] = (uint32_t)rppp::batch_status(results[b], &recs);
        uint64_t var = 0;
        for (uint32_t i = 0; i < recs; i++) {
            if ((uint64_t)results[b].index_first + i >= nindex) return 4;
            var += rppp::object_var(index[results[b].index_first + i]);
        }
        b_off[b] = var;
        b_recs[b] = recs;
    }
    // ---- pp_range_kernel
    for (uint32_t g = 0; g < nranges; g++) {
        uint64_t run = 0;
        uint32_t recs = 0;
        const uint32_t r = r_resp[g];
        if (r != rppp::kNone && r_stat[g] == RPGPU_PP_OK) {
            const rpgpu_pp_range rg = ranges[g];
            const uint32_t pos = g - responses[r].first_range;
            const uint64_t each = 1ull + rppp::object_fixed(rg.topic_len, rg.partition);
            for (uint32_t j = 0; j < rg.count; j++) {
                const uint32_t b = rg.first + j;
                if (b_stat[b] != RPGPU_PP_OK) {
                    event(r, rppp::event_key(pos, j + 1));
                    break;
                }
                const uint64_t sz = b_off[b] + b_recs[b] * each;
                b_off[b] = run;
                b_range[b] = g;
                run += sz;
                recs += b_recs[b];
            }
        }
        r_off[g] = run;
        r_recs[g] = recs;
    }
    // ---- pp_response_kernel, the slots
    std::vector<rpgpu_pp_result> res(nresponses);
    uint64_t next_slot = 0;
    for (uint32_t r = 0; r < nresponses; r++) {
        const rpgpu_pp_response R = responses[r];
        const bool past = (uint64_t)R.first_range + R.range_count > nranges;
        uint64_t run = 0;
        uint32_t recs = 0;
        for (uint32_t pos = 0; !past && pos < R.range_count; pos++) {
            const uint32_t g = R.first_range + pos;
            const uint64_t sz = r_off[g];
            r_off[g] = run;
            run += sz;
            recs += r_recs[g];
        }
        rpgpu_pp_result q = {0, 0, 0, RPGPU_PP_OK, 0, 0};
        if (past) {
            q.status = RPGPU_PP_BAD_RANGE;
            q.bad_batch = nranges;
        } else if (key[r] != rppp::kNoEvent) {
            const uint32_t g = R.first_range + (uint32_t)(key[r] >> 32), sub = (uint32_t)key[r];
            if (sub == 0) {
                q.status = (int32_t)r_stat[g];
                q.bad_batch = g;
            } else {
                q.bad_batch = ranges[g].first + sub - 1;
                q.status = (int32_t)b_stat[q.bad_batch];
            }
        } else {
            q.out_len = rppp::response_len(run);
            q.records = recs;
        }
        q.out_off = next_slot;
        next_slot += rppp::slot_size(q.out_len);
        res[r] = q;
    }

    // ---- run: pp_open_kernel and the two pp_emit_kernel passes, a response at a time
    uint64_t lane_fields = 0, wave_fields = 0;
    for (uint32_t r = 0; r < nresponses; r++) {
        const rpgpu_pp_result q = res[r];
        if (fwrite(&q, sizeof(q), 1, out) != 1) return 2;
        if (q.status != RPGPU_PP_OK) continue;
        uint8_t* buf = exact_block((size_t)q.out_len);
        if (!buf) return 2;
        if (q.records == 0) buf[0] = '[';
        buf[q.out_len - 1] = ']';
        uint64_t written = 1;
        const rpgpu_pp_response R = responses[r];
        for (uint32_t pos = 0; pos < R.range_count; pos++) {
            const uint32_t g = R.first_range + pos;
            const rpgpu_pp_range rg = ranges[g];
            const uint64_t each = 1ull + rppp::object_fixed(rg.topic_len, rg.partition);
            uint8_t* base = buf + r_off[g];
            for (uint32_t j = 0; j < rg.count; j++) {
                const uint32_t b = rg.first + j;
                if (b_range[b] != g) return 5;
                const uint8_t* batch = data.data() + descs[b].offset;
                uint64_t at = b_off[b];
                for (uint32_t i = 0; i < b_recs[b]; i++) {
                    const rpgpu_record_index& e = index[results[b].index_first + i];
                    const uint64_t sz = rppp::object_var(e) + each;
                    uint8_t* end = rppp::put_object(base + at, rppp::lead_byte(r_off[g], at), topics.data() + rg.topic_off,
                                                    rg.topic_len, rg.partition, e, batch, RPGPU_PP_LANE_FIELD_MAX);
                    if (end != base + at + sz) return 6;
                    const rppp::Fields fl = rppp::locate_fields(base + at, rg.topic_len, e, RPGPU_PP_LANE_FIELD_MAX);
                    if (fl.kdst) encode_by_wave(fl.kdst, batch + e.key_off, (uint32_t)e.key_len);
                    if (fl.vdst) encode_by_wave(fl.vdst, batch + e.val_off, (uint32_t)e.val_len);
                    wave_fields += (fl.kdst != nullptr) + (fl.vdst != nullptr);
                    lane_fields += (e.key_len > 0 && !fl.kdst) + (e.val_len > 0 && !fl.vdst);
                    at += sz;
                    written += sz;
                }
            }
        }
        if (q.records ? written != q.out_len : q.out_len != 2) return 7;
        if (fwrite(buf, 1, (size_t)q.out_len, out) != q.out_len) return 2;
        free(buf);
    }
    fclose(out);
    printf("lane %llu wave %llu\n", (unsigned long long)lane_fields, (unsigned long long)wave_fields);
    return 0;
}
