// produce_host.cpp — the per-row core of building produce batches from records
// (redpanda_amd/csrc/rpgpu_produce.h: the partitioners, murmur2, the record
// sizes, the guard rails) compiled for the host and run over a case file.  TEST
// INFRASTRUCTURE, built and run by tests/test_produce_records.py, once plainly
// and once with -fsanitize=address,undefined.
//
// Case file (little-endian): uint64 data_bytes, nrows, nrequests; the data; the
// rpgpu_produce_row rows; the rpgpu_produce_request rows.
// Output: per request "q status rr_next nbatches", then per row
// "r partition delta bytes" (the record's bytes in its body), or "r - - -" for
// the rows of a refused request.  The serial grouping here stands for the
// kernels' sort and scans; every per-row decision is the header's.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <vector>

#include "rpgpu_produce.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[3];
    if (fread(h, 8, 3, f) != 3) return 2;
    const uint64_t data_bytes = h[0], n = h[1], nreq = h[2];
    // exactly data_bytes on the heap: a read past the arena is an ASan finding
    std::vector<uint8_t> data(data_bytes);
    std::vector<rpgpu_produce_row> rows(n);
    std::vector<rpgpu_produce_request> reqs(nreq);
    if (data_bytes && fread(data.data(), 1, data_bytes, f) != data_bytes) return 2;
    if (n && fread(rows.data(), sizeof(rpgpu_produce_row), n, f) != n) return 2;
    if (nreq && fread(reqs.data(), sizeof(rpgpu_produce_request), nreq, f) != nreq) return 2;
    fclose(f);
    // the vectors of include/rpgpu.h, at every misalignment of a 16-byte load
    {
        const char* key = "lkjh234lh9fiuh90y23oiuhsafujhadof229phr9h19h89h8";
        for (size_t a = 0; a < 16; a++) {
            std::vector<uint8_t> buf(a + 48);
            memcpy(buf.data() + a, key, 48);
            if (rpproduce::murmur2(buf.data() + a, 48, rpproduce::kMurmurSeed) != 0xfc7d49cdu) return 3;
        }
        if (rpproduce::murmur2(nullptr, 0, rpproduce::kMurmurSeed) != 0x106e08d9u) return 3;
    }
    uint64_t sum = 0;
    for (const auto& q : reqs) sum += q.nrows;
    struct RowOut {
        bool live;
        int32_t partition;
        uint32_t delta;
        uint64_t bytes;
    };
    std::vector<RowOut> out(n, RowOut{false, 0, 0, 0});
    uint64_t first = 0;
    for (uint64_t r = 0; r < nreq; r++) {
        const rpgpu_produce_request& q = reqs[r];
        int32_t status = RPGPU_PRODUCE_OK;
        uint32_t rr = 0, nbatches = 0;
        if (sum != n || !rpproduce::request_ok(q)) status = RPGPU_PRODUCE_BAD_REQUEST;
        if (status == RPGPU_PRODUCE_OK)
            for (uint64_t i = first; i < first + q.nrows; i++)
                if (!rpproduce::row_ok(rows[i], data_bytes)) status = RPGPU_PRODUCE_BAD_ROW;
        std::map<int32_t, std::vector<uint64_t>> groups;  // ascending signed partition id
        if (status == RPGPU_PRODUCE_OK) {
            for (uint64_t i = first; i < first + q.nrows; i++) {
                int32_t p = 0;
                if (rpproduce::row_rule(rows[i], data.data(), q.partition_count, &p) == rpproduce::kRuleRoundRobin)
                    p = rpproduce::round_robin(q.rr_initial, rr++, q.partition_count);
                groups[p].push_back(i);
            }
            if ((uint64_t)q.rr_initial + rr > 0x7fffffffull) status = RPGPU_PRODUCE_BAD_REQUEST;
        }
        if (status == RPGPU_PRODUCE_OK) {
            // the sort key orders the groups as the map does
            int64_t prev = -1;
            for (const auto& g : groups) {
                const int64_t k = rpproduce::partition_key(g.first);
                if (k <= prev) return 4;
                prev = k;
                uint64_t body = 0;
                for (size_t d = 0; d < g.second.size(); d++) body += rpproduce::record_bytes((uint32_t)d, rows[g.second[d]]);
                if (!rpproduce::body_fits(body)) status = RPGPU_PRODUCE_TOO_LARGE;
            }
        }
        if (status == RPGPU_PRODUCE_OK) {
            nbatches = (uint32_t)groups.size();
            for (const auto& g : groups)
                for (size_t d = 0; d < g.second.size(); d++) {
                    const rpgpu_produce_row& w = rows[g.second[d]];
                    const uint64_t len = rpproduce::record_len((uint32_t)d, w);
                    // the encoder's 32-bit length agrees with the 64-bit one wherever a batch is emitted
                    if (len != rplegacy::record_len((uint32_t)d, rpproduce::encoded_key_len(w.key_len), w.val_len)) return 5;
                    out[g.second[d]] = RowOut{true, g.first, (uint32_t)d, rpproduce::record_bytes((uint32_t)d, w)};
                }
        }
        printf("q %d %d %u\n", status, q.rr_initial + (status == RPGPU_PRODUCE_OK ? (int32_t)rr : 0), nbatches);
        first += sum == n ? q.nrows : 0;
    }
    for (uint64_t i = 0; i < n; i++) {
        if (out[i].live) printf("r %d %u %llu\n", out[i].partition, out[i].delta, (unsigned long long)out[i].bytes);
        else printf("r - - -\n");
    }
    return 0;
}
