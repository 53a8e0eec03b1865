// segidx_host.cpp — redpanda_amd/csrc/rpgpu_segidx.h on the host: the code the
// kernels of rpgpu_segidx.hip call, run on one thread over the files that
// tests/segment_index_file.py writes, so tests/test_segment_index_file.py can
// compare it with the Python model and run it under ASan + UBSan.  Every
// state's entries, every file and every blob lives in a heap block of exactly
// its size, so a read or write past an end is a sanitizer report.
//
//   segidx_host write   IN OUT   states + entries -> (status, length, blob) per state
//   segidx_host hydrate IN OUT   (entry_cap, length, bytes) per file -> the hydrated
//                                row, then on OK the state row and the entries
//   segidx_host find    IN OUT   states + entries + queries -> found rows
//   segidx_host track   IN OUT   per segment: state, its entries, step, batches ->
//                                status, tracked, the state row, the entries
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "rpgpu_segidx.h"

namespace {

std::vector<uint8_t> slurp(const char* path) {
    FILE* f = fopen(path, "rb");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", path);
        exit(2);
    }
    std::vector<uint8_t> d;
    uint8_t buf[1 << 16];
    size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) d.insert(d.end(), buf, buf + n);
    fclose(f);
    return d;
}

struct Reader {
    const std::vector<uint8_t>& d;
    size_t at = 0;
    template <class T>
    T get() {
        if (at + sizeof(T) > d.size()) {
            fprintf(stderr, "input truncated\n");
            exit(2);
        }
        T v;
        memcpy(&v, d.data() + at, sizeof(T));
        at += sizeof(T);
        return v;
    }
    const uint8_t* bytes(size_t n) {
        if (at + n > d.size()) {
            fprintf(stderr, "input truncated\n");
            exit(2);
        }
        const uint8_t* p = d.data() + at;
        at += n;
        return p;
    }
};

template <class T>
void put(FILE* f, const T& v) {
    fwrite(&v, sizeof(T), 1, f);
}

// a heap block of exactly n rows (one byte for none, never read)
template <class T>
std::unique_ptr<T[]> exact(const T* src, size_t n) {
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    if (n) memcpy(p.get(), src, n * sizeof(T));
    return p;
}

struct Table {
    std::vector<rpgpu_segidx_state> states;
    std::vector<std::unique_ptr<rpgpu_index_entry[]>> slots;  // one block per state
};
Table read_table(Reader& r) {
    Table t;
    const uint32_t ns = r.get<uint32_t>();
    const uint64_t ne = r.get<uint64_t>();
    for (uint32_t i = 0; i < ns; i++) t.states.push_back(r.get<rpgpu_segidx_state>());
    const rpgpu_index_entry* e = reinterpret_cast<const rpgpu_index_entry*>(r.bytes(ne * 16));
    for (const rpgpu_segidx_state& s : t.states) {
        if (!rpsx::slot_ok(s, ne)) {
            fprintf(stderr, "state slot outside the entries\n");
            exit(2);
        }
        std::vector<rpgpu_index_entry> tmp(s.entries);
        if (s.entries) memcpy(tmp.data(), reinterpret_cast<const uint8_t*>(e) + 16ull * s.entry_first, 16ull * s.entries);
        t.slots.push_back(exact(tmp.data(), tmp.size()));
    }
    return t;
}

int do_write(Reader& r, FILE* out) {
    Table t = read_table(r);
    for (size_t i = 0; i < t.states.size(); i++) {
        const rpgpu_segidx_state& s = t.states[i];
        const int32_t status = rpsx::too_big(s.entries) ? RPGPU_SEGIDX_TOO_BIG : RPGPU_SEGIDX_OK;
        const uint32_t n = status == RPGPU_SEGIDX_OK ? (uint32_t)rpsx::blob_bytes(s.entries) : 0;
        std::unique_ptr<uint8_t[]> blob(new uint8_t[n ? n : 1]);
        if (n) rpsx::blob_put(s, t.slots[i].get(), blob.get());
        put(out, status);
        put(out, n);
        fwrite(blob.get(), 1, n, out);
    }
    return 0;
}

int do_hydrate(Reader& r, FILE* out) {
    const uint32_t nf = r.get<uint32_t>();
    for (uint32_t i = 0; i < nf; i++) {
        const uint32_t cap = r.get<uint32_t>(), len = r.get<uint32_t>();
        std::unique_ptr<uint8_t[]> file = exact(r.bytes(len), len);
        rpsx::View v;
        if (rpsx::parse_head(file.get(), len, &v)) {
            uint64_t sum;
            if (v.legacy) {
                if (!rpsx::xxh_ok(v.sum_len)) {
                    fprintf(stderr, "hashed length %llu\n", (unsigned long long)v.sum_len);
                    return 3;
                }
                sum = rpsx::xxh64_mult8(file.get() + v.sum_at, v.sum_len);
            } else {
                sum = rpsx::crc32c_bytes(file.get() + v.sum_at, v.sum_len);
            }
            rpsx::parse_body(file.get(), &v, sum);
            if (v.status == RPGPU_SEGIDX_OK && v.entries > cap)
                rpsx::view_fail(&v, RPGPU_SEGIDX_NO_ROOM, RPGPU_SEGIDX_R_ENTRY_CAP);
        }
        rpgpu_segidx_hydrated h;
        h.status = v.status, h.reason = v.reason, h.version = v.version, h.entries = v.entries;
        put(out, h);
        if (v.status != RPGPU_SEGIDX_OK) continue;
        rpgpu_segidx_state s;
        memset(&s, 0, sizeof s);
        s.entry_cap = cap;
        rpsx::view_state(v, &s);
        put(out, s);
        std::unique_ptr<rpgpu_index_entry[]> e(new rpgpu_index_entry[cap ? cap : 1]);
        for (uint64_t k = 0; k < v.entries; k++) e[k] = rpsx::view_entry(file.get(), v, k);
        fwrite(e.get(), 16, v.entries, out);
    }
    return 0;
}

int do_find(Reader& r, FILE* out) {
    Table t = read_table(r);
    const uint32_t nq = r.get<uint32_t>();
    for (uint32_t i = 0; i < nq; i++) {
        const rpgpu_segidx_query q = r.get<rpgpu_segidx_query>();
        rpgpu_segidx_found o;
        memset(&o, 0, sizeof o);
        o.status = RPGPU_SEGIDX_BAD_QUERY;
        if (q.state < t.states.size()) rpsx::find(t.states[q.state], t.slots[q.state].get(), q.kind, q.key, &o);
        put(out, o);
    }
    return 0;
}

struct BatchRow {  // 48 bytes
    int64_t base_offset, first_timestamp, max_timestamp;
    int32_t size_bytes, last_offset_delta;
    uint8_t user_data, pad[7];
    uint64_t position;
};

int do_track(Reader& r, FILE* out) {
    const uint32_t nsegs = r.get<uint32_t>();
    for (uint32_t i = 0; i < nsegs; i++) {
        rpgpu_segidx_state s = r.get<rpgpu_segidx_state>();
        const uint32_t step = r.get<uint32_t>(), nb = r.get<uint32_t>();
        if (s.entries > s.entry_cap) return 2;
        std::unique_ptr<rpgpu_index_entry[]> e(new rpgpu_index_entry[s.entry_cap ? s.entry_cap : 1]);
        memcpy(e.get(), r.bytes(16ull * s.entries), 16ull * s.entries);
        int32_t status = RPGPU_V_OK;
        uint32_t tracked = 0;
        for (uint32_t k = 0; k < nb; k++) {
            const BatchRow row = r.get<BatchRow>();
            if (status != RPGPU_V_OK) continue;
            rpsx::Batch b;
            b.base_offset = row.base_offset, b.first_timestamp = row.first_timestamp;
            b.max_timestamp = row.max_timestamp, b.size_bytes = row.size_bytes;
            b.last_offset_delta = row.last_offset_delta, b.user_data = row.user_data != 0, b.position = row.position;
            status = rpsx::track_step(&s, e.get(), step, b);
            if (status == RPGPU_V_OK) tracked++;
        }
        put(out, status);
        put(out, tracked);
        put(out, s);
        fwrite(e.get(), 16, s.entries, out);
    }
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 4) {
        fprintf(stderr, "usage: segidx_host write|hydrate|find|track IN OUT\n");
        return 2;
    }
    static_assert(sizeof(BatchRow) == 48, "batch rows of the track file");
    const std::vector<uint8_t> in = slurp(argv[2]);
    Reader r{in};
    FILE* out = fopen(argv[3], "wb");
    if (!out) return 2;
    const std::string mode = argv[1];
    int rc = 2;
    if (mode == "write") rc = do_write(r, out);
    else if (mode == "hydrate") rc = do_hydrate(r, out);
    else if (mode == "find") rc = do_find(r, out);
    else if (mode == "track") rc = do_track(r, out);
    if (rc == 0 && r.at != in.size()) {
        fprintf(stderr, "input not consumed\n");
        rc = 2;
    }
    fclose(out);
    return rc;
}
