// txfilter_host.cpp — rpgpu_txfilter.h on the host: the functions the kernels of
// rpgpu_txfilter.hip call, driven by one thread over the calls of
// tests/test_tx_compaction.py.  Built plain and with -fsanitize=address,undefined;
// every array lives in a heap block of exactly its size, so a read past a
// scope's batches, ranges, markers or index entries is an error, not a guess.
//
//   txfilter_host <input> <output>
// input:  u64 data_bytes, n, index_cap, nscopes, nranges; then data, descs,
//         results, index, scopes, ranges.
// output: discard[n], stats[nscopes].
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <tuple>
#include <vector>

#include "rpgpu_txfilter.h"

template <class T>
static std::unique_ptr<T[]> exact(size_t count) {
    return std::unique_ptr<T[]>(new T[count]);  // count == 0: a block of no bytes
}

template <class T>
static std::unique_ptr<T[]> read_rows(FILE* f, size_t count) {
    auto p = exact<T>(count);
    if (count && fread(p.get(), sizeof(T), count, f) != count) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return p;
}

struct Group {  // one (scope, producer): its abort markers, the interval minima
    std::vector<uint32_t> markers;
    std::unique_ptr<uint32_t[]> sorted, cellm;
    uint32_t cellh = rptx::kNone;
};
using Pid = std::tuple<uint32_t, int64_t, int16_t>;

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t hd[5];
    if (fread(hd, 8, 5, f) != 5) return 2;
    const uint64_t data_bytes = hd[0], index_cap = hd[2];
    const uint32_t n = (uint32_t)hd[1], nscopes = (uint32_t)hd[3], nranges = (uint32_t)hd[4];
    auto data = read_rows<uint8_t>(f, data_bytes);
    auto descs = read_rows<rpgpu_batch_desc>(f, n);
    auto res = read_rows<rpgpu_batch_result>(f, n);
    auto index = read_rows<rpgpu_record_index>(f, index_cap);
    auto scopes = read_rows<rpgpu_tx_scope>(f, nscopes);
    auto ranges = read_rows<rpgpu_tx_range>(f, nranges);
    fclose(f);

    auto discard = exact<uint8_t>(n);
    memset(discard.get(), RPGPU_TX_NOT_REACHED, n);
    auto stats = exact<rpgpu_tx_stats>(nscopes);
    for (uint32_t s = 0; s < nscopes; s++) {
        const rpgpu_tx_scope sc = scopes[s];
        rpgpu_tx_stats st;
        memset(&st, 0, sizeof(st));
        st.bad_batch = UINT32_MAX;
        if ((uint64_t)sc.first_batch + sc.batch_count > n || (uint64_t)sc.range_first + sc.range_count > nranges) {
            st.status = RPGPU_TX_BAD_SCOPE;
            stats[s] = st;
            continue;
        }
        const bool nontx = (sc.flags & RPGPU_TX_NON_TRANSACTIONAL) != 0;
        // classify up to the stop
        std::vector<rptx::Class> cls;
        for (uint32_t i = 0; i < sc.batch_count; i++) {
            const uint32_t b = sc.first_batch + i;
            // the batch's bytes in a block of their own: a key or a header read past them is caught
            auto bytes = exact<uint8_t>(descs[b].length);
            memcpy(bytes.get(), data.get() + descs[b].offset, descs[b].length);
            const rptx::Class c = rptx::classify(res[b], descs[b], bytes.get(), index.get(), index_cap, nontx);
            if (c.stop != RPGPU_TX_OK) {
                st.status = c.stop, st.bad_batch = b;
                break;
            }
            cls.push_back(c);
        }
        const uint32_t m = st.processed = (uint32_t)cls.size();
        st.all_batches = nontx ? 0 : m;
        auto M = exact<int64_t>(m);
        rptx::MaxOp run = rptx::max_identity();
        std::map<Pid, Group> groups;
        for (uint32_t i = 0; i < m; i++) {
            const uint32_t b = sc.first_batch + i;
            run = rptx::max_combine(run, rptx::MaxOp{rptx::last_offset(res[b])});
            M[i] = run.v;
            discard[b] = cls[i].flag;
            st.tx_control_batches_discarded += cls[i].flag == RPGPU_TX_MARKER;
            st.non_tx_control_batches_discarded += cls[i].flag == RPGPU_TX_PREPARE;
            if (cls[i].kind != rptx::kKindNone) {
                Group& g = groups[Pid(s, cls[i].pid, cls[i].epoch)];
                if (cls[i].kind == rptx::kKindAbort) g.markers.push_back(b);
            }
        }
        for (auto& kv : groups) {
            Group& g = kv.second;
            const size_t k = g.markers.size();
            g.sorted = exact<uint32_t>(k), g.cellm = exact<uint32_t>(k);
            for (size_t j = 0; j < k; j++) g.sorted[j] = g.markers[j], g.cellm[j] = rptx::kNone;
        }
        auto cell = [&](Group& g, uint32_t x) -> uint32_t& {
            const uint32_t iv = rptx::interval_of(g.sorted.get(), 0, (uint32_t)g.markers.size(), x);
            return iv == rptx::kNone ? g.cellh : g.cellm[iv];
        };
        for (uint32_t j = 0; j < sc.range_count; j++) {
            const rpgpu_tx_range r = ranges[sc.range_first + j];
            if (!rptx::takes_part(r, sc)) continue;
            st.num_aborted_txes++;
            if (nontx) continue;
            const uint32_t c = rptx::consume_pos(M.get(), m, r.first);
            if (c == m) continue;
            auto it = groups.find(Pid(s, r.producer_id, r.producer_epoch));
            if (it == groups.end()) continue;
            uint32_t& v = cell(it->second, sc.first_batch + c);
            if (sc.first_batch + c < v) v = sc.first_batch + c;
        }
        for (uint32_t i = 0; i < m; i++) {
            if (cls[i].kind != rptx::kKindData) continue;
            const uint32_t b = sc.first_batch + i;
            if (rptx::aborted(cell(groups[Pid(s, cls[i].pid, cls[i].epoch)], b), b)) {
                discard[b] = RPGPU_TX_ABORTED_DATA;
                st.tx_data_batches_discarded++;
            }
        }
        st.all_batches_discarded = st.tx_data_batches_discarded + st.tx_control_batches_discarded +
                                   st.non_tx_control_batches_discarded;
        stats[s] = st;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (n) fwrite(discard.get(), 1, n, o);
    if (nscopes) fwrite(stats.get(), sizeof(rpgpu_tx_stats), nscopes, o);
    fclose(o);
    return 0;
}
