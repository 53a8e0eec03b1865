// copy_prims.cpp — the LZ77 copy primitives of redpanda_amd/csrc/rpgpu_copy.h
// on the host, each against a byte-at-a-time loop: for every off in 0..40 and
// n in 0..80 at four destination alignments mod 16 the wild and exact match
// copies (and, for the same n, the forward copies and the fill), period16 for
// 1 <= off < 16, and the write-combined register path driven through a WcBuf
// for ll <= 34, ml <= 36, off <= 40 at four fills of the pending buffer, then
// flushed.  Exact copies must leave dst + n onward untouched, wild copies
// dst + n + 64 onward, the register path everything from 16 bytes past the
// sequence's end.  Prints the first failing case and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "rpgpu_copy.h"

using namespace rpcodec;
typedef std::vector<uint8_t> Bytes;
typedef unsigned long long ull;

static const int kAligns[4] = {0, 1, 7, 13};
static const uint64_t kPre = 64, kGuard = 256;  // bytes before dst (history) and after dst + n

static uint32_t rng_state = 0x9E3779B9u;
static uint8_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}
static Bytes random_bytes(uint64_t n) {
    Bytes v(n);
    for (auto& b : v) b = rnd();
    return v;
}

static long cases = 0;
static void fail(const char* what, int a, uint64_t off, uint64_t n, uint64_t at, const char* why) {
    fprintf(stderr, "copy_prims: %s align %d off %llu n %llu: %s at byte %llu\n", what, a, (ull)off, (ull)n, why, (ull)at);
    exit(1);
}

// `init` = kPre + a bytes of history, then the bytes the copy finds at dst.
// After run(dst): dst[0, n) is `want`, and the history and everything from
// dst + n + reach on are as they were.
template <class F>
static void check_copy(const char* what, int a, uint64_t off, uint64_t n, uint64_t reach, const Bytes& init,
                       const Bytes& want, F&& run) {
    Bytes buf = init;
    uint8_t* dst = buf.data() + kPre + a;
    run(dst);
    cases++;
    for (uint64_t i = 0; i < kPre + a; i++)
        if (buf[i] != init[i]) fail(what, a, off, n, i, "history changed");
    for (uint64_t i = 0; i < n; i++)
        if (dst[i] != want[i]) fail(what, a, off, n, i, "wrong byte");
    for (uint64_t i = kPre + a + n + reach; i < buf.size(); i++)
        if (buf[i] != init[i]) fail(what, a, off, n, i - kPre - a, "written past the allowed reach");
}

static void match_copies() {
    for (int a : kAligns)
        for (uint64_t off = 0; off <= 40; off++)
            for (uint64_t n = 0; n <= 80; n++) {
                const Bytes init = random_bytes(kPre + a + n + kGuard);
                Bytes want(n);  // dst[i] = dst[i - off]; off 0: zeros
                for (uint64_t i = 0; i < n; i++) want[i] = off == 0 ? 0 : i < off ? init[kPre + a + i - off] : want[i - off];
                check_copy("copy_match", a, off, n, 64, init, want, [&](uint8_t* d) { copy_match(d, off, n); });
                check_copy("match_exact", a, off, n, 0, init, want, [&](uint8_t* d) { match_exact(d, off, n); });
                if (off >= 1)
                    check_copy("copy_seq_match", a, off, n, 0, init, want, [&](uint8_t* d) { copy_seq_match(d, off, n); });
            }
}

static void forward_copies() {
    const Bytes src = random_bytes(80 + 16 + 64);
    for (int a : kAligns)
        for (int sa : kAligns)
            for (uint64_t n = 0; n <= 80; n++) {
                const Bytes init = random_bytes(kPre + a + n + kGuard);
                const uint8_t* s = src.data() + sa;
                const Bytes want(s, s + n);
                check_copy("copy_fwd", a, 0, n, 64, init, want, [&](uint8_t* d) { copy_fwd(d, s, n); });
                check_copy("copy_exact", a, 0, n, 0, init, want, [&](uint8_t* d) { copy_exact(d, s, n); });
                check_copy("copy_lits", a, 0, n, 0, init, want, [&](uint8_t* d) { copy_lits(d, s, n); });
                check_copy("fill_bytes", a, 0, n, 0, init, Bytes(n, (uint8_t)(n + 3)),
                           [&](uint8_t* d) { fill_bytes(d, (uint8_t)(n + 3), n); });
            }
    // copy_lits down onto itself: src = dst + k
    for (int a : kAligns)
        for (uint64_t k : {0, 1, 15, 16, 33})
            for (uint64_t n = 0; n <= 80; n++) {
                const Bytes init = random_bytes(kPre + a + n + k + kGuard);
                const Bytes want(init.begin() + kPre + a + k, init.begin() + kPre + a + k + n);
                check_copy("copy_lits onto itself", a, k, n, 0, init, want, [&](uint8_t* d) { copy_lits(d, d + k, n); });
            }
}

static void periods() {
    for (uint64_t off = 1; off < 16; off++)
        for (int rep = 0; rep < 64; rep++) {
            const Bytes x = random_bytes(16);
            uint8_t y[16];
            v16_st(y, period16(v16_ld(x.data()), off));
            cases++;
            for (uint64_t i = 0; i < 16; i++)
                if (y[i] != x[i % off]) fail("period16", 0, off, 16, i, "wrong byte");
            const uint64_t s = period_step(off);
            if (s % off != 0 || s > 16 || s + off <= 16) fail("period_step", 0, off, s, 0, "not the most whole periods in 16 bytes");
        }
}

// One sequence as the lane decoders run it: the register path where wc_fits,
// else the exact copies (the callers' fallback)
static void drive(WcBuf<uint64_t>& b, uint8_t* out, uint64_t& o, const uint8_t*& lp, uint64_t ll, uint64_t ml, uint64_t off,
                  Bytes& model) {
    for (uint64_t i = 0; i < ll; i++) model.push_back(lp[i]);
    for (uint64_t i = 0; i < ml; i++) model.push_back(model[model.size() - off]);
    if (!wc_fits(ll, ml, off)) {
        wc_flush(b, out, o);
        copy_lits(out + o, lp, ll);
        copy_seq_match(out + o + ll, off, ml);
        b.ca = o + ll + ml;
    } else {
        V16 L0{0, 0}, L1{0, 0};
        if (ll > 0) L0 = v16_ld(lp);
        if (ll > 16) L1 = v16_ld(lp + 16);
        wc_exec(b, out, o, L0, L1, ll, ml, off);
    }
    lp += ll;
    o += ll + ml;
}

static void executor() {
    static const uint64_t kFills[4] = {0, 5, 16, 27};  // bytes pending in the buffer when the sequence arrives
    const uint64_t kOut = 512;
    const Bytes lits = random_bytes(4096);
    Bytes model;
    for (int fi = 0; fi < 4; fi++)
        for (uint64_t ll = 0; ll <= 34; ll++)
            for (uint64_t ml = 1; ml <= 36; ml++)
                for (uint64_t off = 1; off <= 40; off++) {
                    const int a = kAligns[fi];
                    Bytes buf(16 + kOut, 0xA5);
                    uint8_t* out = buf.data() + a;
                    const uint8_t* lp = lits.data() + ((ll * 37 + ml * 11 + off) & 1023);
                    WcBuf<uint64_t> b{};
                    uint64_t o = 0;
                    model.clear();
                    drive(b, out, o, lp, 41, 4, 3, model);  // history for every offset; not write-combined
                    if (fi == 1) drive(b, out, o, lp, 2, 3, 1, model);
                    if (fi >= 2) drive(b, out, o, lp, 8, 8, 5, model);
                    if (fi == 3) drive(b, out, o, lp, 5, 6, 20, model);
                    if (o - b.ca != kFills[fi]) fail("wc_exec prelude", a, off, ml, o - b.ca, "unexpected fill");
                    drive(b, out, o, lp, ll, ml, off, model);
                    const uint64_t seq_end = o;
                    drive(b, out, o, lp, 3, 4, 2, model);  // overwrites the sequence's overshoot
                    wc_flush(b, out, o);
                    cases++;
                    uint64_t bad = ~0ull;
                    const char* why = "";
                    for (uint64_t i = kOut; i-- > seq_end + 16;)
                        if (out[i] != 0xA5) bad = i, why = "written 16 or more bytes past the sequence";
                    for (uint64_t i = o; i-- > 0;)
                        if (out[i] != model[i]) bad = i, why = "wrong byte";
                    for (int i = 0; i < a; i++)
                        if (buf[i] != 0xA5) bad = 0, why = "written before the output";
                    if (bad != ~0ull) {
                        fprintf(stderr, "copy_prims: wc_exec fill %llu ll %llu ml %llu off %llu (sequence at %llu): %s at byte %llu\n",
                                (ull)kFills[fi], (ull)ll, (ull)ml, (ull)off, (ull)(seq_end - ll - ml), why, (ull)bad);
                        exit(1);
                    }
                }
}

int main() {
    periods();
    match_copies();
    forward_copies();
    executor();
    printf("copy_prims: %ld cases ok\n", cases);
    return 0;
}
