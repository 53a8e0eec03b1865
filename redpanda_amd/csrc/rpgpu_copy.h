// rpgpu_copy.h — the LZ77 copy primitives every decoder's byte-exactness
// rests on: 16-byte register values, wild and exact copies, the period
// pattern of a short-offset match, and the write-combined register path that
// executes one whole sequence in one memory round trip.
//
// Plain C++, host and device: the device decoders (rpgpu_codec.h,
// rpgpu_zstd.h, rpgpu_wave.h, rpgpu_zblk.h, rpgpu_zseq.h, rpgpu_inflate.h)
// and the host differential tests (tests/native/) compile the same code.
//
// Contracts.  "match" means dst[i] = dst[i - off] in increasing i, i.e. the
// period-`off` extension of the `off` bytes before dst.
//
//   wild copies -- stores run past n; a later sequence overwrites the
//   overshoot (as liblz4's own wild copies), so an output buffer needs
//   rpcodec::kSlack writable bytes past its planned capacity and an input
//   buffer 64 readable bytes past its end (kInPad, RPGPU_ARENA_TAIL_PAD):
//     copy_fwd(dst, src, n)    writes < dst + max(n, 16) rounded up to 64 (at
//                              most n + 63); reads src as far as it writes
//                              dst; ranges must not overlap within 64 bytes.
//     copy_match(dst, off, n)  writes at most n + 63 bytes (n + 15 for
//                              off < 64); reads [dst - off, dst - off + 16)
//                              for off < 16, else the source as far as it
//                              writes.  off == 0 yields zeros, which is what
//                              liblz4's offset-0 copy produces
//                              (LZ4_write32(op, 0) before the self-copy).
//
//   exact copies -- nothing is written at or past dst + n, for outputs whose
//   next bytes are someone else's (another lane's split block or chunk, the
//   zstd literals in the slot tail right behind the output, another lane of
//   the wave-cooperative round):
//     copy_exact(dst, src, n)  disjoint ranges; reads up to src + n + 15.
//     copy_lits(dst, src, n)   src >= dst or disjoint (each 16-byte chunk is
//                              read before it is written; the last,
//                              overlapping chunk is read up front); reads
//                              [src, src + n), or [src, src + 16) for n < 16.
//     match_exact(dst, off, n) reads [dst - off, dst - off + 16) for off < 16
//                              and up to 15 bytes past the source's end for
//                              off >= 16; off == 0: zeros.
//     copy_seq_match(dst, off, n)  off >= 1; reads [dst - off, dst - off + 16)
//                              for off < 16 or n < 16, else nothing past the
//                              source's end.
//     fill_bytes(dst, v, n), st_part(p, lo, hi, n < 16)  no reads.
//   copy_exact / match_exact are the plain 16-byte loops lz4_block_lane's
//   fallback can afford: with copy_lits / copy_seq_match there (64-byte steps,
//   a last chunk held across the loop) lz_lane_kernel and part_kernel<0> spill
//   156 bytes of scratch per lane instead of 76 at their 128-VGPR ceiling.
//
//   register path (WcBuf, wc_fits, wc_exec, wc_flush) -- see below; stores
//   reach at most 15 bytes past the sequence's end, off >= 1.
#ifndef RPGPU_COPY_H
#define RPGPU_COPY_H

#include <stdint.h>
#include <string.h>

#include <type_traits>

#ifdef __HIPCC__
#define RPC_HD __host__ __device__ __forceinline__
#else
#define RPC_HD static inline
#endif
// member functions (a static specifier does not apply to them on the host)
#if defined(__HIPCC__)
#define RPC_MF __host__ __device__ __forceinline__
#else
#define RPC_MF inline
#endif

namespace rpcodec {

// 16 bytes as a vector value (a struct with an array member would be kept in
// scratch memory by the device compiler when live across branches)
typedef uint32_t B16 __attribute__((vector_size(16)));
RPC_HD void ld16(B16& v, const uint8_t* p) { __builtin_memcpy(&v, p, 16); }
RPC_HD void st16(uint8_t* p, const B16& v) { __builtin_memcpy(p, &v, 16); }
RPC_HD uint32_t le16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
RPC_HD uint32_t le32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
RPC_HD uint64_t le64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
RPC_HD uint32_t be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

// 16 bytes as two 64-bit halves, for values composed by shifts and masks
struct V16 {
    uint64_t lo, hi;
};
RPC_HD V16 v16_ld(const uint8_t* p) {
    B16 v;
    ld16(v, p);
    return V16{((uint64_t)v[1] << 32) | v[0], ((uint64_t)v[3] << 32) | v[2]};
}
RPC_HD void v16_st(uint8_t* p, const V16& x) {
    B16 v;
    v[0] = (uint32_t)x.lo, v[1] = (uint32_t)(x.lo >> 32), v[2] = (uint32_t)x.hi, v[3] = (uint32_t)(x.hi >> 32);
    st16(p, v);
}
RPC_HD uint64_t funnel(uint64_t a, uint64_t b, uint32_t s) {  // bytes [s, s + 8) of a|b, s < 8
    return s ? (a >> (8 * s)) | (b << (64 - 8 * s)) : a;
}
// bytes [r, r + 16) of the 32 bytes x|y (bytes past 32 read as zero), r < 32
RPC_HD V16 v16_ext(const V16& x, const V16& y, uint32_t r) {
    const uint32_t k = r >> 3, s = r & 7;
    const uint64_t a = k == 0 ? x.lo : k == 1 ? x.hi : k == 2 ? y.lo : y.hi;
    const uint64_t b = k == 0 ? x.hi : k == 1 ? y.lo : k == 2 ? y.hi : 0;
    const uint64_t c = k == 0 ? y.lo : k == 1 ? y.hi : 0;
    return V16{funnel(a, b, s), funnel(b, c, s)};
}
// x moved up by t bytes (t <= 16), zeros shifted in
RPC_HD V16 v16_shl(const V16& x, uint32_t t) { return v16_ext(V16{0, 0}, x, 16 - t); }
// bytes [0, k) of a, [k, 16) of b (k <= 16)
RPC_HD V16 v16_merge(const V16& a, const V16& b, uint32_t k) {
    const uint64_t ml = k >= 8 ? ~0ull : (1ull << (8 * k)) - 1;
    const uint64_t mh = k >= 16 ? ~0ull : k > 8 ? (1ull << (8 * (k - 8))) - 1 : 0ull;
    return V16{(a.lo & ml) | (b.lo & ~ml), (a.hi & mh) | (b.hi & ~mh)};
}
// bytes of x (output offset xb) that lie in [pb, pb + 16) replaced by p's
RPC_HD V16 v16_overlay(const V16& x, int32_t xb, const V16& p, int32_t pb) {
    const int32_t e = pb - xb;  // x's byte e is p's byte 0
    if (e >= 16 || e <= -16) return x;
    if (e >= 0) return v16_merge(x, v16_shl(p, (uint32_t)e), (uint32_t)e);
    return v16_merge(v16_ext(p, V16{0, 0}, (uint32_t)-e), x, (uint32_t)(16 + e));
}

// n < 16 bytes of lo|hi, exactly
RPC_HD void st_part(uint8_t* p, uint64_t lo, uint64_t hi, uint64_t n) {
    if (n & 8) {
        __builtin_memcpy(p, &lo, 8);
        p += 8;
        lo = hi;
    }
    if (n & 4) {
        const uint32_t v = (uint32_t)lo;
        __builtin_memcpy(p, &v, 4);
        p += 4;
        lo >>= 32;
    }
    if (n & 2) {
        const uint16_t v = (uint16_t)lo;
        __builtin_memcpy(p, &v, 2);
        p += 2;
        lo >>= 16;
    }
    if (n & 1) *p = (uint8_t)lo;
}
RPC_HD void fill_bytes(uint8_t* dst, uint8_t v, uint64_t n) {
    const uint64_t x = 0x0101010101010101ull * v;
    B16 p;
    p[0] = p[1] = p[2] = p[3] = (uint32_t)x;
    uint64_t i = 0;
    for (; i + 16 <= n; i += 16) st16(dst + i, p);
    if (i < n) st_part(dst + i, x, x, n - i);
}

// ---------------------------------------------------------- period pattern
// A match with 1 <= off < 16 is a 16-byte register holding its period -- the
// first `off` bytes of x, the 16 bytes at dst - off -- repeated (two 64-bit
// halves, doubled by shifts; no per-byte array, which would live in scratch
// memory on the device), stored period_step(off) bytes apart: a whole number
// of periods.
RPC_HD V16 period16(const V16& x, uint64_t off) {
    uint64_t lo = x.lo, hi = x.hi;
    if (off <= 8) {
        if (off < 8) lo &= (1ull << (8 * off)) - 1;
        hi = 0;
    } else {
        hi &= (1ull << (8 * (off - 8))) - 1;
    }
    for (uint64_t w = off; w < 16; w *= 2) {
        const uint64_t sh = 8 * w;  // 8..120 bits
        if (sh < 64) {
            hi |= (hi << sh) | (lo >> (64 - sh));
            lo |= lo << sh;
        } else {
            hi |= lo << (sh - 64);
        }
    }
    return V16{lo, hi};
}
RPC_HD uint64_t period_step(uint64_t off) { return off * (16 / off); }

// -------------------------------------------------------------- wild copies
// 64 bytes per step, four loads in flight
RPC_HD void copy_fwd(uint8_t* dst, const uint8_t* src, uint64_t n) {
    if (n <= 16) {
        if (n) {
            B16 v;
            ld16(v, src);
            st16(dst, v);
        }
        return;
    }
    for (uint64_t i = 0; i < n; i += 64) {
        B16 a, b, c, d;
        ld16(a, src + i);
        ld16(b, src + i + 16);
        ld16(c, src + i + 32);
        ld16(d, src + i + 48);
        st16(dst + i, a);
        st16(dst + i + 16, b);
        st16(dst + i + 32, c);
        st16(dst + i + 48, d);
    }
}
RPC_HD void copy_match(uint8_t* dst, uint64_t off, uint64_t n) {
    if (off >= 64) {
        copy_fwd(dst, dst - off, n);  // each 64-byte source block is already written
        return;
    }
    if (off >= 16) {
        for (uint64_t i = 0; i < n; i += 16) {
            B16 v;
            ld16(v, dst - off + i);
            st16(dst + i, v);
        }
        return;
    }
    const V16 p = off ? period16(v16_ld(dst - off), off) : V16{0, 0};
    const uint64_t step = off ? period_step(off) : 16;
    for (uint64_t i = 0; i < n; i += step) v16_st(dst + i, p);
}

// ------------------------------------------------------------- exact copies
RPC_HD void copy_exact(uint8_t* dst, const uint8_t* src, uint64_t n) {
    uint64_t i = 0;
    for (; i + 16 <= n; i += 16) {
        B16 v;
        ld16(v, src + i);
        st16(dst + i, v);
    }
    if (i < n) st_part(dst + i, le64(src + i), le64(src + i + 8), n - i);
}
RPC_HD void match_exact(uint8_t* dst, uint64_t off, uint64_t n) {
    if (off >= 16) {
        uint64_t i = 0;
        for (; i + 16 <= n; i += 16) {
            B16 v;
            ld16(v, dst - off + i);
            st16(dst + i, v);
        }
        if (i < n) st_part(dst + i, le64(dst - off + i), le64(dst - off + i + 8), n - i);
        return;
    }
    const V16 p = off ? period16(v16_ld(dst - off), off) : V16{0, 0};
    const uint64_t step = off ? period_step(off) : 16;
    uint64_t i = 0;
    for (; i + 16 <= n; i += step) v16_st(dst + i, p);
    if (i < n) st_part(dst + i, p.lo, p.hi, n - i);
}
RPC_HD void copy_lits(uint8_t* dst, const uint8_t* src, uint64_t n) {
    if (n < 16) {
        if (n) st_part(dst, le64(src), le64(src + 8), n);
        return;
    }
    B16 last;
    ld16(last, src + n - 16);
    uint64_t i = 0;
    for (; i + 64 <= n; i += 64) {
        B16 a, b, c, d;
        ld16(a, src + i);
        ld16(b, src + i + 16);
        ld16(c, src + i + 32);
        ld16(d, src + i + 48);
        st16(dst + i, a);
        st16(dst + i + 16, b);
        st16(dst + i + 32, c);
        st16(dst + i + 48, d);
    }
    for (; i + 16 <= n; i += 16) {
        B16 a;
        ld16(a, src + i);
        st16(dst + i, a);
    }
    st16(dst + n - 16, last);
}
RPC_HD void copy_seq_match(uint8_t* dst, uint64_t off, uint64_t n) {
    if (off >= 16) {
        if (n < 16) {
            st_part(dst, le64(dst - off), le64(dst - off + 8), n);
            return;
        }
        uint64_t i = 0;
        if (off >= 64) {
            for (; i + 64 <= n; i += 64) {
                B16 a, b, c, d;
                ld16(a, dst - off + i);
                ld16(b, dst - off + i + 16);
                ld16(c, dst - off + i + 32);
                ld16(d, dst - off + i + 48);
                st16(dst + i, a);
                st16(dst + i + 16, b);
                st16(dst + i + 32, c);
                st16(dst + i + 48, d);
            }
        }
        for (; i + 16 <= n; i += 16) {
            B16 a;
            ld16(a, dst - off + i);
            st16(dst + i, a);
        }
        if (i < n) {  // the last 16 bytes, whose source is written by now
            B16 a;
            ld16(a, dst + n - 16 - off);
            st16(dst + n - 16, a);
        }
        return;
    }
    const V16 p = period16(v16_ld(dst - off), off);
    const uint64_t step = period_step(off);
    uint64_t i = 0;
    for (; i + 16 <= n; i += step) v16_st(dst + i, p);
    if (i < n) st_part(dst + i, p.lo, p.hi, n - i);
}

// ------------------------------------------------- write-combined sequences
// The lane decoders' register path (rpcodec::lz4_block_lane, rpzstd::wc_seq).
// A lane decodes one stream while 63 other lanes of its wavefront decode
// theirs in lockstep; time is set by the dependent memory round trips per
// sequence, not by instructions.  A sequence with <= 32 literal bytes and a
// match of <= 32 bytes whose source lies before it (offset >= 16 per 16-byte
// chunk), or any match with offset < 16 (its period rebuilt in registers) --
// wc_fits -- issues all its loads at once, composes the match bytes that come
// from its own literal run in registers (those bytes are not stored yet when
// the loads issue), and then stores.  Sequences of <= 16 bytes are appended
// to a 32-byte register buffer (cur | cur1, output [ca, o)) that leaves as
// one 32-byte store per 32 bytes filled; match sources still in the buffer
// are overlaid from it.  So most sequences issue no store, and the next
// sequence's loads do not wait behind stores (gfx9 counts loads and stores in
// one vmcnt).  Longer sequences store their 16-byte chunks at once, up to 15
// bytes past their end (wild: the next sequence overwrites them).  Each
// caller decides when that overshoot is not allowed, runs its own exact
// copies then (wc_flush first, b.ca = the sequence's end after), and loads
// the literal registers its own way.  P: the caller's position type
// (lz4_block_lane keeps 32-bit positions: it is held at 128 VGPRs).
template <class P>
struct WcBuf {
    V16 cur, cur1;
    P ca;  // output below ca is in memory; [ca, o) in cur | cur1 (o - ca < 32)
};
template <class P>
RPC_HD void wc_flush(WcBuf<P>& b, uint8_t* out, P o) {
    const uint64_t f = (uint64_t)(o - b.ca);
    if (f >= 16) {
        v16_st(out + b.ca, b.cur);
        if (f > 16) st_part(out + b.ca + 16, b.cur1.lo, b.cur1.hi, f - 16);
    } else if (f) {
        st_part(out + b.ca, b.cur.lo, b.cur.hi, f);
    }
    b.ca = o;
}
template <class P>
RPC_HD bool wc_fits(P ll, P ml, P off) {
    const bool pat = off < 16;
    const P nch = pat ? 1 : (ml + 15) >> 4;
    return !(ll > 32 || (!pat && (ml > 32 || off < 16 * nch)));
}
// literals L0 | L1 (the first min(ll, 32) bytes of the run, loaded by the
// caller) at out + o, then a match of ml bytes at distance off >= 1;
// wc_fits(ll, ml, off), positions below 2^31
template <class P>
RPC_HD void wc_exec(WcBuf<P>& b, uint8_t* out, P o, const V16& L0, const V16& L1, P ll, P ml, P off) {
    typedef typename std::make_signed<P>::type S;
    const P op_m = o + ll, end = op_m + ml;
    const bool pat = off < 16;
    const P nch = pat ? 1 : (ml + 15) >> 4;
    // one round trip: every load of the sequence, then its stores
    const S rel = (S)ll - (S)off;  // match source start - literal start
    const uint8_t* src = out + op_m - off;
    V16 A0{0, 0}, A1{0, 0};
    if (rel < 0) A0 = v16_ld(src);
    if (!pat && nch > 1 && rel + 16 < 0) A1 = v16_ld(src + 16);
    if (o > b.ca && rel < 0) {
        // source bytes in [ca, o) are still in cur | cur1 (bytes from o on
        // are the literal run's, merged below)
        const int32_t sb = (int32_t)(op_m - off), ca = (int32_t)b.ca;
        A0 = v16_overlay(v16_overlay(A0, sb, b.cur, ca), sb, b.cur1, ca + 16);
        if (!pat && nch > 1 && rel + 16 < 0)
            A1 = v16_overlay(v16_overlay(A1, sb + 16, b.cur, ca), sb + 16, b.cur1, ca + 16);
    }
    // 16 source bytes at literal-relative r: stored bytes (A) below the
    // literal run, the run's own bytes (registers) from it on
    const S r0 = rel, r1 = rel + 16;
    const V16 c0 = r0 >= 0 ? v16_ext(L0, L1, (uint32_t)r0)
                   : r0 <= -16 ? A0 : v16_merge(A0, v16_shl(L0, (uint32_t)-r0), (uint32_t)-r0);
    const V16 first = pat ? period16(c0, (uint64_t)off) : c0;  // the match's first 16 bytes
    if (ll + ml <= 16) {
        // the whole sequence in one 16-byte piece (most text sequences),
        // appended to `cur`; a store only when 32 bytes are complete (no
        // store: the next sequence's loads wait for none)
        const V16 sq = ll ? v16_merge(L0, v16_shl(first, (uint32_t)ll), (uint32_t)ll) : first;
        const uint32_t f = (uint32_t)(o - b.ca);
        if (f < 16) {  // f + ll + ml < 32: nothing to store
            b.cur = f ? v16_merge(b.cur, v16_shl(sq, f), f) : sq;
            b.cur1 = v16_ext(sq, V16{0, 0}, 16 - f);
        } else {
            const uint32_t g = f - 16;
            const V16 c1 = g ? v16_merge(b.cur1, v16_shl(sq, g), g) : sq;
            if (f + (uint32_t)(ll + ml) >= 32) {
                v16_st(out + b.ca, b.cur);
                v16_st(out + b.ca + 16, c1);
                b.cur = v16_ext(sq, V16{0, 0}, 16 - g);
                b.ca += 32;
            } else {
                b.cur1 = c1;
            }
        }
        return;
    }
    if (o > b.ca) v16_st(out + b.ca, b.cur);  // wild: the stores below overwrite [o, ca + 32)
    if (o > b.ca + 16) v16_st(out + b.ca + 16, b.cur1);
    b.ca = end;
    if (ll > 0) v16_st(out + o, L0);
    if (ll > 16) v16_st(out + o + 16, L1);
    if (pat) {
        const uint64_t step = period_step((uint64_t)off);
        for (uint64_t i = 0; i < (uint64_t)ml; i += step) v16_st(out + op_m + i, first);
    } else {
        v16_st(out + op_m, c0);
        if (nch > 1) {
            const V16 c1 = r1 >= 0 ? v16_ext(L0, L1, (uint32_t)r1)
                           : r1 <= -16 ? A1 : v16_merge(A1, v16_shl(L0, (uint32_t)-r1), (uint32_t)-r1);
            v16_st(out + op_m + 16, c1);
        }
    }
}

}  // namespace rpcodec
#endif
