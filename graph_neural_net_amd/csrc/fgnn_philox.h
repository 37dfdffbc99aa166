// The counter-based randomness of the pair streams (pairgen.hip, planted.hip): raw 32-bit draw t of stream s of pair k is word t & 7
// (low half first) of Philox4x64-10 at counter (t >> 3, k, s, 0) under key (seed, 0).  Integers in [0, k) are (u32 * k) >> 32
// (tests/pairgen_ref.py restates it in numpy, bit for bit).
#pragma once
#include "fgnn_common.h"

struct P4 {
    unsigned long long v0, v1, v2, v3;
};

// Random123 Philox4x64-10 (Salmon et al., SC'11) on counter (c0, c1, c2, c3), key (k0, 0); c3 = 0 for every pair stream
DEVI P4 philox(unsigned long long c0, unsigned long long c1, unsigned long long c2, unsigned long long k0, unsigned long long c3 = 0) {
    const unsigned long long M0 = 0xD2E7470EE14C6C93ull, M1 = 0xCA5A826395121157ull;
    unsigned long long k1 = 0;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B97F4A7C15ull;
            k1 += 0xBB67AE8584CAA73Bull;
        }
        const unsigned long long hi0 = __umul64hi(M0, c0), lo0 = M0 * c0;
        const unsigned long long hi1 = __umul64hi(M1, c2), lo1 = M1 * c2;
        const unsigned long long n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
    }
    return P4{c0, c1, c2, c3};
}

DEVI unsigned word_of(const P4 &r, int w) {
    const unsigned long long x = w < 2 ? r.v0 : w < 4 ? r.v1 : w < 6 ? r.v2 : r.v3;
    return (w & 1) ? (unsigned)(x >> 32) : (unsigned)x;
}

struct Pair {
    unsigned long long seed, k;
    DEVI unsigned draw(int stream, unsigned long long t) const { return word_of(philox(t >> 3, k, stream, seed), (int)(t & 7)); }
    DEVI P4 block(int stream, unsigned long long q) const { return philox(q, k, stream, seed); }
};

DEVI int below(unsigned u, int k) { return (int)(((unsigned long long)u * (unsigned)k) >> 32); }
DEVI int uni(int x) { return __builtin_amdgcn_readfirstlane(x); }
