// The draw of msat_pool_generate (include/marlsat.h): planted random k-SAT, one Philox4x32-10 block per clause
// and per 128 hidden bits.  The semantics are the reference generator's (src/utils/generate_cnf_dataset.py:5-42:
// a hidden assignment; per clause K distinct variables, one uniformly chosen slot forced to agree with the
// hidden assignment, a coin for every other sign); the words are Philox's, not the Mersenne Twister's, so the
// instances are of the same family, not the same bytes.
//
// Plain C++ (host and device): pool_generate_kernel (pool_gen.hip) calls pg_block / pg_hidden_bit / pg_clause
// for every word it stores, tests/pool_gen_check.cpp calls the same functions on the host under ASan + UBSan
// and prints what they give, and tests/pool_generate_replay.py restates them on oracle.rng.philox4x32_10.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MSAT_PG_HD __host__ __device__ __forceinline__
#else
#define MSAT_PG_HD inline
#endif

namespace msat {

constexpr int kPgMaxWidth = 3;            // K <= 3: q0..q2 drive the K picks, q3 the anchor and the signs
constexpr uint32_t kPgMaxBlocks = 1u << 24;  // HB + C < 2^24: the block shares counter word 3 with the attempt
constexpr int kPgMaxAttempts = 255;       // attempt < 2^8

struct PgWords {
    uint32_t q[4];
};

MSAT_PG_HD uint32_t pg_mulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * (uint64_t)b) >> 32); }

// Philox4x32-10 (Salmon et al., SC'11), the function of csrc/common.h and oracle/rng.py.
MSAT_PG_HD PgWords pg_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = pg_mulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = pg_mulhi(M1, c2), lo1 = M1 * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0;
        c1 = lo1;
        c2 = n2;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return PgWords{{c0, c1, c2, c3}};
}

// Hidden-bit blocks of V variables: HB = ceil(V / 128).
MSAT_PG_HD int pg_hidden_blocks(int V) { return (V + 127) / 128; }

// Block `block` of instance n at `attempt`: key (seed lo, seed hi), counter (counter lo, counter hi, n,
// (attempt << 24) | block).  Blocks 0 .. HB-1 are the hidden bits, block HB + c is clause c.
MSAT_PG_HD PgWords pg_block(uint64_t seed, uint64_t counter, uint32_t n, uint32_t attempt, uint32_t block) {
    return pg_philox((uint32_t)counter, (uint32_t)(counter >> 32), n, (attempt << 24) | block, (uint32_t)seed,
                     (uint32_t)(seed >> 32));
}

// Hidden bit of variable v (0-based) from the words of ITS block v / 128: word (v % 128) / 32, bit v % 32, the
// layout of the reset stream's assignment blocks.  The HB blocks laid end to end are a bit array: variable v is
// bit v % 32 of word v / 32.
MSAT_PG_HD uint32_t pg_hidden_bit(const PgWords &blk, int v) { return (blk.q[(v & 127) >> 5] >> (v & 31)) & 1u; }

// Clause from the words of its block.  hidden: the HB * 4 hidden words end to end.  lits[0..K-1]: signed
// 1-based literals in pick order.
//   Variables: Floyd's sample of K of V (the msat_bc_corrupt formulation): for i = 0..K-1, j = V - K + i,
//   t = (q_i * (j + 1)) >> 32; slot i takes t unless an earlier slot holds t, then j (j is never held before:
//   earlier slots hold values <= j - 1).
//   Anchor slot a = ((q3 & 0xFFFF) * K) >> 16: its literal is positive iff the hidden bit of its variable is 1.
//   Every other slot i is positive iff bit 16 + i of q3 is 1.
// Needs 1 <= K <= min(V, kPgMaxWidth).
MSAT_PG_HD void pg_clause(const PgWords &blk, const uint32_t *hidden, int V, int K, int32_t *lits) {
    int var[kPgMaxWidth] = {0, 0, 0};
    for (int i = 0; i < K; ++i) {
        const int j = V - K + i;
        const int t = (int)pg_mulhi(blk.q[i], (uint32_t)j + 1u);
        bool held = false;
        for (int e = 0; e < i; ++e) held = held || (var[e] == t);
        var[i] = held ? j : t;
    }
    const uint32_t q3 = blk.q[3];
    const int anchor = (int)(((q3 & 0xFFFFu) * (uint32_t)K) >> 16);
    for (int i = 0; i < K; ++i) {
        const int v = var[i];
        const uint32_t pos = i == anchor ? (hidden[v >> 5] >> (v & 31)) & 1u : (q3 >> (16 + i)) & 1u;
        lits[i] = pos ? v + 1 : -(v + 1);
    }
}

}  // namespace msat
