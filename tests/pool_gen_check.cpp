// Host run of the device generator's draw (marl-sat_amd/csrc/pool_gen.h, the functions pool_generate_kernel
// stores every word with).  Built under ASan + UBSan by the Makefile target pool_gen_check and run by
// tests/test_pool_generate_cpu.py, which compares every printed word with tests/pool_generate_replay.py.
//
//   pool_gen_check SEED COUNTER N ATTEMPT V C K
// prints one attempt of one instance: a line "hidden" with V bits, then C lines "clause" with K signed literals,
// then "pool_gen_check: ok".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pool_gen.h"

int main(int argc, char **argv) {
    if (argc != 8) {
        std::fprintf(stderr, "usage: %s SEED COUNTER N ATTEMPT V C K\n", argv[0]);
        return 2;
    }
    const uint64_t seed = std::strtoull(argv[1], nullptr, 0), counter = std::strtoull(argv[2], nullptr, 0);
    const uint32_t n = (uint32_t)std::strtoul(argv[3], nullptr, 0), attempt = (uint32_t)std::strtoul(argv[4], nullptr, 0);
    const int V = std::atoi(argv[5]), C = std::atoi(argv[6]), K = std::atoi(argv[7]);
    if (V < 1 || C < 1 || K < 1 || K > msat::kPgMaxWidth || K > V || attempt > (uint32_t)msat::kPgMaxAttempts ||
        (uint64_t)msat::pg_hidden_blocks(V) + (uint64_t)C >= msat::kPgMaxBlocks) {
        std::fprintf(stderr, "pool_gen_check: bad shape\n");
        return 2;
    }
    const int HB = msat::pg_hidden_blocks(V);
    // exactly the words the kernel keeps in LDS: no slack, so an index past them is an ASan report
    std::vector<uint32_t> hidden((size_t)HB * 4);
    std::vector<msat::PgWords> blocks((size_t)HB);
    for (int b = 0; b < HB; ++b) {
        blocks[b] = msat::pg_block(seed, counter, n, attempt, (uint32_t)b);
        for (int k = 0; k < 4; ++k) hidden[(size_t)4 * b + k] = blocks[b].q[k];
    }
    std::printf("hidden");
    for (int v = 0; v < V; ++v) {
        const uint32_t bit = msat::pg_hidden_bit(blocks[v / 128], v);
        if (bit != ((hidden[v >> 5] >> (v & 31)) & 1u)) {  // the block form and the flat bit array agree
            std::fprintf(stderr, "pool_gen_check: hidden bit %d differs between its two forms\n", v);
            return 1;
        }
        std::printf(" %u", bit);
    }
    std::printf("\n");
    std::vector<int32_t> lits((size_t)K);
    for (int c = 0; c < C; ++c) {
        const msat::PgWords w = msat::pg_block(seed, counter, n, attempt, (uint32_t)(HB + c));
        msat::pg_clause(w, hidden.data(), V, K, lits.data());
        std::printf("clause");
        for (int k = 0; k < K; ++k) std::printf(" %" PRId32, lits[k]);
        std::printf("\n");
    }
    std::printf("pool_gen_check: ok\n");
    return 0;
}
