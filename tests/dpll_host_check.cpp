// Host-only driver of msat_dpll's argument validation, built against the AddressSanitizer objects of the
// library (marl-sat_amd/Makefile `debug`) and run on the CPU by tests/test_dpll_cpu.py.  Every call below is
// answered by the host glue before anything reaches a GPU: the validation branches, the LDS plan arithmetic and
// the error channel run under ASan.  Exit 0 when every check holds.
#include <stdio.h>
#include <string.h>

#include "marlsat.h"

static int g_fail = 0;

static void expect(int rc, int want, const char *needle, const char *what) {
    const char *msg = msat_last_error();
    if (rc != want || (needle && !strstr(msg, needle))) {
        printf("FAIL %s: rc %d (want %d), message '%s' (want '%s')\n", what, rc, want, msg, needle ? needle : "");
        g_fail = 1;
    }
}

struct Args {
    const uint16_t *lits;
    int N, V, C;
    const int32_t *pidx, *cube;
    int S, cube_bits, max_nodes;
    uint8_t *status, *x;
    int32_t *nodes, *conflicts, *props;
};

static int call(const Args &a) {
    return msat_dpll(a.lits, a.N, a.V, a.C, a.pidx, a.cube, a.S, a.cube_bits, a.max_nodes, a.status, a.x, a.nodes,
                     a.conflicts, a.props, nullptr);
}

// the header's plan: 8 C + 14 V + V rounded up to 16
static long long plan(long long V, long long C) { return 8 * C + 14 * V + ((V + 15) / 16) * 16; }

int main() {
    static uint16_t lits[4];
    static int32_t i32[4];
    static uint8_t u8[4];
    // never dereferenced: validation fails first
    const Args ok = {lits, 1, 20, 91, i32, nullptr, 2, 0, 10, u8, u8, i32, i32, i32};
    Args a = ok;
    a.V = 0;
    expect(call(a), MSAT_EBADARG, "num_vars 0", "num_vars 0");
    a = ok;
    a.V = 32001;
    expect(call(a), MSAT_EBADARG, "num_vars 32001", "num_vars 32001");
    a = ok;
    a.C = 0;
    expect(call(a), MSAT_EBADARG, "num_clauses 0", "num_clauses 0");
    a = ok;
    a.N = 0;
    expect(call(a), MSAT_EBADARG, "num_problems 0", "num_problems 0");
    a = ok;
    a.S = -1;
    expect(call(a), MSAT_EBADARG, "num_samples -1", "num_samples -1");
    a = ok;
    a.max_nodes = -1;
    expect(call(a), MSAT_EBADARG, "max_nodes -1", "max_nodes -1");
    a = ok;
    a.cube_bits = -1;
    expect(call(a), MSAT_EBADARG, "cube_bits -1", "cube_bits -1");
    a = ok;
    a.cube_bits = 31;
    expect(call(a), MSAT_EBADARG, "cube_bits 31", "cube_bits 31");
    a = ok;
    a.lits = nullptr;
    expect(call(a), MSAT_EBADARG, "NULL", "NULL lits");
    a = ok;
    a.pidx = nullptr;
    expect(call(a), MSAT_EBADARG, "NULL", "NULL problem_idx");
    a = ok;
    a.status = nullptr;
    expect(call(a), MSAT_EBADARG, "NULL", "NULL status");
    a = ok;
    a.x = nullptr;
    expect(call(a), MSAT_EBADARG, "NULL", "NULL assign_out");
    a = ok;
    a.nodes = nullptr;
    expect(call(a), MSAT_EBADARG, "NULL", "NULL nodes");
    a = ok;
    a.conflicts = nullptr;
    expect(call(a), MSAT_EBADARG, "NULL", "NULL conflicts");
    a = ok;
    a.props = nullptr;
    expect(call(a), MSAT_EBADARG, "NULL", "NULL propagations");
    // the LDS plan on both sides of the bound, at the largest dimensions the entry accepts and far past them
    // (S = 0: an accepted shape returns MSAT_OK without a launch)
    const int shapes[][2] = {{1, 1},     {300, 1290}, {1, 8188},  {1, 8189},       {4368, 1},
                             {4369, 1},  {2000, 4442}, {2000, 4443}, {32000, 1},   {32000, 2147483647},
                             {1, 2147483647}, {3000, 3000}};
    for (const auto &vc : shapes) {
        a = ok;
        a.V = vc[0];
        a.C = vc[1];
        a.S = 0;
        const bool fits = plan(vc[0], vc[1]) <= 65536;
        char what[64];
        snprintf(what, sizeof what, "plan V %d C %d", vc[0], vc[1]);
        expect(call(a), fits ? MSAT_OK : MSAT_EBADARG, fits ? nullptr : "LDS", what);
    }
    a = ok;
    a.S = 0;
    a.lits = nullptr;
    a.pidx = nullptr;
    a.status = nullptr;
    a.x = nullptr;
    a.nodes = a.conflicts = a.props = nullptr;
    expect(call(a), MSAT_OK, nullptr, "empty batch");
    printf(g_fail ? "dpll_host_check: FAILED\n" : "dpll_host_check: ok\n");
    return g_fail;
}
