// Host-only driver of msat_walksat's argument validation, built against the AddressSanitizer objects of the
// library (marl-sat_amd/Makefile `debug`) and run on the CPU by tests/test_walksat_cpu.py.  Every call below is
// answered by the host glue before anything reaches a GPU: the validation branches, the LDS plan arithmetic of
// every kernel form and the error channel run under ASan.  Exit 0 when every check holds.
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
    const int32_t *pidx;
    int S, max_flips, form;
    uint8_t *x, *solved;
    int32_t *flips, *nun;
};

static int call(const Args &a) {
    return msat_walksat(a.lits, a.N, a.V, a.C, a.pidx, a.S, nullptr, a.max_flips, 0x80000000u, 1, 2, a.form, a.x,
                        a.solved, a.flips, a.nun, nullptr);
}

int main() {
    static uint16_t lits[4];
    static int32_t i32[4];
    static uint8_t u8[4];
    const Args ok = {lits, 1, 20, 91, i32, 2, 10, 0, u8, u8, i32, i32};  // never dereferenced: validation fails first
    const int forms = msat_walksat_forms();
    if (forms < 1) g_fail = 1;
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
    a.max_flips = -1;
    expect(call(a), MSAT_EBADARG, "max_flips -1", "max_flips -1");
    a = ok;
    a.S = -1;
    expect(call(a), MSAT_EBADARG, "num_samples -1", "num_samples -1");
    a = ok;
    a.form = forms + 1;
    expect(call(a), MSAT_EBADARG, "form", "form past the last");
    a = ok;
    a.form = -1;
    expect(call(a), MSAT_EBADARG, "form -1", "form -1");
    a = ok;
    a.lits = nullptr;
    expect(call(a), MSAT_EBADARG, "NULL", "NULL lits");
    a = ok;
    a.nun = nullptr;
    expect(call(a), MSAT_EBADARG, "NULL", "NULL num_unsat");
    const int caps[4] = {128, 256, 512, 1023};
    for (int f = 1; f <= 4 && f <= forms; ++f) {
        a = ok;
        a.form = f;
        a.C = caps[f - 1] + 1;
        expect(call(a), MSAT_EBADARG, "holds num_clauses", "forced register form past its clauses");
    }
    // the LDS plans at the largest dimensions the entry accepts, and far past them
    const int big[][2] = {{32000, 1}, {32000, 4200}, {1, 8200}, {32000, 2147483647}, {3000, 3000}};
    for (const auto &vc : big) {
        for (int f = 0; f <= forms; ++f) {
            a = ok;
            a.V = vc[0];
            a.C = vc[1];
            a.form = f;
            a.S = 0;  // an accepted shape returns MSAT_OK without a launch
            const int rc = call(a);
            if (rc != MSAT_OK && rc != MSAT_EBADARG) {
                printf("FAIL plan V %d C %d form %d: rc %d\n", vc[0], vc[1], f, rc);
                g_fail = 1;
            }
        }
    }
    a = ok;
    a.V = 32000;
    a.C = 4200;
    expect(call(a), MSAT_EBADARG, "LDS", "shape past the LDS bound");
    a = ok;
    a.S = 0;
    a.lits = nullptr;
    a.pidx = nullptr;
    expect(call(a), MSAT_OK, nullptr, "empty batch");
    printf(g_fail ? "walksat_host_check: FAILED\n" : "walksat_host_check: ok\n");
    return g_fail;
}
