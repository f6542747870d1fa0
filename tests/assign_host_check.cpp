// Host-only driver of msat_assign_loss' argument validation (csrc/assign_loss.hip), built against the
// AddressSanitizer objects of the library (marl-sat_amd/Makefile `debug`) and run on the CPU by
// tests/test_assign_host_cpu.py.  Every call below is answered by the host glue before anything reaches a GPU:
// bad arguments get MSAT_EBADARG with a message, an empty batch MSAT_OK without a launch.  Exit 0 when every check
// holds.
#include <stdio.h>
#include <string.h>

#include "marlsat.h"
#include "marlsat_net.h"

static int g_fail = 0;

static void expect(int rc, int want, const char *needle, const char *what) {
    const char *msg = msat_last_error();
    if (rc != want || (want != MSAT_OK && (!msg || !*msg)) || (needle && !strstr(msg, needle))) {
        printf("FAIL %s: rc %d (want %d), message '%s' (want '%s')\n", what, rc, want, msg ? msg : "(null)",
               needle ? needle : "");
        g_fail = 1;
    }
}

struct Args {
    const float *logits;
    int S, V;
    const uint8_t *labels;
    int minibatch;
    const uint16_t *lits;
    int N, C;
    const int32_t *problem_idx;
    float *dlogits;
    uint8_t *pred;
    float *sample_nll;
    int32_t *sample_correct, *sample_unsat;
    uint8_t *sample_solved;
    double *sums;
};

static int call(const Args &a) {
    return msat_assign_loss(a.logits, a.S, a.V, a.labels, a.minibatch, a.lits, a.N, a.C, a.problem_idx, a.dlogits,
                            a.pred, a.sample_nll, a.sample_correct, a.sample_unsat, a.sample_solved, a.sums, nullptr);
}

int main() {
    static float f[16], g[16], nll[8];
    static uint8_t lab[8], pred[8], solved[8];
    static uint16_t lits[16];
    static int32_t idx[8], correct[8], unsat[8];
    static double d[8];
    // the pointers are never dereferenced: validation fails first
    const Args ok = {f, 2, 4, lab, 2, lits, 1, 1, idx, g, pred, nll, correct, unsat, solved, d};
    Args a = ok;
    a.S = -1;
    expect(call(a), MSAT_EBADARG, "S -1", "S < 0");
    a = ok;
    a.V = 0;
    expect(call(a), MSAT_EBADARG, "V 0", "V < 1");
    a = ok;
    a.V = 32001;
    expect(call(a), MSAT_EBADARG, "V 32001", "V above WalkSAT's bound");
    a = ok;
    a.C = 0;
    expect(call(a), MSAT_EBADARG, "num_clauses 0", "num_clauses < 1");
    a = ok;
    a.N = 0;
    expect(call(a), MSAT_EBADARG, "num_problems 0", "num_problems < 1");
    a = ok;
    a.minibatch = 0;
    expect(call(a), MSAT_EBADARG, "minibatch 0", "minibatch < 1");
    a.S = 0;  // an empty batch does not excuse it
    expect(call(a), MSAT_EBADARG, "minibatch 0", "minibatch < 1, S = 0");
    a = ok;
    a.dlogits = nullptr;
    expect(call(a), MSAT_EBADARG, "labels and dlogits", "labels without dlogits");
    a = ok;
    a.labels = nullptr;
    expect(call(a), MSAT_EBADARG, "labels and dlogits", "dlogits without labels");
    for (int k = 0; k < 9; ++k) {  // training mode: every pointer is required
        a = ok;
        if (k == 0) a.logits = nullptr;
        if (k == 1) a.lits = nullptr;
        if (k == 2) a.problem_idx = nullptr;
        if (k == 3) a.pred = nullptr;
        if (k == 4) a.sample_unsat = nullptr;
        if (k == 5) a.sample_solved = nullptr;
        if (k == 6) a.sample_nll = nullptr;
        if (k == 7) a.sample_correct = nullptr;
        if (k == 8) a.sums = nullptr;
        expect(call(a), MSAT_EBADARG, "NULL", "NULL pointer with labels");
    }
    for (int k = 0; k < 6; ++k) {  // predict only: sample_nll, sample_correct and sums may be NULL, the rest not
        a = ok;
        a.labels = nullptr;
        a.dlogits = nullptr;
        a.sample_nll = nullptr;
        a.sample_correct = nullptr;
        a.sums = nullptr;
        if (k == 0) a.logits = nullptr;
        if (k == 1) a.lits = nullptr;
        if (k == 2) a.problem_idx = nullptr;
        if (k == 3) a.pred = nullptr;
        if (k == 4) a.sample_unsat = nullptr;
        if (k == 5) a.sample_solved = nullptr;
        expect(call(a), MSAT_EBADARG, "NULL", "NULL pointer, predict only");
    }
    a = ok;
    a.S = 0;
    expect(call(a), MSAT_OK, nullptr, "S = 0");
    const Args none = {nullptr, 0, 1, nullptr, 1, nullptr, 1, 1, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr};
    expect(call(none), MSAT_OK, nullptr, "S = 0 with NULL pointers");
    printf(g_fail ? "assign_host_check: FAILED\n" : "assign_host_check: ok\n");
    return g_fail;
}
