// Host-only driver of the single-agent PPO entry points' argument validation (csrc/single_ppo.hip), built against the
// AddressSanitizer objects of the library (marl-sat_amd/Makefile `debug`) and run on the CPU by
// tests/test_single_rl_host_cpu.py.  Every call below is answered by the host glue before anything reaches a GPU:
// bad arguments get MSAT_EBADARG with a message, empty batches MSAT_OK without a launch.  Exit 0 when every check holds.
#include <math.h>
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

struct Loss {
    const float *logits;
    int S, V;
    const int32_t *action;
    const float *old_logp, *adv, *value, *targets;
    float clip_eps;
    int minibatch;
    float *dlogits, *dvalue, *row_terms;
    double *sums;
};

static int call(const Loss &a) {
    return msat_ppo_single_loss(a.logits, a.S, a.V, a.action, a.old_logp, a.adv, a.value, a.targets, a.clip_eps, 0.01f,
                                0.5f, a.minibatch, a.dlogits, a.dvalue, a.row_terms, a.sums, nullptr);
}

int main() {
    static float f[8];
    static int32_t i32[8];
    static uint8_t u8[8];
    static double d[8];
    // ---- msat_ppo_single_loss: the pointers are never dereferenced, validation fails first
    const Loss ok = {f, 2, 4, i32, f, f, f, f, 0.2f, 2, f, f, f, d};
    Loss a = ok;
    a.S = -1;
    expect(call(a), MSAT_EBADARG, "S -1", "loss S < 0");
    a = ok;
    a.V = 0;
    expect(call(a), MSAT_EBADARG, "V 0", "loss V < 1");
    a = ok;
    a.minibatch = 0;
    expect(call(a), MSAT_EBADARG, "minibatch 0", "loss minibatch < 1");
    const float bad_eps[] = {0.0f, -0.2f, NAN, INFINITY, -INFINITY};
    for (float e : bad_eps) {
        a = ok;
        a.clip_eps = e;
        expect(call(a), MSAT_EBADARG, "clip_eps", "loss clip_eps");
        a.S = 0;  // an empty batch does not excuse it
        expect(call(a), MSAT_EBADARG, "clip_eps", "loss clip_eps, S = 0");
    }
    for (int k = 0; k < 10; ++k) {
        a = ok;
        if (k == 0) a.logits = nullptr;
        if (k == 1) a.action = nullptr;
        if (k == 2) a.old_logp = nullptr;
        if (k == 3) a.adv = nullptr;
        if (k == 4) a.value = nullptr;
        if (k == 5) a.targets = nullptr;
        if (k == 6) a.dlogits = nullptr;
        if (k == 7) a.dvalue = nullptr;
        if (k == 8) a.row_terms = nullptr;
        if (k == 9) a.sums = nullptr;
        expect(call(a), MSAT_EBADARG, "NULL", "loss NULL pointer");
    }
    a = ok;
    a.S = 0;
    expect(call(a), MSAT_OK, nullptr, "loss S = 0");
    const Loss none = {nullptr, 0, 1, nullptr, nullptr, nullptr, nullptr, nullptr, 0.2f, 1,
                       nullptr, nullptr, nullptr, nullptr};
    expect(call(none), MSAT_OK, nullptr, "loss S = 0 with NULL pointers");

    // ---- msat_standardize_pop
    expect(msat_standardize_pop(nullptr, 0, nullptr, nullptr), MSAT_OK, nullptr, "standardize n = 0");
    expect(msat_standardize_pop(f, 0, d, nullptr), MSAT_OK, nullptr, "standardize n = 0 with pointers");
    expect(msat_standardize_pop(nullptr, 4, d, nullptr), MSAT_EBADARG, "NULL", "standardize NULL x");
    expect(msat_standardize_pop(f, 4, nullptr, nullptr), MSAT_EBADARG, "NULL", "standardize NULL moments");

    // ---- msat_clip_global_norm
    if (msat_clip_global_norm_workspace_doubles(0) < 1 || msat_clip_global_norm_workspace_doubles(1) < 1 ||
        msat_clip_global_norm_workspace_doubles((size_t)1 << 40) > 1024) {
        printf("FAIL clip workspace sizes\n");
        g_fail = 1;
    }
    const float bad_norm[] = {0.0f, -1.0f, NAN, INFINITY, -INFINITY};
    for (float m : bad_norm) {
        expect(msat_clip_global_norm(f, 4, m, d, f, nullptr), MSAT_EBADARG, "max_norm", "clip max_norm");
        expect(msat_clip_global_norm(nullptr, 0, m, d, f, nullptr), MSAT_EBADARG, "max_norm", "clip max_norm, n = 0");
    }
    expect(msat_clip_global_norm(nullptr, 4, 1.0f, d, f, nullptr), MSAT_EBADARG, "NULL", "clip NULL grads");
    expect(msat_clip_global_norm(f, 4, 1.0f, nullptr, f, nullptr), MSAT_EBADARG, "NULL", "clip NULL workspace");
    expect(msat_clip_global_norm(f, 4, 1.0f, d, nullptr, nullptr), MSAT_EBADARG, "NULL", "clip NULL norm_out");
    expect(msat_clip_global_norm(nullptr, 0, 1.0f, nullptr, f, nullptr), MSAT_EBADARG, "NULL",
           "clip n = 0, NULL workspace");
    expect(msat_clip_global_norm(nullptr, 0, 1.0f, d, f, nullptr), MSAT_OK, nullptr, "clip n = 0");
    expect(msat_clip_global_norm(f, 0, 0.5f, d, f, nullptr), MSAT_OK, nullptr, "clip n = 0 with a pointer");

    // ---- msat_episode_track
    expect(msat_episode_track(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), MSAT_OK,
           nullptr, "track B = 0");
    expect(msat_episode_track(-1, 0, f, u8, u8, f, i32, u8, u8, nullptr), MSAT_EBADARG, "B -1", "track B < 0");
    expect(msat_episode_track(2, -1, f, u8, u8, f, i32, u8, u8, nullptr), MSAT_EBADARG, "step index", "track t < 0");
    expect(msat_episode_track(0, -1, f, u8, u8, f, i32, u8, u8, nullptr), MSAT_EBADARG, "step index",
           "track t < 0, B = 0");
    for (int k = 0; k < 7; ++k) {
        expect(msat_episode_track(2, 0, k == 0 ? nullptr : f, k == 1 ? nullptr : u8, k == 2 ? nullptr : u8,
                                  k == 3 ? nullptr : f, k == 4 ? nullptr : i32, k == 5 ? nullptr : u8,
                                  k == 6 ? nullptr : u8, nullptr),
               MSAT_EBADARG, "NULL", "track NULL pointer");
    }
    printf(g_fail ? "single_ppo_host_check: FAILED\n" : "single_ppo_host_check: ok\n");
    return g_fail;
}
