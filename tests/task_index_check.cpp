// Host sweep of the sparse task loop's carried index (marl-sat_amd/csrc/obs_sparse.h: task_first, task_stride,
// task_advance -- the functions the env kernel runs) against t / U, t % U.  Stand-alone, built with the host compiler
// under ASan + UBSan (Makefile target task_index_check); tests/test_env_delta_width_cpu.py builds and runs it.
//
// T in {64, 128, 256, 512} x every U in [3, 200] x A in [1, 65], every lane, every pass of the kernel's loop
// (for t0 = 0; t0 < A U; t0 += T), one pass past the end included.  The sweep must have met U > T, U dividing T,
// A U < T and A U an exact multiple of T.
#include <stdio.h>

#include <vector>

#include "obs_sparse.h"

using namespace msat;

int main() {
    long checked = 0;
    bool u_gt_t = false, u_div_t = false, au_lt_t = false, au_mult_t = false;
    for (int T : {64, 128, 256, 512}) {
        for (int U = 3; U <= 200; ++U) {
            const TaskIdx stride = task_stride(T, U);
            if (stride.i * U + stride.s != T || stride.s < 0 || stride.s >= U) {
                printf("task_stride(%d, %d) = (%d, %d)\n", T, U, stride.i, stride.s);
                return 1;
            }
            u_gt_t |= U > T;
            u_div_t |= T % U == 0;
            for (int A = 1; A <= 65; ++A) {
                au_lt_t |= A * U < T;
                au_mult_t |= (A * U) % T == 0;
                std::vector<int> seen((size_t)A * U, 0);  // every task exactly once (ASan guards the index)
                for (int lane = 0; lane < T; ++lane) {
                    TaskIdx k = task_first(lane, U);
                    for (int t0 = 0; t0 < A * U + T; t0 += T) {  // (the kernel stops one pass earlier)
                        const int t = t0 + lane;
                        if (k.i != t / U || k.s != t % U) {
                            printf("T %d U %d A %d lane %d t %d: carried (%d, %d), want (%d, %d)\n", T, U, A, lane, t,
                                   k.i, k.s, t / U, t % U);
                            return 1;
                        }
                        const bool live = k.i < A;
                        if (live != (t < A * U)) {
                            printf("T %d U %d A %d t %d: live %d\n", T, U, A, t, (int)live);
                            return 1;
                        }
                        if (live && t0 < A * U) ++seen[(size_t)k.i * U + k.s];
                        task_advance(k, stride, U);
                        ++checked;
                    }
                }
                for (int v : seen)
                    if (v != 1) {
                        printf("T %d U %d A %d: a task taken %d times\n", T, U, A, v);
                        return 1;
                    }
            }
        }
    }
    if (!(u_gt_t && u_div_t && au_lt_t && au_mult_t)) {
        printf("sweep missed a case: %d %d %d %d\n", u_gt_t, u_div_t, au_lt_t, au_mult_t);
        return 1;
    }
    printf("task_index_check: ok (%ld index pairs)\n", checked);
    return 0;
}
