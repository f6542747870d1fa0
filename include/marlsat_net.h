/*
 * marlsat_net.h — C-ABI of the MAPPO network / update kernels in libmarlsat.so
 * (gfx950).  Same conventions as marlsat.h: device pointers owned by the caller,
 * explicit dims, stream last, 0 on success / negative + msat_last_error().
 *
 * Reference computations replaced (kongqg/marl-sat):
 *   msat_gemm / msat_gemm_wgrad  <- every flax nn.Dense / nn.GRUCell matmul of
 *        GNN_ActorCritic (src/learners/mappo_gnn_sat_learner.py:44-80, :213-240,
 *        :311-349) and their jax.value_and_grad transposes (:647-649)
 */
#ifndef MARLSAT_NET_H
#define MARLSAT_NET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* C[M,N] (+)= A[M,K] @ op(B) (+ bias[N]); op(B) = B[K,N] (transB=0) or B[N,K]^T (transB=1).
 * Row-major with leading dims; fp32 in / fp32 accumulate on the matrix cores.
 * `accumulate` is a flag (here and in every export below): 0 overwrites, any nonzero value adds to
 * what the output holds.  Only the M x N (K x N for the weight gradients) elements are written; the
 * ld - N gap of every output row is left as it was, and the ld - K gaps of the inputs are never read.
 * K = 0 is admitted: C = bias (zero without bias), or C += bias with accumulate. */
int msat_gemm(const float *A, int32_t lda, const float *B, int32_t ldb, int32_t transB, float *C,
              int32_t ldc, const float *bias, int32_t M, int32_t N, int32_t K, int32_t accumulate,
              void *stream);

/* C[M,N] (+)= op(A)[M,K] @ op(B)[K,N], fp32 operands, fp64 accumulation, one rounding per
 * element; op(A) = A[M,K] (transA=0) or A[K,M]^T, op(B) = B[K,N] (transB=0) or B[N,K]^T.
 * For the small folded-weight products of the phi folding (F = W Wi per forward, dW = dF Wi^T and
 * dWi = W^T dF per backward) that stand in for the reference's separate Dense layers
 * (src/learners/mappo_gnn_sat_learner.py:66-79). */
int msat_gemm_f64acc(const float *A, int32_t lda, int32_t transA, const float *B, int32_t ldb, int32_t transB,
                     float *C, int32_t ldc, int32_t M, int32_t N, int32_t K, int32_t accumulate, void *stream);

/* fp32 GEMM on the bf16 matrix cores (gemm_x3.hip): operands split exactly into three bf16
 * parts, six bf16 MFMAs per 16-deep k step keep every product term above fp32 rounding.
 * msat_split_bf16x3: planes (3 x rows x cols bf16, contiguous) of W (rows x cols, ldw).
 * msat_gemm_x3: C[M,N] (+)= A[M,K] @ W^T (+ bias), W [N][K] given as its split planes;
 *   K % 16 == 0, lda % 4 == 0, 16-byte aligned A / planes. */
int msat_split_bf16x3(const float *W, int32_t rows, int32_t cols, int32_t ldw, void *planes, void *stream);
/* the same with the columns rotated: planes[q][r][c] = part q of W[r][(c + rot) % cols] */
int msat_split_bf16x3_rot(const float *W, int32_t rows, int32_t cols, int32_t ldw, int32_t rot, void *planes,
                          void *stream);
int msat_gemm_x3(const float *A, int32_t lda, const void *Wplanes, float *C, int32_t ldc, const float *bias,
                 int32_t M, int32_t N, int32_t K, int32_t accumulate, void *stream);
/* fp16x2 form of msat_gemm_x3 for A = a GRU backward's packed rows with their row scale exponents
 * (rexp, msat_gru_ln_bwd_g4fe): three fp16 MFMAs per product.  Wplanes_h2 = msat_split_f16x2_rot of W
 * (fp16x2 planes of 2^10 W, *wbad = 1 if that overflowed), Wplanes_x3 = msat_split_bf16x3_rot of the
 * same W: with *wbad set the kernel runs the bf16x3 product instead.  K % 32 == 0. */
int msat_split_f16x2_rot(const float *W, int32_t rows, int32_t cols, int32_t ldw, int32_t rot, void *planes,
                         int32_t *wbad, void *stream);
/* Both data gradients of a GRU cell's packed backward rows in one launch: C0 (+)= A0 @ W0^T (N0 columns)
 * and C1 (+)= A1 @ W1^T (N1) over the same M rows (row exponents rexp), each as msat_gemm_h2. */
int msat_gemm_h2_dual(const float *A0, int32_t lda0, const void *W0_h2, const void *W0_x3, const int32_t *wbad0,
                      float *C0, int32_t ldc0, int32_t N0, int32_t acc0, const float *A1, int32_t lda1,
                      const void *W1_h2, const void *W1_x3, const int32_t *wbad1, float *C1, int32_t ldc1, int32_t N1,
                      int32_t acc1, const int32_t *rexp, int32_t M, int32_t K, void *stream);
/* The same with A0 / A1 the packed rows as fp16x2 planes (msat_gru_ln_bwd_g4fe with flags bit 3): lda in
 * fp16 elements (% 8), the lo plane plo elements after the hi plane (% 8); the rows are taken as split.
 * Bitwise the result of msat_gemm_h2_dual on the fp32 rows (the planes are the split it would make). */
int msat_gemm_h2_dual_planes(const void *A0, int32_t lda0, const void *W0_h2, const void *W0_x3,
                             const int32_t *wbad0, float *C0, int32_t ldc0, int32_t N0, int32_t acc0, const void *A1,
                             int32_t lda1, const void *W1_h2, const void *W1_x3, const int32_t *wbad1, float *C1,
                             int32_t ldc1, int32_t N1, int32_t acc1, int32_t plo, const int32_t *rexp, int32_t M,
                             int32_t K, void *stream);
int msat_gemm_h2(const float *A, int32_t lda, const int32_t *rexp, const void *Wplanes_h2, const void *Wplanes_x3,
                 const int32_t *wbad, float *C, int32_t ldc, const float *bias, int32_t M, int32_t N, int32_t K,
                 int32_t accumulate, void *stream);

/* W[K,N] (+)= A[M,K]^T @ G[M,N]: split over M, partial slabs reduced in a fixed order.
 * K <= 8 (feature / degree columns) streams G once instead of running 128-row MFMA tiles.
 * M = 0 is admitted by msat_gemm_wgrad, _rot, _h2 and the duals: accumulate = 0 writes zeros to
 * W[:, :N], accumulate != 0 leaves W unchanged; neither touches the ldw - N gaps. */
size_t msat_gemm_wgrad_workspace_bytes(int32_t M, int32_t K, int32_t N);
int msat_gemm_wgrad(const float *A, int32_t lda, const float *G, int32_t ldg, float *W, int32_t ldw,
                    int32_t M, int32_t K, int32_t N, int32_t accumulate, void *workspace, void *stream);
/* W[:, (n + rot) % N] (+)= (A^T G)[:, n], 0 <= rot < N: the packed GRU backward rows' gate blocks
 * (n | r | z) into a weight stored (r | z | n) in one pass (learner:62-80 update cells' input rows). */
/* The same in fp16x2 (three fp16 MFMAs per product) for G = a GRU backward's packed rows with their
 * row scale exponents rexp (msat_gru_ln_bwd_g4fe): K > 8, N <= 384, rot % 4 == 0.
 * A is split as 2^8 a: full accuracy for 2^-15 <= |a| < 2^7; |a| >= 2^7 sends its workgroup to the bf16x3
 * fixup (correct, slower), and below 2^-15 an element carries an absolute error up to 2^-33. */
int msat_gemm_wgrad_h2(const float *A, int32_t lda, const float *G, int32_t ldg, const int32_t *rexp, float *W,
                       int32_t ldw, int32_t M, int32_t K, int32_t N, int32_t rot, int32_t accumulate, void *workspace,
                       void *stream);
/* Both weight gradients of a GRU cell's packed backward rows in one fp16x2 launch: W0 (+)= A0^T G0 and
 * W1 (+)= A1^T G1 (columns rotated by rot0 / rot1) over the same M rows, row exponents rexp. */
size_t msat_gemm_wgrad_dual_workspace_bytes(int32_t M, int32_t K0, int32_t N0, int32_t K1, int32_t N1);
int msat_gemm_wgrad_h2_dual(const float *A0, int32_t lda0, const float *G0, int32_t ldg0, float *W0, int32_t ldw0,
                            int32_t K0, int32_t N0, int32_t rot0, const float *A1, int32_t lda1, const float *G1,
                            int32_t ldg1, float *W1, int32_t ldw1, int32_t K1, int32_t N1, int32_t rot1,
                            const int32_t *rexp, int32_t M, int32_t accumulate, void *workspace, void *stream);
/* The same with G0 / G1 the packed rows as fp16x2 planes (msat_gru_ln_bwd_g4fe, flags bit 3): ldg in fp16
 * elements (% 8), the lo plane plo elements after the hi plane (% 8, >= N), N % 8 == 0.  G is staged by
 * LDS-DMA with no split; the split-wide scale moves to A (a 2^(ge - e_r)). */
int msat_gemm_wgrad_h2_dual_planes(const float *A0, int32_t lda0, const void *G0, int32_t ldg0, float *W0,
                                   int32_t ldw0, int32_t K0, int32_t N0, int32_t rot0, const float *A1, int32_t lda1,
                                   const void *G1, int32_t ldg1, float *W1, int32_t ldw1, int32_t K1, int32_t N1,
                                   int32_t rot1, int32_t plo, const int32_t *rexp, int32_t M, int32_t accumulate,
                                   void *workspace, void *stream);
int msat_gemm_wgrad_rot(const float *A, int32_t lda, const float *G, int32_t ldg, float *W, int32_t ldw,
                        int32_t M, int32_t K, int32_t N, int32_t rot, int32_t accumulate, void *workspace,
                        void *stream);
/* Arithmetic path of msat_gemm_wgrad / msat_gemm_wgrad_rot: MSAT_PRECISION_FP16X2 (default) and
 * MSAT_PRECISION_BF16X3 run the fp32-accurate split kernels, MSAT_PRECISION_FP32 the fp32 MFMA tiles.
 * Set once per process (the Python host calls it at import with its validated MARLSAT_PRECISION);
 * until then the library reads MARLSAT_PRECISION once, and an unknown value there makes every weight
 * gradient fail with MSAT_EBADARG instead of picking a path.  Unknown `mode`: MSAT_EBADARG. */
#define MSAT_PRECISION_FP16X2 0
#define MSAT_PRECISION_BF16X3 1
#define MSAT_PRECISION_FP32 2
int msat_set_precision(int32_t mode);
int msat_get_precision(void); /* the mode in force, or MSAT_EBADARG if MARLSAT_PRECISION is unknown */

/* ---- graph batch assembly (learner:148-195 features + the agents' local graphs) ----
 * Block per sample: instantiate the per-instance templates (marlsat/learners/graphs.py) at the
 * sample's row bases (sample_bases (S,3) = var row, clause row, incidence starts) and compute the
 * node features from the sample's assignment x (S,V): vfeat (Nv,8) = [x, deg+/C, deg-/C, 0, n+, n-, 0, 0]
 * (static var features, then the var row's positive / negative incidence counts in its graph),
 * cfeat (Nc,3) = [is_sat, ntrue/3, 1], cdeg (Nc,4, nullable) = [n+, n-, 0, 0] positive / negative
 * literal slots of the clause row.  The counts carry the phi biases through the gather-first
 * message passing (sum_{edges} (h W + b) = (sum h) W + n b).  G = 1 (critic graph only) or A+1. */
int msat_assemble_graph_batch(
    int32_t S, int32_t G, int32_t A, int32_t V, int32_t C, const int32_t *inst, const uint8_t *x, const float *svf,
    const uint16_t *pool, const int32_t *sample_bases, const int32_t *t_vgid, const int32_t *t_cgid,
    const int32_t *t_slots, const int32_t *t_ptr, const int32_t *t_inc, const int32_t *voff, const int32_t *coff,
    const int32_t *eoff, const int32_t *poff, const int32_t *gv, const int32_t *gc, float *vfeat, float *cfeat,
    float *cdeg, int32_t *slots, int32_t *ptr, int32_t *inc, int32_t *g_vbase, int32_t *g_nv, int32_t *g_cbase, int32_t *g_nc,
    int32_t Nv, int32_t nnz, void *stream);
/* The same for graphs g0 .. g0+G-1 of each sample's instance (0 <= g0, G >= 1, g0 + G <= A+1):
 * g0 = 0 is msat_assemble_graph_batch bit for bit; g0 = 1, G = A is the actor-only batch (the agents'
 * masked encoders, learner:243-276, without the critic's unmasked one, :340-342).  The templates keep
 * graph 0 first and instance-relative row ids, so the kernel rebases t_ptr values, the var rows in
 * t_slots and the clause rows in t_inc by graph g0's starts; sample_bases, Nv and nnz are those of the
 * G graphs alone (msat_graph_bases over the per-instance counts of graphs g0 .. g0+G-1), and
 * g_vbase / g_nv / g_cbase / g_nc get G entries per sample. */
int msat_assemble_graph_batch_from(
    int32_t S, int32_t g0, int32_t G, int32_t A, int32_t V, int32_t C, const int32_t *inst, const uint8_t *x,
    const float *svf, const uint16_t *pool, const int32_t *sample_bases, const int32_t *t_vgid, const int32_t *t_cgid,
    const int32_t *t_slots, const int32_t *t_ptr, const int32_t *t_inc, const int32_t *voff, const int32_t *coff,
    const int32_t *eoff, const int32_t *poff, const int32_t *gv, const int32_t *gc, float *vfeat, float *cfeat,
    float *cdeg, int32_t *slots, int32_t *ptr, int32_t *inc, int32_t *g_vbase, int32_t *g_nv, int32_t *g_cbase, int32_t *g_nc,
    int32_t Nv, int32_t nnz, void *stream);

/* ---- message passing: signed literal gathers (the encoder's A^T M and A M, learner:66-74) ----
 * clause_gather: dst[c] (+)= [sum_{pos slots} src[v][0:H] | sum_{neg slots} src[v][H:2H]],
 *                slots (Nc,3) = (var_row << 1) | neg, or -1.
 * var_gather:    dst[v] (+)= [sum_{pos entries} src[c][0:H] | sum_{neg entries} src[c][H:2H]],
 *                CSR ptr (Nv+1), entries (clause_row << 1) | neg.  Each is the other's transpose. */
int msat_clause_gather(const float *src, int32_t ld_src, const int32_t *slots, float *dst, int32_t ld_dst,
                       int32_t num_clause_rows, int32_t H, int32_t accumulate, void *stream);
int msat_var_gather(const float *src, int32_t ld_src, const int32_t *ptr, const int32_t *inc, float *dst,
                    int32_t ld_dst, int32_t num_var_rows, int32_t H, int32_t accumulate, void *stream);
/* General forms (16-byte aligned rows, H % 32 == 0):
 * clause_gather2: positive slots read src_pos rows, negative slots src_neg rows (H wide each);
 *   merged = 0: dst[c] (+)= [sum_pos src_pos[v] | sum_neg src_neg[v]] (2H wide);
 *   merged = 1: dst[c] (+)= sum_pos src_pos[v] + sum_neg src_neg[v] (H wide; the transpose of
 *   var_gather2 with src_pos == src_neg).
 * var_gather2: dst_pos[v] (+)= sum_pos src_pos[c], dst_neg[v] (+)= sum_neg src_neg[c]. */
int msat_clause_gather2(const float *src_pos, const float *src_neg, int32_t ld_src, const int32_t *slots, float *dst,
                        int32_t ld_dst, int32_t num_clause_rows, int32_t H, int32_t merged, int32_t accumulate,
                        void *stream);
int msat_var_gather2(const float *src_pos, const float *src_neg, int32_t ld_src, const int32_t *ptr,
                     const int32_t *inc, float *dst_pos, float *dst_neg, int32_t ld_dst, int32_t num_var_rows,
                     int32_t H, int32_t accumulate, void *stream);

/* ---- fused flax GRUCell + LayerNorm (learner:69-80) ----
 * Gi = x Wi + bi, Gh = h Wh + [0,0,b_hn] (gates [r|z|n]); out = LN(GRU(h, x)).
 * Backward: dGi, dGh, dhprev (+=), LN scale/bias grads ([scale|bias] contiguous, (+)=). */
int msat_gru_ln_fwd(const float *Gi, int32_t ldi, const float *Gh, int32_t ldh, const float *hprev,
                    int32_t ldp, const float *ln_scale, const float *ln_bias, float *out, int32_t ldo,
                    int32_t R, int32_t H, void *stream);
size_t msat_gru_ln_bwd_partial_floats(int32_t R, int32_t H);
int msat_gru_ln_bwd(const float *dy, int32_t ldy, const float *Gi, int32_t ldi, const float *Gh, int32_t ldh,
                    const float *hprev, int32_t ldp, const float *ln_scale, float *dGi, int32_t lddi,
                    float *dGh, int32_t lddh, float *dhprev, int32_t lddp, float *dln_scale,
                    float *dln_bias, float *partial, int32_t R, int32_t H, int32_t accumulate_ln,
                    void *stream);
/* One kernel per GRU call on the fp32 matrix cores (gru_fused.hip): x = [x0 | x1 | x2]
 * (segment widths multiples of 4, 16-byte aligned rows; w1/w2 may be 0), Wi (Kx, 3H),
 * Wh (H, 3H), bi/bh (3H), out = LN(GRU(hprev, x)).  g4 (nullable, ldg >= 4H) receives the
 * pre-activations [r_pre | z_pre | gin | ghn] for msat_gru_ln_bwd_g4.
 * Placement: segments, hprev, wi and wh 16-byte aligned with ld % 4 == 0 (segment ld >= width, ldp >= H);
 * out, g4, bi, bh, ln_scale and ln_bias at any float address, ldo >= H and ldg >= 4H of any value.
 * Nothing outside the R rows and the named columns of an operand is read into a result or written.
 * Replaces the two gate GEMMs + msat_gru_ln_fwd of update_c / update_v_pos / update_v_neg
 * + LayerNorm_k (learner:68-80). */
int msat_gru_ln_fused_fwd(const float *x0, int32_t ld0, int32_t w0, const float *x1, int32_t ld1, int32_t w1,
                          const float *x2, int32_t ld2, int32_t w2, const float *hprev, int32_t ldp,
                          const float *wi, const float *bi, const float *wh, const float *bh,
                          const float *ln_scale, const float *ln_bias, float *out, int32_t ldo, float *g4,
                          int32_t ldg, int32_t R, int32_t H, void *stream);
/* Same cell on the bf16 matrix cores (exact bf16x3 split, fp32-accurate; H = 128; register-A on
 * 16x16x32 bf16 MFMAs: activations read straight into registers, only the weights staged): weights given as msat_split_bf16x3_t planes of Wi^T zero-padded
 * to kxp columns (kxp >= Kx, multiple of 32) and of Wh^T (kxp = H).  out and g4 rows 16-byte aligned
 * (pointer and ldo / ldg % 4 == 0); bi, bh, ln_scale, ln_bias at any float address. */
int msat_gru_ln_fused_fwd_x3r(const float *x0, int32_t ld0, int32_t w0, const float *x1, int32_t ld1, int32_t w1,
                              const float *x2, int32_t ld2, int32_t w2, const float *hprev, int32_t ldp,
                              const void *wiT_planes, int32_t kxp, const float *bi, const void *whT_planes,
                              const float *bh, const float *ln_scale, const float *ln_bias, float *out, int32_t ldo,
                              float *g4, int32_t ldg, int32_t R, int32_t H, void *stream);
/* planes[q][n][k] = bf16x3 part q of (k < K ? W[k][n] : 0) for n < N, k < Kp: the transposed,
 * zero-padded split of a (K, N) weight (row stride ldw) for msat_gru_ln_fused_fwd_x3r. */
int msat_split_bf16x3_t(const float *W, int32_t K, int32_t N, int32_t ldw, int32_t Kp, void *planes, void *stream);
/* The same GRU cell with fp16x2 operands (x = x1 + x2, three fp16 MFMAs per product instead of six
 * bf16 ones; weights from msat_split_f16x2_t, scaled by 2^10; activations scaled by 2^7 before their split so
 * that small ones keep 22 bits).  fp16's range is checked per 128-row tile: a tile whose activations reach
 * |a| >= 256 (2^15 after the scale), or every tile when a weight split flagged wbad[0]
 * (wi) or wbad[1] (wh), is recomputed by the bf16x3 kernel from wiT_x3 / whT_x3 (msat_split_bf16x3_t
 * planes) in a second launch on the same stream.  tile_flags: >= ceil(R / 128) ints of workspace. */
int msat_gru_ln_fused_fwd_h2r(const float *x0, int32_t ld0, int32_t w0, const float *x1, int32_t ld1, int32_t w1,
                              const float *x2, int32_t ld2, int32_t w2, const float *hprev, int32_t ldp,
                              const void *wiT_h2, const void *whT_h2, const void *wiT_x3, const void *whT_x3,
                              int32_t kxp, const float *bi, const float *bh, const float *ln_scale,
                              const float *ln_bias, float *out, int32_t ldo, float *g4, int32_t ldg, int32_t R,
                              int32_t H, int32_t *tile_flags, const int32_t *wbad, void *stream);
/* planes[q][n][k] = fp16x2 part q of 2^10 (k < K ? W[k][n] : 0) (n < N, k < Kp) for
 * msat_gru_ln_fused_fwd_h2r; *bad (device int, cleared first) = 1 if a scaled weight is not in
 * (-2^15, 2^15). */
int msat_split_f16x2_t(const float *W, int32_t K, int32_t N, int32_t ldw, int32_t Kp, void *planes, int32_t *bad,
                       void *stream);
/* msat_gru_ln_bwd from the fused forward's g4 tape (same outputs).  dbi (3H) / dbh_n (H), both
 * or neither, receive (+=) the gate-bias gradients sum_rows dGi and sum_rows dGh[:, 2H:3H]
 * (b_ir|b_iz|b_in and b_hn) from the same pass.  partial >= msat_gru_ln_bwd_partial_floats.
 * accumulate_ln: bit 0 accumulates the LN grads (else overwrites them); bit 1 overwrites dhprev
 * (its prior contents are never read) instead of accumulating into it; bit 2 packs each row as
 * [dan | dar | daz | dan*r] (4H, dGh = dGi + H, lddi = lddh >= 4H): dGi is then in gate order
 * (n, r, z) and the r / z columns are written once for both. */
/* msat_gru_ln_bwd_g4 plus (+=) the gradient of the input-matrix rows that multiply nfeat per-row
 * features (nfeat 0, 2 or 6; feat (R, ldf)): dfeat[k][g H + j] = sum_rows feat[r][k] dG_g[r][j]
 * (dfeat nfeat x 3H contiguous, gates r, z, n), reduced with the gate-bias partials in one pass. */
int msat_gru_ln_bwd_g4f(const float *dy, int32_t ldy, const float *g4, int32_t ldg, const float *hprev, int32_t ldp,
                        const float *ln_scale, float *dGi, int32_t lddi, float *dGh, int32_t lddh, float *dhprev,
                        int32_t lddp, float *dln_scale, float *dln_bias, float *dbi, float *dbh_n, const float *feat,
                        int32_t ldf, int32_t nfeat, float *dfeat, float *partial, int32_t R, int32_t H,
                        int32_t accumulate_ln, void *stream);
/* msat_gru_ln_bwd_g4f (packed rows) + rexp[r] = the fp16x2 scale exponent of row r's largest |dG|
 * (max |dG| 2^e in [2^14, 2^15); 0x3fff for an all-zero row) for msat_gemm_wgrad_h2 / msat_gemm_h2.
 * Flags bit 3 (with the bias outputs and nfeat 2 or 6): the packed row is stored as fp16x2 planes at that
 * exponent instead of fp32 -- the row's 4H floats at dGi + r lddi hold [hi (4H fp16) | lo (4H fp16)] with
 * hi = fp16(x 2^e), lo = fp16(x 2^e - hi) (e = 0 for an all-zero row), for the *_planes products. */
int msat_gru_ln_bwd_g4fe(const float *dy, int32_t ldy, const float *g4, int32_t ldg, const float *hprev, int32_t ldp,
                         const float *ln_scale, float *dGi, int32_t lddi, float *dGh, int32_t lddh, float *dhprev,
                         int32_t lddp, float *dln_scale, float *dln_bias, float *dbi, float *dbh_n, const float *feat,
                         int32_t ldf, int32_t nfeat, float *dfeat, float *partial, int32_t R, int32_t H,
                         int32_t accumulate_ln, int32_t *rexp, void *stream);
int msat_gru_ln_bwd_g4(const float *dy, int32_t ldy, const float *g4, int32_t ldg, const float *hprev,
                       int32_t ldp, const float *ln_scale, float *dGi, int32_t lddi, float *dGh, int32_t lddh,
                       float *dhprev, int32_t lddp, float *dln_scale, float *dln_bias, float *dbi, float *dbh_n,
                       float *partial, int32_t R, int32_t H, int32_t accumulate_ln, void *stream);
/* out[N] (+)= column sums of G (M x N) — bias gradients; workspace >= msat_colsum_workspace_floats. */
size_t msat_colsum_workspace_floats(int32_t M, int32_t N);
int msat_colsum(const float *G, int32_t ldg, int32_t M, int32_t N, float *out, int32_t accumulate,
                float *workspace, void *stream);
int msat_relu(float *x, size_t n, void *stream);
int msat_relu_bwd(float *dy, const float *y, size_t n, void *stream);

/* ---- heads (learner:264-350): graph batch = per sample G graphs (0 critic, 1+i agent i) ---- */
int msat_critic_pool(const float *Hp, const float *Hn, const float *Hc, int32_t H, const int32_t *vbase,
                     const int32_t *nv, const int32_t *cbase, const int32_t *nc, int32_t G, int32_t S,
                     float *pooled, void *stream);
int msat_critic_pool_bwd(const float *Hp, const float *Hn, const float *Hc, int32_t H, const int32_t *vbase,
                         const int32_t *nv, const int32_t *cbase, const int32_t *nc, int32_t G, int32_t S,
                         const float *dpooled, float *dHp, float *dHn, float *dHc, void *stream);
int msat_actor_pool(const float *Hp, const float *Hn, const float *Hc, int32_t H, const int32_t *vbase,
                    const int32_t *nv, const int32_t *cbase, const int32_t *nc, int32_t G, int32_t S,
                    int32_t A, int32_t M, int32_t base_sz, int32_t rem, const float *id_emb, int32_t E,
                    float *my_emb, float *ctx, void *stream);
int msat_actor_pool_bwd(int32_t H, const int32_t *vbase, const int32_t *nv, const int32_t *cbase,
                        const int32_t *nc, int32_t G, int32_t S, int32_t A, int32_t M, int32_t base_sz,
                        int32_t rem, int32_t E, const float *dmy, const float *dctx, float *dHp, float *dHn,
                        float *dHc, float *did, void *stream);
/* The actor pools (learner:287-301) on a batch whose agent i graph is slot ag0 + i of its sample's G
 * graphs: ag0 = 1 (G = A+1, the two above) or ag0 = 0 (G = A, an actor-only batch). */
int msat_actor_pool_from(const float *Hp, const float *Hn, const float *Hc, int32_t H, const int32_t *vbase,
                         const int32_t *nv, const int32_t *cbase, const int32_t *nc, int32_t G, int32_t ag0,
                         int32_t S, int32_t A, int32_t M, int32_t base_sz, int32_t rem, const float *id_emb,
                         int32_t E, float *my_emb, float *ctx, void *stream);
int msat_actor_pool_bwd_from(int32_t H, const int32_t *vbase, const int32_t *nv, const int32_t *cbase,
                             const int32_t *nc, int32_t G, int32_t ag0, int32_t S, int32_t A, int32_t M,
                             int32_t base_sz, int32_t rem, int32_t E, const float *dmy, const float *dctx,
                             float *dHp, float *dHn, float *dHc, float *did, void *stream);
int msat_bcast_add_relu(float *Q, const float *P, int32_t R, int32_t M, int32_t W, void *stream);
int msat_group_sum(const float *dQ, int32_t R, int32_t M, int32_t W, float *dP, void *stream);
int msat_assemble_logits(const float *flip, const float *noop, int32_t SA, int32_t A, int32_t M,
                         int32_t base_sz, int32_t rem, float *logits, void *stream);
int msat_mask_var_logits(float *logits, int32_t SA, int32_t A, int32_t M, int32_t base_sz, int32_t rem,
                         void *stream);
int msat_split_dlogits(const float *dlogits, int32_t SA, int32_t M, float *dflip, float *dnoop, void *stream);

/* ---- policy / loss / optimiser (learner:397-403, :597-650; mappo_runner.py:198) ---- */
int msat_sample_actions(const float *logits, int32_t R, int32_t W, int32_t greedy, uint64_t seed,
                        uint64_t counter, int32_t *action, float *logp, void *stream);
/* Gumbel-max sampling at a temperature (the policy solver's sampled restarts, marlsat/solvers/policy.py):
 * every logit is first rounded to fp32 as logits[j] * inv_temperature (inv_temperature = 1 / T); from there
 * the arithmetic is msat_sample_actions' with greedy = 0 -- the same Philox counters (counter lo, counter hi,
 * row, j) keyed by seed, the Gumbel noise added at finite slots only, the lowest index on ties, -inf slots
 * never chosen beside a finite one, and action 0 with log-prob 0 for a row with no finite logit.  logp is the
 * log-probability of the action under the tempered distribution softmax(logits * inv_temperature).  The
 * outputs are bitwise those of msat_sample_actions on logits pre-multiplied in fp32; at inv_temperature = 1
 * those of msat_sample_actions on the logits themselves.
 * inv_temperature <= 0, NaN or inf, R < 0, W < 1, or a NULL pointer with R > 0: MSAT_EBADARG.
 * (Additive entry point: msat_version() stays 3, no struct changed.) */
int msat_sample_actions_t(const float *logits, int32_t R, int32_t W, float inv_temperature, uint64_t seed,
                          uint64_t counter, int32_t *action, float *logp, void *stream);
/* msat_sample_actions_t for a piece of a larger batch: row r of the call draws the Philox stream of row
 * row0 + r, counters (counter lo, counter hi, row0 + r, j), so a batch cut into pieces of any size samples, row
 * for row, what one call on the whole batch samples (the policy solver's slabs).  row0 = 0 is
 * msat_sample_actions_t.  Additionally row0 < 0 or row0 + R > 2^32 - 1: MSAT_EBADARG.
 * (Additive entry point: msat_version() stays 3, no struct changed.) */
int msat_sample_actions_from(const float *logits, int32_t R, int32_t W, int64_t row0, float inv_temperature,
                             uint64_t seed, uint64_t counter, int32_t *action, float *logp, void *stream);
int msat_ppo_loss(const float *logits, int32_t S, int32_t A, int32_t M, int32_t action_mode,
                  int32_t base_sz, int32_t rem, const int32_t *action, const float *old_logp,
                  const float *gae, const float *value, const float *old_value, const float *targets,
                  float clip_eps, float vf_clip, float ent_coef, float vf_coef, int32_t minibatch,
                  float *dlogits, float *dvalue, float *row_terms, double *loss_sums, void *stream);
/* Behavioural-cloning joint cross-entropy (src/runners/behavioral_cloning.py:243-256), action mode 0:
 * loss = -mean over (sample, agent) of log_softmax(logits)[label].  logits (S*A, M+1), -inf at padded
 * variable slots; labels (S,A) int32 in [0, M] (M = no-op); minibatch = the number of samples the mean is
 * over (as msat_ppo_loss: micro-batch gradients add up to the minibatch's).
 * A row is valid when 0 <= label <= M and logits[label] is finite.  Valid row: dlogits[j] =
 * (softmax_j - [j == label]) / (minibatch * A) at finite slots, 0 at -inf slots; row_terms[2r] =
 * -log p[label]; row_terms[2r+1] = 1 if the argmax (lowest index on ties) is the label, else 0.
 * Invalid row (the reference's loss is inf / NaN there): dlogits row and both row terms are 0, nothing
 * outside the row is read.  sums[0..3] += (sum nll, sum correct, valid rows, invalid rows), fp64, fixed
 * order.  dlogits as logits; row_terms 2*S*A floats.  The row's softmax is evaluated in fp64 (its
 * residuals cancel in the bias gradients), the outputs are rounded to fp32 once.
 * S < 0, A < 1, M < 1, minibatch < 1, or a NULL pointer with S > 0: MSAT_EBADARG.
 * (Additive entry point: msat_version() stays 3, no struct changed.) */
int msat_bc_loss(const float *logits, int32_t S, int32_t A, int32_t M, const int32_t *labels,
                 int32_t minibatch, float *dlogits, float *row_terms, double *sums, void *stream);
int msat_adam(float *params, const float *grads, float *m, float *v, size_t n, float lr, float b1, float b2,
              float eps, int32_t count, float grad_scale, void *stream);
/* msat_adam + a fail-loud guard: if an updated parameter is not finite, *first_bad = min(*first_bad,
 * count) (device int32, the caller initialises it to INT32_MAX).  No host sync: the runner reads the
 * flag once per train cycle (mappo_runner.py:313-317's loop) and raises, instead of carrying NaN
 * parameters forward -- the hazard of an instance with a variable in no clause at zero-initialised
 * biases (tests/test_isolated_variable.py). */
int msat_adam_checked(float *params, const float *grads, float *m, float *v, size_t n, float lr, float b1, float b2,
                      float eps, int32_t count, float grad_scale, int32_t *first_bad, void *stream);
/* ---- collectives (RCCL over xGMI, one communicator per process) ----
 * The gradient is ONE flat fp32 buffer (the grads of every parameter, 16-B aligned tensors): before
 * msat_adam(..., grad_scale = 1 / world) every rank SUM-all-reduces it in place (learner:647-650 is the
 * single-device update this replaces).  The Python learner reaches RCCL either through torch.distributed
 * (whose "nccl" backend is RCCL on ROCm; the default) or through these entry points
 * (marlsat/learners/collectives.py CapiComm, MARLSAT_COLLECTIVES=capi); a cgo / JNI host uses these.
 * Rank 0 draws the id, the host broadcasts its msat_comm_id_bytes() bytes, every rank calls
 * msat_comm_init.  Errors: MSAT_EBADARG, MSAT_ECOMM (message from RCCL). */
size_t msat_comm_id_bytes(void);
int msat_comm_unique_id(uint8_t *id_out);
int msat_comm_init(const uint8_t *id, int32_t rank, int32_t world, void **comm_out);
/* in place: buf[0..count) = sum over ranks; dtype 0 = fp32, 1 = fp64; enqueued on `stream` */
int msat_allreduce_sum(void *comm, void *buf, size_t count, int32_t dtype, void *stream);
int msat_comm_destroy(void *comm);

/* ---- learner glue (learner:562-592 minibatching, :661-719 metrics) ---- */
/* out[0..N) = a keyed pseudo-random permutation of [0, N) (4-round Feistel + cycle walking), for the
 * PPO epoch's minibatch rows (replaces jax.random.permutation, learner:576; deterministic in
 * (seed, counter)). */
int msat_permutation(int32_t N, uint64_t seed, uint64_t counter, int32_t *out, void *stream);
/* dst[f][s] = src[f][idx[s]] for nfields <= 8 fields of row_bytes[f] bytes per row (the micro-batch's
 * transition rows, learner:597-602); src / dst / row_bytes are host arrays of device pointers. */
int msat_gather_rows(const int32_t *idx, int32_t S, int32_t nfields, const void *const *src, void *const *dst,
                     const int32_t *row_bytes, void *stream);
/* Row bases of a graph batch (learner:148-195 batch assembly): per sample s of instance inst[s],
 * bases[s] = exclusive prefix sums of the instances' (var rows, clause rows, incidences) counts
 * nv / nc / ne, totals[3] = their sums (the batch's Nv, Nc, nnz), or -1 for a sum above INT32_MAX
 * (the batch cannot be indexed in int32; the caller must split it). */
int msat_graph_bases(int32_t S, const int32_t *inst, const int32_t *nv, const int32_t *nc, const int32_t *ne,
                     int32_t *bases, int32_t *totals, void *stream);
/* The graph templates of a problem pool on the device: the twelve arrays that learners/graphs.py::build_templates
 * makes on the host, element for element (the layouts msat_assemble_graph_batch reads).  clauses (N,C,K) int32,
 * signed and 1-based; literal 0 names no variable and adds no edge (the network's adjacency, not the env's
 * literal-0 quirk), and so does a literal with |l| > V.  Graph 0 of an instance is all V variables and all C
 * clauses in order; graph 1 + i is agent i's: its own variables in order (lo = i * (V / A) + min(i, V % A),
 * V / A + (i < V % A) of them), then its neighbours ascending (the variables of real literals of related clauses
 * that are not its own), and the related clauses ascending (those with a real literal on an own variable).
 *   msat_graph_template_counts: gv, gc, ge (N, A+2): the var-row, clause-row and incidence starts of each graph
 *   within its instance; the last column is the instance total.
 *   The caller scans the totals over N: voff, coff, eoff (N+1,) and poff = voff + n.
 *   msat_graph_template_fill: vgid (total var rows), cgid (total clause rows), slots (total clause rows, 3):
 *   (instance-relative var row << 1) | neg, -1 for literal 0 and the columns past K; ptr (total var rows + N): per
 *   instance a CSR over all its var rows (rows + 1 entries); inc (total incidences): (instance-relative clause
 *   row << 1) | neg, per var row in (clause row, slot) order, a variable twice in a clause being two entries.
 *   total_var_rows / total_clause_rows / total_incidences are voff[N], coff[N], eoff[N].
 * One workgroup per instance with the instance in LDS: msat_graph_templates_lds_bytes(V, C, K) bytes (0 for
 * dimensions outside the ranges below); a shape that needs more than 65536 is MSAT_EBADARG (the caller keeps the
 * host builder for it).  Enqueue only.  N == 0: MSAT_OK without a launch.  MSAT_EBADARG also: N < 0, V outside
 * [1, 32000], C < 1, K outside [1, 3], A outside [1, V], a NULL pointer with N > 0 (cgid, slots and inc may be NULL
 * when their total is 0). */
size_t msat_graph_templates_lds_bytes(int32_t num_vars, int32_t num_clauses, int32_t clause_width);
int msat_graph_template_counts(const int32_t *clauses, int32_t num_problems, int32_t num_clauses,
                               int32_t clause_width, int32_t num_vars, int32_t num_agents, int32_t *gv, int32_t *gc,
                               int32_t *ge, void *stream);
int msat_graph_template_fill(const int32_t *clauses, int32_t num_problems, int32_t num_clauses, int32_t clause_width,
                             int32_t num_vars, int32_t num_agents, const int32_t *voff, const int32_t *coff,
                             const int32_t *eoff, const int32_t *poff, int32_t total_var_rows,
                             int32_t total_clause_rows, int32_t total_incidences, int32_t *vgid, int32_t *cgid,
                             int32_t *slots, int32_t *ptr, int32_t *inc, void *stream);
/* fp64 cycle sums over N transitions (learner:661-719): out[9] = sum reward, sum done, sum solved&done,
 * sum unsat*done, sum episode_step*(solved&done), sum tg, sum tg^2, sum d, sum d^2 (d = tg - vpred). */
int msat_cycle_metrics(int32_t N, const float *reward, const uint8_t *done, const uint8_t *solved,
                       const int32_t *num_unsatisfied, const int32_t *episode_step, const float *targets,
                       const float *vpred, double *out, void *stream);

/* ---- single-agent PPO baseline (src/learners/single_rl_learner.py, src/runners/single_rl_runner.py) ----
 * Additive entry points: msat_version() stays 3, no struct changed.  All enqueue only. */
/* The single-agent PPO loss and its gradient (single_rl_learner.py:118-158) from the network's outputs.
 * logits (S, V), all finite; action (S) int32; old_logp, adv_n (the minibatch-normalised advantage), value,
 * targets (S).  Per row, p = softmax(logits): lp = log p[a]; ratio = exp(lp - old_logp); actor =
 * -min(ratio * adv_n, clip(ratio, 1 - clip_eps, 1 + clip_eps) * adv_n); vl = (value - target)^2 (no 0.5, no value
 * clipping: the reference's clipped form is commented out); ent = -sum p log p.  total = mean(actor) +
 * vf_coef * mean(vl) - ent_coef * mean(ent), the means dividing by `minibatch` (as msat_ppo_loss: micro-batch
 * gradients add up to the minibatch's).  dlogits (S, V) and dvalue (S) are d total; row_terms (S, 3) holds
 * (actor, vl, ent) per row; sums[0..3] += (sum actor, sum vl, sum ent, invalid rows) in fp64, fixed order.
 * Ties of the minimum and the clip edges follow msat_ppo_loss (jnp.minimum / jnp.clip: 0.5 / 0.5); inside the
 * clip interval both branches are the same function and the gradient is the full one.  A row whose action is
 * outside [0, V) is invalid: its dlogits row, dvalue and row terms are 0 and nothing else of the row is read.
 * The row's softmax, entropy and ratio are evaluated in fp64 and every output is rounded to fp32 once.
 * S < 0, V < 1, minibatch < 1, clip_eps <= 0 or not finite, or a NULL pointer with S > 0: MSAT_EBADARG.
 * S == 0: MSAT_OK without a launch. */
int msat_ppo_single_loss(const float *logits, int32_t S, int32_t V, const int32_t *action, const float *old_logp,
                         const float *adv_n, const float *value, const float *targets, float clip_eps,
                         float ent_coef, float vf_coef, int32_t minibatch, float *dlogits, float *dvalue,
                         float *row_terms, double *sums, void *stream);
/* Population standardisation of a minibatch's advantages (single_rl_learner.py:142): x = (x - mean) /
 * (std + 1e-8) with mean = moments2[0] / n and std = sqrt(max(moments2[1] / n - mean^2, 0)) (ddof 0), moments2
 * being msat_moments' device output (sum x, sum x^2) for the same x: nothing is read back to the host.  fp64 per
 * element, rounded once; a constant vector becomes all zeros.  n == 0: MSAT_OK without a launch; a NULL pointer
 * with n > 0: MSAT_EBADARG. */
int msat_standardize_pop(float *x, size_t n, const double *moments2, void *stream);
/* optax.clip_by_global_norm (single_rl_learner.py:52-60) on the flat gradient: norm = sqrt(sum g^2) in fp64 (two
 * stages, fixed order); norm < max_norm leaves the gradient untouched bitwise, otherwise g *= (float)(max_norm /
 * norm).  *norm_out (device float) receives the norm before the clip.  A NaN gradient element gives a NaN norm and
 * NaN gradients (msat_adam_checked's guard then reports the step); nothing is masked.  workspace: at least
 * msat_clip_global_norm_workspace_doubles(n) doubles.  Two launches, no host read.  n == 0: MSAT_OK without a launch
 * (*norm_out is left as it was); max_norm <= 0, NaN or inf, a NULL workspace / norm_out, or NULL grads with n > 0:
 * MSAT_EBADARG. */
size_t msat_clip_global_norm_workspace_doubles(size_t n);
int msat_clip_global_norm(float *grads, size_t n, float max_norm, double *workspace, float *norm_out, void *stream);
/* Bookkeeping of a greedy evaluation without auto-reset (single_rl_runner.py:218-229), per env b < B, from step
 * t's reward, done and solved (the step's outputs): while finished[b] == 0, ret[b] += reward[b] (fp32, in step
 * order) and, when done[b], len[b] = t + 1, ep_solved[b] = solved[b] != 0, finished[b] = 1.  A finished env is
 * left unchanged by later steps.  The caller zeroes ret / len / ep_solved / finished before step 0.
 * B < 0, t < 0, or a NULL pointer with B > 0: MSAT_EBADARG.  B == 0: MSAT_OK without a launch. */
int msat_episode_track(int32_t B, int32_t t, const float *reward, const uint8_t *done, const uint8_t *solved,
                       float *ret, int32_t *len, uint8_t *ep_solved, uint8_t *finished, void *stream);

/* ---- assignment predictor (src/learners/bc_learner.py, src/runners/bc_runner.py) ----
 * Additive entry point: msat_version() stays 3, no struct changed.  Enqueue only. */
/* The per-variable two-class cross-entropy (bc_learner.py:28-31, jnp.mean over (batch, variable)), its gradient,
 * the arg-max assignment and whether that assignment satisfies the sample's formula.
 * Layout: logits (S*V, 2) fp32, row s*V + v = variable v of sample s (graph 0's row order in a critic-only batch),
 * at any float address; labels (S, V) u8; lits the packed pool (num_problems, num_clauses, MSAT_LIT_SLOTS) of
 * marlsat.h; problem_idx (S) int32.
 * Prediction: pred[s, v] = (l1 > l0) ? 1 : 0 for every row whatever its label; a tie gives 0 (jnp.argmax's lowest
 * index) and so does a NaN.
 * A row is valid when label is 0 or 1 and both logits are finite.  With d = l[label] - l[1 - label] in fp64:
 * nll = max(-d, 0) + log1p(exp(-|d|)); p_other = 1 / (1 + exp(d)), taken through exp(-|d|) so that nothing
 * overflows; dlogits[label] = -p_other / (minibatch * V), dlogits[1 - label] = +p_other / (minibatch * V): one fp32
 * value with both signs, so a row sums to exactly 0.  Each output is rounded to fp32 once (below FLT_MIN to an fp32
 * denormal).  `minibatch` is the number of samples the mean is over: micro-batch gradients add up to the
 * minibatch's, as in msat_bc_loss / msat_ppo_single_loss.
 * An invalid row gets a zero dlogits row, is not counted as correct, adds nothing to the nll and is counted in
 * sums[3]; nothing outside the row is read for it.
 * Per sample: sample_nll[s] = the fp64 sum of its valid rows' nll, rounded once; sample_correct[s] = its valid
 * rows with pred == label; sample_unsat[s] = the clauses of instance clamp(problem_idx[s], 0, num_problems - 1)
 * that pred[s] leaves false, by msat_walksat's clause rule (a code c < MSAT_LIT_ABSENT is true iff
 * (pred[c >> 1] ^ c) & 1, MSAT_LIT_NULL is false, MSAT_LIT_ABSENT is inert; a clause with no true slot is false);
 * sample_solved[s] = (sample_unsat[s] == 0).
 * sums[0..4] += (sum nll, sum correct, valid rows, invalid rows, solved samples) in fp64; sums[0] adds the fp64
 * row terms, not the rounded sample_nll.  The order of every sum is fixed by (S, V) alone: two identical calls
 * leave bitwise identical words everywhere.  Every output word has one writer.  Two launches, no host read.
 * Predict only: labels == NULL (then dlogits must be NULL too) writes pred, sample_unsat, sample_solved and
 * sums[4]; sample_nll, sample_correct and sums may be NULL, and with sums NULL nothing is accumulated.
 * S == 0: MSAT_OK without a launch.  MSAT_EBADARG: S < 0, V outside [1, 32000] (msat_walksat's bound),
 * num_clauses < 1, num_problems < 1, minibatch < 1, labels set with dlogits NULL or the reverse, any other
 * required pointer NULL with S > 0 (with labels set: sample_nll, sample_correct and sums too). */
int msat_assign_loss(const float *logits, int32_t S, int32_t V, const uint8_t *labels, int32_t minibatch,
                     const uint16_t *lits, int32_t num_problems, int32_t num_clauses, const int32_t *problem_idx,
                     float *dlogits, uint8_t *pred, float *sample_nll, int32_t *sample_correct,
                     int32_t *sample_unsat, uint8_t *sample_solved, double *sums, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* MARLSAT_NET_H */
