/* ifseg_hip.h -- C ABI of libifseg_hip.so (MI355X / gfx950).
 *
 * The reference (alinlab/ifseg) has no FFI on this path: its hot path is
 * PyTorch Python calling stock ATen ops.  This library is the layer that sits
 * *below* the reference's nn.Module boundary (models/segofa/ (all .py files)): every entry
 * point replaces a group of ATen calls the reference makes, cited per function
 * as file:line under /root/reference.  Plain pointers and sizes only; all
 * pointers are DEVICE pointers unless noted; `stream` is a hipStream_t.
 * Every function returns 0 on success, a hipError_t value (>0) if the launch
 * failed, or one of the IFSEG_ERR_* codes (<0) for argument errors.  Nothing
 * here allocates, synchronises or falls back to the host.
 *
 * Layout conventions: activations are bf16, token-major [rows, C] with
 * row = b*T + t ("batch-first"); heads are column blocks of 64 (h*64..h*64+63).
 */
#ifndef IFSEG_HIP_H
#define IFSEG_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define IFSEG_ABI_VERSION 21
#define IFSEG_ERR_BAD_SHAPE (-2)
#define IFSEG_ERR_BAD_ARG (-3)

int ifseg_abi_version(void);
/* non-zero when the library was compiled with a measurement switch that leaves work out or changes results (IFSEG_EXP_*,
 * RING_ABLATE / RING_NOBAR / RING_NOWAIT builds of tools/variant.py): bench.py refuses to report a number from such a build */
int ifseg_experimental_build(void);

/* ------------------------------------------------------------------ GEMM */
#define IFSEG_GEMM_NT 0 /* C[M,N] = A[M,K] . B[N,K]^T   (F.linear forward)        */
#define IFSEG_GEMM_NN 1 /* C[M,N] = A[M,K] . B[K,N]     (dX = dY . W)             */
#define IFSEG_GEMM_TN 2 /* C[M,N] = A[K,M]^T . B[K,N]   (dW = dY^T . X)           */
#define IFSEG_GEMM_RELU 1
#define IFSEG_GEMM_OUT_F32 2
#define IFSEG_GEMM_ACCUMULATE 4 /* C += result */
#define IFSEG_GEMM_COLSUM 8     /* TN, ldc == N: also sum_k A[k][m] -- the bias gradient of a Linear whose weight gradient
                                   is this GEMM (dW = dY^T X, db = colsum dY).  splitk > 1: every k-slice slab is
                                   [M x N | round4(M)] floats (summed by the same ifseg_reduce_parts pass); splitk == 1 (bf16
                                   output): db is written as M bf16 right behind dW [M x N] (honours ACCUMULATE) */

/* bf16 MFMA GEMM, fp32 accumulate, epilogue
 *   C = ((A.B + bias[n]) * alpha[for n < alpha_ncols]) + resid[m,n]  (+relu)
 * Replaces nn.Linear / F.linear and their autograd (addmm / mm) as used by
 * q/k/v/out_proj (unify_multihead_attention.py:327-346,513), fc1/fc2
 * (unify_transformer_layer.py:279-283,556-560), image_proj
 * (encoder_module.py:416), pos_{q,k}_linear (encoder_module.py:765-770,
 * decoder_module.py:350-363); `alpha` carries the reference's `q *= scaling`
 * (unify_multihead_attention.py:346) and `* pos_scaling`; `resid` the
 * residual_connection (unify_transformer_layer.py:196,289).
 * N, lda, ldb must be multiples of 8 (16-byte rows); bias/resid bf16.
 * alpha_ncols < 0 means all N columns; 0 <= alpha_ncols < N must be a multiple of 4 when alpha != 1 (the epilogue
 * works on runs of 4 columns), anything else is refused with IFSEG_ERR_BAD_ARG.
 * splitk > 1: the reduction is cut into ceil(K/kchunk) slices (kchunk = K/splitk rounded up
 * to 64); slice z writes its partial product to the fp32 workspace C + z*M*ldc (requires
 * IFSEG_GEMM_OUT_F32, no epilogue terms); the caller sums the slices (ifseg_reduce_parts).
 * Used for the weight-gradient GEMMs whose K is the token count. */
int ifseg_gemm_bf16(int layout, const void* A, const void* B, void* C, int M, int N, int K, int lda,
                    int ldb, int ldc, const void* bias, float alpha, int alpha_ncols,
                    const void* resid, int ldr, int flags, int batch, long long strideA,
                    long long strideB, long long strideC, long long strideR, int splitk, void* stream);
/* Grouped weight-gradient GEMM: n <= IFSEG_GEMM_GROUP_MAX independent products C_i[M,N] = A_i[K,M]^T . B_i[K,N]
 * (dW = dY^T X of the Linear modules of ONE transformer layer: fc1, fc2, q|k|v, out_proj, cross q, cross k|v --
 * unify_transformer_layer.py:279-283,556-560, unify_multihead_attention.py:327-346,513 under autograd) in one launch,
 * one workgroup per 128x128 tile over all K tokens: no split-K slabs, no reduction launches.  C_i is bf16 [M, N]
 * (ldc == N); colsum != 0 also writes db_i[M] = column sums of A_i (bf16) right behind C_i (a Linear's weight and
 * bias are adjacent in the gradient arena); accumulate != 0 adds to what C_i / db_i hold. */
#define IFSEG_GEMM_GROUP_MAX 8
typedef struct {
  const void* A; const void* B; void* C;
  int M, N, K, lda, ldb, colsum, accumulate;
} ifseg_gemm_tn_problem;
int ifseg_gemm_tn_group(int n, const ifseg_gemm_tn_problem* probs, int max_workgroups, void* stream);
/* max_workgroups > 0 caps the grid (a workgroup then walks several tiles): 256 = one per CU, so that a launch on a side
 * stream leaves half of every CU to the kernels of the dependent chain it runs next to; <= 0: one workgroup per tile. */
/* C[M,N] = A[M,K] . B[K,N] (NN, bf16 out) and, from the same epilogue, the per-head row dots with a second operand:
 *   dot_out[(m / rows_per_batch) * (N/64) + h][m % rows_per_batch] = sum_{c<64} C[m][64h+c] (as stored) * dot[m][64h+c]
 * i.e. the attention backward's delta = rowsum(dO * O) ([B,H,T] fp32) while dO = d(attn_ln input) . W_out is produced
 * (unify_multihead_attention.py:503-513 backward); N % 64 == 0.  Replaces phase 1 of ifseg_attn_bwd. */
int ifseg_gemm_nn_rowdot(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                         const void* dot, int ldd, float* dot_out, int rows_per_batch, void* stream);

/* The FFN's ffn_layernorm(gelu(fc1(x))) -> fc2 on the way back (unify_transformer_layer.py:279-283 under autograd) without a
 * 3072-wide LayerNorm-backward pass.  dY [M, J] = gradient of the fc2 output t [M, J] (J = embed dim), W2 [J, N] (N = ffn
 * dim), u [M, N] the saved fc1 output, gamma / beta fp32 [N] of ffn_layernorm, mean / rstd [M] its saved row statistics:
 *   ifseg_ffn_ln_coef       coef[0][j] = sum_k gamma_k W2[j,k],  coef[1][j] = b2_j + sum_k beta_k W2[j,k]        (per step)
 *   ifseg_ffn_ln_rowstats   c[m][0] = mean_k(gamma_k dz_k), c[m][1] = mean_k(gamma_k xh_k dz_k) with dz = dY W2, computed as
 *                           row dots of dY with coef[0] and with (t - coef[1]) -- linear in dz, no 3072-wide tensor is read
 *   ifseg_gemm_nn_gelu_ln_bwd   C = du [M, N] (bf16) = rstd (gamma dz - c1 - xh c2) gelu'(u), dz = A . B in the accumulators
 *                           (A = dY [M, K = J], B = W2 [K, N]); dz never reaches HBM
 *   ifseg_ffn_ln_param_grads    dbeta_k = sum_j db2_j W2[j,k], dgamma_k = (sum_j W2[j,k] dW2[j,k] - beta_k dbeta_k) / gamma_k
 *                           from the (bf16) weight / bias gradient of fc2, written as bf16
 * Refused with IFSEG_ERR_BAD_ARG before any launch: a null pointer (b2, and dy with its operands, may be NULL), L outside
 * 1..32, J, N, rows <= 0, N % 8, ldw % 8, (rowstats; param_grads with dy) J % 8, lddy % 8, ldt % 8, with dy J > 1024 or M <= 0,
 * and a misaligned operand: 16 bytes for what is read 16 bytes at a time -- w2[l], gamma[l], beta[l] (coef); dy, t, coef
 * (rowstats); w2, dw2 and dy (param_grads) --, the element's own size for the rest that is checked: 4 bytes for coef[l]
 * (coef), c (rowstats), gamma, beta and workspace (param_grads), 2 bytes for b2[l].  Without dy, param_grads takes any J. */
int ifseg_ffn_ln_coef(const void* const* w2, int ldw, const float* const* gamma, const float* const* beta,
                      const void* const* b2 /* bf16 [J] each, or NULL */, float* const* coef /* [2][J] each */,
                      int L /* layers in this launch (host arrays of L device pointers), <= 32 */, int J, int N, void* stream);
int ifseg_ffn_ln_rowstats(const void* dy, int lddy, const void* t, int ldt, const float* coef, float* c /* [rows][2] */,
                          int rows, int J, int N, void* stream);
int ifseg_gemm_nn_gelu_ln_bwd(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                              const void* u, int ldu, const float* gamma, const float* mean, const float* rstd,
                              const float* cstats, void* stream);
int ifseg_ffn_ln_param_grads(const void* w2, const void* dw2, const void* db2, const float* gamma, const float* beta,
                             void* dgamma, void* dbeta, float* workspace /* >= 16 N floats: partial column sums of 8 row slabs */,
                             int J, int N,
                             /* rescue of the columns whose gain is too small to divide by (|gamma_k| < 0.05 max(1, |beta_k|), 0 included):
                              * dgamma_k = sum_m (dY W2)[m][k] xhat[m][k] from its definition.  dy [M, J] (the gradient of fc2's output), u [M, N]
                              * (fc1's output), mean / rstd [M] of ffn_layernorm; dy == NULL: no rescue (a zero gain then yields 0, not NaN) */
                             const void* dy, int lddy, const void* u, int ldu, const float* mean, const float* rstd, int M,
                             void* stream);

/* Implicit-GEMM conv on NHWC bf16 with folded FrozenBatchNorm (+residual, +ReLU).
 * `w` is [Cout][KH][KW][Cin] with the BN scale already folded in, `shift` the
 * folded BN bias.  Replaces Conv2d + FrozenBatchNorm2d + ReLU (+ identity add)
 * of Bottleneck.forward (resnet.py:117-137; frozen_bn.py:36-57). Cin % 64 == 0. */
int ifseg_conv2d_nhwc_bf16(const void* in, const void* w, const void* shift, const void* resid,
                           void* out, int B, int H, int W, int Cin, int Cout, int KH, int KW,
                           int stride, int pad, int relu, void* stream);

/* ------------------------------------------------------------- attention */
/* Fused position-biased attention forward (flash-style, nothing [T,S]-sized in HBM):
 *   S = q k^T + pos_q pos_k^T + rel(i,j) (+causal mask);  O = softmax_fp32(S) v
 * q is expected pre-scaled by (2*64)^-0.5 and pos_q by pos_scaling (GEMM epilogue).
 * Replaces bmm + bias add + mask add + softmax + bmm of
 * unify_multihead_attention.py:459-501 together with the bias construction of
 * encoder_module.py:757-771,790-809 / decoder_module.py:335-366,553-558,601-631.
 * q,k,v,out: bf16, row stride ld*, batch stride *_bs (elements), head h at columns
 * [h*64, h*64+64).  pos_q [T,ldpq], pos_k [S,ldpk] batch-invariant (may be NULL).
 * lse: fp32 [B,H,T], the log-sum-exp of the scores in log2 units (natural lse x log2 e; the backward
 * consumes it with exp2).  Token order: grid tokens [0,P) then tail tokens [P,T)
 * (decoder: bos is moved to the end by the caller).  rel_mode=1:
 *   i,j <  P : rel2d[h][gcode[i]-gcode[j]+code_bias]     (image / seg grid)
 *   i,j >= P : rel1d[h][(i-j)+Lt-1], Lt=T-P               (text; decoder bos corner)
 *   i<P<=j   : relx[h][0]          i>=P>j : relx[h][1]    (decoder bos col / row)
 * causal=1 uses "tail-first" order: grid query i sees grid keys j<=i and all tail
 * keys; tail query i sees tail keys j<=i only.  dense_bias: optional fp32 [H,T,dense_ld]
 * (resized grids: ifseg_resized_rel_bias; dense_ld >= S is the row stride, 0 = S; a multiple of 4 with no rel_mode / causal
 * takes the seeded path: four 16-byte loads per 32-key block into the score accumulator, -inf entries = masked keys).
 * Requires P % 64 == 0 when rel_mode or causal.
 * Refused (nothing is launched): q, k, v, out, pos_q, pos_k not 16-byte aligned or a row / batch stride of theirs (ldpq and
 * ldpk included) that is no multiple of 8 elements -- every row is read 16 bytes at a time; pos_q without pos_k or the
 * reverse; rel_mode without gcode / rel2d / rel1d / relx; a NULL q, k, v, out or lse; a dense_bias that takes the seeded path
 * (no rel_mode, dense_ld % 4 == 0) from a base that is not 16-byte aligned (its rows are read as float4; any other dense_ld
 * takes the scalar path and needs no alignment).  ifseg_attn_bwd refuses the same, and any pointer a requested phase
 * dereferences that is NULL: out / dout / delta (DELTA), q, k, v, dout, lse, delta (DKV, DQ), dk, dv, dpos_k_part with pos_k
 * and the three table partials with rel_mode (DKV), dq and dpos_q_part with pos_q (DQ); and `out`, dpos_q_part or dpos_k_part
 * not 16-byte aligned or out_bs no multiple of 8 (the delta launch reads `out` and the abs-pos partials are stored 16 bytes at a
 * time). */
int ifseg_attn_fwd(const void* q, const void* k, const void* v, const void* pos_q, const void* pos_k,
                   void* out, float* lse, int B, int H, int T, int S, int ldq, int ldk, int ldv, int ldo,
                   int ldpq, int ldpk, long long q_bs, long long k_bs, long long v_bs, long long o_bs,
                   int rel_mode, int P, const int* gcode, int code_bias, int n2d, const float* rel2d,
                   const float* rel1d, const float* relx, int causal, const float* dense_bias,
                   const void* gain /* fp32 [H] or NULL */,
                   int grid_w /* token-grid width if gcode is the raster code y*(2w-1)+x, else 0; 32 enables
                                 the row-aligned bias lookup; any other multiple of 8 >= 32: seeds per group of 8 */,
                   int dense_ld /* row stride of dense_bias (0: S) */,
                   void* stream);

/* Backward of ifseg_attn_fwd (autograd of the same reference lines).  Launches
 *   delta[b,h,t] = sum_d dout*out;  a key-stationary dK/dV kernel that also
 *   histograms d(rel2d/rel1d/relx) in LDS;  a query-stationary dQ kernel.
 * `gain` [H] (fp32) is the per-head c_attn applied to `out` by the forward
 * (unify_multihead_attention.py:509-512); d(gain)[h] = sum_{b,t} delta / gain[h].
 * dq is scaled by dq_scale (the reference's q scaling), the abs-pos halves of
 * dQ_ext / dK_ext are written as bf16 per-batch partials dpos_q_part [B,T,H*64]
 * (scaled by dpq_scale) and dpos_k_part [B,S,H*64]; rel-table gradients as
 * per-workgroup partials [H][nparts][n] with nparts = B*ceil(S/128) (sum them with
 * ifseg_attn_bwd_reduce).  No atomics on global memory: results are deterministic. */
typedef struct ifseg_attn_bwd_args {
  const void *q, *k, *v, *pos_q, *pos_k, *out, *dout;
  const float* lse;
  float* delta;               /* workspace [B,H,T] */
  void *dq, *dk, *dv;
  void *dpos_q_part, *dpos_k_part; /* bf16 */
  int B, H, T, S;
  int ldq, ldk, ldv, ldpq, ldpk, ldout, lddo, lddq, lddk, lddv;
  long long q_bs, k_bs, v_bs, out_bs, do_bs, dq_bs, dk_bs, dv_bs;
  int rel_mode, P, code_bias, n2d, causal, nparts;
  const int* gcode;
  const float *rel2d, *rel1d, *relx;
  const void* gain; /* fp32 [H] or NULL */
  float *drel2d_part, *drel1d_part, *drelx_part;
  float dq_scale, dpq_scale;
  int grid_w; /* width of the token grid (0 if unknown); 32 enables the row-aligned bias-gradient reduction */
  int phases; /* 0 = everything; else a mask: 1 = delta, 2 = dK/dV kernel, 4 = dQ kernel.  The dQ kernel only needs
                 delta, so a caller may launch {1|2} and {4} on two streams (ordered by an event after delta): the two
                 kernels then fill each other's partially occupied last round of workgroups. */
  float* dgain_rows; /* optional fp32 [B,H,T], written by the dQ kernel: sum_j P_ij dP_ij = dout_i . (P v)_i -- the per-row terms of
                 d c_attn[h] without the division of delta by c_attn (0 / 0 at c_attn = 0): sum them instead of delta / gain */
} ifseg_attn_bwd_args;
#define IFSEG_ATTN_BWD_DELTA 1
#define IFSEG_ATTN_BWD_DKV 2
#define IFSEG_ATTN_BWD_DQ 4
int ifseg_attn_bwd(const ifseg_attn_bwd_args* args, void* stream);

/* Everything the partial outputs of ifseg_attn_bwd still need, in ONE launch (the autograd reductions behind
 * unify_multihead_attention.py:459-512 + the bias construction encoder_module.py:757-809 / decoder_module.py:553-631:
 * sum over the batch of the abs-pos operand gradients, sum over the workgroup partials of the rel-pos table gradients
 * followed by embedding_dense_backward into the bucket tables, and the gradient of c_attn):
 *   dpos_q_acc[T*C]  (=|+=) sum_b dpos_q_part[b]        dpos_k_acc[S*C] (=|+=) sum_b dpos_k_part[b]
 *   dgain[h] (bf16)  = sum_{b,t} delta[b,h,t] / gain[h]          (delta = rowsum(dO * O), O includes the gain)
 *   for each of up to 3 tables i:  acc_i[idx_i[j]][h] += sum_p part_i[h][p][j]   (idx < 0: no bucket)
 * Tables of up to 2048 entries (token offsets: several entries may share a bucket) are summed per bucket in entry order,
 * larger ones (the image / seg grids: entries and buckets one-to-one) by one atomic add per entry: bit-reproducible either way.
 * Replaces 2 + 4 + 2 per table launches of ifseg_reduce_parts / ifseg_rel_scatter_add / elementwise kernels. */
typedef struct ifseg_attn_reduce_args {
  int B, H, T, S, C, nparts, accumulate_pos;
  const void *dpos_q_part, *dpos_k_part;    /* bf16 [B,T,C], [B,S,C] (as ifseg_attn_bwd writes them) */
  float *dpos_q_acc, *dpos_k_acc;           /* [T,C], [S,C] */
  const float* delta;                       /* [B,H,T] */
  const float* gain;                        /* fp32 [H] */
  void* dgain;                              /* bf16 [H] or NULL */
  int ntab;
  const float* tab_part[3];                 /* [H,nparts,n_i] */
  const int* tab_idx[3];                    /* [n_i] bucket of entry j of the delta table */
  float* tab_acc[3];                        /* fp32 [n_bucket_i, H] accumulators */
  int tab_n[3];
  int tab_nbucket[3];                       /* rows of tab_acc_i */
} ifseg_attn_reduce_args;
int ifseg_attn_bwd_reduce(const ifseg_attn_reduce_args* args, void* stream);

/* ---- attention backward with the batch as a workgroup's inner dimension (csrc/attention_bi.hip) ----
 * The reference builds abs-pos + rel-pos bias ONCE per layer and broadcasts it over the batch
 * (encoder_module.py:757-771,790-809 with the expand at :317,791; decoder_module.py:553-558,603-627;
 * unify_multihead_attention.py:459-465).  These three entry points keep that structure:
 *
 * ifseg_attn_dense_bias: D[h][i][j] = pos_q[i].pos_k[j] + rel(i,j) as bf16 [H,Tp,Sp] (computed in fp32, rounded once; the
 *   reference holds this tensor in half precision under --fp16, unify_multihead_attention.py:464; Sp / Tp = S / T rounded up
 *   to 32; D 16-byte aligned); -inf where the causal mask ("tail-first" order of ifseg_attn_fwd) hides (i,j), for padded columns j >= S
 *   and padded rows i >= T.  Parameters only: built once per layer and step.  (Causal: 32 x 32 tiles no kernel's block
 *   schedule reaches are not written.)
 *   rel(i,j) as documented at ifseg_attn_fwd (rel_mode = 1), pos_q / pos_k may be NULL (no abs-pos term); both 16-byte aligned
 *   with ldpq, ldpk multiples of 8 (refused otherwise). */
int ifseg_attn_dense_bias(const void* pos_q, const void* pos_k, int ldpq, int ldpk, int H, int T, int S, int rel_mode,
                          int P, const int* gcode, int code_bias, int n2d, const float* rel2d, const float* rel1d,
                          const float* relx, int causal, void* D, int Sp, int Tp, void* stream);

/* ifseg_attn_bwd_bi: dq (x dq_scale), dk, dv of S_b = q_b k_b^T + D (autograd of unify_multihead_attention.py:459-512)
 *   and dbias[g][h][i][j] = sum over the batch elements 4g .. 4g+3 of dS_b[h][i][j] (bf16 [ceil(B/4), H, T, Sp]).
 *   One workgroup = (head, 64 rows, 4 batch elements): the bias tile is fetched once for the four, sum_b dS leaves the
 *   kernel once per tile.  delta [B,H,T] = rowsum(dout * out) must exist (ifseg_attn_bwd phase 1 or
 *   ifseg_gemm_nn_rowdot).  Causal launches skip 32-blocks above the diagonal: those entries of dbias are NOT written --
 *   the caller zero-fills the buffer once (the set of skipped blocks depends only on the shape).  No atomics. */
typedef struct ifseg_attn_bi_args {
  const void *q, *k, *v, *dout;
  const float *lse, *delta;
  const void* D;                /* bf16 [H, Tp, Sp] (ifseg_attn_dense_bias) */
  const void* gain;            /* fp32 [H] or NULL */
  void *dq, *dk, *dv, *dbias;
  int B, H, T, S, Sp, Tp;
  int ldq, ldk, ldv, lddo, lddq, lddk, lddv;
  long long q_bs, k_bs, v_bs, do_bs, dq_bs, dk_bs, dv_bs;
  int causal, P;               /* P: grid tokens (multiple of 64) when causal */
  float dq_scale;
  int phases;                  /* 0 = both; IFSEG_ATTN_BWD_DKV | IFSEG_ATTN_BWD_DQ */
  float* dgain_rows;           /* optional fp32 [B,H,T]: sum_j P_ij dP_ij = dout_i . (P v)_i, the per-row terms of d c_attn[h]
                                  (unify_multihead_attention.py:509-512) computed WITHOUT dividing delta by c_attn: exact at c_attn = 0 */
  void* out;                   /* ifseg_attn_fwd_bi: O [B,T,ldout] bf16 (x gain) */
  int ldout; long long out_bs;
  const int* kv_len;           /* optional device int32 [B]: key padding (unify_multihead_attention.py:477-489 with the suffix masks of
                                  encoder_module.py:730-752): keys j >= kv_len[b] are masked for batch element b in the forward and in
                                  all three gradients; NULL = no padding.  kv_len[b] >= 1 */
  float drop_p;                /* attention dropout (unify_multihead_attention.py:498: dropout_module(attn_weights)): P o keep / (1 - p)
                                  between the softmax and P V, keep ~ Bernoulli(1 - p) from a counter-based hash of
                                  (drop_seed + *drop_seed_add, b, h, query, key) that forward and the three gradients regenerate
                                  (ifseg_attn_dropout_mask writes it out); 0 = off.  `delta` must come from the dropped output. */
  unsigned long long drop_seed;
  const unsigned long long* drop_seed_add;   /* device word or NULL (as ifseg_drop_args.seed_add) */
  /* Refused by both entry points (nothing is launched): q, k, v, out / dout, dq, dk, dv, dbias or D not 16-byte aligned (rows
     and bias tiles move 16 bytes per lane), row / batch strides that are no multiple of 8 elements, Sp / Tp no multiple of 32;
     by ifseg_attn_bwd_bi also a NULL q, k, v, dout, lse or delta, and a NULL output of any requested phase (all of them are
     looked at before the first launch). */
} ifseg_attn_bi_args;
int ifseg_attn_bwd_bi(const ifseg_attn_bi_args* args, void* stream);
/* ifseg_attn_fwd_bi: the forward of the same formulation -- out = gain softmax_fp32(q k^T + D) v, `lse` (written) as
 * ifseg_attn_fwd's (log2 units); reads q, k, v, D, gain, causal / P (tile schedule only: the mask is inside D).  A workgroup
 * holds four batch elements and fetches each 32 x 32 bias tile once for them (unify_multihead_attention.py:459-512). */
int ifseg_attn_fwd_bi(const ifseg_attn_bi_args* args, void* stream);
/* keep[b, h, i, j] in {0, 1} (uint8 [B, H, T, S]): the attention-dropout mask of the kernels above for these seeds */
int ifseg_attn_dropout_mask(unsigned char* keep, int B, int H, int T, int S, float p, unsigned long long seed,
                            const unsigned long long* seed_add, void* stream);

/* ifseg_attn_dbias_grads: everything downstream of dbias (two launches: operand gradients, tables) (the autograd of the bias construction,
 *   encoder_module.py:757-771,790-809 / decoder_module.py:553-558,603-627), with dB = sum_g dbias[g]:
 *     dpos_q_acc[i][h*64+c] (=|+=) dpq_scale * sum_j dB[h][i][j] pos_k[j][h*64+c]       (fp32 [T,C])
 *     dpos_k_acc[j][h*64+c] (=|+=)             sum_i dB[h][i][j] pos_q[i][h*64+c]       (fp32 [S,C])
 *     drel2d[h][p][(dy+gh-1)(2gw-1) + dx+gw-1] = sum of dB over grid pairs with (y_i-y_j, x_i-x_j) = (dy, dx)  (raster grid gh x gw = P, gw % 8 == 0)
 *     drel1d[h][p][(i-j)+Lt-1] = sum over tail pairs;  drelx[h][p][0] = sum_{i<P<=j<S} dB,  drelx[h][p][1] = sum_{j<P<=i<T} dB
 *   as NP = ifseg_attn_dbias_nparts() partial tables per head (part p = the rows i = p mod NP): they feed
 *   ifseg_attn_bwd_reduce with nparts = NP.  pos_q == NULL skips the operand gradients, drel2d == NULL the tables.
 *   Fixed summation order.  Any ng: the slabs are taken two per launch pair, later pairs add to the first's results.
 *   dbias, pos_q and pos_k must be 16-byte aligned (refused otherwise). */
typedef struct ifseg_attn_dbias_args {
  const void* dbias;           /* bf16 [ng][H][T][Sp] */
  int ng, H, T, S, Sp, C;
  const void *pos_q, *pos_k;   /* bf16 [T,ldpq], [S,ldpk] */
  int ldpq, ldpk;
  float *dpos_q_acc, *dpos_k_acc;
  int accumulate_pos;
  float dpq_scale;
  int P, grid_h, grid_w;
  float *drel2d, *drel1d, *drelx;
  int causal;                  /* dbias comes from a causal launch of ifseg_attn_bwd_bi: the blocks it skipped are not read */
} ifseg_attn_dbias_args;
int ifseg_attn_dbias_grads(const ifseg_attn_dbias_args* args, void* stream);
int ifseg_attn_dbias_nparts(void);

/* ---- attention with a bias the caller computed (csrc/attention_ops.hip; torch.ops.ifseg.attention_bias) ----
 * The reference's attention module takes the bias as an ordinary tensor (unify_multihead_attention.py:130,464-465, `attn_bias`).
 * ifseg_attn_bias_pack: D[h][i][j] (bf16 [H,Tp,Sp], the operand of ifseg_attn_fwd_bi / _bwd_bi) = bf16_rne(bias[h][i][j]) for
 *   i < T, j < S; -inf for the padding rows / columns and, when `causal`, for the pairs ifseg_attn_dense_bias masks
 *   ("tail-first" order with P grid tokens; P % 64 == 0, P <= min(T, S)).  EVERY element of D is written.  bias: fp32
 *   (bias_is_f32) or bf16 [H,T,S], last dimension contiguous, head / row strides in elements; NULL = a zero bias.
 * ifseg_attn_dbias_sum: out[h][i][j] = sum_{g < ng} dbias[g][h][i][j] for j < S (dbias: the bf16 slabs [ng][H][T][Sp] of
 *   ifseg_attn_bwd_bi), added in fp32 in slab order (bit-reproducible), stored as fp32 (out_is_f32) or bf16 with the strides
 *   of `out` in elements.
 * One pass each, 16-byte accesses along j wherever the unpadded side allows them. */
int ifseg_attn_bias_pack(const void* bias, int bias_is_f32, long long head_stride, long long row_stride, int H, int T, int S,
                         int causal, int P, void* D, int Sp, int Tp, void* stream);
int ifseg_attn_dbias_sum(const void* dbias, int ng, int H, int T, int S, int Sp, void* out, int out_is_f32,
                         long long head_stride, long long row_stride, void* stream);

/* -------------------------------------------------------------- row ops */
/* Row addressing used below: logical row r lives at element offset
 *   (r / rpb) * bs + (r % rpb) * ld      (rpb = rows per batch segment; rpb<=0: r*ld)
 * which lets a kernel read / write a token range of a [B, T, C] buffer in place
 * (the reference's torch.cat of image|text tokens, encoder_module.py:427, and of
 * bos|patch tokens, decoder_module.py:537). */

/* y = [resid +] LayerNorm(act(x)) * gamma + beta, act = identity | GELU(fp32).
 * mean/rstd (fp32 [rows]) are saved for the backward when non-NULL.
 * Replaces fairseq LayerNorm (modules/layer_norm.py:30-35) at the sites
 * unify_transformer_layer.py:258,270,278,282,465,513,522,546,554,559 and
 * encoder_module.py:408,423,757-759,829 / decoder_module.py:344,576,668, fused with
 * activation_fn GELU (modules/gelu.py:24-25) and residual_connection (:196). */
/* Optional fused dropout + DropPath of the LayerNorm output (forward) / of dy (backward): the mask is the one
 * ifseg_dropout generates for the same (seed, logical row, column), so stand-alone and fused calls can be mixed
 * (FairseqDropout after attn_ln / cross_attn_ln / the embedding LayerNorms, drop_path in residual_connection:
 * unify_transformer_layer.py:19-35,196).  NULL = no dropout. */
typedef struct ifseg_drop_args {
  float p;                       /* drop probability in [0, 1) */
  unsigned long long seed;
  const float* drop_path_scale;  /* [batch] fp32 keep/(1-rate) per sample, or NULL */
  int rows_per_batch;            /* logical rows per sample (indexes drop_path_scale) */
  const unsigned long long* seed_add; /* device word added to `seed`, or NULL: the per-update part of the seed lives in
                                       * device memory so that a HIP-graph-captured step draws new masks on every replay */
} ifseg_drop_args;
/* `act_gelu` / `flags` of the LayerNorm entry points: IFSEG_LN_GELU = the input goes through GELU first (ffn_layernorm(gelu(fc1)));
 * IFSEG_LN_PARAMS_F32 = gamma / beta (and gamma2 / beta2) point at fp32 values (the optimizer's master copy) instead of bf16. */
#define IFSEG_LN_GELU 1
#define IFSEG_LN_PARAMS_F32 2
int ifseg_ln_fwd(const void* x, const void* gamma, const void* beta, const void* resid, void* y, float* mean,
                 float* rstd, int rows, int C, float eps, int act_gelu, int rpb, long long x_bs, int ldx,
                 long long y_bs, int ldy, long long r_bs, int ldr, const ifseg_drop_args* drop, void* stream);
/* Two LayerNorms of one residual-stream row in one pass (post-LN of a block + pre-LN of the next,
 * unify_transformer_layer.py:256-292,463-568): y = [resid +] drop(LN(x; gamma, beta)), y2 = LN(y as stored in bf16;
 * gamma2, beta2).  Bit-identical to ifseg_ln_fwd followed by ifseg_ln_fwd on y.  gamma == beta == NULL makes the
 * first stage the identity: y = [resid +] drop(x) (the dropout + residual after fc2, identical to ifseg_dropout),
 * y2 = LN(y) -- the pre-LN of the next layer. */
int ifseg_ln_fwd_pair(const void* x, const void* gamma, const void* beta, const void* resid, void* y, float* mean,
                      float* rstd, const void* gamma2, const void* beta2, void* y2, float* mean2, float* rstd2, int rows,
                      int C, float eps, int flags, int rpb, long long x_bs, int ldx, long long y_bs, int ldy, long long r_bs, int ldr,
                      long long y2_bs, int ldy2, const ifseg_drop_args* drop, void* stream);
/* dx = [dx_add +] d/dx of the above (dy is first masked like the forward output when `drop` is given);
 * per-block partials of dgamma / dbeta are written to dgamma_part / dbeta_part [nblocks][C]
 * (sum with ifseg_reduce_parts).  Rows are read and written 16 bytes at a time: C and every leading dimension in use a
 * multiple of 8 (IFSEG_ERR_BAD_SHAPE), here and in every entry point that takes a (rpb, bs, ld) row map. */
int ifseg_ln_bwd(const void* dy, const void* x, const void* gamma, const float* mean, const float* rstd,
                 const void* dx_add, void* dx, float* dgamma_part, float* dbeta_part, int nblocks, int rows,
                 int C, int act_gelu, int rpb, long long dy_bs, int lddy, long long x_bs, int ldx,
                 long long dx_bs, int lddx, long long add_bs, int ldadd, const ifseg_drop_args* drop, void* stream);
/* ifseg_ln_bwd (C <= 1024, no GELU) with a second output dx2 = drop2(dx as stored in bf16): the pre-LN backward that
 * closes a block of the backward and the adjoint of the dropout + DropPath after fc2 (unify_transformer_layer.py:288-292,
 * 564-568) that opens the next one, in one launch.  Bit-identical to ifseg_ln_bwd followed by ifseg_dropout.  IFSEG_LN_GELU in `flags`:
 * IFSEG_ERR_BAD_ARG (there is no GELU instantiation). */
int ifseg_ln_bwd_drop(const void* dy, const void* x, const void* gamma, const float* mean, const float* rstd,
                      const void* dx_add, void* dx, float* dgamma_part, float* dbeta_part, void* dx2, int nblocks, int rows,
                      int C, int flags, int rpb, long long dy_bs, int lddy, long long x_bs, int ldx, long long dx_bs, int lddx,
                      long long add_bs, int ldadd, long long dx2_bs, int lddx2, const ifseg_drop_args* drop2, void* stream);
/* Input validation in one launch, the verdict (0 / 1) written to PINNED host memory in stream order (read it after an event):
 * mode 0: any int64 x[i] == value; mode 1: rows of row_len int64: `value` entries that are not a suffix of their row (fairseq pads on
 * the right: encoder_module.py:730-752); mode 2: any byte x[i] == 0 (the bool `patch_masks`); mode 3: *x (int32 device flag) != 0,
 * and the flag is cleared.  Mode 1 needs n to be a multiple of row_len (IFSEG_ERR_BAD_ARG).  Replaces compare + reduce + cast + copy torch kernels on the main queue between two steps. */
int ifseg_check_inputs(const void* x, long long n, int mode, long long value, long long row_len,
                       unsigned char* verdict_host_pinned, void* stream);
/* fp32 master copy <- bf16 arena wherever bf16(master[i]) != p16[i] (an optimizer outside this library stepped the bf16
 * parameters: fp16_optimizer.py:198-222 writes the model copy); agreeing entries keep their fp32 value. */
int ifseg_sync_master(float* master, const void* p16, long long n, void* stream);
/* out[o][i] (+)= scale * sum_p in[o][p][i]   (fp32 in; fp32 or bf16 out) */
int ifseg_reduce_parts(const float* in, void* out, int outer, int parts, long long n, int accumulate,
                       int out_bf16, float scale, void* stream);
/* Up to 16 such reductions in one launch (the LayerNorm dgamma / dbeta partials of one layer block). */
typedef struct ifseg_reduce_task {
  const float* in; void* out;
  int outer, parts; long long n;
  int accumulate, out_bf16; float scale;
} ifseg_reduce_task;
int ifseg_reduce_parts_multi(int ntask, const ifseg_reduce_task* tasks, void* stream);
/* part[k][n] = column sums of the k-th row slab of x[M,N] (bias gradients; autograd of
 * the bias add in F.linear). */
int ifseg_colsum_bf16(const void* x, float* part, int nblk_rows, int M, int N, int rpb, long long x_bs, int ldx,
                      void* stream);
/* out[r] = table[ids[r]] + add  (embed_tokens + type_embedding, encoder_module.py:400-406) */
/* gw [N, C] (bf16, a key projection's weight gradient dK^T x) -= db [N] (x) mean_rows(x) [C]: sum_j dK_j = 0 in exact arithmetic
 * (softmax shift invariance; the reference's k_proj.bias gradient is float noise), so this removes only the product of the
 * spurious bf16 column sum of dK with the token-common component of x.  xmean [C] fp32: the column means of x
 * (ifseg_colsum_bf16 + ifseg_reduce_parts).  Autograd of unify_multihead_attention.py:327-346. */
int ifseg_kproj_common_mode(void* gw, const void* db, const float* xmean, int N, int C, void* stream);
int ifseg_embed_rows(const void* table, const long long* ids, const void* add, void* out, int n, int C, int rpb,
                     long long o_bs, int ldo, void* stream);
/* Backward of the embedding look-ups above into the token table's gradient (trainable token embeddings:
 * --freeze-encoder-embedding / --freeze-decoder-embedding false, unify_transformer.py:362-371; nn.Embedding /
 * nn.EmbeddingBag(mean) backward).  m entries sorted by token id (stable); entry j adds weight[j] (NULL: 1) x src[src_row[j], :]
 * (bf16 [*, C] contiguous) to row sorted_ids[j] of table_grad (bf16 [V, C], accumulated in place); ids outside [0, V) and
 * skip_id (the padding index, -1: none) are skipped.  Deterministic: the first entry of a run sums the run in order. */
int ifseg_rows_segment_sum(const void* src, const long long* src_row, const float* weight, const long long* sorted_ids,
                           void* table_grad, long long m, int C, long long V, long long skip_id, void* stream);
/* Image-free patch embeddings: out[b,p,:] = mean of table rows ids[b, ends[b,p-1]:ends[b,p]] + add
 * (nn.EmbeddingBag(mode='mean') sharing embed_tokens.weight, encoder_module.py:147-148,529-538, + the image
 * type embedding :589-591).  ids int64 [B,maxlen] (row-padded), ends int64 [B,P] per-sample cumulative bag ends
 * exactly as the collater produces them (segmentation_dataset.py:327-328,99-100); out bf16 rows addressed like
 * ifseg_embed_rows. */
int ifseg_embed_bag_mean(const void* table, const long long* ids, const long long* ends, const void* add, void* out,
                         int B, int P, int C, int maxlen, int rpb, long long o_bs, int ldo, void* stream);
int ifseg_cast_f32_bf16(const float* in, void* out, long long n, float scale, void* stream);
int ifseg_add_bf16(const void* a, const void* b, void* out, long long n, void* stream);
/* NCHW (fp32 / bf16) image -> NHWC bf16 with channels zero-padded to Cpad (round to nearest even; -0, infinities and NaN are
 * kept; the pad channels are +0).  Refused before any launch: a null or misaligned pointer, B, C, H or W <= 0, Cpad < C
 * (IFSEG_ERR_BAD_ARG); B H W Cpad >= 2^31 (IFSEG_ERR_BAD_SHAPE). */
int ifseg_nchw_to_nhwc_bf16(const void* in, int in_is_f32, void* out, int B, int C, int H, int W, int Cpad,
                            void* stream);

/* out[h][i] = table[idx[i]][h] (fp32; idx<0 -> 0): turns a rel-pos bucket table
 * [num_buckets, H] into the per-head delta table the attention kernels index
 * (F.embedding(rp_bucket, table) of encoder_module.py:313-331, decoder_module.py:327-333).
 * ifseg_rel_scatter_add is its adjoint (embedding_dense_backward) into an fp32 buffer. */
int ifseg_rel_gather(const void* table, const int* idx, float* out, int n, int H, void* stream);
/* the same gather for L <= 16 tables of one shape in one launch (all layers' tables at the start of a forward):
 * tables = host array of L device pointers, out fp32 [L][H][n] */
int ifseg_rel_gather_multi(const void* const* tables, int L, const int* idx, float* out, int n, int H, void* stream);
int ifseg_rel_scatter_add(const float* d, const int* idx, float* acc, int n, int H, void* stream);

/* Variable-aspect evaluation (criterions/seg_criterion.py:194-217 feeds images at their native aspect ratio): the reference
 * resizes its [H, P0, P0] relative-position bias with two bilinear interpolations per layer when the feature grid (h, w)
 * differs from the trained (oh, ow) one (encoder_module.py:802-808, decoder_module.py:603-627).  out fp32 [H, T, T],
 * T = h*w + Lt, internal order [grid | tail]: grid x grid = the doubly resized bias, evaluated as 4 x 4 taps of the ORIGINAL
 * delta table table2d [H, (2oh-1)(2ow-1)] (ifseg_rel_gather on the original geometry); tail x tail = rel1d [H, 2Lt-1]
 * (NULL: 0); grid x tail / tail x grid = relx [H, 2] (NULL: 0) -- the decoder's bos column / row, which the reference's
 * resize passes through.  causal != 0 (decoder_module.py:592-600, buffered_future_mask in the internal order with the tail =
 * bos first): -inf where the key lies after the query.  The delta table of one head is staged in LDS: tables above
 * 160 000 bytes (trained grids beyond 100 x 100) are refused with IFSEG_ERR_BAD_SHAPE. */
int ifseg_resized_rel_bias(float* out, const float* table2d, const float* rel1d, const float* relx, int H, int h, int w,
                           int oh, int ow, int Lt, int causal, int ld /* row stride of out, >= T (0: T) */, void* stream);
/* dst bf16 [h*w, C] = bilinear resize (align_corners = False, fp32 arithmetic, one rounding) of the oh x ow grid of rows
 * src[(y * src_stride + x + src_off) * ld_src + c]: the position-embedding tables of encoder_module.py:360-368 and
 * decoder_module.py:541-548 on a resized grid */
int ifseg_resize_rows_bilinear(const void* src, void* dst, int C, int h, int w, int oh, int ow, int src_stride, int src_off,
                               int ld_src, void* stream);

/* out = [resid +] drop_path_scale[row / rows_per_batch] * keep * x / (1 - p) on [rows, C] bf16 (row addressing as above);
 * keep ~ Bernoulli(1-p) from a counter-based hash of (seed, element): calling it again with x = dy,
 * resid = NULL is the backward.  FairseqDropout (fairseq_dropout.py:23-27) + drop_path
 * (unify_transformer_layer.py:19-35, residual_connection :196). */
int ifseg_dropout(const void* x, const void* resid, void* out, long long rows, int C, float p,
                  unsigned long long seed, const float* drop_path_scale, int rows_per_batch, int rpb, long long x_bs,
                  int ldx, long long r_bs, int ldr, long long o_bs, int ldo, const unsigned long long* seed_add, void* stream);
/* out[i] = keep(i) ? x[i] : fill on n contiguous bf16 elements (n % 8 == 0), ifseg_dropout's mask, NO rescaling: the
 * activation dropout between GELU and the FFN LayerNorm (unify_transformer_layer.py:280,556) applied to the pre-activation
 * with fill = -30 (gelu and gelu' are exactly 0 there); the 1 / (1 - p) cancels in the LayerNorm: pass eps (1 - p)^2 to
 * ifseg_ln_fwd (csrc/rowops.hip). */
int ifseg_dropout_fill(const void* x, void* out, long long n, float p, unsigned long long seed,
                       const unsigned long long* seed_add, float fill, void* stream);
/* DropPath keep masks (drop_path, unify_transformer_layer.py:19-35): out[i][b] = Bernoulli(keep[i]) / keep[i] for residual
 * branch i < n and sample b < B, from the counter-based generator of ifseg_dropout (seed + *seed_add). */
int ifseg_droppath_scale(float* out, const float* keep, int n, int B, unsigned long long seed,
                         const unsigned long long* seed_add, void* stream);

/* ------------------------------------------------------------ ResNet stem */
/* conv1 7x7/2 (3->64) + folded FrozenBN + ReLU on an NHWC(4) bf16 image; w fp32
 * [7][7][3][64] with the BN scale folded, shift fp32 [64] (resnet.py:215-218).
 * Non-finite values pass as torch.relu and F.max_pool2d pass them (the ReLU and the pool use the IEEE 754-2019 maximum, one
 * v_maximum3_f32): relu(NaN) = NaN, relu(+inf) = +inf, relu(-inf) = +0, and a pool window that holds a NaN gives NaN -- an image
 * of NaNs (the poisoned sample of ifseg_train_load) leaves stem and pool as NaN.  The matrix-core kernel multiplies its zero
 * weights (tap kx = 7: the input column 2 ox + 4, right of the window) with the patch as well: a NaN or an infinity in that
 * column makes the output NaN too, and an infinity inside the window gives +inf only where all three weight terms are positive
 * (inf * 0 and inf - inf are NaN).
 * All three entries refuse, before any launch: a null pointer, B, H, W (pool: C) <= 0, a pointer the kernels' wide accesses
 * need aligned -- in_nhwc4 8 bytes; out, wt and the matrix-core kernel's shift, the pool's in and out 16 bytes; w and
 * the direct kernel's shift 4 bytes -- with IFSEG_ERR_BAD_ARG; C % 8 != 0, and an input, output or workgroup count of
 * 2^31 or more with IFSEG_ERR_BAD_SHAPE. */
int ifseg_stem_conv7x7(const void* in_nhwc4, const float* w, const float* shift, void* out, int B, int H, int W,
                       void* stream);
/* The same on the matrix cores: wt bf16 [3][64][224], wt[0][c][ky*32 + kx*4 + ci] = bf16(w[ky][kx][ci][c]) (BN scale folded; the
 * entries with kx = 7 or ci = 3 are zero), wt[1] = bf16(w - wt[0]), wt[2] = bf16(w - wt[0] - wt[1]): implicit GEMM,
 * K = 7 x 8 x 4, the fp32 weights as three bf16 terms (resnet.py:215-218). */
int ifseg_stem_conv7x7_mfma(const void* in_nhwc4, const void* wt, const float* shift, void* out, int B, int H, int W,
                            void* stream);
/* MaxPool2d(3, 2, 1) on NHWC bf16 (resnet.py:219). */
int ifseg_maxpool3x3s2(const void* in, void* out, int B, int H, int W, int C, void* stream);

/* ------------------------------------------------------------- criterion */
/* Fused segmentation loss: bilinear x16 upsample of the per-patch logits
 * (logits[:, :P] viewed as [hp, wp]; align_corners=False), masked mean cross entropy, its
 * gradient w.r.t. the logits, argmax and the per-class area histograms, replacing
 * upsample_logits + F.cross_entropy + compute_metric (criterions/seg_criterion.py:237-244,
 * :269-347, :349-362) and their autograd.  Step 1 (one workgroup per 16x16 pixel tile) writes
 *   tile_partial [B*hp*wp][3][3][nseg]  gradient of the tile w.r.t. its 3x3 stencil cells
 *   stats_part   [B*hp*wp][2 + 3*nseg]  loss sum, valid-pixel count, intersect|pred|label hist
 * the caller sums stats_part over tiles (ifseg_reduce_parts) into stats[2+3*nseg]; step 2
 * gathers dlogits (bf16 [B, P+1, ldl], eos row and padding columns zero) scaled by 1/valid and
 * writes the mean loss.  target: int64 [B, H*W+1] dictionary ids; a pixel is ignored when its
 * target is pad, eos or <seg_nseg>.  label_smoothing in [0, 1]: F.cross_entropy's epsilon (seg_criterion.py:265; 0 = plain CE,
 * bit-identical to ABI <= 14).  Requires H == 16*hp, W == 16*wp, 1 <= nseg <= 512.  Every tile entry point of this section
 * (csrc/seg_tile.h: check_tile_args) refuses NULL / misaligned logits or target and batch strides below a sample with
 * IFSEG_ERR_BAD_ARG, B, hp, wp < 1, H != 16 hp, W != 16 wp, nseg outside 1..512, ldl < nseg, B*hp*wp >= 2^31 with
 * IFSEG_ERR_BAD_SHAPE.  ifseg_seg_loss_gather, ifseg_seg_loss_gather_sum and ifseg_seg_loss_gather3 below are three doors of ONE
 * kernel (csrc/loss.hip: seg_loss_gather_kernel), which sums the partials of the sources it is given -- a NULL source is not
 * added as a zero -- and writes 1, 3 or 4 words of loss_out; this entry passes the CE source alone. */
int ifseg_seg_loss_tiles(const void* logits, int ldl, long long logits_bs, const long long* target,
                         long long target_bs, int B, int hp, int wp, int H, int W, int nseg,
                         long long seg_id_offset, long long pad_id, long long eos_id, float* tile_partial,
                         float* stats_part, int* bad_label /* device flag, set to 1 when a target is neither a class nor
                         pad / eos / ignore (F.cross_entropy would raise); may be NULL */, float label_smoothing, void* stream);
int ifseg_seg_loss_gather(const float* tile_partial, const float* stats, void* dlogits, int ldl,
                          long long dlogits_bs, int B, int hp, int wp, int nseg, float* loss_out, void* stream);
/* ifseg_seg_loss_tiles with a weight per pixel and per class (ifseg_amd.criterions.seg_criterion.weighted_loss_reference is
 * the specification; F.cross_entropy(weight=class_weight, reduction="none", label_smoothing) per pixel, times q):
 *   pixel_weight  uint8 [B][H*W] on the device, batch stride pw_bs >= H*W bytes, q in 0..255; NULL: q = 1
 *   class_weight  fp32 [nseg] on the device, non-negative (the caller's duty); NULL: ones
 *   stats_part[tile][0] = sum q l over the tile's valid pixels
 *   stats_part[tile][1] = its share of the normaliser Z: sum q cw[y] (norm_pixels == 0, torch's weighted mean; the loss does
 *                         not depend on the scale of q), or qmax per valid pixel (norm_pixels != 0; qmax = 255 with a plane,
 *                         else 1: a batch of unsure pixels gives a smaller gradient)
 * the histograms and bad_label count valid pixels whatever their weights, and tile_partial carries the weighted gradient, so
 * ifseg_reduce_parts and ifseg_seg_loss_gather follow unchanged: loss = stats[0] / stats[1], 0 with a zero gradient when
 * Z = 0.  No global atomics.  The refusals of ifseg_seg_loss_tiles; pw_bs < H*W, class_weight not 4-byte aligned:
 * IFSEG_ERR_BAD_ARG. */
int ifseg_seg_loss_tiles_weighted(const void* logits, int ldl, long long logits_bs, const long long* target,
                                  long long target_bs, int B, int hp, int wp, int H, int W, int nseg,
                                  long long seg_id_offset, long long pad_id, long long eos_id,
                                  const unsigned char* pixel_weight, long long pw_bs, const float* class_weight,
                                  int norm_pixels, float* tile_partial, float* stats_part, int* bad_label,
                                  float label_smoothing, void* stream);

/* ---- online hard example mining (mmseg's OHEMPixelSampler with `thresh` given) as a producer of the pixel_weight plane above;
 * csrc/ohem.hip, ifseg_amd.criterions.seg_criterion.hardness_reference / ohem_reference are the specifications ----
 * ifseg_seg_hardness: the front half of ifseg_seg_loss_tiles (same logits, target, x16 bilinear upsample, same validity
 * predicate) -> hardness fp32 [B][H*W] (batch stride hardness_bs >= H*W floats): the softmax probability of the pixel's own
 * label, clamped to <= 1, on a valid pixel, -1 elsewhere.  One launch, no atomics.  NULL / misaligned pointers, strides below a
 * sample: IFSEG_ERR_BAD_ARG; B, hp, wp < 1, H != 16 hp, W != 16 wp, nseg outside 1..512, ldl < nseg: IFSEG_ERR_BAD_SHAPE. */
int ifseg_seg_hardness(const void* logits, int ldl, long long logits_bs, const long long* target, long long target_bs, int B,
                       int hp, int wp, int H, int W, int nseg, long long seg_id_offset, long long pad_id, long long eos_id,
                       float* hardness, long long hardness_bs, void* stream);
/* ifseg_ohem_select: hardness fp32 [B][n] (contiguous) -> out uint8 [B][n] and info int64 [4], four launches, nothing read back.
 * Values are compared as the uint32 bit patterns of their fp32; an entry is a candidate iff bits <= 0x3F800000 (0 <= v <= 1, sign
 * clear).  k = min(min_kept * B, #candidates - 1), kth = the k-th smallest candidate (from 0) by an exact radix select (three
 * digits of 10 bits, 64-bit integer counters: bit-reproducible), tau = max(bits(thresh), kth); out = weight[i] (uint8 [B][n],
 * NULL: 255) where the entry is a candidate below tau (strictly), else 0.  info = #candidates, #kept, tau, kth (0 without a
 * candidate).  work: uint64 [3 * 1024 + 16], zeroed once by the caller; every call leaves every word of it zero again, so
 * the same sequence replays inside a captured graph.  out must not overlap hardness or weight (the caller's duty).
 * NULL / misaligned pointers (hardness 4 bytes, info and work 8), thresh outside [0, 1] or NaN, min_kept outside [0, 2^40):
 * IFSEG_ERR_BAD_ARG; B outside [1, 2^20), n < 1, B*n >= 2^31: IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_ohem_select(const float* hardness, int B, long long n, float thresh, long long min_kept, const unsigned char* weight,
                      unsigned char* out, long long* info, unsigned long long* work, void* stream);
/* Per-sample soft Dice on the same x16 upsample (csrc/dice.hip; criterions/seg_criterion.py: dice_sums_reference and
 * dice_loss_reference state the rule).  With p_ic = softmax_c(v_i) over the valid pixels i of sample b (the validity predicate of
 * ifseg_seg_loss_tiles): I_bc = sum p_ic [y_i = c], P_bc = sum p_ic^2, Y_bc = sum [y_i = c], N = 2 I + smooth, Q = P + Y + smooth,
 *   dice_weight L_dice = sum_b sum_c k_c (1 - N_bc / Q_bc),   k_c = dice_weight class_weight[c] / (B nseg)   (NULL: ones).
 * ifseg_seg_dice_sums (pass A): sums_part fp32 [B*hp*wp][3*nseg] = every tile's I, P, Y; ifseg_reduce_parts(outer = B,
 *   parts = hp*wp, n = 3*nseg) gives sums [B][3][nseg] in a fixed order.
 * ifseg_seg_dice_tiles (pass B): from sums, tile_partial fp32 [B*hp*wp][9][nseg] = the adjoint of the interpolation applied to
 *   d (dice_weight L_dice) / d v, in final scale, and dice_out[0] = dice_weight L_dice (summed by workgroup 0 in a fixed order).
 * ifseg_seg_loss_gather_sum: ifseg_seg_loss_gather's kernel with two sources, dlogits = bf16(sum of the CE partials * (1 / stats[1]) +
 *   sum of the Dice partials) in one rounding (eos row and padding columns zero), loss_out[3] = total, CE (stats[0] / stats[1], 0
 *   when stats[1] = 0), Dice.  ce_partial NULL (stats is then not read): Dice alone, CE = 0.
 * One workgroup of 256 per cell, no atomics: two runs give equal bits.  Refusals, nothing launched: NULL / misaligned pointers
 * (class_weight 4 bytes), strides below a sample, smooth or dice_weight <= 0 or not finite: IFSEG_ERR_BAD_ARG; B, hp, wp < 1,
 * H != 16 hp, W != 16 wp, nseg outside 1..512, ldl < nseg, B*hp*wp >= 2^31: IFSEG_ERR_BAD_SHAPE. */
int ifseg_seg_dice_sums(const void* logits, int ldl, long long logits_bs, const long long* target, long long target_bs, int B,
                        int hp, int wp, int H, int W, int nseg, long long seg_id_offset, long long pad_id, long long eos_id,
                        float* sums_part, void* stream);
int ifseg_seg_dice_tiles(const void* logits, int ldl, long long logits_bs, const long long* target, long long target_bs, int B,
                         int hp, int wp, int H, int W, int nseg, long long seg_id_offset, long long pad_id, long long eos_id,
                         const float* sums, const float* class_weight, float dice_weight, float smooth, float* tile_partial,
                         float* dice_out, void* stream);
int ifseg_seg_loss_gather_sum(const float* ce_partial, const float* stats, const float* dice_partial, const float* dice_value,
                              void* dlogits, int ldl, long long dlogits_bs, int B, int hp, int wp, int nseg, float* loss_out,
                              void* stream);
/* Distillation on the same x16 upsample (csrc/distill.hip; criterions/seg_criterion.py: distill_loss_reference states the rule).
 * With s_i, t_i the upsampled student / teacher logits, p_i = softmax(s_i / T), q_i = softmax(t_i / T), M the pixels the loss
 * kernel calls valid (mask_all = 0) or every pixel (mask_all != 0; target may then be NULL), N = |M| over the batch:
 *   L_kd = T^2 (1 / N) sum_{i in M} KL(q_i || p_i),   d (w L_kd) / d s_ic = w (T / N) (p_ic - q_ic) on M.
 * ifseg_seg_distill_tiles: teacher bf16 [B, >= hp*wp, ldt >= nseg] with strides of its own (its padding columns and eos row are
 *   never read); tile_partial fp32 [B*hp*wp][9][nseg] = the adjoint of the interpolation applied to p - q on M, unnormalised;
 *   kd_part fp32 [B*hp*wp][2] = every tile's sum of KL and its pixels in M.  ifseg_reduce_parts(outer = 1, parts = B*hp*wp, n = 2)
 *   gives kd_stats [2] in a fixed order.
 * ifseg_seg_loss_gather3: ifseg_seg_loss_gather's kernel with all three sources; any source may be NULL, not all three (a NULL
 *   source's term enters neither dlogits nor the total, its loss_out word is 0):
 *   dlogits = bf16(CE partials * (1 / stats[1]) + Dice partials + KD partials * (kd_weight T / max(kd_stats[1], 1))) in one
 *   rounding (eos row and padding columns zero), loss_out[4] = total, CE, Dice, KD = kd_weight T^2 kd_stats[0] / kd_stats[1]
 *   (0 when kd_stats[1] = 0).
 * One workgroup of 256 per cell, no atomics: two runs give equal bits.  Refusals, nothing launched: NULL / misaligned pointers, a
 * source without its value / statistics, strides below a sample, kd_weight <= 0 or not finite: IFSEG_ERR_BAD_ARG; B, hp, wp < 1,
 * H != 16 hp, W != 16 wp, nseg outside 1..512, ldl or ldt < nseg, B*hp*wp >= 2^31, T <= 0 or not finite: IFSEG_ERR_BAD_SHAPE. */
int ifseg_seg_distill_tiles(const void* logits, int ldl, long long logits_bs, const void* teacher, int ldt, long long teacher_bs,
                            const long long* target, long long target_bs, int B, int hp, int wp, int H, int W, int nseg,
                            long long seg_id_offset, long long pad_id, long long eos_id, float temperature, int mask_all,
                            float* tile_partial, float* kd_part, void* stream);
int ifseg_seg_loss_gather3(const float* ce_partial, const float* stats, const float* dice_partial, const float* dice_value,
                           const float* kd_partial, const float* kd_stats, float kd_weight, float kd_temperature, void* dlogits,
                           int ldl, long long dlogits_bs, int B, int hp, int wp, int nseg, float* loss_out, void* stream);

/* ---------------------------------------------------- image-free samples */
/* The artificial image of `--artificial-image-type rand_k-L-R` (data/mm_data/segmentation_dataset.py:303-345) and its collater
 * layout (:85-107), generated on the device (csrc/imfree.hip; ifseg_amd/artificial.py is the bit-exact host specification).
 *
 * ifseg_imfree_draw: for sample ordinal n = first + b (first = *first_ordinal_dev when that device int64 word is given -- a
 * captured step then draws new images on every replay -- otherwise first_ordinal, 0 <= first, first + B <= 2^32), with
 * u(n, i) = splitmix64(seed + (n << 32) + i) (mod 2^64, the generator of ifseg_dropout):
 *   sh = l + (((u(n,0) >> 32) * (r - l)) >> 32),  sw = l + (((u(n,1) >> 32) * (r - l)) >> 32)        uniform in [l, r)
 *   coarse[y][x] = ((u(n, 2 + y*sw + x) >> 32) * nseg) >> 32                                          uniform in [0, nseg)
 * shapes int32 [B, 2] = (sh, sw); coarse int32 [B, (r-1)^2]: the sh x sw map row-major in the leading entries, 0 beyond.
 * 1 <= l < r <= 129, 1 <= nseg <= 65535, else IFSEG_ERR_BAD_ARG.
 *
 * ifseg_imfree_expand: from shapes / coarse (int32 [B, max_side^2], drawn with r = max_side + 1 or supplied by the caller; sh, sw
 * are clamped to [1, max_side], classes to [0, nseg]), the name table name_ids int64 [nseg+1, Lmax] / name_len int32 [nseg+1]
 * (clamped to [0, Lmax]) and the hp x wp patch grid (image S_h x S_w = 16hp x 16wp), with iy / ix PyTorch's `nearest` index
 * src = min((int)floorf(dst * ((float)in / (float)out)), in - 1):
 *   low[p] = coarse[iy(py)][ix(px)]                                              p = py*wp + px, P = hp*wp
 *   ends int64 [B, P]                 inclusive running sum of name_len[low[p]] per sample
 *   ids  int64 [B, P*Lmax]            the bags' tokens back to back, `pad` behind ends[b, P-1] (static width: no host sync;
 *                                     ifseg_embed_bag_mean never reads past `ends`)
 *   prev_output_tokens int64 [B, P+1] bos, seg_id_offset + low[p]
 *   text2seg_target int64 [B, S_h*S_w + 1]   seg_id_offset + coarse[iy(y)][ix(x)], eos
 * 1 <= max_side <= 128, 1 <= Lmax <= 16, 1 <= nseg <= 65535 (IFSEG_ERR_BAD_ARG); 1 <= P <= 4096, wp <= 2048
 * (IFSEG_ERR_BAD_SHAPE).  All outputs contiguous; 8-byte alignment suffices. */
int ifseg_imfree_draw(unsigned long long seed, long long first_ordinal, const long long* first_ordinal_dev, int B, int l, int r,
                      int nseg, int* shapes, int* coarse, void* stream);
int ifseg_imfree_expand(const int* shapes, const int* coarse, int max_side, const long long* name_ids, const int* name_len,
                        int nseg, int Lmax, int B, int hp, int wp, long long seg_id_offset, long long bos, long long eos,
                        long long pad, long long* ids, long long* ends, long long* prev_output_tokens,
                        long long* text2seg_target, void* stream);

/* -------------------------------------------------------------- optimizer */
/* ---- eval-time post-processing of the criterion (BASELINE config 5) ----------------------
 * top-k neighbour smoothing (criterions/seg_criterion.py:197-213):
 *   f = ifseg_l2norm_rows_bf16(trunk features [B*P, D]);  sim = f f^T (ifseg_gemm_bf16 NT, fp32 out, per batch);
 *   idx = ifseg_topk_rows_f32(sim, k);  prob = ifseg_softmax_rows(logits / temperature);
 *   iters x: prob = ifseg_gather_mean(prob, idx)
 * metrics at the original image resolution (:289-347): ifseg_seg_eval resizes the [hp, wp, n] fp32 score grid
 * bilinearly (align_corners=False, any ratio) to [h, w], takes the argmax and accumulates hist[3][n] =
 * {intersect, predicted, label} pixel counts (uint64, caller zeroes them) and per-block {CE sum, pixel count}
 * partials loss_part[nblocks][2], nblocks = ceil(h*w / 256).  target: int64 [h*w] dictionary ids
 * (seg_id_offset + class; anything outside [0, n) after the offset is ignored).
 * ifseg_topk_rows_f32 orders like torch.topk: NaN first, then the larger value, the lower index first among equals; the k
 * indices of a row are distinct and inside [0, N). */
int ifseg_l2norm_rows_bf16(const void* x, void* out, int rows, int D, void* stream);
int ifseg_topk_rows_f32(const float* sim, int* idx, int rows, int N, int k /* <= 8 */, void* stream);
int ifseg_softmax_rows(const void* logits /* bf16 */, long long batch_stride, int rows_per_batch, int ld, float* prob,
                       int rows, int n, float inv_temperature, int do_softmax /* 0: fp32 copy only */, void* stream);
int ifseg_gather_mean(const float* in, const int* idx, float* out, int B, int P, int n, int k, void* stream);
int ifseg_seg_eval(const float* scores, int hp, int wp, int n, const long long* target, int h, int w,
                   long long seg_id_offset, unsigned long long* hist, float* loss_part, int nblocks, void* stream);

/* ---- label maps at image resolution (ifseg_amd/predict.py; the reference's demo: softmax, resize to the image, argmax) ----
 * ifseg_seg_predict resizes the class scores [B, hp*wp, n] (fp32, class fastest: the layout of ifseg_softmax_rows /
 * ifseg_gather_mean) bilinearly to [B, h, w] with ifseg_seg_eval's value rule (align_corners=False, any ratio, downscaling
 * included):
 *   sy = max((y + 0.5f) * ((float)hp / (float)h) - 0.5f, 0),  y0 = min((int)sy, hp-1),  y1 = min(y0+1, hp-1),  ly = sy - y0
 *   (the same in x),  v_c = w00 p00[c] + w01 p01[c] + w10 p10[c] + w11 p11[c]
 * and writes, in one pass and without a [n, h, w] intermediate,
 *   labels [B, h, w]     the smallest c with maximal v_c (torch.argmax's tie rule); label_bytes 1 -> uint8 (n <= 256), 2 -> int16
 *   conf   [B, h, w]     fp32 v_label, or NULL
 *   probs  [B, n, h, w]  fp32, every v_c, class-major (ifseg_crf_update's input layout), or NULL
 * 1 <= n <= 512, label_bytes 1 or 2 (1 only for n <= 256), labels / conf 16-byte aligned: else IFSEG_ERR_BAD_ARG.
 * B, hp, wp, h, w >= 1, B*h*w < 2^31, hp*wp < 2^22: else IFSEG_ERR_BAD_SHAPE.
 * A workgroup owns 16 x 64 pixels and stages the patch rows they touch in LDS; a tile whose footprint exceeds the staging
 * buffer reads global memory instead (same values).  ifseg_seg_predict_staging sets the size of that buffer in bytes for
 * the launches that follow (0: every tile reads global memory; < 0 or above the built-in limit: the limit) and returns
 * the previous setting -- a test and measurement switch, process-wide. */
int ifseg_seg_predict(const float* scores, int B, int hp, int wp, int n, int h, int w, void* labels, int label_bytes,
                      float* conf, float* probs, void* stream);
int ifseg_seg_predict_staging(int max_bytes);

/* ---- K views into one label map (Segmenter.segment_raw(scales=..., flip=...): mmseg's MultiScaleFlipAug with img_ratios and
 * flip, the "ms+flip" evaluation) ----
 * A view is the score grid [B, hp*wp, n] of one forward at one scale; flip != 0 says that the network saw the image mirrored
 * along its width, so the view's logical column x is the grid's column wp-1-x. */
typedef struct {
  const float* scores; /* device, fp32 [B, hp*wp, n], class fastest, 4-byte aligned */
  int hp, wp, flip;
} ifseg_predict_view;
/* ifseg_seg_predict_views resizes every view to [B, h, w] by ifseg_seg_predict's rule (coordinates and the flat four-weight
 * value v_c per view, on the view's logical columns), adds the K values of a class in fp32 in view order, multiplies by
 * (float)(1.0 / K) and writes labels / conf / probs of that mean exactly as ifseg_seg_predict does (first maximum; conf and
 * probs may be NULL).  With K = 1 and flip = 0 the three outputs are bit-identical to ifseg_seg_predict's.
 * `views` is a HOST array of K entries; it travels as a kernel argument, so the call copies nothing to the device and does
 * not synchronise.  All views share B and n.  One launch, no atomics, no scratch buffer, and no [n, h, w] intermediate unless
 * probs is given.
 * NULL views / labels / a view's scores, K outside 1..16, n outside 1..512, label_bytes other than 1 or 2 (1 only for n <= 256),
 * labels / conf not 16-byte aligned: IFSEG_ERR_BAD_ARG.  B, h, w, a view's hp, wp < 1, B*h*w >= 2^31, a view's
 * hp*wp >= 2^22: IFSEG_ERR_BAD_SHAPE.
 * A workgroup owns 16 x 64 pixels and walks the classes in chunks of 16; per chunk it stages the footprints of the views in
 * LDS, in view order while the buffer lasts, and a view that does not fit reads global memory (same values).
 * ifseg_seg_predict_views_staging sets the size of that buffer like ifseg_seg_predict_staging, for this entry point only. */
int ifseg_seg_predict_views(const ifseg_predict_view* views, int K, int B, int n, int h, int w, void* labels, int label_bytes,
                            float* conf, float* probs, void* stream);
int ifseg_seg_predict_views_staging(int max_bytes);

/* ---- scoring against ground truth on the device (Segmenter.evaluate_raw; the reference's valid_step metric,
 * seg_criterion.py:306-314, 349-362, for any number of images and views) ----
 * Counters: areas uint64 [3, n] = per class #(pred = c and gt = c), #(pred = c), #(gt = c) over the SCORED pixels, tally
 * uint64 [2] = #scored pixels, #pixels whose ground truth is out of range.  Ground truth is uint8 (gt_bytes 1) or int16 (2):
 *   raw_labels != 0   0 and 255 are ignored, any other x is class x - 1 (segmentation_dataset.py:231-233)
 *   raw_labels == 0   n and 255 are ignored, any other x is class x
 * a class outside [0, n) is out of range: not scored, counted in tally[1].  Every entry point ADDS to areas and tally (64-bit
 * integer atomics, one per workgroup and non-zero bin; the sums do not depend on the order) and never clears them.
 * A predicted label outside [0, n) -- only ifseg_seg_areas can be handed one -- is counted in tally[0] and areas[2] alone.
 *
 * ifseg_seg_areas scores npix predicted labels (uint8, label_bytes 1, or int16, 2) against npix ground-truth values; both
 * pointers may have any element alignment.  NULL labels / gt / areas / tally, label_bytes or gt_bytes outside {1, 2}, n
 * outside 1..512, an int16 pointer at an odd address, areas or tally not 8-byte aligned: IFSEG_ERR_BAD_ARG; npix < 1 or
 * >= 2^31: IFSEG_ERR_BAD_SHAPE.
 *
 * ifseg_seg_score / ifseg_seg_score_views are ifseg_seg_predict / ifseg_seg_predict_views with the counting in the kernel's
 * epilogue: gt is [B, h, w].  labels, conf and probs are ALL optional here (NULL: not written; label_bytes is then ignored);
 * what is written is what the predict entry point writes, bit for bit, for the same staging decision (the counters' table
 * takes (3 n + 2) * 4 bytes of the LDS staging budget).  The refusals of the predict entry points, and as above for gt,
 * gt_bytes, areas and tally; nothing is launched on a refusal.  The *_staging setters apply. */
int ifseg_seg_areas(const void* labels, int label_bytes, const void* gt, int gt_bytes, long long npix, int n, int raw_labels,
                    unsigned long long* areas, unsigned long long* tally, void* stream);
/* ifseg_seg_confusion counts which class is taken for which: confusion uint64 [n][n + 1], ADDED to and never cleared.  Inputs,
 * the ground-truth rule and the set of scored pixels are ifseg_seg_areas'; a scored pixel of ground-truth class c with
 * predicted label p adds 1 to confusion[c][p] where 0 <= p < n, else to confusion[c][n] (the "outside" column).  So, over
 * the same inputs: the sum of all entries is tally[0], the diagonal of the first n columns areas[0], their column sums
 * areas[1], the row sums areas[2].  Integer sums: exact and bit-reproducible.
 * A workgroup counts in a private LDS table -- the matrix itself up to n = 127, a hashed table of 4096 (class, label) pairs
 * above, a pair that finds no slot adding to global memory directly -- and only the pairs it met leave it, one 64-bit atomic
 * each.  NULL labels / gt / confusion, label_bytes or gt_bytes outside {1, 2}, n outside 1..512, an int16 pointer at an odd
 * address, confusion not 8-byte aligned: IFSEG_ERR_BAD_ARG; npix < 1 or >= 2^31: IFSEG_ERR_BAD_SHAPE; nothing is launched on
 * a refusal. */
int ifseg_seg_confusion(const void* labels, int label_bytes, const void* gt, int gt_bytes, long long npix, int n, int raw_labels,
                        unsigned long long* confusion, void* stream);
/* the kernel's table sizes, for callers that size an input against them: which = 0 the entries of the direct table (n (n + 1)
 * up to this counts in it), 1 the slots of the hashed table, 2 the pixels a workgroup takes per step, 3 the workgroups of a
 * launch at most; any other which: IFSEG_ERR_BAD_ARG. */
int ifseg_seg_confusion_limit(int which);
/* ifseg_seg_boundary_areas counts Boundary IoU's band areas (Cheng et al., CVPR 2021, semantic form; csrc/boundary.hip):
 * labels and gt are [B][h][w] maps (uint8, bytes 1, or int16, 2; any element alignment).  A pixel p of a map is IN THE BAND of
 * that map iff some position q with |dx| <= d and |dy| <= d lies outside the image or carries another value than p; values are
 * compared as they are (an ignore value of the ground truth, a label outside [0, n) are values of their own).  The
 * ground-truth rule and the set of scored pixels are ifseg_seg_areas'; over the scored pixels only
 *   bareas[2][c] += #(gt class c and in the gt band)         bareas[1][c] += #(pred = c and in the pred band)
 *   bareas[0][c] += #(gt class = pred = c and in both bands)
 * a predicted label outside [0, n) being in no bin of rows 0 and 1.  bareas uint64 [3][n] is ADDED to and never cleared
 * (64-bit integer atomics, one per workgroup and non-zero bin: exact and bit-reproducible).  band, where not NULL, is uint8
 * [B][h][w] and is written for EVERY pixel, scored or not: bit 0 = in the gt band, bit 1 = in the pred band.  d >= max(h, w)
 * puts every pixel in both bands: bareas then takes what ifseg_seg_areas adds to areas.
 * NULL labels / gt / bareas, label_bytes or gt_bytes outside {1, 2}, an int16 map at an odd address, bareas not 8-byte
 * aligned, n outside 1..512, d outside 1..64: IFSEG_ERR_BAD_ARG; B, h or w < 1 or B h w >= 2^31: IFSEG_ERR_BAD_SHAPE; nothing
 * is launched on a refusal.  Nothing is allocated.  The dynamic LDS of a launch grows with d (71 488 bytes at d = 64, n = 512). */
int ifseg_seg_boundary_areas(const void* labels, int label_bytes, const void* gt, int gt_bytes, int B, int h, int w, int n, int d,
                             int raw_labels, void* bareas, void* band, void* stream);
/* which = 0: the largest d, 1: the largest n; any other which: IFSEG_ERR_BAD_ARG. */
int ifseg_seg_boundary_limit(int which);
/* ifseg_seg_distance writes the exact squared Euclidean distance of every pixel of labels [B][h][w] (uint8, bytes 1, or int16,
 * 2; any element alignment) to the nearest pixel of ANOTHER value of the same image (csrc/distance.hip;
 * ifseg_amd/predict.py distance_reference is the specification): out uint16 [B][h][w] (2-byte aligned) =
 * D2(p) = min over q with L(q) != L(p) of (px - qx)^2 + (py - qy)^2 where D2 <= R^2, R = max_distance in 1..128, and 65535
 * where D2 > R^2 or the image holds no other value.  Values are compared as they are.  border != 0: every position outside
 * the image counts as another value as well.  Distances never cross from one image into the next.
 * work: B h w bytes, the clamped vertical distances (1..R, 255 for none), written by the first of the two launches and read
 * by the second.  Integers, no atomics, one writer per element: two calls give equal bits.  Dynamic LDS (16 + 2 R) 128 bytes
 * for the first launch (34 816 at R = 128) and 48 (64 + 2 R) for the second (15 360).
 * NULL labels / work / out, label_bytes outside {1, 2}, int16 labels or out at an odd address, max_distance outside 1..128,
 * any two of labels / work / out sharing a byte: IFSEG_ERR_BAD_ARG; B, h or w < 1 or B h w >= 2^31: IFSEG_ERR_BAD_SHAPE;
 * nothing is launched on a refusal.  Nothing is allocated, nothing synchronises. */
int ifseg_seg_distance(const void* labels, int label_bytes, int B, int h, int w, int max_distance, int border, void* work,
                       void* out, void* stream);
/* ifseg_seg_trimap_areas counts ifseg_seg_areas' three rows per distance ring (trimap_areas_reference is the specification):
 * labels and gt [B][h][w] as in ifseg_seg_areas (the same ground-truth rule and scored pixels), dist uint16 [B][h][w] the
 * ground truth's plane from ifseg_seg_distance with max_distance >= radii[K - 1], radii K ints on the HOST, strictly
 * ascending in 1..128, 1 <= K <= 8.  Ring k holds the pixels with radii[k - 1]^2 < dist <= radii[k]^2 (radii[-1] = 0); a
 * pixel beyond the last radius (65535 among them) is in none.  trimap uint64 [K][3][n] is ADDED to:
 * [k][0][c] += #(pred = gt = c), [k][1][c] += #(pred = c), [k][2][c] += #(gt = c) over the scored pixels of ring k.  One
 * launch; a workgroup counts into K 3 n uint32 of LDS (48 KiB at K = 8, n = 512) and only non-zero bins leave, one 64-bit
 * integer atomic each.
 * NULL labels / gt / dist / radii / trimap, an element size outside {1, 2}, an int16 map or dist at an odd address, trimap not
 * 8-byte aligned, n outside 1..512, K outside 1..8, radii out of range or not ascending, trimap sharing a byte with a map:
 * IFSEG_ERR_BAD_ARG; B, h or w < 1 or B h w >= 2^31: IFSEG_ERR_BAD_SHAPE; nothing is launched on a refusal. */
int ifseg_seg_trimap_areas(const void* labels, int label_bytes, const void* gt, int gt_bytes, const void* dist, int B, int h,
                           int w, int n, const int* radii, int K, int raw_labels, void* trimap, void* stream);
/* which = 0: the largest max_distance, 1: the "far" value, 2: the largest K, 3: the largest n; any other which:
 * IFSEG_ERR_BAD_ARG. */
int ifseg_seg_distance_limit(int which);
int ifseg_seg_score(const float* scores, int B, int hp, int wp, int n, int h, int w, void* labels, int label_bytes, float* conf,
                    float* probs, const void* gt, int gt_bytes, int raw_labels, unsigned long long* areas,
                    unsigned long long* tally, void* stream);
int ifseg_seg_score_views(const ifseg_predict_view* views, int K, int B, int n, int h, int w, void* labels, int label_bytes,
                          float* conf, float* probs, const void* gt, int gt_bytes, int raw_labels, unsigned long long* areas,
                          unsigned long long* tally, void* stream);

/* ---- raw images in (ifseg_amd/predict.py Segmenter.segment_raw; the reference's evaluation transform: Resize(keep_ratio),
 * Normalize of :148-156; the dataset's two channel reversals, :218 and :256, cancel, so reverse_channels is 0 for a
 * checkpoint tuned by the reference) ----
 * ifseg_image_load turns uint8 images [B, H0, W0, 3] (HWC, contiguous, any byte alignment) into patch_images
 * [B, 3, oh, ow] (NCHW; out_bytes 4 -> fp32, 2 -> bf16 round-to-nearest-even).  Per output element:
 *   source coordinate in integers, per axis (d of `out` samples over `in`):
 *     num = max((2d+1) in - out, 0),  i0 = min(num / (2 out), in-1),  i1 = min(i0+1, in-1),
 *     l = float(num - i0 2 out) / float(2 out),  0 when i0 == i1          (align_corners=False, no antialiasing)
 *   v = w00 a + w01 b + w10 c + w11 d in fp32 (w00 = (1-ly)(1-lx), ...),  q = clamp(floor(v + 0.5), 0, 255),
 *   out = lut[c_out][q], where channel c_out reads source channel 2 - c_out when reverse_channels != 0, else c_out.
 * lut: fp32 [3][256] on the device, built by the caller ((k/255 - mean[c]) / std[c]): the normalised value is a table entry,
 * whatever the device's division does.
 * The staging loads are aligned dwords: up to 3 bytes in front of `images` and behind its last byte may be READ (never past
 * a page boundary, so a view at the start or end of an allocation is safe); nothing outside `out` is written.
 * NULL images / lut / out, out_bytes other than 2 or 4, out not 16-byte aligned: IFSEG_ERR_BAD_ARG.
 * B, H0, W0, oh, ow >= 1; B*H0*W0*3, B*3*oh*ow, 2*H0*oh and 2*W0*ow < 2^31: else IFSEG_ERR_BAD_SHAPE.
 * A workgroup owns 16 x 64 output pixels and stages the source bytes they touch in LDS; a tile whose footprint exceeds the
 * staging buffer reads global memory instead (same values), and so does every tile when the bound of the largest footprint
 * exceeds it (no buffer is requested then).  ifseg_image_load_staging sets the size of that buffer in
 * bytes for the launches that follow (0: every tile reads global memory; < 0 or above the built-in limit: the limit) and
 * returns the previous setting -- a test and measurement switch, process-wide. */
int ifseg_image_load(const void* images, int B, int H0, int W0, int oh, int ow, const float* lut, int reverse_channels,
                     void* out, int out_bytes, void* stream);
int ifseg_image_load_staging(int max_bytes);

/* ---- sliding-window inference (Segmenter.segment_raw(slide=...): mmseg's test_cfg mode='slide') ----
 * The window rule, per axis of o samples with crop c and stride s (1 <= s <= c): g = max(o - c + s - 1, 0) / s + 1 windows of
 * e = min(c, o) samples, window i starting at max(min(i s + c, o) - c, 0) -- the last window is pulled back inside, an axis
 * shorter than the crop has one shorter window.  The windows of an [oh, ow] plane are the cross product, rows outer:
 * window k = iy gx + ix, Nw = gy gx <= IFSEG_SLIDE_MAX_WINDOWS, all of extent (ch, cw) = (e_y, e_x).  Every entry point below
 * derives the windows from (oh, ow, crop_h, crop_w, stride_h, stride_w); a crop or stride < 1, a stride above its crop, oh or
 * ow < 1 and Nw above the limit are IFSEG_ERR_BAD_SHAPE. */
#define IFSEG_SLIDE_MAX_WINDOWS 64
/* ifseg_image_load_windows writes the window batch [B Nw, 3, ch, cw] of ifseg_image_load's [B, 3, oh, ow] directly: element
 * (b Nw + k, c, y, x) is ifseg_image_load's element (b, c, ys[k] + y, xs[k] + x), bit for bit (a window is a slice of the
 * loaded image, never a resize of its own), and no [B, 3, oh, ow] image is written.  Arguments, alignment, reads around
 * `images`, refusals and staging (ifseg_image_load_staging) as ifseg_image_load; B*Nw*3*ch*cw < 2^31. */
int ifseg_image_load_windows(const void* images, int B, int H0, int W0, int oh, int ow, int crop_h, int crop_w, int stride_h,
                             int stride_w, const float* lut, int reverse_channels, void* out, int out_bytes, void* stream);
/* ifseg_seg_predict_windows merges the per-window class scores [B, Nw, hpw*wpw, n] (fp32, class fastest; window k of image b
 * ran the network on its own hpw x wpw grid) into one label map [B, h, w], in one launch:
 *   u_k  = window k's grid resized to (ch, cw) by ifseg_seg_predict's rule (coordinates and the flat four-weight value)
 *   m    = (sum of u_k over the windows that cover a pixel of the [oh, ow] plane, in window order) / their number
 *   v    = m resized to (h, w) by the same coordinate rule, sum of weight * m over the taps of NON-ZERO weight
 * labels / conf / probs of v as ifseg_seg_predict writes them (first maximum; conf and probs may be NULL).  Neither the u_k nor
 * m is written.  With one window that covers the plane and (h, w) == (oh, ow) the outputs are ifseg_seg_predict's bit for
 * bit.  ifseg_seg_score_windows is the same launch with ifseg_seg_score's counting in its epilogue (labels optional).
 * Refusals: those of ifseg_seg_predict for scores, n, labels, label_bytes, conf, probs, B, h, w; the window rule's;
 * hpw, wpw < 1 or Nw*hpw*wpw >= 2^22: IFSEG_ERR_BAD_SHAPE; and ifseg_seg_score's for gt, gt_bytes, areas, tally.  Nothing is
 * launched on a refusal.
 * A workgroup owns 16 x 64 pixels and walks the classes in chunks of 16; per chunk it stages the patches of every window
 * under the tile in LDS, or, where they do not fit the staging buffer, reads global memory (same values).
 * ifseg_seg_predict_windows_staging sets the size of that buffer like ifseg_seg_predict_staging, for these two only. */
int ifseg_seg_predict_windows(const float* scores, int B, int hpw, int wpw, int n, int oh, int ow, int crop_h, int crop_w,
                              int stride_h, int stride_w, int h, int w, void* labels, int label_bytes, float* conf, float* probs,
                              void* stream);
int ifseg_seg_score_windows(const float* scores, int B, int hpw, int wpw, int n, int oh, int ow, int crop_h, int crop_w,
                            int stride_h, int stride_w, int h, int w, void* labels, int label_bytes, float* conf, float* probs,
                            const void* gt, int gt_bytes, int raw_labels, unsigned long long* areas, unsigned long long* tally,
                            void* stream);
int ifseg_seg_predict_windows_staging(int max_bytes);

/* ---- multi-scale + flip OVER sliding windows (Segmenter(slide_views=True): mmseg's MultiScaleFlipAug over test_cfg mode='slide') ----
 * ifseg_image_load_windows_mirrored is ifseg_image_load_windows on the MIRRORED resized image: element (b Nw + k, c, y, x) is
 * ifseg_image_load's element (b, c, ys[k] + y, ow - 1 - (xs[k] + x)), bit for bit -- the image is mirrored after the resize, as
 * mmseg does, and still never written.  (The window starts are not symmetric, the last window being pulled back inside: these
 * are not the unmirrored windows flipped.)  Everything else as ifseg_image_load_windows. */
int ifseg_image_load_windows_mirrored(const void* images, int B, int H0, int W0, int oh, int ow, int crop_h, int crop_w,
                                      int stride_h, int stride_w, const float* lut, int reverse_channels, void* out, int out_bytes,
                                      void* stream);
/* View k of ifseg_seg_predict_slide_views is an input of ifseg_seg_predict_windows at its own plane: the window rule on
 * (oh, ow) with the call's crop and stride, every window on an hpw x wpw grid; flip: the network saw the resized image
 * mirrored along its width. */
typedef struct {
  const float* scores; /* device, fp32 [B, Nw, hpw*wpw, n], class fastest, 4-byte aligned */
  int hpw, wpw, oh, ow, flip;
} ifseg_slide_view;
/* ifseg_seg_predict_slide_views merges 1 .. 16 such views of the same images into one label map [B, h, w], in one launch:
 *   v_k  = ifseg_seg_predict_windows' v of view k (the same operations: with K = 1, flip = 0 and softmax = 0 the three outputs
 *          are that entry point's, bit for bit), a flipped view taken at the mirrored output column w - 1 - x
 *   softmax != 0:  v_k <- exp(v_k - max_c v_k) / sum_c exp(v_k - max_c v_k), the sum in class order (mmseg's order: the views'
 *          logits are merged and resized, THEN normalised, un-mirrored and averaged); softmax == 0: v_k as it is (scores that
 *          are probabilities already: everything after the per-patch softmax is linear)
 *   mean = (v_0 + ... + v_{K-1}, added in view order) * (float)(1.0 / K)
 * labels / conf / probs of the mean as ifseg_seg_predict writes them.  ifseg_seg_score_slide_views is the same launch with
 * ifseg_seg_score's counting in its epilogue (labels optional).
 * Refusals: K outside 1..16, a NULL or misaligned view: IFSEG_ERR_BAD_ARG; per view those of ifseg_seg_predict_windows
 * (window rule, at most IFSEG_SLIDE_MAX_WINDOWS windows, Nw*hpw*wpw < 2^22); the rest as ifseg_seg_predict_views /
 * ifseg_seg_score_views.  Nothing is launched on a refusal.
 * A workgroup owns 16 x 64 pixels and walks the classes in chunks of 16.  softmax takes three walks (maximum, sum, mean) and
 * keeps max and sum of every pixel and view in LDS, 8 KiB per view on top of the 64 KiB the other kernels budget (gfx950 gives
 * a workgroup 160 KiB; a device that cannot hold them: IFSEG_ERR_BAD_SHAPE).  Views are staged in LDS in view order while the
 * buffer lasts; a view that does not fit reads global memory (same values).  ifseg_seg_predict_slide_views_staging sets the
 * size of that buffer like ifseg_seg_predict_staging, for these two only. */
int ifseg_seg_predict_slide_views(const ifseg_slide_view* views, int K, int B, int n, int crop_h, int crop_w, int stride_h,
                                  int stride_w, int h, int w, int softmax, void* labels, int label_bytes, float* conf,
                                  float* probs, void* stream);
int ifseg_seg_score_slide_views(const ifseg_slide_view* views, int K, int B, int n, int crop_h, int crop_w, int stride_h,
                                int stride_w, int h, int w, int softmax, void* labels, int label_bytes, float* conf, float* probs,
                                const void* gt, int gt_bytes, int raw_labels, unsigned long long* areas,
                                unsigned long long* tally, void* stream);
int ifseg_seg_predict_slide_views_staging(int max_bytes);

/* ---- the label map as a picture (Segmenter.render_raw; cell 4 of the reference's visualize_segmentation_web.ipynb:
 * `cmap[labels]` and `image * (1 - opacity) + cmap[labels] * opacity`) ----
 * ifseg_seg_render colours labels [B, H, W] (uint8, label_bytes 1, or int16, 2) over image uint8 [B, H, W, 3] (HWC) into
 * out uint8 [B, H, W, 3], one launch, in integers (ifseg_amd/predict.py render_reference is the specification):
 *   a    = alpha (0..256, the opacity in 256ths); with conf (fp32 [B, H, W], may be NULL):
 *          q = clamp(floor(conf * 255 + 0.5), 0, 255) in fp32 (a rounded product, a rounded sum), NaN -> 0,  a = (alpha q + 127) / 255
 *   out  = (image (256 - a) + palette[l] a) >> 8 per channel for a label 0 <= l < n (palette uint8 [n, 3]);
 *          the image's pixel for any other label (255 "ignore", a negative int16)
 *   boundary = r (0..4): a pixel with a pixel INSIDE the image at |dx| <= r and |dy| <= r whose raw label value differs becomes
 *          boundary_rgb (r | g << 8 | b << 16) unblended, whatever its own label; r = 0: no contours.
 * alpha = 128 is the demo's (image * 0.5 + cmap * 0.5).astype(uint8) bit for bit, alpha = 256 its cmap[labels].
 * image, palette and out may sit at ANY byte address and labels at any element address: rows are 3 W bytes, of any residue
 * modulo 4.  Reads of the image are aligned dwords as in ifseg_image_load (up to 3 bytes in front of and behind it may be
 * READ, never past a page boundary).  Nothing outside out's B H W 3 bytes is written: a workgroup owns 16 x 64 pixels and
 * stores aligned dwords where a dword lies inside its bytes of a row and single bytes at the two ends, so no dword has two
 * writers.  out must not overlap image or labels (the caller's duty: rows are read by other workgroups than write them).
 * NULL labels / image / palette / out, label_bytes outside {1, 2}, int16 labels at an odd address, conf not 4-byte aligned,
 * n outside 1..512, boundary outside 0..4, alpha outside 0..256, boundary_rgb outside 0..0xffffff: IFSEG_ERR_BAD_ARG;
 * B, H, W < 1 or B*H*W >= 2^31: IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_seg_render(const void* labels, int label_bytes, const void* image, const void* palette, int n, const float* conf,
                     int B, int H, int W, int alpha, int boundary, int boundary_rgb, void* out, void* stream);

/* ---- confidence-filtered pseudo-labels (Segmenter.pseudo_label_raw: self-training on unlabeled photographs, the CBST /
 * MaskCLIP+ recipe; the reference has no counterpart) ----  Everything is integer: bin(conf) = clamp(floor(conf * 256), 0, 255)
 * in fp32 (the product is exact), NaN -> 0 (fmaxf(NaN, 0) = 0), +inf -> 255.  ifseg_amd/predict.py states the rules
 * (confidence_histogram_reference, pseudo_thresholds, pseudo_label_reference); csrc/pseudo.hip.
 *
 * ifseg_seg_conf_hist counts npix predicted labels (uint8, label_bytes 1, or int16, 2; any element alignment) with their
 * confidences conf fp32 [npix]: hist uint64 [n][256] += #(label = c and bin(conf) = b), tally uint64 [2] += #labels in [0, n),
 * #labels outside.  Both are ADDED to and never cleared; integer sums, exact and bit-reproducible.  A workgroup counts in a
 * private LDS table -- the histogram itself up to n = 64, a hashed table of 4096 (label, bin) pairs above, a pair that finds no
 * slot adding to global memory directly -- and only the pairs it met leave it, one 64-bit atomic each.  NULL labels / conf /
 * hist / tally, label_bytes outside {1, 2}, n outside 1..512, an int16 pointer at an odd address, conf not 4-byte aligned, hist
 * or tally not 8-byte aligned: IFSEG_ERR_BAD_ARG; npix < 1 or >= 2^31: IFSEG_ERR_BAD_SHAPE; nothing is launched on a refusal. */
int ifseg_seg_conf_hist(const void* labels, int label_bytes, const float* conf, long long npix, int n,
                        unsigned long long* hist, unsigned long long* tally, void* stream);
/* ifseg_seg_calibration counts how often a confidence is right (the reliability diagram and ECE, Guo et al., ICML 2017, per
 * predicted class; csrc/calib.hip; predict.py: calibration_reference): npix predicted labels (uint8, label_bytes 1, or int16,
 * 2; any element alignment), their confidences conf fp32 [npix] and npix ground-truth values (uint8 / int16, gt_bytes; any
 * element alignment of their own).  The ground-truth rule and the set of scored pixels are ifseg_seg_areas'.  A scored pixel
 * with predicted label l in [0, n) adds 1 to calibration[l][bin(conf)][hit], hit = (l == the ground truth's class), bin as
 * above; calibration is uint64 [n][256][2].  tally uint64 [2] += #scored pixels with a label in [0, n), #scored pixels with a
 * label outside it.  Pixels that are not scored (an ignored ground truth, or one outside the classes) are counted nowhere.
 * Both are ADDED to and never cleared; integer sums, exact and bit-reproducible.  So, over the same inputs: calibration summed
 * over bins and hit is the per-class count of the scored, in-range labels (areas[1]), calibration[.][.][1] summed over bins is
 * areas[0], and the sum of all entries is tally[0] here.
 * A workgroup counts in a private LDS table -- the counters themselves up to n = 32, a hashed table of 4096 (label, bin, hit)
 * keys above, a key that finds no slot adding to global memory directly -- and only the keys it met leave it, one 64-bit
 * atomic each.  NULL labels / conf / gt / calibration / tally, label_bytes or gt_bytes outside {1, 2}, n outside 1..512, an
 * int16 pointer at an odd address, conf not 4-byte aligned, calibration or tally not 8-byte aligned: IFSEG_ERR_BAD_ARG;
 * npix < 1 or >= 2^31: IFSEG_ERR_BAD_SHAPE; nothing is launched on a refusal. */
int ifseg_seg_calibration(const void* labels, int label_bytes, const float* conf, const void* gt, int gt_bytes, long long npix,
                          int n, int raw_labels, unsigned long long* calibration, unsigned long long* tally, void* stream);
/* the kernel's table sizes: which = 0 the classes up to which the direct table counts, 1 the slots of the hashed table, 2 the
 * pixels a workgroup takes per step, 3 the workgroups of a launch at most; any other which: IFSEG_ERR_BAD_ARG. */
int ifseg_seg_calibration_limit(int which);
/* ifseg_seg_temperature_sweep scores K score grids of the same images against one ground truth in one launch (temperature
 * scaling, Guo et al., ICML 2017: the grids are one forward's logits softmaxed at K temperatures; csrc/tsweep.hip; predict.py:
 * temperature_sweep_reference).  grids fp32 [K][B][hp*wp][n], class fastest, contiguous, PROBABILITIES; gt [B][h][w] uint8 /
 * int16 (gt_bytes).  Per pixel and k: p_kc is ifseg_seg_predict's value of class c on grid k, bit for bit (the coordinate rule
 * and the flat four-weight value above), l_k the smallest c with maximal p_kc, conf_k = p_{k,l_k}.  The ground-truth rule and
 * the set of scored pixels are ifseg_seg_areas'; tally uint64 [2] += #scored pixels, #pixels whose ground truth is out of
 * range, once per pixel, not per k.  A pixel that is not scored contributes nowhere.  Over the scored pixels, t the true class:
 *   hist[k][bin(conf_k)][l_k == t] += 1          uint64 [K][256][2], all classes together; bin as for ifseg_seg_conf_hist
 *   sums[k][0] += -log(max(p_kt, FLT_MIN))       the negative log likelihood: fp64 log of the fp32 value, so a probability
 *                                                that underflowed to 0 costs 87.3, not infinity
 *   sums[k][1] += sum_c p_kc^2 - 2 p_kt + 1      the Brier score: every product and sum in fp64 on the fp32 values
 * hist, tally and sums (fp64 [K][2]) are ADDED to and never cleared.  The integers leave a workgroup's private LDS table as
 * one 64-bit atomic per non-zero bin: exact.  The floats are reduced in a fixed order -- lanes by a butterfly, the four waves
 * in order, into partials fp64 [tiles][K][2], tiles = B * ceil(h / 16) * ceil(w / 64) (limits 2 and 3), which the caller
 * provides and the call overwrites; a second launch adds the tiles in index order into sums -- so two calls give equal bits
 * and there are no floating-point atomics.  Nothing else is written, nothing is allocated, and the call does not synchronise.
 * hist row k is ifseg_seg_calibration's counters of (l_k, conf_k) summed over the classes.
 * A workgroup owns 16 x 64 pixels and stages the footprint of one grid at a time in LDS; what is left of 64 KiB beside the
 * table (2 KiB per temperature) and the waves' sums is the staging buffer, and a footprint that exceeds it reads global
 * memory instead (same bits).  ifseg_seg_temperature_sweep_staging sets the size of that buffer like
 * ifseg_seg_predict_staging, for this entry point only.
 * NULL or misaligned pointers (grids 4 bytes; hist, tally, sums, partials 8; an int16 gt at an odd address), K outside 1..16,
 * n outside 1..512, gt_bytes outside {1, 2}: IFSEG_ERR_BAD_ARG; B, hp, wp, h, w < 1, 2 hp h or 2 wp w >= 2^31, B*h*w >= 2^31,
 * hp*wp >= 2^22: IFSEG_ERR_BAD_SHAPE; nothing is launched on a refusal. */
int ifseg_seg_temperature_sweep(const float* grids, int K, int B, int hp, int wp, int n, int h, int w, const void* gt,
                                int gt_bytes, int raw_labels, unsigned long long* hist, unsigned long long* tally, double* sums,
                                double* partials, void* stream);
int ifseg_seg_temperature_sweep_staging(int max_bytes);
/* which = 0: the largest K, 1: the largest n, 2 / 3: the rows / columns of a tile (partials holds one [K][2] block per tile),
 * 4: the staging buffer's bytes at the largest K; any other which: IFSEG_ERR_BAD_ARG. */
int ifseg_seg_temperature_sweep_limit(int which);
/* Per-class logit bias (prior-shift correction; logit adjustment, Menon et al., ICLR 2021; the calibration factor of the
 * zero-shot segmentation tables; csrc/bsweep.hip).  The rule: bias fp32 [n] on the device, in logit units, is SUBTRACTED in
 * front of the temperature -- a_c = (z_c - bias[c]) * inv_temperature, z the bf16 logit widened to fp32, the difference one
 * fp32 subtraction.
 * ifseg_softmax_rows_bias is ifseg_softmax_rows on a: prob = softmax(a) (do_softmax != 0), else prob = z_c - bias[c] (the
 * temperature is not applied, as there).  With bias = 0 it gives ifseg_softmax_rows' bits in both modes.  NULL logits / bias /
 * prob, logits at an odd address, bias or prob not 4-byte aligned, bias overlapping prob, n < 1 or rows_per_batch < 1:
 * IFSEG_ERR_BAD_ARG; rows <= 0 does nothing; nothing is launched on a refusal. */
int ifseg_softmax_rows_bias(const void* logits /* bf16 */, long long batch_stride, int rows_per_batch, int ld, const float* bias,
                            float* prob, int rows, int n, float inv_temperature, int do_softmax, void* stream);
/* ifseg_seg_score_grids scores K score grids of the same images against one ground truth in one launch (the sweep over K
 * strengths of a bias direction; predict.py: bias_sweep_reference).  grids fp32 [K][B][hp*wp][n], class fastest, contiguous,
 * ANY values (probabilities or logits); gt [B][h][w] uint8 / int16 (gt_bytes).  Per pixel and k: l_k is ifseg_seg_predict's
 * label on grid k, bit for bit (the coordinate rule, the flat four-weight value, the smallest c of maximal value; a NaN never
 * wins and an all-NaN pixel is class 0).  The ground-truth rule and the set of scored pixels are ifseg_seg_areas'.  Over the
 * scored pixels, t the true class:
 *   areas[k][0][t] += (l_k == t),  areas[k][1][l_k] += 1,  areas[k][2][t] += 1        uint64 [K][3][n]
 * so row k is ifseg_seg_score's areas of grid k; tally uint64 [2] += #scored pixels, #pixels whose ground truth is out of
 * range, once per pixel, not per k.  areas and tally are ADDED to and never cleared.  A workgroup owns 16 x 64 pixels, stages
 * the footprint of one grid at a time in LDS and keeps ONE private uint32 table [3][n] (+ the tallies), whose non-zero bins
 * leave behind every k as one 64-bit atomic each: integers only, so two calls give equal bits.  Nothing else is written,
 * nothing is allocated, and the call does not synchronise.  What is left of 64 KiB beside the table is the staging buffer,
 * and a footprint that exceeds it reads global memory instead (same bits).  ifseg_seg_score_grids_staging sets the size of
 * that buffer like ifseg_seg_predict_staging, for this entry point only.
 * NULL or misaligned pointers (grids 4 bytes; areas, tally 8; an int16 gt at an odd address), areas or tally overlapping each
 * other, grids or gt, K outside 1..16, n outside 1..512, gt_bytes outside {1, 2}: IFSEG_ERR_BAD_ARG; B, hp, wp, h, w < 1,
 * 2 hp h or 2 wp w >= 2^31, B*h*w >= 2^31, hp*wp >= 2^22: IFSEG_ERR_BAD_SHAPE; nothing is launched on a refusal. */
int ifseg_seg_score_grids(const float* grids, int K, int B, int hp, int wp, int n, int h, int w, const void* gt, int gt_bytes,
                          int raw_labels, unsigned long long* areas, unsigned long long* tally, void* stream);
int ifseg_seg_score_grids_staging(int max_bytes);
/* which = 0: the largest K, 1: the largest n, 2 / 3: the rows / columns of a tile, 4: the staging buffer's bytes at the
 * largest K and n; any other which: IFSEG_ERR_BAD_ARG. */
int ifseg_seg_score_grids_limit(int which);
/* ifseg_seg_pseudo filters labels [B, H, W] (uint8 / int16) by conf fp32 [B, H, W] into out uint8 [B, H, W], one launch: a
 * pixel of label l is KEPT iff 0 <= l < n, bin(conf) >= thresholds[l] (int32 [n] on the device, 0 keeps every bin, 256 none)
 * and, with boundary = r (0..4), no pixel INSIDE the image at |dx| <= r and |dy| <= r carries a different label value
 * (ifseg_seg_render's contour predicate, on the labels given, not on the filtered ones).  A kept pixel becomes l + 1 with
 * raw_labels != 0 (the label-PNG convention ifseg_train_draw / ifseg_train_load undo), l without; every other pixel 255.
 * kept uint64 [2][n] is ADDED to: kept[1][c] += #(label = c), kept[0][c] += those that were kept; one 64-bit atomic per
 * workgroup and non-zero entry.  out may sit at any byte address with rows of W bytes; plain per-lane byte stores, nothing
 * outside out's B H W bytes is written.  out must not overlap labels (the caller's duty).
 * NULL labels / conf / thresholds / out / kept, label_bytes outside {1, 2}, int16 labels at an odd address, conf or thresholds
 * not 4-byte aligned, kept not 8-byte aligned, n outside 1..254 (1..255 with raw_labels == 0), boundary outside 0..4:
 * IFSEG_ERR_BAD_ARG; B, H, W < 1 or B*H*W >= 2^31: IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_seg_pseudo(const void* labels, int label_bytes, const float* conf, const int* thresholds, int n, int B, int H, int W,
                     int boundary, int raw_labels, void* out, unsigned long long* kept, void* stream);
/* ifseg_seg_pseudo that also writes the loss weight of every pixel, weight uint8 [B, H, W] (any byte address, not out): 0
 * where out is 255, max(bin(conf), 1) where the pixel was kept -- what ifseg_train_load_plane carries to the batch and
 * ifseg_seg_loss_tiles_weighted reads.  Same launch, same refusals; a NULL weight: IFSEG_ERR_BAD_ARG. */
int ifseg_seg_pseudo_weighted(const void* labels, int label_bytes, const float* conf, const int* thresholds, int n, int B, int H,
                              int W, int boundary, int raw_labels, void* out, void* weight, unsigned long long* kept,
                              void* stream);

/* ---- connected regions of a label map (csrc/regions.hip; ifseg_amd/predict.py regions_reference and
 * region_drop_reference are the specifications; the reference has no counterpart) ----
 * labels [B][H][W], uint8 (label_bytes 1) or int16 (2).  Two pixels of one image are adjacent under connectivity 4 iff they
 * differ by one step in x or in y, under 8 the diagonal steps count too.  A region is a maximal set of pixels connected
 * through adjacency that carry the same value; values are compared as they are (255, negative shorts and anything outside a
 * class range are values of their own), and regions never cross from one image into the next.
 * ifseg_seg_regions writes root int32 [B][H][W] = the smallest y W + x inside its image over the pixels of p's region, and
 * size int32 [B][H][W] = the region's pixel count: four launches on `stream` (a union-find per 16 x 64 tile in LDS; the unions
 * across the tiles' seams, every access to the plane an agent-scope atomic; the chains flattened into `root` and the tiles'
 * counts added at the regions' roots, one 32-bit integer atomic per tile-local region; size gathered), three where an image
 * is one tile.  work and count: int32 [B][H][W] each, the caller's, written in full (nothing needs zeroing).  The results are
 * canonical, so two calls give equal bits.  Every loop's step count is bounded (a chase: H W + 1, a union: 2 H W + 1); a
 * thread that runs out sets *flag to 1 and leaves.  flag is never cleared here: the caller zeroes it, and one word can watch
 * many calls.
 * NULL pointers, label_bytes outside {1, 2}, int16 labels at an odd address, a plane or flag not 4-byte aligned, two of
 * work / count / root / size / labels / flag sharing a byte, connectivity other than 4 or 8: IFSEG_ERR_BAD_ARG; B, H, W < 1 or
 * B*H*W >= 2^31: IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_seg_regions(const void* labels, int label_bytes, int B, int H, int W, int connectivity, int* work, int* count,
                      int* root, int* size, int* flag, void* stream);
/* ifseg_seg_regions on uint8 labels with the drop rule in its last launch: out uint8 [B][H][W] (any byte address) = fill
 * where labels != fill and size < min_region, labels elsewhere (regions of the value fill are never touched); weight uint8
 * [B][H][W] or NULL: set to 0 where the pixel was dropped, left as it is elsewhere; dropped uint64 [n] is ADDED to: the
 * dropped pixels per class, class = value - 1 with raw_labels != 0, else the value; values outside the classes are dropped
 * but not counted.  One 64-bit atomic per workgroup and non-zero entry.
 * Also refused with IFSEG_ERR_BAD_ARG: NULL out / dropped, dropped not 8-byte aligned, min_region < 1, fill outside 0..255,
 * n outside 1..255, out / weight / labels / the planes sharing a byte. */
int ifseg_seg_region_drop(const void* labels, int B, int H, int W, int connectivity, int min_region, int fill, int n,
                          int raw_labels, int* work, int* count, int* root, int* size, void* out, void* weight,
                          unsigned long long* dropped, int* flag, void* stream);
/* which = 0 / 1: the rows / columns of a tile, 2: the largest n of the drop; any other which: IFSEG_ERR_BAD_ARG. */
int ifseg_seg_regions_limit(int which);

/* ---- the sieve of a label map (csrc/sieve.hip; ifseg_amd/predict.py sieve_reference is the specification and states the
 * rule; the reference has no counterpart; a relative of GDAL's sieve filter) ----
 * labels [B][H][W], uint8 (label_bytes 1) or int16 (2), values compared as they are.  One pass, everything decided from the
 * pass's input map: a region of ifseg_seg_regions (connectivity 4 or 8) with the key (size, -root) is small iff size <
 * min_region and its value is not `ignore` (read only with has_ignore != 0); a small region takes the value of the region
 * with the largest key among those that hold a pixel one step in x or y from one of its pixels and do not carry `ignore`,
 * and only if that key exceeds its own.  `passes` (1 .. 8) repeats this on the previous pass's output.  Per pass:
 * ifseg_seg_regions' launches, then three of this file's on the same stream (best cleared; the votes, one 64-bit integer
 * atomic maximum each, into best[the region's root]; the map written).  The result is canonical: a maximum does not depend on
 * the order of its operands.
 * out [B][H][W] of the labels' type: the last pass's map.  tmp: the same, the other side of the passes' ping-pong, NULL
 * allowed with passes == 1.  conf fp32 [B][H][W] or NULL: set to 0 where out != labels, untouched elsewhere.  moved uint64
 * [2][n] is ADDED to: moved[0][c] the pixels that were class c in labels and are not in out, moved[1][c] those that are and
 * were not; class = value - 1 with raw_labels != 0, else the value; values outside [0, n) are not counted.  One 64-bit atomic
 * per workgroup and non-zero entry.  work / count / root / size: int32 [B][H][W], best: uint64 [B][H][W], all the caller's,
 * written in full (nothing needs zeroing); flag: ifseg_seg_regions', passed through.
 * NULL pointers (conf, and tmp with one pass, may be NULL), label_bytes outside {1, 2}, int16 maps at an odd address, a
 * plane, conf or flag not 4-byte aligned, best or moved not 8-byte aligned, any two buffers sharing a byte, connectivity
 * other than 4 or 8, min_region < 1, passes outside 1..8, n outside 1..512: IFSEG_ERR_BAD_ARG; B, H, W < 1 or B*H*W >= 2^31:
 * IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_seg_sieve(const void* labels, int label_bytes, int B, int H, int W, int connectivity, int min_region, int passes,
                    int ignore, int has_ignore, int n, int raw_labels, int* work, int* count, int* root, int* size,
                    unsigned long long* best, void* tmp, void* out, float* conf, unsigned long long* moved, int* flag,
                    void* stream);
/* which = 0 / 1: the rows / columns of a tile, 2: the passes of a call at most, 3: the largest n; any other which:
 * IFSEG_ERR_BAD_ARG. */
int ifseg_seg_sieve_limit(int which);

/* ---- the region table of a label map (csrc/regiontab.hip; ifseg_amd/predict.py region_table_reference is the specification
 * and states the rule; the reference has no counterpart) ----
 * labels [B][H][W], uint8 (label_bytes 1) or int16 (2); conf fp32 [B][H][W] or NULL.  Regions, root and size are
 * ifseg_seg_regions' (connectivity 4 or 8).  A region is listed iff size >= min_region and its value is not `ignore` (read
 * only with has_ignore != 0); the listed regions of an image are numbered 0, 1, ... in ascending order of root.
 *   nreg int32 [B]        the listed regions of each image; it may exceed R
 *   rows int32 [B][R][8]  row s < min(nreg[b], R) = (value, root, size, x0, y0, x1, y1, 0), the box inclusive
 *   sums int64 [B][R][3]  row s = (sum x, sum y, sum q) over the region's pixels, q = clamp(floor(conf * 65536), 0, 65535) in
 *                         fp32 (NaN -> 0, +inf -> 65535; q >> 8 is the confidence bin of ifseg_seg_conf_hist); 0 without conf
 *   slot int32 [B][H][W]  the row of the pixel's region, -1 where it is not listed or its number is >= R
 * Rows from min(nreg[b], R) on are NOT written.  ifseg_seg_regions' launches, then four on the same stream (the listed roots
 * counted per block of 1024 flat pixels of one image; one workgroup per image scans its blocks' counts; the rows' headers and
 * the roots' slots; per 16 x 64 tile the statistics, through a workgroup-private LDS table, as 32-bit integer min / max and
 * 64-bit integer add atomics per tile-local region).  Integers throughout: canonical, two calls give equal bits.
 * work / count / root / size: ifseg_seg_regions' planes, blk: int32 [B][ceil(H W / 1024)], all the caller's, written in full
 * (nothing needs zeroing); flag: ifseg_seg_regions', passed through.
 * NULL pointers (conf may be NULL), label_bytes outside {1, 2}, int16 labels at an odd address, a buffer not 4-byte aligned,
 * sums not 8-byte aligned, any two buffers sharing a byte, connectivity other than 4 or 8, min_region < 1, R outside
 * 1..2^20: IFSEG_ERR_BAD_ARG; B, H, W < 1 or B*H*W >= 2^31: IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_seg_region_table(const void* labels, int label_bytes, const float* conf, int B, int H, int W, int connectivity,
                           int min_region, int ignore, int has_ignore, int R, int* work, int* count, int* root, int* size,
                           int* blk, int* rows, long long* sums, int* nreg, int* slot, int* flag, void* stream);
/* which = 0 / 1: the rows / columns of a tile, 2: the flat pixels of a block, 3: the largest R; any other which:
 * IFSEG_ERR_BAD_ARG. */
int ifseg_seg_region_table_limit(int which);

/* ---- run-length label maps in COCO's run order (csrc/rle.hip; ifseg_amd/predict.py rle_encode_reference and
 * rle_decode_reference are the specifications; the reference has no counterpart) ----
 * labels [B][H][W], uint8 (label_bytes 1) or int16 (2).  Per image f[i] = labels[i % H][i / H], 0 <= i < H W: column-major, the
 * order of COCO's RLE.  Position i starts a run iff i == 0 or f[i] != f[i - 1], the values compared as they are; a run goes on
 * across a column boundary and never from one image into the next.  Runs are numbered 0, 1, ... in ascending order of start.
 *   count int32 [B]        the runs of each image; it may exceed R
 *   runs  int32 [B][R][2]  run s < min(count[b], R) = (start, value), one 8-byte store; entries behind are NOT written
 * A run's length is the next run's start (H W for the last one) minus its own.  Three launches on the stream (per 64 columns x
 * 32 rows the run starts counted per column segment; one workgroup per image scans the segments' counts; the walk again with
 * the ranks).  seg: int32 [B][W ceil(H / 32)], the caller's, written in full.  Integers, one writer per word, no atomics: two
 * calls give equal bits.
 * NULL pointers, label_bytes outside {1, 2}, int16 labels at an odd address, seg / count not 4-byte aligned, runs not 8-byte
 * aligned, any two buffers sharing a byte, R outside 1..2^24: IFSEG_ERR_BAD_ARG; B, H, W < 1 or B*H*W >= 2^31:
 * IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_seg_rle_encode(const void* labels, int label_bytes, int B, int H, int W, int R, int* seg, int* runs, int* count,
                         void* stream);
/* The way back, one launch: with m = min(count[b], R), out[b][y][x] = (uint8 or int16 by label_bytes) value[s], s the largest
 * index below m with start[s] <= x H + y (s = 0 where there is none); with m <= 0 the image is `fill`.  *flag |= 1 where
 * count[b] > R (a truncated table: the tail carries the last written run's value), |= 2 where m <= 0 or start[0] != 0; the
 * word is never cleared here.  No index into the table leaves [0, m) whatever it holds.
 * NULL pointers, label_bytes outside {1, 2}, int16 out at an odd address, count / flag not 4-byte aligned, runs not 8-byte
 * aligned, any two buffers sharing a byte, R outside 1..2^24, fill outside the output type: IFSEG_ERR_BAD_ARG; B, H, W < 1 or
 * B*H*W >= 2^31: IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_seg_rle_decode(const int* runs, const int* count, int B, int H, int W, int R, int label_bytes, int fill, void* out,
                         int* flag, void* stream);
/* which = 0: the rows of a chunk, 1: the columns of a workgroup, 2: the largest R; any other which: IFSEG_ERR_BAD_ARG. */
int ifseg_seg_rle_limit(int which);

/* ---- pixel-adaptive mask refinement (PAMR: Araslanov & Roth, CVPR 2020; Segmenter(pamr_iters=); the reference has no
 * counterpart) ----  A few iterations of a local, image-adaptive, convex averaging of the class values of ONE image at image
 * resolution, linear in the pixels; csrc/pamr.hip; ifseg_amd/predict.py pamr_reference is the specification.
 * image uint8 [H][W][3] (HWC, any byte address); dilations: D ints on the HOST, 1 <= D <= 8, each 1..32.  Neighbour
 * k = 8 i + t of pixel p is the pixel at p + dilations[i] (oy, ox), (oy, ox) = (-1,-1) (-1,0) (-1,1) (0,-1) (0,1) (1,-1) (1,0)
 * (1,1) for t = 0..7, every coordinate clamped to the image (replicate padding).
 *
 * ifseg_pamr_affinity writes w fp32 [8 D][H][W], one launch: per channel S1, S2 = the sums of x and x^2 (grey levels) over the
 * 9 taps of every dilation, the centre counted once per dilation, M = 9 D, in integers; std = sqrt((M S2 - S1^2) / (M (M - 1)))
 * (the integer numerator rounded to fp32 once, IEEE division and square root);
 *   a_k = -(sum_ch |x_ch(p) - x_ch(q_k)| / (1e-8 + 0.1 std_ch)) / 3    channels added in order, IEEE divisions
 *   w_k = exp(a_k - max a) / sum_k exp(a_k - max a)                    the accurate expf, the sum in order k = 0 .. 8 D - 1
 * ifseg_pamr_iterate is one iteration, one launch: dst[c][p] = sum_k w[k][p] src[c][q_k(p)], fused multiply-adds in order
 * k = 0 .. 8 D - 1 from 0, for src / dst fp32 [n][H][W]; dst must share no byte with src or w (refused).  labels (uint8,
 * label_bytes 1, n <= 256, or int16, 2) and conf fp32 [H][W], each may be NULL: per pixel the smallest c with maximal dst[c][p]
 * and that value (the caller asks on its last iteration; there is no argmax pass).  No atomics, no sum across threads: two
 * calls give equal bits.  A workgroup owns 16 x 64 pixels (8 x 64 for D > 2), keeps its pixels' weights in registers and
 * stages one class plane's tile plus a halo of max d in LDS at a time (40 KiB at d = 32).
 * NULL or misaligned pointers (w, src, dst, conf 4 bytes; int16 labels 2), D outside 1..8, a dilation outside 1..32, n outside
 * 1..512, label_bytes outside {1, 2} or 1 with n > 256, dst overlapping src or w: IFSEG_ERR_BAD_ARG; H, W < 1, n H W >= 2^31 or
 * 8 D H W >= 2^31: IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_pamr_affinity(const void* image, int H, int W, const int* dilations, int D, float* w, void* stream);
int ifseg_pamr_iterate(const float* w, const float* src, float* dst, int n, int H, int W, const int* dilations, int D,
                       void* labels, int label_bytes, float* conf, void* stream);
/* which = 0: the dilations of a call at most, 1: the largest dilation, 2: the largest n; any other which: IFSEG_ERR_BAD_ARG. */
int ifseg_pamr_limit(int which);

/* ---- raw images and raw label maps in, a training batch out (ifseg_amd/augment.py is the specification, bit for bit; the
 * reference's training transform, segmentation_dataset.py:157-163, 239-251: Resize(ratio_range), RandomCrop(cat_max_ratio 0.75),
 * RandomFlip, PhotoMetricDistortion, Normalize) ----
 * A batch is described by a table of B entries, once in host memory (read by the entry points for their checks) and once on
 * the device (read by the kernels; the caller copies it on the stream of the call). */
typedef struct {
  const void* image; /* device, uint8 [H0, W0, 3] RGB, contiguous, any byte alignment (unused by ifseg_train_draw) */
  const void* label; /* device, uint8 [H0, W0], contiguous */
  int H0, W0;
} ifseg_train_src;
/* ifseg_train_draw writes the records int32 [B, 16] of the samples at ordinals first_ordinal + b from
 * t(n, i) = splitmix64(seed + (n << 32) + i) >> 32 (slots and layout: the docstring of ifseg_amd/augment.py):
 *   0 new_h  1 new_w  2 off_h  3 off_w  4 k  5 flip  6 brightness on  7 contrast on  8 saturation on  9 hue on  10 mode
 *   11 beta  12 alpha_c  13 alpha_s (fp32 bit patterns)  14 delta  15 zero
 * new_short = max(P, (P (ratio_lo2 2^32 + ratio_span2 t)) >> 33); the crop is the first of candidates 0..9 whose P x P window
 * of the remapped (raw_labels != 0: raw 0 and 255 -> nseg, x -> x - 1), nearest-resized label map has 4 max(count) < 3 P^2,
 * else candidate 10.  enable: bit 0 flips, bit 1 the photometric stage (a cleared bit leaves the on-bits zero).
 * One memset node and one launch of 10 B workgroups; integer counts only, so the result does not depend on arrival order.
 * NULL or misaligned pointers, nseg outside 1..255, a ratio outside 0 <= lo2, span2, lo2 + span2 <= 64, ordinals outside
 * [0, 2^32): IFSEG_ERR_BAD_ARG.  B outside 1..65535, P not a multiple of 16 in 16..4096, H0 or W0 < 1, H0*W0*3 >= 2^31, or
 * 2 in out >= 2^31 on an axis at the largest size the ratio can draw: IFSEG_ERR_BAD_SHAPE. */
int ifseg_train_draw(const ifseg_train_src* table_host, const ifseg_train_src* table, int B, int P, int nseg, int raw_labels,
                     unsigned long long seed, long long first_ordinal, int ratio_lo2, int ratio_span2, int enable, int* params,
                     void* stream);
/* ifseg_train_load: records (device) -> out [B, 3, P, P] (out_bytes 4 -> fp32, 2 -> bf16) and target int64 [B, P*P + 1]
 * (seg_id_offset + class, then eos), one launch.  Window pixel (y, x) is pixel (off_h + y, off_w + xs) of the source resized
 * to new_h x new_w, xs = x or P - 1 - x under flip: the image by ifseg_image_load's rule (integer source coordinates, the
 * four-weight sum in fp32, q = clamp(floor(v + 0.5), 0, 255)), the label by src = min(dst in / out, in - 1).  The grey levels go
 * through the photometric chain (brightness; contrast if mode 1; saturation; hue; contrast if mode 0; convert() as a single
 * fp32 operation, HSV in exact integers) and then lut fp32 [3][256]; reverse_channels reverses the order of the output planes.
 * params_host (may be NULL): the same records in host memory, when the caller has them -- then a record with new_h or new_w
 * < P, an offset outside the resized image or 2 in out >= 2^31 is refused with IFSEG_ERR_BAD_SHAPE and nothing is launched.
 * Without it such a record poisons its sample on the device (NaN images, target -1) and reads nothing through it.
 * The staging loads are aligned dwords, as in ifseg_image_load; ifseg_train_load_staging is the same switch.
 * NULL / misaligned pointers (out 16 bytes, target 8), out_bytes, nseg: IFSEG_ERR_BAD_ARG; B < 1, P not a multiple of 16 in
 * 16..4096, B*3*P*P >= 2^31, a bad table entry: IFSEG_ERR_BAD_SHAPE. */
int ifseg_train_load(const ifseg_train_src* table_host, const ifseg_train_src* table, const int* params, const int* params_host,
                     int B, int P, int nseg, int raw_labels, long long seg_id_offset, long long eos, const float* lut,
                     int reverse_channels, void* out, int out_bytes, long long* target, void* stream);
int ifseg_train_load_staging(int max_bytes);
/* ifseg_train_load_plane: uint8 planes [H0, W0] of any sizes, given through the `label` pointers of the table (`image` is not
 * read), under the same records -> out uint8 [B, P*P]: ifseg_train_load's label tap (src = min(dst in / out, in - 1), the
 * window at the record's offset, mirrored under flip) on the plane's bytes, nothing remapped -- per-pixel loss weights that
 * follow their label map.  One launch, one 16 x 64 tile per workgroup, byte stores; any 1 <= P <= 4096.  params_host as in
 * ifseg_train_load; without it a bad record writes 0 for its sample.  Refusals as ifseg_train_load's. */
int ifseg_train_load_plane(const ifseg_train_src* table_host, const ifseg_train_src* table, const int* params,
                           const int* params_host, int B, int P, void* out, void* stream);

/* ---- ClassMix / CutMix of a labelled (source) batch into a pseudo-labelled (destination) batch, both in ifseg_train_load's
 * layout and of one B and P (ifseg_amd/augment.py, "the batch mix", is the specification, bit for bit; csrc/mix.hip; the
 * reference has no counterpart: DACS / ClassMix choose with torch.unique and numpy on the host) ----
 * The class of a source pixel is c = target - seg_id_offset in 64 bits, a class only if 0 <= c < nseg.
 * ifseg_mix_draw writes the records int32 [B, 16] of the samples at ordinals first_ordinal + b, from the transform's stream
 * t(n, i) = splitmix64(seed + (n << 32) + i) >> 32 on the slots behind the transform's 28:
 *   0..7 chosen-class bits (class c is bit c & 31 of word c >> 5)   8 y0  9 x0  10 y1  11 x1 (exclusive)   12 n present
 *   13 m chosen   14, 15 zero
 * box == 0 (ClassMix): c_0 < .. < c_{n-1} the classes present in src_target[b] (int64 [B, P*P + 1], the last entry of a row is
 * not read), m = (n + 1) / 2; for i = 0 .. m-1: j = i + ((t(32 + i) (n - i)) >> 32), swap c_i and c_j; chosen c_0 .. c_{m-1};
 * words 8..11 zero.  box == 1 (CutMix): bh, bw = P/4 + ((t28|t29 (P/2 + 1)) >> 32), y0 = (t30 (P - bh + 1)) >> 32,
 * x0 = (t31 (P - bw + 1)) >> 32, y1 = y0 + bh, x1 = x0 + bw; words 0..7, 12, 13 zero and src_target is not read.
 * One launch of B workgroups, no scratch, nothing read back.  NULL or misaligned pointers (target 8 bytes, records 4), nseg
 * outside 1..255, box outside {0, 1}, ordinals outside [0, 2^32): IFSEG_ERR_BAD_ARG; B outside 1..65535, P not a multiple of
 * 16 in 16..4096: IFSEG_ERR_BAD_SHAPE. */
int ifseg_mix_draw(const long long* src_target, int B, int P, int nseg, long long seg_id_offset, unsigned long long seed,
                   long long first_ordinal, int box, int* records, void* stream);
/* ifseg_mix_apply pastes, one launch: pixel (y, x) of sample b is selected if its source class's bit is set in the record or
 * y0 <= y < y1 and x0 <= x < x1 (the union; a box outside the image selects less, bits at or above nseg are not consulted).
 * Selected pixels take the source's three image values (elem_bytes 4: fp32, 2: bf16; copied as bits), target and weight,
 * the others the destination's; out_target[b][P*P] is the destination's.  A NULL weight plane reads as 255; out_weight is
 * NULL exactly when both planes are.  An output may be the destination tensor it replaces, the same pointer; any other
 * shared byte between an output and an input, the records or another output: IFSEG_ERR_BAD_ARG.  NULL / misaligned pointers
 * (images 16 bytes, targets and weights 8, records 4), elem_bytes, nseg outside 1..255: IFSEG_ERR_BAD_ARG; B outside
 * 1..65535, P not a multiple of 16 in 16..4096, B*3*P*P >= 2^31: IFSEG_ERR_BAD_SHAPE.  Nothing is launched on a refusal. */
int ifseg_mix_apply(const int* records, const void* src_images, const long long* src_target, const void* src_weight,
                    const void* dst_images, const long long* dst_target, const void* dst_weight, int B, int P, int nseg,
                    long long seg_id_offset, int elem_bytes, void* out_images, long long* out_target, void* out_weight,
                    void* stream);

/* ---- The strong augmentation of a mixed batch: colour jitter, then Gaussian blur, on images [B, 3, P, P] (fp32 or bf16) in
 * ifseg_train_load's layout (ifseg_amd/augment.py, "the strong augmentation", is the specification, bit for bit;
 * csrc/strong.hip; DACS' strong_transform behind the mix) ----
 * The record of a sample, int32 [16]:
 *   0 brightness on  1 contrast on  2 saturation on  3 hue on  4 mode  5 beta  6 alpha_c  7 alpha_s (fp32 bit patterns)
 *   8 delta  9 sigma index (-1: blur off)  10..14 blur weights w0..w4, w0 + 2 (w1 + w2 + w3 + w4) = 4096  15 zero
 * ifseg_strong_blur_table copies the 64 x 5 weight table (sigma = 0.15 + s / 64) to HOST memory out[320]; no device is
 * touched.  NULL: IFSEG_ERR_BAD_ARG. */
int ifseg_strong_blur_table(int* out);
/* ifseg_strong_draw writes the records of the samples at ordinals first_ordinal + b from the transform's stream
 * t(n, i) = splitmix64(seed + (n << 32) + i) >> 32 on slots 192..199: jitter gate (t192 >> 24) < jitter_p8, bits of t193 in
 * slot 23's positions (the four "on" bits ANDed with the gate), beta / alpha_c / alpha_s / delta from t194..t197 by the
 * formulas of slots 24..27, blur gate (t198 >> 24) < blur_p8, sigma index t199 >> 26.  One launch, one thread per sample.
 * NULL or misaligned records (4 bytes), a gate outside 0..256, ordinals outside [0, 2^32): IFSEG_ERR_BAD_ARG; B < 1:
 * IFSEG_ERR_BAD_SHAPE. */
int ifseg_strong_draw(int B, unsigned long long seed, long long first_ordinal, int jitter_p8, int blur_p8, int* records,
                      void* stream);
/* ifseg_strong_apply, one launch: per pixel the grey level q = #{k in 1..255 : x >= (lut[c][k-1] + lut[c][k]) / 2} of each
 * plane (plane c is colour 2 - c under reverse_channels), the photometric chain of ifseg_train_load under the record, the
 * separable 9-tap blur with the record's weights on a border reflected without repeating the edge,
 * q'' = (v + 2^23) >> 24, and out = lut[c][q''] in the images' type (elem_bytes 4: fp32, 2: bf16).  lut: fp32 [3, 256] on
 * the device, increasing per row.  A record is valid iff words 0..4 are 0 or 1, the three floats are finite, every weight is
 * >= 0 and they sum to 4096 as above; delta is reduced mod 180; an invalid record writes NaN for its sample.  No address
 * depends on a record.  NULL or misaligned pointers (images and out 16 bytes, records and lut 4), elem_bytes, or any byte
 * shared between out and images, the records or lut (the blur reads neighbours: there is no in-place form):
 * IFSEG_ERR_BAD_ARG; B < 1, P not a multiple of 16 in 16..4096, B*3*P*P >= 2^31: IFSEG_ERR_BAD_SHAPE.  Nothing is launched on
 * a refusal. */
int ifseg_strong_apply(const int* records, const void* images, int B, int P, int elem_bytes, const float* lut,
                       int reverse_channels, void* out, void* stream);

/* sum of squares of a bf16 gradient arena -> out_sumsq[0] (device).  workspace: 1024 floats.  g is read 16 bytes at a time:
 * NULL g / workspace / out_sumsq, g not 16-byte aligned, workspace or out_sumsq not 4-byte aligned, n < 0: IFSEG_ERR_BAD_ARG,
 * nothing launched.  n == 0 writes 0. */
int ifseg_grad_sumsq_bf16(const void* g, long long n, float* workspace, float* out_sumsq, void* stream);
/* Fused grad scaling + clip-by-global-norm + Adam with decoupled weight decay over a
 * flat arena; writes the bf16 model copy.  Mirrors trainer.py:874-907 +
 * fairseq/optim/adam.py:158-240 + fp16_optimizer.py (fp32 masters).  A non-finite *sumsq skips the whole update and
 * sets overflow[0] = 1 (device int, may be NULL): trainer.py:895-904 raises FloatingPointError there. */
int ifseg_adam_step(float* p32, const void* g, float* m, float* v, void* p16, long long n, float lr, float beta1,
                    float beta2, float eps, float weight_decay, int step, float grad_scale, float max_norm,
                    const float* sumsq, int* overflow, const float* hyper, void* stream);
/* `hyper` (device, may be NULL): {lr, 1 - beta1^step, 1 - beta2^step, grad_scale} override the by-value arguments --
 * a captured training step (HIP graph) is replayed with the schedule's current values.
 * n <= 0 returns 0 and launches nothing.  With n > 0 (here and in ifseg_adam_ema_step): p32, m, v are read and written 16 bytes
 * at a time, g and p16 8 bytes at a time -- a NULL p32 / g / m / v / p16, p32 / m / v not 16-byte aligned, g / p16 not 8-byte
 * aligned: IFSEG_ERR_BAD_ARG, nothing launched. */
/* ifseg_adam_step with a teacher averaged in the same launch (fairseq/models/ema/ema.py:134-167 with ema_fp32 on a 16-bit
 * model; ifseg_amd/ema.py is the specification).  Per element, with q the bf16 weight this launch stores to p16:
 *     e32 = fma(ema_rest, float(q), round32(e32 * ema_decay))        e16 = bf16_rne(e32)
 * -- a rounded product and ONE fused multiply-add, which is what `ema.mul_(decay); ema.add_(p.float(), alpha=1 - decay)`
 * computes; ema_rest = float(1.0 - decay) is formed by the caller in double.  (p32, m, v, p16) come out bit-equal to
 * ifseg_adam_step.  `hyper` (device, may be NULL) has SIX floats here: the four above, then {ema_decay, ema_rest}.
 * (ema_decay, ema_rest) == (1, 0) neither reads nor writes the teacher (the off-updates of ema_update_freq in a captured
 * step); a non-finite *sumsq skips the teacher with the update.  e32 / e16: n elements, aligned like p32 / p16 (16 / 8
 * bytes); NULL or misaligned: IFSEG_ERR_BAD_ARG.  40 bytes of traffic per element against ifseg_adam_step's 30. */
int ifseg_adam_ema_step(float* p32, const void* g, float* m, float* v, void* p16, float* e32, void* e16, long long n,
                        float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale,
                        float max_norm, const float* sumsq, int* overflow, const float* hyper, float ema_decay,
                        float ema_rest, void* stream);
/* p32 <-> e32 (fp32) and p16 <-> e16 (bf16), n elements each, in place and without a temporary: student and teacher change
 * places (fairseq's EMA.reverse without a second model).  The two sides must not overlap (the binding checks); a NULL
 * pointer: IFSEG_ERR_BAD_ARG.  24 bytes of traffic per element. */
int ifseg_ema_swap(float* p32, void* p16, float* e32, void* e16, long long n, void* stream);

/* ------------------------------------------------- dense-CRF post-processing (crf.py:19-37) */
/* Mean-field inference of the reference's DenseCRF2D (pydensecrf, third party, absent: parity unpinned) with the EXACT
 * dense kernels instead of the permutohedral-lattice approximation.  All tensors class-major ([C][N], N = H*W pixels).
 * ifseg_crf_bilateral: out[c][i] = sum_j gx[|xi-xj|] gy[|yi-yj|] exp2(-|f_i - f_j|^2) qn[c][j]; feat4 [N][4] fp32 =
 *   (pre-scaled r, g, b, bit pattern x | y << 16), qn bf16 [Cp][ldq] (Cp % 32 == 0, ldq % 64 == 0, zero padded), out fp32
 *   [Cp][N].  ifseg_crf_spatial: the sxy = 1 Gaussian as a (2R+1)^2 stencil on fp32 [C][N].
 * ifseg_crf_update: Q = softmax_c(log clip(prob, 1e-5, 1) + wpos npos mpos + wbi nbi mbi) -> Q, qpos = npos Q (fp32),
 *   qbi = nbi Q (bf16 [Cp][ldq]); mpos / mbi / npos / nbi may be NULL.  ifseg_crf_norm: n = rsqrt(k1 + 1e-20). */
int ifseg_crf_bilateral(const float* feat4, const float* gx, const float* gy, const void* qn, int ldq, float* out, int Cp,
                        int H, int W, void* stream);
int ifseg_crf_spatial(const float* qn, const float* g, int R, float* out, int C, int H, int W, void* stream);
int ifseg_crf_update(const float* prob, const float* mpos, const float* mbi, const float* npos, const float* nbi, float wpos,
                     float wbi, float* Q, float* qpos, void* qbi, int ldq, int C, int N, void* stream);
int ifseg_crf_norm(const float* k1, float* n, int N, void* stream);

/* -------------------------------------------------------------- profiling */
/* Per-kernel-family timing with HIP events recorded on the launch stream (bench.py's
 * roofline object).  kinds: 0 GEMM_NT, 1 GEMM_NN, 2 GEMM_TN, 3 CONV, 4 ATTN_FWD,
 * 5 ATTN_BWD_DKV, 6 ATTN_BWD_DQ, 7 LN_FWD, 8 LN_BWD.  ifseg_prof_read returns the summed
 * kernel time and the summed ALGORITHMIC flops / bytes of the recorded launches. */
int ifseg_prof_enable(unsigned mask);
int ifseg_prof_stride(int stride); /* time only every stride-th launch of an enabled family (default 1) */
int ifseg_prof_reset(void);
int ifseg_prof_read(int kind, double* ms, double* flops, double* bytes, int* launches);

#ifdef __cplusplus
}
#endif
#endif /* IFSEG_HIP_H */
