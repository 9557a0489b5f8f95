/* m3vit_hip.h - C ABI of libm3vit_hip.so: the MI355X (gfx950) implementation of the
 * M3ViT MoE-ViT forward/backward hot path.
 *
 * This is the drop-in boundary described in SURVEY.md section 8(b).  The reference
 * reaches this path through the python package `fmoe` (laekov/fastmoe, absent from
 * /root/reference) whose native half is the `fmoe_cuda` extension; the entry points
 * below are what a binding for that layer would call.  Each one cites the reference
 * call site (path:line relative to the reference root) whose work it replaces.
 *
 * Conventions
 *   - plain C, no torch types: device pointers, sizes, an opaque hipStream_t (void*).
 *   - every call is asynchronous on `stream`, allocates nothing, takes no locks and
 *     never synchronises the device; the caller owns all buffers and workspaces.
 *   - return value: 0 = ok, negative = M3_ERR_* ; m3_last_error() gives the text of
 *     the last failure on the calling thread.  Shape/alignment violations are
 *     rejected on the host before anything is launched.
 *   - dtype codes (M3_F32, M3_F16, M3_BF16) describe ACTIVATION storage; accumulation is
 *     always fp32; parameters/gradients of parameters are fp32.
 *   - indices are int32 on the device-internal path and int64 where the reference
 *     API exposes them (gate_top_k_idx from torch.topk).
 */
#ifndef M3VIT_HIP_H
#define M3VIT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3_F32 0
#define M3_F16 1
#define M3_BF16 2            /* every entry point */

#define M3_OK 0
#define M3_ERR_ARG (-1)      /* bad shape / alignment / null pointer */
#define M3_ERR_LAUNCH (-2)   /* hipLaunch failed (text in m3_last_error) */
#define M3_ERR_UNSUPPORTED (-3)

#define M3_ACT_NONE 0
#define M3_ACT_GELU 1        /* exact erf GELU, nn.GELU(): vision_transformer_moe.py:409-412 */

int m3_version(void);
const char *m3_last_error(void);
/* fills name[0..len) with the gcnArchName of the current device; returns CU count or <0 */
int m3_device_query(char *name, int len);
/* Tuning knob, no reference counterpart: cache policy by tensor lifetime.  One bit per kernel family; a family whose bit is
 * set launches the instance of its kernel whose loads of a tensor that is dead for the rest of the pass, and whose stores
 * of a tensor that is next read a whole backward later, carry the non-temporal hint.  Tensors that the next kernels read
 * (hand-offs) are never hinted.  The hint moves no arithmetic: every result is bit-identical under every mask.
 *   M3_HINT_GEMM_PRE   m3_gemm_nt, GELU kind of the LDS-DMA kernel: the store of pre_out
 *   M3_HINT_GEMM_GPRE  m3_gemm_nt, GPRE kind of the LDS-DMA kernel: the load of gelu_grad_pre
 * mask: an OR of the bits, or -1 = re-read M3_CACHE_HINTS (unset: M3_HINT_DEFAULT, the families that measured faster in the
 * training step).  Takes effect with the next launch; a captured graph keeps the instances it was captured with. */
#define M3_HINT_GEMM_PRE 1
#define M3_HINT_GEMM_GPRE 2
#define M3_HINT_ALL 3
#define M3_HINT_DEFAULT 3
int m3_set_cache_hints(int mask);

/* ---------------------------------------------------------------- gate (a1-a3)
 * NoisyGate_VMoE.forward, models/moe/ckpt/noisy_gate_vmoe.py:91-93,168,197-207:
 *   logit = x @ w_gate (+ logit_bias) ; noisy = logit + noise*noise_std ;
 *   p = softmax(noisy) ; top-(k+1) ; score/idx = first k (not renormalised).
 * x [T,D] (x_dtype, row stride ldx elements), w_gate [D,E] fp32 row-major,
 * logit_bias [E] fp32 or NULL (task-conditioned term tsf @ w_gate[D:], the
 * cat at custom_moe_layer.py:176-179 folded into a bias), noise [T,E] fp32 or NULL.
 * Outputs: idx i64 [T,k], score f32 [T,k], top_logits f32 [T,min(k+1,E)];
 * optional dense clean/noisy/gates f32 [T,E] (NULL to skip), optional
 * idx32 i32 [T,k] copy for the routing kernels.
 * part_importance f32 [nblk,E], part_load i32 [nblk,E] with nblk =
 * m3_gate_num_blocks(T): per-block partial sums of gates.sum(0) and (gates>0).sum(0)
 * (vision_transformer_moe.py:453-459), reduced in fixed order by m3_gate_reduce /
 * m3_balance_loss.
 * E in {2..64}, k < = 8, k <= E. */
int m3_gate_num_blocks(int64_t T);
int m3_gate_dw_blocks(int64_t T);
typedef struct m3_gate_fwd_args {
  const void *x; int32_t x_dtype; int64_t T; int32_t D; int64_t ldx;
  const float *w_gate; int32_t E;
  const float *logit_bias;          /* [E] or NULL */
  const float *noise;               /* [T,E] N(0,1) draws or NULL (randn_like at noisy_gate_vmoe.py:168) */
  float noise_std;                  /* noise_std / E_tot * training, :92-93 */
  int32_t k;
  int64_t *idx; int32_t *idx32;     /* [T,k]; idx32 optional */
  int32_t *idx_next;                /* [T] index of the (k+1)-th expert (top_idx[:, k], :198-200) or NULL */
  float *score; float *top_logits;  /* [T,k], [T,min(k+1,E)] */
  float *clean; float *noisy; float *gates;   /* dense [T,E] or NULL */
  float *part_importance; int32_t *part_load; /* [nblk,E] */
  float *part_load_prob;            /* [nblk,E] or NULL: partial sums of _prob_in_top_k
                                       (vision_transformer_moe.py:33-71), the load of noisy training
                                       (:456-457; needs noise, noise_std != 0, k < E, clean and noisy) */
  int32_t *part_count;              /* [nblk,E] or NULL: tokens of each 64-token block whose top-k holds expert e - the
                                       routing histogram m3_route_build would count from idx (m3_balance_route scans it) */
} m3_gate_fwd_args;
int m3_gate_fwd(const m3_gate_fwd_args *args, void *stream);
/* importance f32 [E], load i64 [E] from the per-block partials */
int m3_gate_reduce(const float *part_importance, const int32_t *part_load, int nblk, int E,
                   float *importance, int64_t *load, void *stream);
/* Block-level balance loss, vision_transformer_moe.py:453-459,540 with cv_squared :73-87 and
 * _gates_to_load :23-31: reduces the partials (fixed order) to importance f32 [E], load i64 [E]
 * (count form) and, when part_load_prob is given, load_prob f32 [E] (Normal-CDF form, which then
 * replaces the count in the loss); loss = cv^2(importance) + cv^2(load) is written to loss_out and
 * added to loss_acc (either may be NULL); d_importance / d_load_prob [E] receive d loss / d(.)
 * (NULL to skip; the count form of load carries no gradient). */
int m3_balance_loss(const float *part_importance, const int32_t *part_load, const float *part_load_prob,
                    int nblk, int E, float *importance, int64_t *load, float *load_prob,
                    float *loss_out, float *loss_acc, float *d_importance, float *d_load_prob, void *stream);
/* Backward of the gate -> d_logits f32 [T,E] through the scatter (:206-207), the softmax (:197)
 * and, for noisy training, the Normal-CDF load term.  Upstream gradients (each may be NULL):
 * d_score [T,k] (from the combine), d_top [T,min(k+1,E)] (w.r.t. top_logits), d_importance [E] and
 * d_load_prob [E] (from m3_balance_loss; both multiplied by balance_scale = the loss weight).
 * probs are recomputed from `noisy` [T,E]; clean / top_logits / idx_next / noise_std are only read
 * for d_load_prob (and idx_next for d_top).  balance_scale_dev (may be NULL): one device-resident float that multiplies
 * balance_scale - the upstream gradient of cv_loss when the caller is torch.autograd (the reference forms
 * cv_loss * moe_noisy_gate_loss_weight, train/train_utils.py:277, and autograd hands the weight back as a tensor); read
 * by the kernel, so a captured launch follows its value. */
typedef struct m3_gate_bwd_args {
  const float *noisy; const float *clean; const float *top_logits;
  const int64_t *idx; const int32_t *idx_next;
  const float *d_score; const float *d_top; const float *d_importance; const float *d_load_prob;
  float balance_scale; float noise_std;
  int64_t T; int32_t E; int32_t k;
  float *d_logits;
  const float *balance_scale_dev;
  void *d_logits_act; int32_t act_dtype;   /* optional second copy of d_logits in M3_F16 / M3_BF16 / M3_F32 (NULL: none) */
} m3_gate_bwd_args;
int m3_gate_bwd_logits(const m3_gate_bwd_args *args, void *stream);
/* m3_balance_loss and the scan pass of m3_route_build in ONE launch (two workgroups): the dispatch metadata of
 * custom_moe_layer.py:263-265 straight from the gate kernel's per-block counts, two launches less on every MoE layer's
 * critical path.  part_count i32 [nblk,E] from m3_gate_fwd; outputs blk_base i32 [nblk,E] (exclusive prefix along the
 * blocks, for m3_route_assign), counts i32 [E], offsets / tile_starts i32 [E+1], counts64 i64 [E] or NULL - as
 * m3_route_build writes them. */
int m3_balance_route(const float *part_importance, const int32_t *part_load, const float *part_load_prob,
                     int nblk, int E, float *importance, int64_t *load, float *load_prob,
                     float *loss_out, float *loss_acc, float *d_importance, float *d_load_prob,
                     const int32_t *part_count, int32_t *blk_base, int32_t *counts, int32_t *offsets,
                     int32_t *tile_starts, int64_t *counts64, void *stream);
/* d_w_gate[D,E] (+)= x^T d_logits ; dx[T,D] (+)= d_logits w_gate^T  (noisy_gate_vmoe.py:91).
 * part_dw f32 [m3_gate_dw_blocks(T), D, E] workspace; dx fp32 accumulate (beta_dx 0/1). */
int m3_gate_bwd_params(const void *x, int x_dtype, int64_t T, int D, int64_t ldx,
                       const float *w_gate, int E, const float *d_logits,
                       float *part_dw, float *d_w_gate, int beta_dw,
                       float *dx, int64_t lddx, int beta_dx, void *stream);

/* ------------------------------------------------------- dispatch metadata (a5)
 * What fastmoe's prepare_forward (count_by_gate + assign_pos) computes behind
 * _fmoe_general_global_forward, models/moe/ckpt/custom_moe_layer.py:263-265, with a
 * stable slot order.  idx32 [n] flat (n = T*k) expert ids in [0,E).
 * Outputs (all device): counts i32 [E], offsets i32 [E+1], pos i32 [n] (slot of flat
 * entry i), row_of_slot i32 [n] (inverse), tile_starts i32 [E+1] (prefix of
 * ceil(count/128) m-tiles per expert, read by the grouped GEMMs),
 * counts64 i64 [E] (optional, fwd_expert_count as the reference API exposes it).
 * ws i32 [m3_route_ws_elems(n,E)] scratch. */
int64_t m3_route_ws_elems(int64_t n, int E);
int m3_route_build(const int32_t *idx32, int64_t n, int E, int32_t *counts, int32_t *offsets,
                   int32_t *pos, int32_t *row_of_slot, int32_t *tile_starts, int64_t *counts64,
                   int32_t *ws, void *stream);

/* The slot pass of m3_route_build on its own: stable slots pos / row_of_slot i32 [n] of the n = T*k entries of idx32 from
 * the per-64-token-block prefixes blk_base and the expert offsets that m3_balance_route wrote.  k must divide 16. */
int m3_route_assign(const int32_t *idx32, int64_t n, int E, int k, const int32_t *blk_base, const int32_t *offsets,
                    int32_t *pos, int32_t *row_of_slot, void *stream);

/* Expert-parallel exchange plan, on the device (what fastmoe's expert_exchange / global_scatter bookkeeping computes
 * on the host behind _fmoe_general_global_forward with world_size > 1, models/moe/ckpt/custom_moe_layer.py:263-265;
 * experts sharded E_loc per rank, utils/common_config.py:179-185).
 * send_counts i64 [W*E_loc]: this rank's route_build counts by GLOBAL expert id (entry d*E_loc+e goes to local expert e
 * of rank d); recv_counts i64 [W*E_loc]: their all-to-all (entry s*E_loc+e = rows rank s sends to my expert e).
 * Outputs: splits i64 [2W] = rows sent to each rank, then rows received from each rank (the a2a-v sizes: the ONLY
 * values the host reads); regroup i32 [regroup_cap >= rows received]: received rows arrive ordered (src, e), the
 * grouped GEMMs take slot i of the (e, src) order from row regroup[i] (as a_row_idx / c_row_idx); offsets,
 * tile_starts i32 [E_loc+1] as m3_route_build writes them.  W * E_loc <= 4096. */
int m3_ep_plan(const int64_t *send_counts, const int64_t *recv_counts, int W, int E_loc, int64_t *splits,
               int32_t *regroup, int64_t regroup_cap, int32_t *offsets, int32_t *tile_starts, void *stream);
/* The same plan for an exchange with a FIXED row capacity per (source, destination) pair (same reference call site): every
 * pair exchanges exactly `cap` rows, the valid ones first, so the all-to-all has equal splits, the host reads nothing and a
 * step with sharded experts can be captured into a hipGraph.  row_of_slot / pos i32 [n_rows]: this rank's m3_route_build
 * output.  Outputs: regroup i32 [W*cap] (indices into the padded received buffer [W*cap, D]; the first offsets[E_loc]
 * entries are valid), offsets / tile_starts i32 [E_loc+1], pad_idx i32 [W*cap] (token-major entry whose row goes to
 * position q of the padded send buffer: gather with m3_gather_rows(div = k)), unpad_idx i32 [n_rows] (position of entry
 * i's expert output in the returned padded buffer), splits i64 [2W] (true row counts, informational), *overflow i32 set to
 * 1 (never cleared) when some pair routes more than cap rows: such a pair keeps its first cap rows on both sides, the
 * results are incomplete and the caller repeats the step with m3_ep_plan.  W <= 64, W * E_loc <= 4096. */
int m3_ep_plan_fixed(const int64_t *send_counts, const int64_t *recv_counts, int W, int E_loc, int cap,
                     const int32_t *row_of_slot, const int32_t *pos, int64_t n_rows, int64_t *splits,
                     int32_t *regroup, int32_t *offsets, int32_t *tile_starts, int32_t *pad_idx,
                     int32_t *unpad_idx, int32_t *overflow, void *stream);

/* The exchange itself over RCCL (xGMI), for a caller that does not go through torch.distributed: what fastmoe's
 * expert_exchange / global_scatter / global_gather do behind _fmoe_general_global_forward (custom_moe_layer.py:263-265,
 * world_size > 1; experts sharded per utils/common_config.py:179-185).  The only state the library keeps: communicators.
 *   m3_ep_unique_id        rank 0: 128 bytes (ncclUniqueId) to hand to every rank out of band (e.g. a broadcast over gloo)
 *   m3_ep_init             collective over the `world` ranks -> *handle; one communicator per expert-parallel group
 *   m3_ep_exchange_counts  all-to-all of e_loc int64 counts per peer (device buffers [world * e_loc], layout as m3_ep_plan takes)
 *   m3_ep_dispatch         all-to-all-v of rows (row_bytes each): peer p gets in_splits[p] consecutive rows of send_rows and
 *                          delivers out_splits[p] rows into recv_rows, in rank order; the split arrays are HOST arrays of
 *                          `world` row counts - what m3_ep_plan returned in `splits`.  One grouped set of ncclSend / ncclRecv
 *                          pairs on the caller's stream: a distinct peer per xGMI link, nothing chunked into ring steps
 *   m3_ep_return           the way home: the same exchange with the two split vectors swapped
 *   m3_ep_destroy          frees the communicator
 * librccl is opened at the first m3_ep_unique_id / m3_ep_init call (dlopen): the library has no link-time dependency on it.
 * Asynchronous on `stream` like every other entry point; errors of the collective library come back as M3_ERR_LAUNCH with
 * its text in m3_last_error().  (The engine's default exchange is torch.distributed, backend nccl = RCCL, which the two-rank
 * gloo rehearsals can test; BackboneEngine(ep_native=True) routes the row exchanges through these entry points instead.) */
int m3_ep_unique_id(void *out128);
int m3_ep_init(const void *unique_id128, int rank, int world, int *handle);
int m3_ep_destroy(int handle);
int m3_ep_exchange_counts(int handle, const int64_t *send_counts, int64_t *recv_counts, int e_loc, void *stream);
int m3_ep_dispatch(int handle, const void *send_rows, const int64_t *in_splits, void *recv_rows, const int64_t *out_splits,
                   int64_t row_bytes, void *stream);
int m3_ep_return(int handle, const void *send_rows, const int64_t *out_splits, void *recv_rows, const int64_t *in_splits,
                 int64_t row_bytes, void *stream);

/* -------------------------------------------------- GEMM family (a6, a8, a10)
 * C[m, n] = epilogue( sum_k A[arow(m), k] * B[g(m)][n, k] )      ("NT": both K-contiguous)
 *   FMoELinear fwd/dgrad: custom_moe_layer.py:32-33,41,43; qkv/proj Linear:
 *   vision_transformer_moe.py:295,297,303,311; Mlp fc1/fc2 :255-261; PatchEmbed :330-341.
 * Dense call: G = 1, group_offsets = tile_starts = NULL, rows 0..M-1.
 * Grouped call: rows are expert-major slots, group g owns rows
 *   [group_offsets[g], group_offsets[g+1]); tile_starts as produced by m3_route_build;
 *   M = upper bound on rows (T*k); B group stride = N*ldb elements.
 * a_row_idx (i32, optional): source row of A for slot m is a_row_idx[m] / a_row_div
 *   (gather fused into the operand load: MOEScatter).  c_row_idx (optional): destination
 *   row of C for slot m (MOEGather back to token-major).
 * Epilogue, in this order: + bias[g][n] (fp32) ; store pre-activation to pre_out (act
 * dtype) if non-NULL ; act (GELU) ; * gelu'(gelu_grad_pre[m,n]) if non-NULL ;
 * * row_scale[srow(m) / row_scale_div] (fp32) if non-NULL, srow(m) = row_scale_idx[m] when that is given, else crow(m)
 * - the per-sample DropPath factor of the residual branch the GEMM closes, vision_transformer_moe.py:167-185,441,450,
 * or (row_scale_idx = the slot -> routed-entry map, div 1) the gate score of a routed row: the backward of the combine
 * bmm(gate_score, moe_outp), custom_moe_layer.py:298-305, is d moe_outp[t*k+j] = score[t,j] * d out[t], a row scaling
 * that commutes with the expert GEMM behind it, so the scaled copy [T*k, D] is never materialised ;
 * + residual[m,n] (fp32) if non-NULL ; store as c_dtype (M3_F32 or the act dtype).
 * Requirements: K*sizeof(elem) % 16 == 0, lda/ldb rows 16-byte aligned, N % 4 == 0.
 * Reach: the kernels add a 32-bit byte offset per lane to the base of A and of a group's weight, so
 * (M + 1) * lda * sizeof(elem) < 4 GiB, N * ldb * sizeof(elem) < 4 GiB (one group; the group stride N*ldb*g is 64-bit) and
 * M < 2^31; a call outside any of these is refused (M3_ERR_ARG, m3_gemm_plan alike).  The A rule is measured with the M rows
 * of the call: with a_row_idx every source row a_row_idx[m] / a_row_div must lie below M - nothing checks the indices, a
 * larger one reads outside the offsets the rule covers.  C, pre_out, gelu_grad_pre and residual are addressed with 64 bits
 * (destination row * leading dimension): no limit on ldc, ld_pre, ld_gpre, ld_res or on c_row_idx beyond the buffer itself. */
typedef struct {
  const void *A; int64_t lda;
  const int32_t *a_row_idx; int32_t a_row_div;
  const void *B; int64_t ldb;
  void *C; int64_t ldc; int32_t c_dtype;
  const int32_t *c_row_idx;
  const float *bias;               /* [G][N] or NULL */
  void *pre_out; int64_t ld_pre;   /* act dtype, or NULL */
  const void *gelu_grad_pre; int64_t ld_gpre;
  const float *residual; int64_t ld_res;
  int32_t act;
  int64_t M; int32_t N; int32_t K;
  int32_t G;
  const int32_t *group_offsets;    /* [G+1] device, or NULL for dense */
  const int32_t *tile_starts;      /* [G+1] device, or NULL for dense */
  int32_t dtype;                   /* M3_F32 / M3_F16 / M3_BF16: element type of A, B, pre */
  const float *row_scale;          /* fp32 [ceil(rows / row_scale_div)] or NULL */
  int32_t row_scale_div;
  const int32_t *row_scale_idx;    /* i32 [M] device or NULL: which row_scale entry slot m takes (before the division) */
} m3_gemm_args;
int m3_gemm_nt(const m3_gemm_args *args, void *stream);
/* Tuning knob, no reference counterpart: which calls of m3_gemm_nt take the 256 x 256-tile kernel for long contractions
 * (16-bit operands, K * 2 bytes a multiple of 128 and >= 1024, at most 64 groups; csrc/gemm_big.hip - the ViT-Base shapes
 * of BASELINE configs[3] / configs[4]).  0 never, 1 every call the kernel can run, 2 (default) those where it measured faster
 * with streamed operands: K >= 2048 and at least 96 tiles; -1 re-reads M3_GEMM_BIG from the environment.  Results are the same up to fp32
 * summation order either way. */
int m3_gemm_set_big(int mode);
/* What m3_gemm_nt would do with `args` under the current m3_gemm_set_big mode and the M3_GEMM_* environment switches, without
 * doing it: host code shared with the launch (the same checks and error codes, the same kernel choice and tile order), no
 * GPU work, no operand pointer is read - a test can plan a call on a machine without a GPU from aligned non-NULL dummies.
 * kernel: which of the four kernels takes the call (M3_GEMM_NONE for M = 0, which launches nothing); epilogue: the kind the
 * two LDS-DMA kernels are instantiated for (M3_GEMM_EPI_*; the register-staged kernels only have M3_GEMM_EPI_ANY, the
 * run-time-flag epilogue); tile_m x tile_n: the output tile; m_band: row tiles per band of the tile order; vec8: N and
 * every leading dimension of C-shaped operands a multiple of 8; n_tiles: column tiles; m_tiles_max: the grid's row tiles
 * (a grouped call: the upper bound, one partial tile per group). */
#define M3_GEMM_NONE (-1)
#define M3_GEMM_STAGED 0         /* csrc/gemm_staged.hip, 128-row tiles */
#define M3_GEMM_STAGED_TALL 1    /* the same with 160-row tiles (fp32, dense, whole K slices) */
#define M3_GEMM_DMA 2            /* csrc/gemm_dma.hip */
#define M3_GEMM_BIG 3            /* csrc/gemm_big.hip, 256 x 256 tiles */
#define M3_GEMM_EPI_ANY 0        /* every option behind a run-time flag */
#define M3_GEMM_EPI_GPRE 1       /* * gelu'(gelu_grad_pre), act-dtype C, no bias / residual */
#define M3_GEMM_EPI_RES 2        /* (+ bias) (* row_scale) + residual, fp32 C */
#define M3_GEMM_EPI_PLAIN 3      /* (+ bias) (* row_scale), act-dtype C */
#define M3_GEMM_EPI_GELU 4       /* (+ bias), pre_out, GELU, act-dtype C */
typedef struct {
  int32_t kernel, epilogue;
  int32_t tile_m, tile_n, m_band, vec8;
  int32_t n_tiles, m_tiles_max;
} m3_gemm_plan_out;
int m3_gemm_plan(const m3_gemm_args *args, m3_gemm_plan_out *plan);

/* Weight gradient ("TN", contraction over rows):
 *   dW[g][n, k] (+)= sum_{m in group g} dC[crow(m), n] * A[arow(m), k]
 *   FMoELinear backward (fastmoe linear_backward behind custom_moe_layer.py:32-33) and
 *   nn.Linear weight grads.  dC [*, N], A [*, K] in the act dtype; dW fp32 [G][N][K].
 * Deterministic split over rows: `splits` partial slabs in ws (fp32
 * [splits][G][N][K]) then m3_wgrad_reduce sums them in order (beta = 1 accumulates
 * into dW, as the joint multi-task backward does: train/train_utils.py:449-457).
 * M < 2^31 rows and row strides (lddc, lda times the element size) below 4 GiB: the kernels form a row's byte offset as one
 * 32 x 32 -> 64-bit product; a call outside either is refused (m3_wgrad_multi alike).  The LDS-DMA kernels and the streaming
 * kernel form whole addresses in 32 bits and run only inside the 4 GiB reach, (M + 1) * lddc and (M + 1) * lda times the
 * element size below 4 GiB (m3_wgrad_kernel: the step-downs).  That rule is measured with the M rows of the call: gathered
 * rows c_row_idx[m] / c_row_div and a_row_idx[m] / a_row_div must lie below M for it to hold - nothing checks the indices. */
/* A slab reduction that has not been launched yet (the arguments of m3_wgrad_reduce, or with chunk_rows > 0 of
 * m3_wgrad_reduce_grouped): the next m3_wgrad_tn call of the stream can carry it out in front of its own work
 * (m3_wgrad_args.prev), which saves one launch per weight-gradient GEMM. */
typedef struct m3_wgrad_reduce_desc {
  const float *ws; int32_t splits; int64_t elems;
  const int32_t *group_offsets; int32_t G; int32_t chunk_rows;
  float *dW; int32_t beta;
  const float *bias_ws; int64_t bias_elems; float *db; int32_t beta_db;
} m3_wgrad_reduce_desc;
typedef struct {
  const void *dC; int64_t lddc; const int32_t *c_row_idx;
  const void *A; int64_t lda; const int32_t *a_row_idx; int32_t a_row_div;
  int64_t M; int32_t N; int32_t K; int32_t G;
  const int32_t *group_offsets;    /* [G+1] device or NULL (dense: rows 0..M-1) */
  int32_t splits;
  float *ws;                       /* [splits][G][N][K] */
  int32_t dtype;
  float *bias_ws;                  /* optional [splits][G][N]: bias-grad column sums of dC, fused into the
                                      same pass (one extra MFMA row); reduced by m3_wgrad_reduce (same launch as
                                      the weight slabs) or m3_wgrad_bias_reduce */
  int32_t chunk_rows;              /* 0: every group is cut into `splits` equal parts.  > 0 (grouped calls, a
                                      multiple of 64): balanced mode - a work unit is chunk_rows rows of one group,
                                      group g gets ceil(rows_g / chunk_rows) consecutive units of equal size (taken from the
                                      device-resident offsets: a hot expert gets proportionally more workgroups), ws is
                                      [units][N][K] (bias_ws [units][N]) and m3_wgrad_reduce_grouped sums each
                                      group's slabs */
  int32_t units;                   /* balanced mode: slab slots >= sum_g ceil(rows_g / chunk_rows)
                                      (M / chunk_rows + G always suffices) */
  int32_t c_row_div;               /* with c_row_idx: the dC row of slot m is c_row_idx[m] / c_row_div (0 or 1: no division) */
  const float *c_row_scale;        /* with c_row_idx, fp32 or NULL: that row is multiplied by c_row_scale[c_row_idx[m]] on
                                      its way in.  Together: dC = the [T, N] gradient of the combine's OUTPUT, read through
                                      the slot -> routed-entry map with div = k and scaled by the entry's gate score - the
                                      combine backward d moe_outp[t*k+j] = score[t,j] * d out[t]
                                      (custom_moe_layer.py:298-305) without materialising the [T*k, N] copy */
  const m3_wgrad_reduce_desc *prev; /* optional (host pointer, read during the call): the PREVIOUS call's slab reduction, whose
                                      slabs must live in another buffer than `ws`; its blocks run first in this launch.  The
                                      caller reduces the last call of a sequence itself (m3_wgrad_reduce*). */
  float *direct_dW;                /* optional: DIRECT mode (needs splits == 1, chunk_rows == 0, bias_ws NULL): every (group, tile)
                                      then belongs to exactly one workgroup, which adds its result into dW [G][N][K] itself
                                      (direct_beta 1: dW += result, 0: dW = result) - no slabs (ws may be NULL), no reduction
                                      call.  For weights whose gradient is large against the rows contracted (the ViT-Base
                                      experts: 151 MB per layer), where slabs + reduction move four times the result. */
  float *direct_db;                /* direct mode, optional: the bias gradient [G][N] (column sums of dC) likewise */
  int32_t direct_beta, direct_beta_db;
  int32_t n_prev;                  /* > 1: prev points to that many descriptors - what one m3_wgrad_multi call left behind
                                      (its reduce_out): dense reductions of the same number of slabs.  0 / 1: one descriptor.
                                      In direct mode no prev reduction may write direct_dW / direct_db: the call is refused
                                      (this launch read-add-writes them while the reduce blocks run). */
} m3_wgrad_args;
int m3_wgrad_tn(const m3_wgrad_args *args, void *stream);
/* Several dense weight gradients over the SAME M rows in one launch - the dense weights of one transformer block's backward
 * (qkv, proj, fc1, fc2), whose operands all exist once the attention backward has run:
 *   dW_j[n, k] (+)= sum_m dC_j[m, n] * A_j[m, k],   db_j[n] (+)= sum_m dC_j[m, n]      j < n <= M3_WGRAD_MULTI_MAX
 * Plain rows only (no gathers, no per-row factor, one group), 16-bit operands, and every (N_j, K_j) a shape m3_wgrad_tn gives
 * to its register-staged 128 x 128 kernel under the current m3_wgrad_set_dma / m3_wgrad_set_big settings: m3_wgrad_multi_plan
 * reports `allowed`, and a caller whose batch is not keeps the call per weight.  All problems are cut into the same `parts`
 * row parts (m3_wgrad_multi_plan: the fewest that fill 432 workgroups without exceeding the 512 resident ones, at most 16, at
 * least 16 32-row steps each), every part of every tile writes one fp32 slab into ws (ws_elems floats: problem j's weight slabs
 * [parts][N_j][K_j] at ws_off[j], its bias slabs [parts][N_j] at bias_off[j]), and the slabs are summed in part order:
 * deterministic, no atomics.  The call does not sum them itself: it fills reduce_out[0 .. n) with the n reductions, which the
 * NEXT m3_wgrad_tn / m3_wgrad_multi call of the stream carries out in front of its own work (prev = reduce_out, n_prev = n)
 * or m3_wgrad_reduce_multi launches.  prev as in m3_wgrad_args (slabs outside this call's ws); a prev reduction that writes a
 * dW / db of this call is refused, and so are two problems with the same dW / db.
 * Same results as the calls one by one up to fp32 summation order (other row parts). */
#define M3_WGRAD_MULTI_MAX 8
typedef struct {
  const void *dC; int64_t lddc;    /* [M, N], row stride in elements */
  const void *A; int64_t lda;      /* [M, K] */
  int32_t N, K;
  float *dW; float *db;            /* fp32 [N, K]; [N] or NULL; 16-byte aligned */
  int32_t beta, beta_db;           /* 1: accumulate */
} m3_wgrad_problem;
typedef struct {
  int64_t M; int32_t dtype; int32_t n;
  int32_t parts;                   /* 0: the library's rule; >= 1: the caller's row parts */
  int32_t N[M3_WGRAD_MULTI_MAX], K[M3_WGRAD_MULTI_MAX], bias[M3_WGRAD_MULTI_MAX];
} m3_wgrad_multi_shape;
typedef struct {
  int32_t allowed;                 /* 0: m3_wgrad_multi refuses this batch */
  int32_t parts, tiles, workgroups; /* row parts, 128 x 128 tiles of all problems, parts * tiles */
  int64_t ws_elems;
  int64_t ws_off[M3_WGRAD_MULTI_MAX], bias_off[M3_WGRAD_MULTI_MAX];
} m3_wgrad_multi_plan_out;
int m3_wgrad_multi_plan(const m3_wgrad_multi_shape *shape, m3_wgrad_multi_plan_out *plan);
typedef struct {
  int64_t M; int32_t dtype; int32_t n;
  m3_wgrad_problem prob[M3_WGRAD_MULTI_MAX];
  int32_t parts;                   /* as in m3_wgrad_multi_shape */
  float *ws;                       /* m3_wgrad_multi_plan's ws_elems floats, 16-byte aligned */
  const m3_wgrad_reduce_desc *prev; int32_t n_prev;
  m3_wgrad_reduce_desc *reduce_out; /* [n], host memory, written during the call */
} m3_wgrad_multi_args;
int m3_wgrad_multi(const m3_wgrad_multi_args *args, void *stream);
/* n == 1: m3_wgrad_reduce / m3_wgrad_reduce_grouped of the descriptor; n > 1: the reductions one m3_wgrad_multi call left
 * behind, in one launch */
int m3_wgrad_reduce_multi(const m3_wgrad_reduce_desc *descs, int n, void *stream);
/* How to cut a call up: fill m3_wgrad_shape, call m3_wgrad_plan (host code, no GPU work), copy splits / chunk_rows / units into
 * m3_wgrad_args and give the call ws_elems floats of workspace (weight slabs first, then the bias slabs).  The plan follows the
 * kernel m3_wgrad_tn takes for the shape under the current m3_wgrad_set_dma / m3_wgrad_set_big settings: the streaming kernel
 * of m3_wgrad_skinny gets at least 64 rows per part and at most 256 parts, a tile kernel as many parts as fill its resident
 * workgroups once (at least 512 rows each, dense calls in whole multiples of the 8 XCDs), and grouped calls of 2 .. 64 groups
 * balanced units.  direct = 1 (only with direct_ok, when one part per group is enough): pass direct_dW / direct_db, no
 * workspace, no reduction.  A caller may still set the three fields by itself - a call planned for one kernel runs correctly
 * on another. */
typedef struct {
  int64_t M; int32_t N, K, G; int32_t dtype;
  int32_t grouped;                 /* the call will pass group_offsets */
  int32_t bias;                    /* the call wants the fused bias gradient (bias_ws / direct_db) */
  int32_t splits;                  /* 0: the library's rule; >= 1: the caller's row parts */
  int32_t direct_ok;               /* the caller can take direct mode (dW 16-byte aligned, adding into it is acceptable) */
} m3_wgrad_shape;
typedef struct {
  int32_t splits, chunk_rows, units;   /* the fields of m3_wgrad_args of the same names */
  int32_t direct;
  int64_t ws_elems;                /* fp32 elements: units * N * (K + bias); 0 in direct mode */
} m3_wgrad_plan_out;
int m3_wgrad_plan(const m3_wgrad_shape *shape, m3_wgrad_plan_out *plan);
/* The unit map of balanced mode as a host query (no GPU work; group_offsets is HOST memory here, [G + 1], 1 <= G <= 64;
 * chunk_rows a multiple of 64): group g gets n_g = ceil(rows_g / chunk_rows) consecutive units, unit j of them covers rows
 * [j * share_g, min((j + 1) * share_g, rows_g)) of the group with share_g = ceil(rows_g / n_g) rounded up to 64 (<= chunk_rows:
 * no unit is empty or longer than chunk_rows, an empty group has none).  Writes the group of `unit` and its rows as indices
 * into the call's M rows; group = -1 and no rows for a unit past the last one (a slab slot without work).  The same two
 * functions compute the map in the kernels and in m3_wgrad_reduce_grouped. */
int m3_wgrad_unit_of(const int32_t *group_offsets, int G, int chunk_rows, int unit, int *group, int *row_begin, int *row_end);
/* Tuning knob, no reference counterpart: which weight-gradient launches take the LDS-DMA kernel (wgrad_dma_kernel,
 * csrc/wgrad_dma.hip: four workgroups per CU, operands global -> LDS directly; fp16 / bf16 / fp32, power-of-two gather divisors, a
 * per-row factor with fp16 / fp32 only).  0 = none (the register-staged kernel everywhere), 2 = every launch the kernel can
 * run, 1 (default) = those where it measured faster with operands streamed from HBM: fp32 always; 16-bit when tiles x groups
 * >= 1024 (one part per group: the ViT-Base experts) or N * K >= 1.5 M elements.  -1 = re-read M3_WGRAD_DMA.  Same results up to
 * fp32 summation order (64 instead of 32 contraction rows per accumulation step in 16 bit). */
int m3_wgrad_set_dma(int on);
/* Tuning knob, no reference counterpart: 256 x 256 output tiles (wgrad_big_kernel, csrc/wgrad_dma.hip: eight waves, one workgroup
 * per CU, two LDS stages filled by LDS-DMA) for 16-bit weights whose N and K are multiples of 256 - the ViT-Base shapes (768,
 * 2304, 3072).  1 = on (default), 0 = 128 x 128 everywhere, -1 = re-read M3_WGRAD_BIG.  m3_wgrad_tile reports (256, 256) for the
 * shapes it takes; switch before sizing workspaces.  Same results up to fp32 summation order. */
int m3_wgrad_set_big(int on);
/* The output tile (n x k) m3_wgrad_tn uses for a shape: 256 x 256 where m3_wgrad_set_big's kernel takes it, else 128 x 128.
 * m3_wgrad_plan sizes `splits` / `units` for ceil(N / tn) * ceil(K / tk) tiles per group. */
int m3_wgrad_tile(int N, int K, int dtype, int *tn, int *tk);
/* 1 when m3_wgrad_tn runs a plain call of this shape (one group, no gathers / factor / bias / balanced units / direct mode) with
 * the streaming kernel for K = 16 / 32 - the router's weight, dW_gate = h^T d_logits (custom_moe_layer.py:213-217) - instead of
 * a 128 x 128 MFMA tile padded eightfold: m3_wgrad_plan then sizes `splits` for a stream over dC.  Slab layout and reduction
 * are unchanged.  The rule is fixed: it depends on the shape only. */
int m3_wgrad_skinny(int N, int K, int G);
/* The kernel m3_wgrad_tn would launch for `args` under the current m3_wgrad_set_dma / m3_wgrad_set_big settings, after the
 * step-downs a call can force (a gather divisor that is no power of two, a per-row factor the family lacks for the dtype or
 * on rows that are not gathered, operands past the 4 GiB reach: 256 x 256 and the streaming kernel -> a 128 x 128 kernel,
 * LDS-DMA -> register-staged), and the template instance: gathered dC rows, gathered A rows, per-row factor.  The reach is
 * measured with M + 1 rows - (M + 1) * lddc * sizeof(elem) < 4 GiB and the same for lda: a row's offset plus a column offset
 * stays below 2^32 - so gathered dC / A source rows must lie below M for the kernels inside it to stay inside.  Host code
 * shared with the launch (the same checks of the call and error codes), no GPU work, no operand pointer is read; the
 * descriptors behind args->prev are not looked at (they do not enter the choice; the launch checks them). */
#define M3_WGRAD_KERNEL_STAGED 0   /* csrc/wgrad_staged.hip */
#define M3_WGRAD_KERNEL_DMA 1      /* csrc/wgrad_dma.hip, 128 x 128 */
#define M3_WGRAD_KERNEL_BIG 2      /* csrc/wgrad_dma.hip, 256 x 256 */
#define M3_WGRAD_KERNEL_SKINNY 3   /* csrc/wgrad.hip, the streaming kernel for K = 16 / 32 */
typedef struct {
  int32_t kernel;
  int32_t gather_c, gather_a, scale_c;
  int32_t tile_n, tile_k;
} m3_wgrad_kernel_out;
int m3_wgrad_kernel(const m3_wgrad_args *args, m3_wgrad_kernel_out *out);
/* balanced mode: dW[g] (+)= sum over group g's units of ws[u] (elems = N*K per group), unit order; optionally the
 * same for the bias slabs (bias_elems = N per group) */
int m3_wgrad_reduce_grouped(const float *ws, const int32_t *group_offsets, int G, int chunk_rows, int64_t elems,
                            float *dW, int beta, const float *bias_ws, int64_t bias_elems, float *db, int beta_db,
                            void *stream);
/* dW (+)= sum over the splits of the weight slabs, fixed order; optionally db (+)= the same over
 * the bias slabs (bias_ws NULL to skip). */
int m3_wgrad_reduce(const float *ws, int splits, int64_t elems, float *dW, int beta,
                    const float *bias_ws, int64_t bias_elems, float *db, int beta_db, void *stream);
/* db[g][n] (+)= sum_s bias_ws[s][g][n], elems = G*N */
int m3_wgrad_bias_reduce(const float *bias_ws, int splits, int64_t elems, float *db, int beta, void *stream);
/* Column sums for bias grads: db[g][n] (+)= sum_{m in group g} dC[crow(m), n].
 * ws fp32 [m3_colsum_ws_elems(M, N, G)]. */
int64_t m3_colsum_ws_elems(int64_t M, int N, int G);
int m3_colsum(const void *dC, int dtype, int64_t lddc, const int32_t *c_row_idx, int64_t M, int N,
              int G, const int32_t *group_offsets, float *ws, float *db, int beta, void *stream);

/* ------------------------------------------------------------- combine (a7)
 * out[t,:] = residual[t,:] + sum_j score[t,j] * y[t*k+j,:]
 *   bmm(gate_score[T,1,k], moe_outp[T,k,D]), custom_moe_layer.py:298-305, fused with
 *   the residual add at vision_transformer_moe.py:450.  y [T*k, D] act dtype (token
 *   major), residual/out fp32 [T, D] (residual may be NULL). */
int m3_combine_fwd(const void *y, int dtype, const float *score, const float *residual,
                   int64_t T, int k, int D, float *out, void *stream);
/* dy[t*k+j,:] = score[t,j] * dout[t,:] (act dtype) ; dscore[t,j] = <dout[t,:], y[t*k+j,:]>.
 * dy may be NULL (d score only): the expert backward can take score * dout straight from dout through
 * m3_gemm_args.row_scale_idx / m3_wgrad_args.c_row_scale instead of reading a materialised dy. */
int m3_combine_bwd(const float *dout, const void *y, int dtype, const float *score,
                   int64_t T, int k, int D, void *dy, float *dscore, void *stream);
/* Input gradient at an MoE layer's branch point, in one pass:
 *   dh[t,:] = sum_j dxe[t*k+j,:]  +  d_logits[t,:] @ w_gate[:D,:]^T
 * the gather-sum of the k routed copies (MOEScatter.backward behind custom_moe_layer.py:254-259) and the gate's share
 * (backward of `inp @ w_gate`, noisy_gate_vmoe.py:91).  dxe [T*k, D] act dtype (token major), d_logits fp32 [T, E],
 * w_gate fp32 [D, E] (row-major, the parameter's own layout; E*(D+4)*4 bytes must fit 64 KB of LDS), dh [T, D] stored as
 * dh_dtype: M3_F32 or the activation dtype (the sum is formed in fp32 either way). */
int m3_combine_gate_bwd(const void *dxe, int dtype, int64_t T, int k, int D, const float *d_logits,
                        const float *w_gate, int E, void *dh, int dh_dtype, void *stream);

/* Row movement of fastmoe's MOEScatter / MOEGather (custom_moe_layer.py:14,263-265) for
 * callers that run an arbitrary expert_fn between them (the fused path does not need it):
 *   dst[i,:] = sum_{j<k} src[idx[i*k+j] / div, :]     (k = 1: plain gather; k > 1: the
 *   backward of the scatter, summing the k routed copies of a token). */
int m3_gather_rows(const void *src, int dtype, const int32_t *idx, int div, int64_t nout, int k,
                   int D, void *dst, void *stream);

/* ------------------------------------------------------- routing statistics
 * What a MoE Block reports in `last_moe_analysis` after every forward
 * (models/moe/ckpt/vision_transformer_moe.py:461-478 inside the checkpointed body, :546-562 for expert_load_cv), which
 * VisionTransformerMoE.forward folds into `latest_moe_stats` (:795-880) - computed on the device, inside the pass, into
 * one record the host copies only when somebody asks (the reference reads seven scalars per MoE block with .item()).
 * Inputs, all read-only: score f32 [T,k] and gates f32 [T,E] (the gate's top-k probabilities, dense: p at the selected
 * experts, 0 elsewhere), clean f32 [T,E] (clean_logits), h [T,D] (norm2(x), row stride ldh elements) and y [T*k,D] (the
 * token-major expert outputs, row stride ldy) in the activation dtype, and the load vector [E] of the block's balance
 * loss as EITHER load_f32 (the Normal-CDF form of noisy training) OR load_i64 (the counts), the other NULL.
 * m = sum_j score[t,j] * y[t*k+j] is the layer output before mlp_drop / DropPath / the residual (fp32 fma, j ascending).
 * The record is M3_MOE_STATS_HIST + E four-byte words:
 *   f32 [M3_MOE_STATS_ENTROPY_SUM]  sum_t sum_e -p ln(max(p, 1e-12))
 *   f32 [M3_MOE_STATS_TOP1_SUM]     sum_t max_e p[t,e]
 *   f32 [M3_MOE_STATS_CLEAN_STD]    mean_t of the population std over E of clean[t,:]   (0 for T = 0)
 *   f32 [M3_MOE_STATS_NORM_RATIO]   |m|_2 / (|h|_2 + 1e-12), Frobenius norms over [T,D]
 *   f32 [M3_MOE_STATS_LOAD_CV]      var_pop(load) / (mean(load)^2 + 1e-10); 0 for E <= 1
 *   f32 [M3_MOE_STATS_M_SUMSQ], [M3_MOE_STATS_H_SUMSQ]   the two sums of squares behind the ratio
 *   i32 [M3_MOE_STATS_TOKENS]       T
 *   i32 [M3_MOE_STATS_HIST + e]     #{t : p[t,e] > 0}  (a selected probability that underflowed to 0 does not count)
 * ws f32 [m3_moe_stats_ws_elems(T,E)]: per-workgroup partials, added in a fixed order by a second one-workgroup launch -
 * no atomics, two runs on the same inputs give the same bits.  E in [1,64], 1 <= k <= E, T < 2^31; rows of h and y are
 * 16-byte multiples at 16-byte aligned addresses. */
#define M3_MOE_STATS_ENTROPY_SUM 0
#define M3_MOE_STATS_TOP1_SUM 1
#define M3_MOE_STATS_CLEAN_STD 2
#define M3_MOE_STATS_NORM_RATIO 3
#define M3_MOE_STATS_LOAD_CV 4
#define M3_MOE_STATS_M_SUMSQ 5
#define M3_MOE_STATS_H_SUMSQ 6
#define M3_MOE_STATS_TOKENS 7
#define M3_MOE_STATS_HIST 8
int64_t m3_moe_stats_ws_elems(int64_t T, int E);
int m3_moe_stats(const float *score, const float *clean, const float *gates, const void *h, int64_t ldh,
                 const void *y, int64_t ldy, int dtype, const float *load_f32, const int64_t *load_i64,
                 int64_t T, int E, int k, int D, float *ws, void *record, void *stream);

/* ----------------------------------------------------------- LayerNorm (a9)
 * nn.LayerNorm(D, eps) on the fp32 residual stream, output in the act dtype
 * (vision_transformer_moe.py:441-442, eps 1e-6 :567).  Saves mean/rstd fp32 [T]. */
int m3_layernorm_fwd(const float *x, int64_t T, int D, const float *gamma, const float *beta,
                     float eps, void *y, int y_dtype, float *mean, float *rstd, void *stream);
/* dx[t,:] = dx_res[t,:] + LN'(dy[t,:]) ; dgamma/dbeta via per-block partials in ws
 * (fp32 [2][m3_ln_bwd_blocks(T, D)][D]) reduced in fixed order (beta = accumulate).
 * dx_act (optional): a copy of dx in the activation dtype for the GEMMs that consume it next. */
int m3_ln_bwd_blocks(int64_t T, int D);
/* dgamma == dbeta == NULL: the per-block partials are left in ws for m3_layernorm_bwd_reduce. */
int m3_layernorm_bwd(const void *dy, int dy_dtype, const float *x, const float *mean,
                     const float *rstd, const float *gamma, const float *dx_res,
                     int64_t T, int D, float *dx, float *ws, float *dgamma, float *dbeta,
                     int beta, void *dx_act, int dx_act_dtype, void *stream);

/* dgamma / dbeta of `count` LayerNorms in ONE launch: layer j (first <= j < first + count) has its partials
 * (written by m3_layernorm_bwd with dgamma = dbeta = NULL) at ws + j * layer_stride floats and its outputs in
 * grads_dev[j] (a DEVICE array); fixed summation order; beta = accumulate.  The reference's autograd produces these one
 * LayerNorm at a time (vision_transformer_moe.py:441-442); here the 24-workgroup reduction behind every LayerNorm
 * backward becomes one launch per group of blocks. */
typedef struct m3_ln_param_grads { float *dgamma; float *dbeta; } m3_ln_param_grads;
int m3_layernorm_bwd_reduce(const float *ws, int64_t layer_stride, int nblk, int D,
                            const m3_ln_param_grads *grads_dev, int first, int count, int beta, void *stream);

/* ----------------------------------------------------------- attention (a8)
 * softmax(q k^T * dh^-0.5) v over the packed qkv activations written by the qkv
 * Linear, Attention.forward vision_transformer_moe.py:299-313.
 * qkv [B*N, 3*C] act dtype laid out [token][3][heads][dh]; o [B*N, C]; lse f32 [B,heads,N].
 * dh in {32, 64}. */
int m3_attention_fwd(const void *qkv, int dtype, int B, int N, int heads, int dh,
                     void *o, float *lse, void *stream);
/* dqkv [B*N, 3*C] from do [B*N, C].  One workgroup per (image, head, 256-key block); for N > 256 the
 * key blocks' dQ contributions go to fp32 slabs in dq_ws ([ceil(N/256)][B*heads][N][dh] =
 * m3_attention_bwd_ws_elems(B,N,heads,dh) floats, contents need no initialisation; NULL when N <= 256)
 * and are summed in key-block order by a second launch. */
int64_t m3_attention_bwd_ws_elems(int B, int N, int heads, int dh);
int m3_attention_bwd(const void *qkv, const void *o, const void *d_o, const float *lse,
                     int dtype, int B, int N, int heads, int dh, void *dqkv, float *dq_ws,
                     void *stream);
/* Which kernels m3_attention_fwd / m3_attention_bwd launch for (dtype, N, dh): host code shared with the two entry points
 * and with the launchers' instance choice, no GPU work.  Family: exact fp32 (any N), the LDS-resident 16-bit kernels
 * (N <= 256) or the streamed 16-bit ones.  fwd_key_tiles: the key-tile count the resident forward is instantiated for (16-key
 * tiles rounded up to 4, 8, 12, 16; keys >= N are masked); bwd_tiles_per_wave: the resident backward's instance (dh 32: 1..4,
 * dh 64: 1..2); both 0 for the other families.  bwd_key_blocks: 256-key blocks of the backward (> 1: dQ slabs + reduction). */
#define M3_ATTN_F32 0
#define M3_ATTN_RESIDENT 1
#define M3_ATTN_STREAMED 2
typedef struct {
  int32_t fwd_family, fwd_key_tiles;
  int32_t bwd_family, bwd_tiles_per_wave, bwd_key_blocks;
} m3_attention_plan_out;
int m3_attention_plan(int dtype, int N, int dh, m3_attention_plan_out *plan);

/* ------------------------------------------------------------- elementwise
 * cast / transpose helpers for parameters (fp32 master -> act dtype operand copies):
 *   dst[g][c][r] = (T) src[g][r][c]  when transpose, else dst = (T) src. */
int m3_cast_matrix(const float *src, int G, int rows, int cols, int transpose,
                   void *dst, int dst_dtype, void *stream);
/* The same for many matrices in ONE launch (all operand copies of a model per optimizer step):
 * descs_dev is a DEVICE array of n_desc descriptors; a job writes dst (same layout as src) and/or dst_t
 * (transposed, [g][cols][rows]) - either may be NULL - from one read of src; tile_start = running sum of
 * G * ceil(rows/32) * ceil(cols/32) over the preceding descriptors, total_tiles = the full sum. */
typedef struct m3_cast_desc {
  const float *src; void *dst; void *dst_t;
  int32_t G, rows, cols;
  int32_t tile_start;
} m3_cast_desc;
int m3_cast_batch(const m3_cast_desc *descs_dev, int n_desc, int total_tiles, int dst_dtype, void *stream);
/* dst[i] += src[i] (fp32, n elements): sums the flat gradient buffers of task passes that ran
 * concurrently (the reference accumulates them through autograd, train/train_utils.py:437-457). */
int m3_add_f32(float *dst, const float *src, int64_t n, void *stream);
/* dst(T)[i] = src(f32)[i] ; n elements */
int m3_cast_f32(const float *src, int64_t n, void *dst, int dst_dtype, void *stream);
/* dst(T)[r, :] = row_scale[r / div] * src(f32)[r, :]  (rows x cols, cols % 4 == 0): the gradient that enters a residual
 * branch behind a DropPath (vision_transformer_moe.py:167-185: d branch = scale[sample] * d x), as the activation-dtype
 * operand of the branch's backward GEMMs. */
int m3_scale_rows_cast(const float *src, int64_t rows, int cols, const float *row_scale, int div, void *dst,
                       int dst_dtype, void *stream);
/* patchify: images [B,3,H,W] fp32 NCHW -> rows [B*(H/P)*(W/P), 3*P*P] act dtype in
 * conv-weight order (c, py, px): PatchEmbed conv16/16, vision_transformer_moe.py:330-341 */
int m3_im2row(const float *img, int B, int Cin, int H, int W, int P, void *rows, int dtype,
              void *stream);
/* tokens[b,0,:] = cls + pos[0] ; tokens[b,1+i,:] = patch[b*np+i,:] + pos[1+i]  (fp32 out)
 * forward_features :782-791.  patch fp32 [B*np, D]. */
int m3_assemble_tokens(const float *patch, const float *cls, const float *pos, int B, int np_,
                       int D, float *tokens, void *stream);

/* backward of m3_assemble_tokens: dpatch (act dtype, may be NULL) [B*np, D] = dtok[:,1:,:];
 * dpos f32 [np+1, D] (+)= sum_b dtok[b] ; dcls f32 [D] (+)= sum_b dtok[b,0]  (beta 0/1). */
int m3_tokens_bwd(const float *dtok, int B, int np_, int D, void *dpatch, int dtype, float *dpos,
                  float *dcls, int beta, void *stream);
/* The same pair with TWO prefix tokens in front of the patches - a distilled model's cls and distillation token,
 * vision_transformer_moe.py:784-790: tokens[b,0,:] = cls + pos[0] ; tokens[b,1,:] = dist + pos[1] ;
 * tokens[b,2+i,:] = patch[b*np+i,:] + pos[2+i]  (fp32 out; pos f32 [np+2, D]).  cls and dist are separate [D] vectors
 * anywhere in memory.  Backward: dpatch (act dtype, may be NULL) [B*np, D] = dtok[:,2:,:] ; dpos f32 [np+2, D] (+)=
 * sum_b dtok[b] ; dcls (+)= sum_b dtok[b,0] ; ddist (+)= sum_b dtok[b,1]  (beta 0/1), summed in the order m3_tokens_bwd
 * uses (the same kernel body): the same bits from run to run.  D % 4 == 0. */
int m3_assemble_tokens2(const float *patch, const float *cls, const float *dist, const float *pos, int B, int np_, int D,
                        float *tokens, void *stream);
int m3_tokens_bwd2(const float *dtok, int B, int np_, int D, void *dpatch, int dtype, float *dpos, float *dcls,
                   float *ddist, int beta, void *stream);

/* ------------------------------------------------------------- optimizer tail
 * What every trainer of the reference runs behind the backward (GradScaler.unscale_, clip_grad_norm_, scaler.step of
 * torch.optim.AdamW / Adam / SGD with parameter groups: pretrain/engine/train_one_epoch.py:35-61,
 * pretrain/optim/optimizer.py:6-46, utils/common_config.py:866-896) in three launches over all parameter tensors.
 *
 * descs_dev: a DEVICE array, one descriptor per parameter tensor (all fp32, n elements each): master p, gradient g (never
 * written), first moment / momentum buffer m, second moment v (NULL for SGD).  One workgroup updates one chunk of
 * M3_OPTIM_CHUNK elements: chunk_start = running sum of ceil(n / M3_OPTIM_CHUNK) over the preceding descriptors,
 * total_chunks the full sum.  vec_ok = 1 when p, g, m and v are all 16-byte aligned (16-byte accesses), else 0 (scalar
 * accesses: a gradient that is a view into a flat buffer may start at any element).
 *
 * hyper: DEVICE fp32 [n_groups][M3_OPTIM_HYPER] = lr, beta1 (SGD: momentum), beta2, eps, weight_decay, flags
 * (M3_OPTIM_DECOUPLED: p *= 1 - lr * wd, AdamW; else wd * p is added to the gradient.  M3_OPTIM_NESTEROV), beta1_lo,
 * beta2_lo where beta = (double) beta_hi + (double) beta_lo restores the host's double (the bias corrections are formed
 * from it in double: 1 - beta2 carries 1e-5 of relative error when beta2 is first rounded to fp32).
 *
 * state: DEVICE, m3_optim_state_elems(n_groups) floats, zero before the first call and then owned by these calls:
 *   [0] skip (int32)  [1] step (int32, counts the steps that were NOT skipped)  [2] total_norm  [3] clip_coef
 *   [4] inv_scale  [5] inv_scale * clip_coef  [6..7] spare, then 8 derived doubles per group (8-byte aligned base).
 *
 * m3_optim_prepare: (a) when want_norm, partials[c] = fp32 sum of squares of chunk c's gradient elements and
 * partials[total_chunks + c] = 1 if one of them is not finite (partials: 2 * total_chunks floats, no initialisation);
 * (b) one workgroup adds the partials in a fixed order in double, total_norm = sqrt(sum) * inv_scale with
 * inv_scale = 1 / *grad_scale (1 when NULL), skip = non-finite | (*found_inf_in != 0, when given),
 * clip_coef = min(1, max_norm / (total_norm + 1e-6)) (1 when max_norm <= 0), step += !skip, and each group's coefficients
 * for step t (Adam: lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t), formed and kept in double).
 * m3_optim_step: p, m (and v) of every tensor updated in one pass from g * inv_scale * clip_coef; with skip set nothing
 * is written.  kind: M3_OPTIM_ADAMW / M3_OPTIM_ADAM (exp_avg, exp_avg_sq as torch; the group's M3_OPTIM_DECOUPLED flag is
 * what tells them apart) or M3_OPTIM_SGD (buf = momentum * buf + g, dampening 0, optional nesterov; a zero buffer gives
 * torch's first step).  The Adam update of an element is evaluated in double: p, m and v are each rounded to fp32
 * once.  `hyper` of m3_optim_step is accepted for symmetry and not read: the step takes its coefficients from `state`.
 * Results are bit-identical from run to run. */
#define M3_OPTIM_CHUNK 4096
#define M3_OPTIM_HYPER 8
#define M3_OPTIM_ADAMW 0
#define M3_OPTIM_ADAM 1
#define M3_OPTIM_SGD 2
#define M3_OPTIM_DECOUPLED 1
#define M3_OPTIM_NESTEROV 2
typedef struct m3_optim_desc {
  float *p; float *g; float *m; float *v;
  int64_t n;
  int32_t group, chunk_start, vec_ok;
} m3_optim_desc;
int m3_optim_state_elems(int n_groups);
int m3_optim_prepare(const m3_optim_desc *descs_dev, int n_desc, int total_chunks, const float *hyper, int n_groups,
                     int kind, const float *grad_scale, const float *found_inf_in, float max_norm, int want_norm,
                     float *partials, float *state, void *stream);
int m3_optim_step(const m3_optim_desc *descs_dev, int n_desc, int total_chunks, const float *hyper, const float *state,
                  int kind, void *stream);

/* -------------------------------------------------- decoder-head element-wise stage ("custom later")
 * ReLU (optional) + bilinear x2 up-sampling with align_corners = False in one pass, channels-last: the element-wise half of a
 * stage of models/heads/vit_up_head.py:181-214 (F.relu(syncbn(conv(x))) then F.interpolate(.., size = 2x, mode='bilinear')).
 * x [N, H, W, C] (x_dtype; C a multiple of 8 for 16-bit, 4 for fp32) -> y [N, 2H, 2W, C] in x's dtype or M3_F32.
 * Backward: dx [N, H, W, C] (x's dtype) = relu'(x) * transpose-resize(dy), dy in x's dtype or M3_F32; a gather over the 4 x 4
 * window of output gradients each input pixel fed (deterministic).  Non-finite inputs give what torch gives (relu(NaN) = NaN,
 * and the gradient passes where x is NaN) and nothing else moves: a pixel that does not read the Inf / NaN keeps its bits. */
int m3_relu_up2x_fwd(const void *x, int x_dtype, int64_t N, int H, int W, int C, int relu, void *y, int y_dtype,
                     void *stream);
int m3_relu_up2x_bwd(const void *dy, int dy_dtype, const void *x, int x_dtype, int64_t N, int H, int W, int C,
                     int relu, void *dx, void *stream);
/* The forward with its output written into the INTERIOR of a zero-bordered image yb [N, 2H+2, 2W+2, C] (x's dtype, 16-bit
 * only): the operand layout of m3_conv3x3_fwd, so that the next stage's convolution reads what this stage wrote.  The border
 * is the caller's: it must already be zero and is not touched.  The backward is m3_relu_up2x_bwd on the dense gradient. */
int m3_relu_up2x_fwd_bordered(const void *x, int dtype, int64_t N, int H, int W, int C, int relu, void *yb, void *stream);

/* -------------------------------------------------- decoder-head 3 x 3 convolutions ("custom later")
 * nn.Conv2d(C, Cout, 3, stride 1, padding 1) of models/heads/vit_up_head.py:181-214 (conv_0..3) and of TamModule
 * (models/models.py:11-134: layers0..3) as GEMMs on this library's own kernels (csrc/conv.hip), opt-in: 16-bit activations,
 * C a multiple of 128, Cout a multiple of 8 (the input gradient: Cout a multiple of 128, C of 8).
 * An activation that feeds a convolution is a zero-bordered channels-last image xb [N, H+2, W+2, C]; the window of output pixel
 * m = (n, y, x) is three contiguous runs of 3 C elements, run dy starting at bordered pixel (n, y + dy, x), so the contraction
 * index is ordered (dy, dx, c) and padding costs nothing.  pix_idx i32 [N H W]: bordered pixel index of (n, y, x), written by
 * m3_conv3x3_index (once per shape).
 *   m3_conv3x3_fwd    y [N H W, Cout] (dense channels-last, the activation dtype) = windows @ w^T (+ bias fp32 [Cout] or NULL);
 *                     w [Cout, 9 C] = weight.permute(0, 2, 3, 1) in the activation dtype.  One launch of the 256 x 256 GEMM
 *                     kernel with segmented A rows.
 *   m3_conv3x3_dgrad  dx [N H W, C] from the zero-bordered dyb [N, H+2, W+2, Cout] and w_flip [C, 9 Cout] =
 *                     weight.flip(2, 3).permute(1, 2, 3, 0): the same launch with the roles of C and Cout exchanged.
 *   m3_conv3x3_wgrad  dw3 fp32 [3][Cout][3 C]: dw3[dy][co][dx C + c] = d weight[co][c][dy][dx], and db fp32 [Cout] (or NULL)
 *                     from xb and the dense dy [N H W, Cout]: three m3_wgrad_tn problems (N = Cout, K = 3 C, one per kernel
 *                     row) and one reduction; ws: m3_conv3x3_plan's wgrad_ws_elems floats.  Overwrites dw3 / db.
 *   m3_pad_border_nhwc  xb = x [N, H, W, C] with a border of zeros (C a multiple of 8, 16-bit); bit-exact copy.
 *   m3_conv3x3_plan   host code, no GPU work, reads no pointer: does the shape take this path (ok; reason = M3_CONV_OK or why
 *                     not; dgrad_ok: the input gradient too), and with what: kernel / epilogue as m3_gemm_plan names them, the
 *                     tile, row / column / K tile counts, K tiles per run (seg_tiles) and the byte jump between runs, the
 *                     weight-gradient tile edge, its row parts and workspace.  A shape that is refused is no error. */
#define M3_CONV_OK 0
#define M3_CONV_REFUSE_DTYPE 1     /* not fp16 / bf16 */
#define M3_CONV_REFUSE_CIN 2       /* input channels not a multiple of 128 */
#define M3_CONV_REFUSE_COUT 3      /* output channels not a multiple of 8 */
#define M3_CONV_REFUSE_REACH 4     /* bordered operand or weight panel past 4 GiB */
typedef struct {
  int32_t ok, reason, dgrad_ok;
  int32_t kernel, epilogue;
  int32_t tile_m, tile_n, m_tiles, n_tiles, k_tiles, seg_tiles;
  int32_t wgrad_tile, wgrad_splits;
  int64_t M, bordered_pixels, seg_jump_bytes, wgrad_ws_elems;
} m3_conv3x3_plan_out;
int m3_conv3x3_plan(int dtype, int64_t N, int H, int W, int C, int Cout, m3_conv3x3_plan_out *plan);
int m3_conv3x3_index(int64_t N, int H, int W, int32_t *pix_idx, void *stream);
int m3_pad_border_nhwc(const void *x, int dtype, int64_t N, int H, int W, int C, void *xb, void *stream);
int m3_conv3x3_fwd(const void *xb, int dtype, int64_t N, int H, int W, int C, const void *w, int Cout, const float *bias,
                   const int32_t *pix_idx, void *y, void *stream);
int m3_conv3x3_dgrad(const void *dyb, int dtype, int64_t N, int H, int W, int C, const void *w_flip, int Cout,
                     const int32_t *pix_idx, void *dx, void *stream);
int m3_conv3x3_wgrad(const void *xb, const void *dy, int dtype, int64_t N, int H, int W, int C, int Cout,
                     const int32_t *pix_idx, float *ws, int64_t ws_elems, float *dw3, float *db, void *stream);

/* ------------------------------------------------------------- dense-prediction losses
 * The criterion between the decoder heads and the backward: the four losses utils/common_config.py:780-807 (get_loss) can
 * return - SoftMaxwithLoss (losses/loss_functions.py:16-33), BalancedCrossEntropyLoss (:36-84, size_average, no void_pixels),
 * DepthLoss('l1') (:126-140) and NormalsLoss(normalize=True, size_average=True, norm = 1 | 2) (:143-197) - each as a forward
 * (two launches: per-workgroup partials, then one workgroup that adds them in block order in double) and one backward launch.
 * No atomics, nothing read back to the host, the same bits from run to run.
 *
 * pred: [B,C,H,W] values of `dtype` (M3_F32 / M3_F16 / M3_BF16) in one of two layouts: M3_LAYOUT_NCHW (contiguous) or
 * M3_LAYOUT_NHWC (channels-last storage, what m3_relu_up2x_fwd writes).  dpred: the same dtype and layout.  Arithmetic is fp32.
 * 16-byte accesses where pred / dpred / lse are 16-byte aligned and rows fill whole vectors (NCHW: H*W % 4 == 0; NHWC cross-
 * entropy: C % 4 == 0; L1 / BCE: B*C*H*W % 4 == 0), scalar accesses otherwise; B*C*H*W < 2^31 - 2^20.
 * label: cross-entropy: one class per pixel, [B*H*W] of label_dtype (M3_LABEL_F32 truncated as `.long()`, M3_LABEL_I64,
 * M3_LABEL_U8); 255 = ignored; a value that is neither 255 nor in [0, C) indexes nothing, is treated as ignored and counted in
 * the record's N_BAD word.  L1 / BCE: f32, the shape AND layout of pred.  Normals: f32 [B,C,H,W] in label_layout.
 * ws: f32 [m3_loss_ws_elems(B*C*H*W)], no initialisation.  lse (cross-entropy): f32 [B*H*W], written by the forward (the
 * log-sum-exp of every pixel, ignored ones included) and read by the backward.
 * record: M3_LOSS_REC_WORDS four-byte words, written by the forward, read by the backward:
 *   f32 [M3_LOSS_REC_VALUE]    the loss
 *   f32 [M3_LOSS_REC_COEF]     what the backward multiplies by: CE, L1: 1 / n_valid (0 when n_valid = 0); normals:
 *                              1 / max(n_valid, 1e-6); BCE: w / numel, the positive elements' factor
 *   f32 [M3_LOSS_REC_COEF2]    BCE: (1 - w) / numel, the negative elements' factor; else 0
 *   i32 [M3_LOSS_REC_N_VALID]  CE: pixels with a class; L1, normals: elements with label != 255; BCE: n_pos (label >= 0.5)
 *   i32 [M3_LOSS_REC_N_AUX]    BCE: n_neg; else 0
 *   i32 [M3_LOSS_REC_N_BAD]    CE: bad labels; else 0
 * grad_out: DEVICE f32 scalar, the upstream gradient (a loss scale and 1 / accumulation_steps arrive here).
 *
 * CE: loss = mean over valid pixels of lse(x) - x[label] (running maximum: finite at |x| = 6e4), C in [2, 255];
 *   dpred = (exp(x - lse) - [c == label]) * COEF * grad_out, 0 at ignored pixels.  No valid pixel: loss NaN, dpred 0.
 * L1: loss = mean of |pred - label| over label != 255; dpred = sign(pred - label) (0 at 0) * COEF * grad_out.  None valid:
 *   loss NaN, dpred 0.
 * normals: t = pred / (|pred|_2 over C + 1e-12); loss = sum over label != 255 of |t - label| (norm 1) or (t - label)^2
 *   (norm 2), / max(n_valid, 1e-6) - 0 when nothing is valid; dpred carries the Jacobian of the normalisation.  C in [1, 8].
 * BCE: y = label >= 0.5, term = x ([x >= 0] - y) + log(1 + exp(-|x|)); w = pos_weight when has_pos_weight, else
 *   the fp32 quotient n_neg / (n_pos + n_neg), as the reference's `labels.float()` sums give it, formed in the finalize launch; loss = (w sum_pos + (1 - w) sum_neg) / numel;
 *   dpred = (sigmoid(x) - y) * (y ? COEF : COEF2) * grad_out. */
#define M3_LAYOUT_NCHW 0
#define M3_LAYOUT_NHWC 1
#define M3_LABEL_F32 0
#define M3_LABEL_I64 1
#define M3_LABEL_U8 2
#define M3_LOSS_MAX_BLOCKS 1024
#define M3_LOSS_NORMALS_MAX_C 8
#define M3_LOSS_REC_VALUE 0
#define M3_LOSS_REC_COEF 1
#define M3_LOSS_REC_COEF2 2
#define M3_LOSS_REC_N_VALID 3
#define M3_LOSS_REC_N_AUX 4
#define M3_LOSS_REC_N_BAD 5
#define M3_LOSS_REC_WORDS 8
int64_t m3_loss_ws_elems(int64_t n);
int m3_loss_ce_fwd(const void *pred, int dtype, const void *label, int label_dtype, int B, int C, int H, int W, int layout,
                   float *lse, float *ws, void *record, void *stream);
int m3_loss_ce_bwd(const void *pred, int dtype, const void *label, int label_dtype, const float *lse, const void *record,
                   const float *grad_out, int B, int C, int H, int W, int layout, void *dpred, void *stream);
int m3_loss_l1_fwd(const void *pred, int dtype, const float *label, int B, int C, int H, int W, int layout, float *ws,
                   void *record, void *stream);
int m3_loss_l1_bwd(const void *pred, int dtype, const float *label, const void *record, const float *grad_out, int B, int C,
                   int H, int W, int layout, void *dpred, void *stream);
int m3_loss_normals_fwd(const void *pred, int dtype, const float *label, int B, int C, int H, int W, int layout,
                        int label_layout, int norm, float *ws, void *record, void *stream);
int m3_loss_normals_bwd(const void *pred, int dtype, const float *label, const void *record, const float *grad_out, int B,
                        int C, int H, int W, int layout, int label_layout, int norm, void *dpred, void *stream);
int m3_loss_bce_fwd(const void *pred, int dtype, const float *label, int B, int C, int H, int W, int layout,
                    int has_pos_weight, double pos_weight, float *ws, void *record, void *stream);
int m3_loss_bce_bwd(const void *pred, int dtype, const float *label, const void *record, const float *grad_out, int B, int C,
                    int H, int W, int layout, void *dpred, void *stream);

/* ------------------------------------------------------------- task metrics
 * What the reference's PerformanceMeter accumulates after every forward (evaluation/eval_semseg.py:109-120,
 * eval_human_parts.py:88-98, eval_depth.py:67-85, eval_normals.py:72-94, eval_sal.py:75-96 with jaccard.py), from the RAW head
 * output: utils/utils.py:60-79 (get_output: argmax, normalise, sigmoid) is fused in, nothing of pred's size is written.  An
 * update is two launches - per-workgroup partials, then one workgroup that adds them in block order (float sums in double)
 * INTO `state`.  No global atomics, nothing read back to the host, the same bits from run to run.
 *
 * pred, dtype, layout, label_dtype, the 16-byte / scalar access rule and the size limit: as for the losses above.  Label 255 is
 * "ignore" for every meter but saliency.
 * ws: m3_meter_ws_elems(kind, B*C*H*W, aux) four-byte words, no initialisation; aux: n_classes (M3_METER_IOU), B
 * (M3_METER_SAL), ignored otherwise.  0 for arguments the update would refuse.
 * state: 8-byte words the update ADDS to (int64 counts, double sums); the caller zeroes them (a memset) to reset, and may sum
 * the states of several processes.  Layouts, as word indices:
 *   IoU      [M3_METER_IOU_WORDS]: int64 [3][M3_METER_IOU_BINS] at M3_METER_IOU_TP (label == prediction == i),
 *            M3_METER_IOU_PRED (prediction == i) and M3_METER_IOU_LABEL (label == i), over the pixels with label != 255; bins
 *            [0, n_classes) are written.  fp = PRED - TP, fn = LABEL - TP.
 *   depth    [M3_METER_DEPTH_WORDS]: f64 SUM_SQ, f64 SUM_LOG_SQ, i64 N_VALID
 *   normals  [M3_METER_NORMALS_WORDS]: f64 SUM_ANGLE, f64 SUM_SQ (degrees, degrees^2), i64 N_11 / N_22 / N_30 (angles below
 *            11.25 / 22.5 / 30 degrees), i64 N
 *   saliency [M3_METER_SAL_WORDS]: f64 [3][M3_METER_SAL_THRESHOLDS] at M3_METER_SAL_JACCARD / _PREC / _REC: per-image values
 *            summed over the images; i64 N_IMAGES
 *
 * IoU: prediction = argmax over C, lowest index on ties, a NaN beats everything and the first NaN wins (torch.max); C in
 *   [2, 255], n_classes in [1, 256].  A float label is class i only where it EQUALS i; a valid label that is no class in
 *   [0, n_classes) matches none and still counts its pixel in PRED.
 * depth: over label != 255: (label - p)^2 and (log label - log p)^2 with p = max(pred, 1e-9); label f32 in pred's layout.
 * normals (C = 3): t = pred / max(|pred|_2, 1e-12); elements with label == 255 are zeroed in t and label; angle =
 *   (180 / pi) acos(clamp(sum_c t label, -1, 1)); a pixel counts where channel 0 of its label is valid.
 * saliency (C = 1, B <= M3_LOSS_MAX_BLOCKS): p = sigmoid(pred) in fp32 against the fp32 values of linspace(0.2, 0.9, 15), label
 *   != 0; per image and threshold jaccard (1 when both masks are empty), tp / (tp + fp + 1e-12) and tp / (tp + fn + 1e-12) in
 *   double from exact counts. */
#define M3_METER_IOU 0
#define M3_METER_DEPTH 1
#define M3_METER_NORMALS 2
#define M3_METER_SAL 3
#define M3_METER_IOU_BINS 256
#define M3_METER_IOU_TP 0
#define M3_METER_IOU_PRED 256
#define M3_METER_IOU_LABEL 512
#define M3_METER_IOU_WORDS 768
#define M3_METER_DEPTH_SUM_SQ 0
#define M3_METER_DEPTH_SUM_LOG_SQ 1
#define M3_METER_DEPTH_N_VALID 2
#define M3_METER_DEPTH_WORDS 4
#define M3_METER_NORMALS_SUM_ANGLE 0
#define M3_METER_NORMALS_SUM_SQ 1
#define M3_METER_NORMALS_N_11 2
#define M3_METER_NORMALS_N_22 3
#define M3_METER_NORMALS_N_30 4
#define M3_METER_NORMALS_N 5
#define M3_METER_NORMALS_WORDS 8
#define M3_METER_SAL_THRESHOLDS 15
#define M3_METER_SAL_JACCARD 0
#define M3_METER_SAL_PREC 15
#define M3_METER_SAL_REC 30
#define M3_METER_SAL_N_IMAGES 45
#define M3_METER_SAL_WORDS 48
int64_t m3_meter_ws_elems(int kind, int64_t n, int aux);
int m3_meter_iou_update(const void *pred, int dtype, const void *label, int label_dtype, int B, int C, int H, int W, int layout,
                        int n_classes, void *ws, void *state, void *stream);
int m3_meter_depth_update(const void *pred, int dtype, const float *label, int B, int C, int H, int W, int layout, void *ws,
                          void *state, void *stream);
int m3_meter_normals_update(const void *pred, int dtype, const float *label, int B, int H, int W, int layout, int label_layout,
                            void *ws, void *state, void *stream);
int m3_meter_sal_update(const void *pred, int dtype, const float *label, int B, int H, int W, void *ws, void *state,
                        void *stream);

/* ------------------------------------------------------------- pretraining recipe
 * What the ImageNet pretraining trainer runs around the model and the optimizer (pretrain/train.py:461-471,498,536,877-905):
 * batch mixing, the soft-target criterion, the evaluation sums and the weight EMA.  Nothing is read back to the host, no float
 * atomics, the same bits from run to run.
 *
 * m3_mix_batch: Mixup / CutMix of x [B,C,H,W] (fp32, NCHW) with its batch-reversed self (the mixup_fn call of
 * pretrain/engine/train_one_epoch.py:32-33): sample i is paired with j = B-1-i, B even.  lam f32 [B], box i32 [B,4] = yl, yh,
 * xl, xh per sample (DEVICE).  Empty box (yl == yh or xl == xh): out_i = lam_i x_i + (1 - lam_i) x_j, lam 1 and 0 bit copies;
 * else out_i = x_j inside the box and x_i outside, bit copies.  Both members of a pair are read before either is written:
 * out == x is valid (out_dtype M3_F32 then), and lam_i != lam_j is.  Out of place out may be M3_F16 / M3_BF16 (one rounding).
 * 16-byte accesses where x and out are 16-byte aligned and W % 4 == 0.
 * m3_mix_target: the dense soft target [B,C] f32 of the same pairing: t_i = lam_i s(y_i) + (1 - lam_i) s(y_j), s(y) = off =
 * smoothing / C everywhere and 1 - smoothing + off at y.  label int64 [B]; a label outside [0, C) adds only the off floor and
 * is counted in *n_bad (DEVICE int32, written). */
int m3_mix_batch(const float *x, int B, int C, int H, int W, const float *lam, const int32_t *box, void *out, int out_dtype,
                 void *stream);
int m3_mix_target(const int64_t *label, const float *lam, int B, int C, double smoothing, float *target, int32_t *n_bad,
                  void *stream);
/* Cross-entropy of row-major logits [B,C] (M3_F32 / M3_F16 / M3_BF16), 1 <= C <= M3_SOFTCE_MAX_C, B*C < 2^31 - 2^20, against
 * EXACTLY ONE of (pretrain/models/losses.py:77-83: SoftTargetCrossEntropy, LabelSmoothingCrossEntropy, nn.CrossEntropyLoss):
 *   target f32 [B,C]: loss = (1/B) sum_i [ S_i lse(x_i) - sum_c t_ic x_ic ], S_i = sum_c t_ic (= sum(-t log_softmax(x)); right
 *     for rows that do not sum to 1 or are all zero); smoothing is not read;
 *   label int64 [B]:  loss = (1/B) sum_i [ lse(x_i) - (1 - s) x_i[y_i] - (s / C) sum_c x_ic ], s = smoothing (0: plain cross-
 *     entropy, pretrain/engine/evaluate.py:12,29).  A label outside [0, C) indexes nothing (its row adds lse - (s / C) sum x)
 *     and is counted in the record's N_BAD.
 * lse f32 [B] (running maximum: finite at |x| = 6e4) and, for a dense target, tsum f32 [B] = S_i are written by the forward and
 * read by the backward (tsum may be NULL with labels).  ws: m3_softce_ws_elems(B) floats, no initialisation.  record: the
 * M3_LOSS_REC_WORDS words of the dense-prediction losses (VALUE the loss, COEF 1 / B, N_VALID B, N_BAD).  Forward: one
 * workgroup per row, then one workgroup that adds the rows in order in double.
 * Backward: dlogits (the logits' dtype) = (softmax(x_i)_c S_i - t_ic) * COEF * *grad_out (DEVICE f32: a loss scale needs no
 * host read); with labels t is the implied target and S_i = 1.  16-byte accesses where C % 4 == 0 and logits / target / dlogits
 * are 16-byte aligned. */
#define M3_SOFTCE_MAX_C 65536
int64_t m3_softce_ws_elems(int B);
int m3_loss_softce_fwd(const void *logits, int dtype, const float *target, const int64_t *label, double smoothing, int B,
                       int C, float *lse, float *tsum, float *ws, void *record, void *stream);
int m3_loss_softce_bwd(const void *logits, int dtype, const float *target, const int64_t *label, double smoothing,
                       const float *lse, const float *tsum, const void *record, const float *grad_out, int B, int C,
                       void *dlogits, void *stream);
/* The teacher term of the distillation loss (pretrain/models/losses.py:50-68) on the student's distillation logits [B,C] and the
 * teacher's logits [B,C], each M3_F32 / M3_F16 / M3_BF16 with a dtype code of its own (a teacher under autocast returns 16 bits
 * while the student's head returns fp32); 1 <= C <= M3_SOFTCE_MAX_C, B*C < 2^31 - 2^20, finite inputs.
 *   M3_DISTILL_SOFT: loss = tau^2 / (B C) sum_i [ sum_c q_ic (t_ic - x_ic) / tau - lse(t_i / tau) + lse(x_i / tau) ], q =
 *     softmax(t / tau): kl_div(log_softmax(x / tau), log_softmax(t / tau), "sum", log_target) tau^2 / numel (:53-60).
 *     COEF = tau / (B C);  dlogits = (softmax(x / tau) - q) * COEF * *grad_out.
 *   M3_DISTILL_HARD: loss = (1 / B) sum_i [ lse(x_i) - x_i[y_i] ], y_i = argmax_c t_ic, ties to the lowest index
 *     (m3_cls_eval_update's rule) - cross_entropy(x, t.argmax(1)) (:61-64); tau is not read.
 *     COEF = 1 / B;  dlogits = (softmax(x_i) - onehot(y_i)) * COEF * *grad_out.
 * Both lse values use running maxima (finite at |x| / tau = 6e4).  The forward writes per row lse f32 [B], the student's, and aux,
 * B four-byte words: the teacher's lse (f32, soft) or y_i (int32, hard); the backward reads them and, hard, not the teacher's
 * logits (teacher may be NULL there).  ws: m3_distill_ws_elems(B) floats, no initialisation.  record: the M3_LOSS_REC_WORDS
 * words (VALUE, COEF, N_VALID B).  Forward: one workgroup per row, then one workgroup that adds the rows in order in double; no
 * float atomics, nothing read back, the same bits from run to run.  grad_out: DEVICE f32.  dlogits has the logits' dtype.
 * 16-byte accesses where logits / teacher / dlogits are 16-byte aligned and C % 4 == 0 (both fp32) or C % 8 == 0 (one of them
 * 16-bit); the scalar path otherwise. */
#define M3_DISTILL_SOFT 0
#define M3_DISTILL_HARD 1
int64_t m3_distill_ws_elems(int B);
int m3_loss_distill_fwd(const void *logits, int dtype, const void *teacher, int teacher_dtype, int kind, double tau, int B, int C,
                        float *lse, void *aux, float *ws, void *record, void *stream);
int m3_loss_distill_bwd(const void *logits, int dtype, const void *teacher, int teacher_dtype, int kind, double tau,
                        const float *lse, const void *aux, const void *record, const float *grad_out, int B, int C,
                        void *dlogits, void *stream);
/* One batch of the evaluation loop (pretrain/engine/evaluate.py:29-37) ADDED to state, M3_CLS_EVAL_WORDS 8-byte words: f64
 * LOSS_SUM, CORRECT1, CORRECT5, COUNT - the vector evaluate.py:44-50 all-reduces - then int64 N_BAD.  Per row the plain cross-
 * entropy lse - x[y] and rank = #{c : x_c > x_y} + #{c < y : x_c == x_y} (ties to the lower index; a NaN logit beats every
 * number and the first NaN wins); CORRECT1 += [rank < 1], CORRECT5 += [rank < min(5, C)].  A label outside [0, C) counts in
 * COUNT and N_BAD, adds lse to LOSS_SUM and is never correct.  ws: m3_cls_eval_ws_elems(B) four-byte words. */
#define M3_CLS_EVAL_LOSS_SUM 0
#define M3_CLS_EVAL_CORRECT1 1
#define M3_CLS_EVAL_CORRECT5 2
#define M3_CLS_EVAL_COUNT 3
#define M3_CLS_EVAL_N_BAD 4
#define M3_CLS_EVAL_WORDS 5
int64_t m3_cls_eval_ws_elems(int B);
int m3_cls_eval_update(const void *logits, int dtype, const int64_t *label, int B, int C, void *ws, void *state, void *stream);
/* The weight EMA behind every step (pretrain/engine/train_one_epoch.py:62-63): ema = decay ema + one_minus_decay src for all
 * tensors of an m3_optim_desc table in one launch - p the fp32 shadow, g the fp32 source, n, chunk_start and vec_ok as for
 * m3_optim_step; m, v and group are not read.  Both factors are formed by the host in double.  decay 1 writes nothing, decay 0
 * copies the source's bits. */
int m3_ema_update(const m3_optim_desc *descs_dev, int n_desc, int total_chunks, float decay, float one_minus_decay,
                  void *stream);

/* ------------------------------------------------------------- dense-prediction augmentation
 * The per-sample transform chain of the multi-task trainer (utils/common_config.py:583-632: RandomHorizontalFlip, ScaleNRotate,
 * FixedResize, AddIgnoreRegions, ToTensor, Normalize of data/custom_transforms.py:18-82,88-138,174-191,243-318; the batch
 * reaches the step at train/train_utils.py:362-368) for every map of a raw batch in ONE launch: flip, warp and resize composed
 * into one resampling, then the map kind's post-operation, stored NCHW.  Nothing is read back; the same bits from run to run.
 *
 * descs: a HOST array of n_maps <= M3_AUG_MAX_MAPS descriptors, passed to the kernel by value.  src [B,H,W,C] ([B,H,W] for
 * C = 1), contiguous, src_dtype M3_F32 or M3_AUG_U8; dst [B,C,Ho,Wo] contiguous, fp32 (an M3_AUG_IMAGE map: fp32 / fp16 / bf16).
 * All maps share B, H, W, Ho, Wo and border.  mats: DEVICE f64 [B,6] = a00 a01 a02 a10 a11 a12, the map from an output pixel
 * (x, y) to source coordinates, u = (a00 x + a01 y) + a02, v = (a10 x + a11 y) + a12, evaluated in double with every product and
 * sum rounded on its own (no fused multiply-add) in exactly that association.  aux: DEVICE f32 [B,4] = sc, cos(rot), sin(rot),
 * flip (non-zero: flipped).
 * mode M3_AUG_NEAREST: the tap (floor(u + 0.5), floor(v + 0.5)), a bit copy.  M3_AUG_LINEAR: x0 = floor(u), t = (float)(u - x0),
 * weights 1 - t, t.  M3_AUG_CUBIC: taps x0 - 1 .. x0 + 2, the Keys kernel with a = -0.75 (cv2.INTER_CUBIC), weights in fp32 from
 * t.  t == 0 on an axis gives exactly the weights (1, 0) / (0, 1, 0, 0); a tap of weight zero is not read.  border
 * M3_AUG_BORDER_ZERO: a tap outside the source is 0 (cv2.warpAffine's default); M3_AUG_BORDER_REPLICATE: its index is clamped
 * (cv2.resize).  The weighted sum runs in fp32.
 * kind M3_AUG_IMAGE (C 3): with quantize, q = trunc(clamp(v, 0, 255)) (ToTensor's astype(uint8), clamped where numpy wraps),
 * then (q / 255 - mean[c]) / std[c].  M3_AUG_LABEL (C 1): nothing more.  M3_AUG_DEPTH (C 1): v / sc, then 0 becomes 255
 * (custom_transforms.py:77-78,264-266).  M3_AUG_NORMALS (C 3): channel 0 negated when flipped (:188-189), (n0, n1) rotated,
 * n0' = n0 cos + n1 sin, n1' = n1 cos - n0 sin (:67-73), n / (|n|_2 + 2^-23) (:131-134), and all three channels 255 where
 * |n|_2 == 0 (:251-256).  The per-sample "no human part anywhere => all 255" rule (:258-262) is not built.
 * Refused (M3_ERR_ARG, nothing launched): n_maps outside [1, M3_AUG_MAX_MAPS]; B, H, W, Ho, Wo < 1; a C that is not the kind's;
 * a uint8 label, depth or normals map resampled other than nearest, a 16-bit output of another kind than the image, a
 * non-positive std; a map of 2^31 - 2^20 elements or more. */
#define M3_AUG_MAX_MAPS 8
#define M3_AUG_U8 3
#define M3_AUG_IMAGE 0
#define M3_AUG_LABEL 1
#define M3_AUG_DEPTH 2
#define M3_AUG_NORMALS 3
#define M3_AUG_NEAREST 0
#define M3_AUG_LINEAR 1
#define M3_AUG_CUBIC 2
#define M3_AUG_BORDER_ZERO 0
#define M3_AUG_BORDER_REPLICATE 1
typedef struct m3_augment_desc {
  void *src; void *dst;
  int32_t kind, mode, C, src_dtype, dst_dtype, quantize;
  float mean[3], std[3];
} m3_augment_desc;
int m3_augment_batch(const m3_augment_desc *descs, int n_maps, int B, int H, int W, int Ho, int Wo, int border,
                     const double *mats, const float *aux, void *stream);

/* ---------------------------------------------------------------------------------------------------- token sharing stage
 * The persistent-sharing stage of a TokenBlock (models/moe/token/vision_transformer_moe.py:873-959): ShareabilityPredictor,
 * transition_stage and apply_shared_broadcast as one row pass over the positions p in [0, P = B*N) of T task tensors, its
 * backward, the predictor alone, the masked mean of Aggregation / AggregationStage, and one small launch for the index
 * compaction and the integer statistics.  No host read, no atomics; the same bits from run to run.
 *
 * Task tensors: T separate contiguous [P, D] allocations in the activation dtype, handed over as a table of device
 * addresses (m3_share_rows, filled by the host); nothing is stacked or copied.  Limits, refused and never worked around:
 * 2 <= T <= M3_SHARE_MAX_T (M3_ERR_UNSUPPORTED); D a multiple of 8 in [8, M3_SHARE_MAX_D] (M3_ERR_UNSUPPORTED: a lane owns
 * the 8-element chunks lane and lane + 64 of a row); Dg >= 0, P < 2^31, 16-byte aligned tensors (M3_ERR_ARG).
 *
 * m3_share_stage_fwd, per position and task t:  logits = [x_t[p] | task_emb[t]] @ w_gate (+ noise[t][p], the caller's Gumbel
 * draws; NULL = none), w_gate f32 [D + Dg][2] in the parameter's layout, task_emb f32 [T][Dg] (NULL with Dg = 0), noise f32
 * [T][P][2];  soft = softmax(logits / tau)[1];  G = soft, or the one-hot's second entry when hard (soft is then written
 * too: the backward's straight-through gradient needs it; soft may be NULL otherwise).  M_t = G_t >= gamma, cleared where
 * fewer than two tasks agree; shared_bits[p] bit t = M_t;  W_t = G_t M_t / (sum_s G_s M_s + eps);  shared_x[p] = sum_t W_t
 * x_t[p] into the DENSE [P][D] buffer (zero rows where bits == 0);  y_t[p] = M_t ? shared_x[p] : x_t[p] (the row's own
 * bits).  g, soft: f32 [T][P].
 * m3_share_stage_bwd: from d y_t (a NULL entry = zeros), d shared_x (dense, NULL = zeros) and d g (f32 [T][P], NULL =
 * zeros) to d x_t, d w_gate [D + Dg][2] and d task_emb [T][Dg] (both overwritten).  ws: m3_share_bwd_ws_elems floats, no
 * initialisation: one partial row per workgroup, added in a fixed order by a second launch.
 * m3_share_predict_fwd / _bwd: the predictor of ONE tensor (task_emb f32 [Dg], noise f32 [P][2], g / soft / d_g f32 [P]),
 * the stage's own code for logits and G.
 * m3_share_aggregate_fwd: v = (bits of mask_bits[p] below T) where agg_needed[p] (one byte per position; NULL = everywhere);
 * agg[p] = sum_{s in v} x_s[p] / (|v| + eps) (dense, optional, zero rows where v is empty);  y_t[p] = v_t ? agg[p] : x_t[p].
 * m3_share_aggregate_bwd: d x_s = v_s (d agg + sum_{t in v} d y_t) / (|v| + eps) + (1 - v_s) d y_s.
 * m3_share_compact (one workgroup, M3_SHARE_SCAN_WIDTH positions per step of its scan): shared_flat_idx i32 [P] = the flat
 * indices with bits != 0, ascending, the tail -1 (NULL: not wanted); count i32 [1] (NULL: not wanted); stats i64
 * [M3_SHARE_STAT_WORDS] at the M3_SHARE_STAT_* words: POSITIONS, TASKTOKENS (set bits), PARTIAL (positions shared by some
 * but not all T tasks) of PARTIAL_TOTAL = P, FLIPS (positions whose bits differ from prev_shared_bits) of FLIP_TOTAL (P, or
 * 0 without prev_shared_bits), and the sharing regulariser's S (= POSITIONS) and S_T + t (positions with bit t, t < T). */
#define M3_SHARE_MAX_T 8
#define M3_SHARE_MAX_D 1024
#define M3_SHARE_MAX_BLOCKS 1024
#define M3_SHARE_SCAN_WIDTH 1024
#define M3_SHARE_STAT_POSITIONS 0
#define M3_SHARE_STAT_TASKTOKENS 1
#define M3_SHARE_STAT_PARTIAL 2
#define M3_SHARE_STAT_PARTIAL_TOTAL 3
#define M3_SHARE_STAT_FLIPS 4
#define M3_SHARE_STAT_FLIP_TOTAL 5
#define M3_SHARE_STAT_S 6
#define M3_SHARE_STAT_S_T 8
#define M3_SHARE_STAT_WORDS 16
typedef struct m3_share_rows { void *p[M3_SHARE_MAX_T]; } m3_share_rows;
int m3_share_num_blocks(int64_t P);
int64_t m3_share_bwd_ws_elems(int64_t P, int T, int D, int Dg);
int m3_share_stage_fwd(const m3_share_rows *x, int dtype, int T, int64_t P, int D, const float *w_gate,
                       const float *task_emb, int Dg, const float *noise, float tau, int hard, float gamma, float eps,
                       const m3_share_rows *y, void *shared_x, int64_t *shared_bits, float *g, float *soft, void *stream);
int m3_share_stage_bwd(const m3_share_rows *x, int dtype, int T, int64_t P, int D, const float *w_gate,
                       const float *task_emb, int Dg, float tau, float eps, const int64_t *shared_bits, const float *g,
                       const float *soft, const void *shared_x, const m3_share_rows *dy, const void *d_shared_x,
                       const float *d_g, const m3_share_rows *dx, float *ws, float *d_w_gate, float *d_task_emb, void *stream);
int m3_share_predict_fwd(const void *x, int dtype, int64_t P, int D, const float *w_gate, const float *task_emb, int Dg,
                         const float *noise, float tau, int hard, float *g, float *soft, void *stream);
int m3_share_predict_bwd(const void *x, int dtype, int64_t P, int D, const float *w_gate, const float *task_emb, int Dg,
                         float tau, const float *g, const float *soft, const float *d_g, void *dx, float *ws,
                         float *d_w_gate, float *d_task_emb, void *stream);
int m3_share_aggregate_fwd(const m3_share_rows *x, int dtype, int T, int64_t P, int D, const int64_t *mask_bits,
                           const void *agg_needed, float eps, const m3_share_rows *y, void *agg, void *stream);
int m3_share_aggregate_bwd(const m3_share_rows *dy, int dtype, int T, int64_t P, int D, const int64_t *mask_bits,
                           const void *agg_needed, float eps, const void *d_agg, const m3_share_rows *dx, void *stream);
int m3_share_compact(const int64_t *shared_bits, const int64_t *prev_shared_bits, int64_t P, int T, int32_t *shared_flat_idx,
                     int32_t *count, int64_t *stats, void *stream);

/* ------------------------------------------------------------------------------------- token blocks: the FFN sublayer
 * Step 5 of TokenBlock.forward (models/moe/token/vision_transformer_moe.py) for the blocks that need no router, over the
 * rows that differ only: the private rows of every task and ONE row per shared position.
 *   mode M3_TOKEN_FFN_ALL     the dense block: dense_mlp_stage(outs, shared_bits), shared_dense_forward(shared_x),
 *                             apply_shared_broadcast (:443-515, :966-984) - private and shared rows, one weight set
 *   mode M3_TOKEN_FFN_SHARED  the shared branch of an MoE block: shared_x + drop_path(shared_ffn(norm2(shared_x))), then the
 *                             broadcast (:1002-1014) - shared rows only, private rows pass through
 * With private(t, p) = bit t of bits[p] clear and F(v) = fc2(gelu(fc1(LayerNorm(v)))):
 *   shared_out[p] = shared_x[p] + shared_path_scale[p] * F(shared_x[p])         where bits[p] != 0
 *   y_t[p]        = x_t[p] + path_scale[p / N] * F(x_t[p])                      where private(t, p), mode ALL
 *   y_t[p]        = x_t[p] (its own bits)                                       where private(t, p), mode SHARED
 *   y_t[p]        = shared_out[p]                                               where bit t of bits[p] is set
 * Dense form: no early return, no nonzero(), no host read; the row count R stays on the device and every buffer and launch
 * is sized by the bound m3_token_ffn_rows_ub = T * P (ALL) or P (SHARED): a position whose word has at most one bit set
 * contributes T rows, any other T - popcount + 1 <= T - 1.  Task tensors are m3_share_rows tables as in the sharing stage;
 * the same limits (2 <= T <= M3_SHARE_MAX_T, D a multiple of 8 in [8, M3_SHARE_MAX_D]: M3_ERR_UNSUPPORTED) and
 * (T + 1) * P < 2^31 (M3_ERR_ARG).  Bits of a word at and above T are ignored.  No atomics: the same bits from run to run.
 *
 * m3_token_ffn_worklist: work row r of segment seg <= T at position p has the entry rows[r] = seg * P + p; segment t < T
 *   lists the private positions of task t (mode ALL; empty in mode SHARED), segment T the positions with bits != 0;
 *   segment-major, ascending p.  rows i32 [M_ub]: entries [0, R) are written, the rest is left alone.  slot_of i32 [T + 1][P]:
 *   the inverse, -1 for a (segment, position) that is not listed.  offsets, tile_starts i32 [2] = {0, R}, {0, ceil(R / 128)}:
 *   exactly what m3_route_build writes for one group (it is what writes them), so m3_gemm_nt / m3_wgrad_tn take them as
 *   group_offsets / tile_starts with G = 1.  count i32 [1] = R.  ws i32 [m3_token_ffn_list_ws_elems(P, T)], no initialisation.
 * m3_token_ffn_ln_fwd (norm2 of the listed rows, gathered): h[r] = LayerNorm(source row of work row r) * gamma + beta into
 *   the compact [M_ub][D] buffer (activation dtype), mean / rstd f32 [M_ub]; two-pass variance in fp32.  Rows at and past
 *   count are neither read nor written.
 * (fc1 / fc2, Mlp.forward token/layers.py: m3_gemm_nt with G = 1 and the work list's offsets.)
 * m3_token_ffn_scatter_fwd (the residual adds of dense_mlp_stage / shared_dense_forward and apply_shared_broadcast): one
 *   pass over the positions writes every y_t[p] by the formulas above from x_t, shared_x, f [M_ub][D] = F of the work rows,
 *   slot_of and the DropPath factors path_scale f32 [P / N] (the reference's one mask per block and sample) and
 *   shared_path_scale f32 [P] (its DropPath over the compact [K, C] tensor: per shared row); NULL = 1.
 * m3_token_ffn_gather_bwd: d f[r] = path_scale * d y_t[p] for a private row, shared_path_scale[p] * (sum over the set bits,
 *   t ascending, of d y_t[p]) for a shared row, rounded once to the activation dtype; rows at and past count untouched.
 * m3_token_ffn_scatter_bwd: from d h [M_ub][D] (the gradient at the LayerNorm's output: fc1's dgrad) writes every
 *   d x_t[p] = d y_t[p] (+ the LayerNorm backward of d h[slot] where the row is listed), EXACT zero where the broadcast
 *   overwrote the row, and d shared_x[p] = sum over the set bits of d y_t[p] + the LayerNorm backward of its d h row, exact
 *   zero where bits[p] == 0; d_gamma, d_beta f32 [D] (overwritten) from one partial row per workgroup added in a fixed order
 *   by a second launch.  ws f32 [m3_token_ffn_bwd_ws_elems(P, D)], no initialisation. */
#define M3_TOKEN_FFN_ALL 0
#define M3_TOKEN_FFN_SHARED 1
int64_t m3_token_ffn_rows_ub(int64_t P, int T, int mode);
int64_t m3_token_ffn_list_ws_elems(int64_t P, int T);
int64_t m3_token_ffn_bwd_ws_elems(int64_t P, int D);
int m3_token_ffn_worklist(const int64_t *bits, int64_t P, int T, int mode, int32_t *rows, int32_t *slot_of,
                          int32_t *offsets, int32_t *tile_starts, int32_t *count, int32_t *ws, void *stream);
int m3_token_ffn_ln_fwd(const m3_share_rows *x, const void *shared_x, int dtype, int T, int64_t P, int D,
                        const int32_t *rows, const int32_t *count, int64_t M_ub, const float *gamma, const float *beta,
                        float eps, void *h, float *mean, float *rstd, void *stream);
int m3_token_ffn_scatter_fwd(const m3_share_rows *x, const void *shared_x, const void *f, int dtype, int T, int64_t P,
                             int N, int D, int mode, const int32_t *slot_of, const int64_t *bits, const float *path_scale,
                             const float *shared_path_scale, const m3_share_rows *y, void *stream);
int m3_token_ffn_gather_bwd(const m3_share_rows *dy, int dtype, int T, int64_t P, int N, int D, const int32_t *rows,
                            const int32_t *count, int64_t M_ub, const int64_t *bits, const float *path_scale,
                            const float *shared_path_scale, void *df, void *stream);
int m3_token_ffn_scatter_bwd(const m3_share_rows *x, const void *shared_x, const m3_share_rows *dy, const void *dh,
                             const float *mean, const float *rstd, int dtype, int T, int64_t P, int D, int mode,
                             const int32_t *slot_of, const int64_t *bits, const float *gamma, const m3_share_rows *dx,
                             void *d_shared_x, float *ws, float *d_gamma, float *d_beta, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* M3VIT_HIP_H */
