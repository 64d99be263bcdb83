/*
 * libwan_hip.so -- C ABI of the MI355X (gfx950) kernels behind the Wan2.1-DiT
 * video denoising path of VideoCoF.
 *
 * The reference is pure Python; it has no FFI.  Its seams are the duck-typed
 * calls listed in SURVEY.md section 8b -- WanTransformer3DModel.forward,
 * attention(), WanRMSNorm.forward, rope_apply_qk -- which the closed `paifuser`
 * package monkey-patches with native code (videox_fun/models/__init__.py:43-109).
 * Each entry point below replaces the arithmetic of one such seam and cites it
 * (file:line relative to the reference root).  INTEGRATION.md shows the ctypes
 * binding a maintainer would add on the reference side.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers;
 *   - the caller owns every buffer (PyTorch caching allocator in practice); the
 *     library keeps no state between calls except the last-error string;
 *   - every call enqueues on `stream` (a hipStream_t passed as void*) and
 *     returns without synchronising;
 *   - bf16 tensors are `void*` to 2-byte bfloat16, fp32 tensors are `float*`;
 *   - `ld*` are row strides in ELEMENTS; rows are contiguous in the last dim;
 *   - return value 0 = WAN_OK, otherwise see wan_last_error().
 */
#ifndef WAN_HIP_H
#define WAN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WAN_ABI_VERSION 11     /* 11: wan_gemm_fp8_ws / wan_gemm_fp8_ws_plan / wan_gemm_fp8_pk_segment (the e4m3 Linear on the persistent stream-K kernel); 10: wan_box_probe (the benchmark's box fingerprint); 9: wan_attention_fwd_varlen (ragged batches in one launch); 8: wan_qk_quantize_fp8 takes either operand alone, wan_gemm_ws_splits + the split-K form of the 128^2 GEMM, tuning key gemm_pk_form replaces gemm_pk_sched (and attn_w4 is gone with the 8-wave attention kernel), the persistent GEMM from K >= 1024, the library communicator records collectives on a capturing stream; 7: the *_split wire entry points (Ulysses head groups); 6: wan_gemm_bf16_ws / wan_gemm_workspace_bytes / wan_gemm_ws_plan (persistent stream-K GEMM with a caller workspace); 5: the fp8 attention family */

typedef enum {
    WAN_OK = 0,
    WAN_ERR_INVALID = 1,     /* bad shape / alignment / null pointer (Python side raises ValueError) */
    WAN_ERR_UNSUPPORTED = 2, /* shape the kernels do not cover (RuntimeError) */
    WAN_ERR_LAUNCH = 3       /* HIP launch failure (RuntimeError) */
} wan_status_t;

int wan_abi_version(void);
const char* wan_last_error(void);

/* Developer switches (A/B harnesses, bring-up).  The matching environment variables (WAN_ATTN_TAIL, WAN_ATTN_FAST,
 * WAN_ATTN_XCD_MAP, WAN_ATTN_REF, WAN_GEMM_W4, WAN_GEMM_GM, WAN_GEMM_PHASES, WAN_GEMM_VARIANT, WAN_CONV_XCD, WAN_DEBUG_CHECKS, WAN_ATTN_PERSIST) are
 * read ONCE, at the first call into the library; the launch paths never call getenv().  Keys: "attn_tail",
 * "attn_fast", "attn_xcd_map", "attn_ref", "conv_head", "gemm_exp", "gemm_w4", "gemm_gm", "gemm_phases", "gemm_variant", "conv_xcd", "debug_checks",
 * "gemm_pk", "gemm_pk_form", "gemm_pk_workers", "gemm_pk_min_units", "gemm_pk_order", "gemm_splitk", "row_group", "sp_inline", "sp_reserve_cus", "conv_patch", "attn_persist" (1: cross-attention on the persistent form of the 4-wave kernel), "conv_mfma" (0 = by the per-frame plane, 32 / 16 = force v_mfma_f32_32x32x16_bf16 / v_mfma_f32_16x16x32_bf16).
 * "sp_reserve_cus" (WAN_SP_RESERVE_CUS, default 0): CUs left free for communication kernels that run on another stream beside the
 * persistent grids.  When > 0, every grid that is "one resident workgroup per CU" -- the persistent stream-K GEMM's (unless
 * "gemm_pk_workers" names a grid explicitly) and the persistent cross-attention form's -- sizes itself from CU count - sp_reserve_cus
 * (rounded down to a multiple of 8, at least 8) instead of the CU count; wan_gemm_workspace_bytes / wan_gemm_pk_grid /
 * wan_gemm_pk_segment follow.  Another worker count moves the stream-K cut points, so results are equal to those at 0 within the
 * kernels' tolerances, not bit for bit.  0 leaves every plan as it is.
 * "debug_checks" = 1 turns on SYNCHRONISING contract checks (V^T pad columns of wan_attention_fwd are finite).
 * wan_set_tuning is an atomic store: safe against concurrent launches, which see the old or the new value.
 * wan_get_tuning returns -1 for an unknown key.  No reference counterpart (the reference has no native code).
 * Read-only key "last_attn_variant": what the most recent wan_attention_fwd call of this process launched, as
 * WAN_ATTN_VARIANT_* (kernel family | WAN_ATTN_VARIANT_XCD_PINNED | WAN_ATTN_VARIANT_SPLIT_TAIL | WAN_ATTN_VARIANT_SPARSE) -- so that a benchmark
 * reports the kernel the dispatcher picked instead of a literal.  Read-only key "dev_experiments": 1 if the library was built with
 * `make EXPERIMENTS=1` (the timing-only instruments of the persistent GEMM behind "gemm_exp" -- cycle stamps, forced waits -- compiled
 * in; never in the product build: there "gemm_exp" does nothing).
 * "cross_fold" (WAN_CROSS_FOLD, default 1): the folded cross-attention branch of wan_dit_block_tail_forward (a9f below): 0 never,
 * 1 by wan_cross_fold_plan's rule, 2 wherever the kernels are legal.  Read-only key "last_cross_fold": 1 if the most recent
 * wan_dit_block_tail_forward of this process ran the folded branch, else 0. */
wan_status_t wan_set_tuning(const char* key, int value);
int wan_get_tuning(const char* key);
#define WAN_ATTN_VARIANT_W4_LAZY 1          /* attn_fwd_w4_kernel<.,.,1|2>: 4 waves, lazy softmax reference, one launch */
#define WAN_ATTN_VARIANT_W4_MAXFREE 2       /* attn_fwd_w4_kernel<.,false,0> + its checked fix-up launch attn_fwd_w4_kernel<.,false,1,true> */
#define WAN_ATTN_VARIANT_W8_RUNNING_MAX 3   /* (rounds 1-4: the 8-wave running-max kernel; retired in round 5, never reported any more) */
#define WAN_ATTN_VARIANT_W4_LAZY_QK8 4      /* attn_fwd_w4_kernel<0,.,1,false,true>: the lazy form with QK^T on the fp8 matrix pipe (wan_attention_fwd_qk8) */
#define WAN_ATTN_VARIANT_W4_F8 5            /* attn_fwd_f8_kernel (fp8 QK^T and fp8 P.V, checked max-free softmax) + the fp8-QK^T lazy kernel on flagged workgroups (wan_attention_fwd_f8) */
#define WAN_ATTN_VARIANT_FAMILY_MASK 15
#define WAN_ATTN_VARIANT_XCD_PINNED 16      /* every (batch, head) pinned to one XCD */
#define WAN_ATTN_VARIANT_SPLIT_TAIL 32      /* the last partial round ran split over the keys (+ merge kernel) */
#define WAN_ATTN_VARIANT_SPARSE 64          /* listed key tiles per query block (wan_attention_fwd_sparse): the lazy form's SPARSE instantiation */

/* ---------------------------------------------------------------------------
 * a4  LayerNorm (no affine) + adaLN modulate, or LayerNorm with affine.
 *     out[r,c] = bf16( LN(x[r,:])[c] * (add_one + scale[b,c]) + shift[b,c] ),  b = r / rows_per_batch
 *     replaces: WanLayerNorm.forward + `norm(x) * (1 + e[1]) + e[0]` then `.to(dtype)`
 *               (wan_transformer3d.py:233-243, 495-496, 507-508, 547) with add_one=1,
 *               and norm3 = LayerNorm(affine) (wan_transformer3d.py:448-450, 504) with
 *               add_one=0, scale=weight, shift=bias, rows_per_batch=rows.
 *     x fp32 [rows, dim] contiguous; scale/shift fp32 [nbatch, dim]; dim % 4 == 0, dim <= 8192.
 * ------------------------------------------------------------------------- */
wan_status_t wan_ln_modulate(const float* x, const float* scale, const float* shift, int add_one,
                             void* out_bf16, int64_t rows, int dim, int64_t rows_per_batch,
                             float eps, void* stream);

/* ---------------------------------------------------------------------------
 * a5+a7  WanRMSNorm over the FULL channel dim, then 3-axis RoPE with the
 *     VideoCoF temporal position map, in place on bf16 rows.
 *     replaces: WanRMSNorm.forward (wan_transformer3d.py:214-230) followed by
 *               rope_apply_qk (wan_transformer3d.py:135-211); the paifuser patch points
 *               are models/__init__.py:78-80 (rms_norm_forward) and :85-109 (fast_rope_apply_qk).
 *     One launch handles two tensors (q and k); pass x1 = NULL for a single tensor.
 *     rope_cos/rope_sin: fp32 [max_pos, head_dim/2] tables (cos/sin of the angles of
 *     rope_params, wan_transformer3d.py:44-52, 692-699); NULL = RMSNorm only (cross-attention).
 *     Row r of the call is token  t = token_offset + (r % rows_per_batch)  of its sample;
 *     tokens >= F*Hp*Wp are normalised but not rotated (wan_transformer3d.py:202).
 *     mode 0: pos_t = f;  mode 1 (paired): f < f_src ? f : f - f_src;
 *     mode 2 (CoF): f < f_src ? f+1 : (f < ground_end ? 0 : f - ground_end + 1).
 *     x0_scale multiplies the x0 result in fp32 before its single bf16 rounding (x1 is not scaled).
 *     Pass WAN_ATTN_QSCALE(softmax_scale) to hand q to wan_attention_fwd(WAN_ATTN_Q_PRESCALED)
 *     -- the `q * softmax_scale` of flash attention folded into the norm -- or 1.0f for none.
 * ------------------------------------------------------------------------- */
typedef struct {
    int F, Hp, Wp;          /* patch grid (frames, rows, cols) */
    int mode;               /* 0 default, 1 paired, 2 CoF */
    int f_src;              /* frame_split_indices[b] */
    int ground_end;         /* ground_frame_indices[b][1] (mode 2) */
    int64_t token_offset;   /* first token of this shard (sequence parallel), else 0 */
    int64_t rows_per_batch; /* rows per sample in this call */
    int max_pos;            /* rows of the cos/sin tables (1024) */
} wan_rope_params;

wan_status_t wan_rmsnorm_rope(void* x0_bf16, const float* w0, void* x1_bf16, const float* w1,
                              int64_t ld, int64_t rows, int dim, int head_dim, float eps,
                              const float* rope_cos, const float* rope_sin,
                              const wan_rope_params* rp, float x0_scale, void* stream);

/* ---------------------------------------------------------------------------
 * a8/a10/a12  nn.Linear on the MFMA cores:  acc[m,n] = sum_k A[m,k] * W[n,k]   (fp32 accumulate)
 *     replaces: nn.Linear -> cuBLAS for q/k/v/o, ffn.0/ffn.2, text_embedding, patch_embedding
 *               (as im2col GEMM) and head.head (wan_transformer3d.py:264-267, 457-459, 662-666, 530).
 *     A bf16 [M,K] (row stride lda), W bf16 [N,K] (nn.Linear layout, row stride ldw),
 *     bias fp32 [N] or NULL.  K % 64 == 0, lda/ldw % 8 == 0.  M, N arbitrary (N % 4 == 0).
 *     Epilogues:
 *       WAN_EPI_BF16        out bf16 [M,N](ldo)  = acc + bias
 *       WAN_EPI_GELU_BF16   out bf16             = gelu_tanh(acc + bias)     (ffn.0 + nn.GELU('tanh'))
 *       WAN_EPI_F32         out fp32             = acc + bias
 *       WAN_EPI_RESID_F32   out fp32 (in place)  += (acc + bias) * gate[b,n]  (gate NULL = 1):
 *                           `x = x + y * e[2]`, `x = x + cross_attn(...)`, `x = x + y * e[5]`
 *                           (wan_transformer3d.py:499, 504, 511); gate fp32 [nbatch, N], b = m / rows_per_batch
 *       WAN_EPI_BF16_T      out bf16 [N, ldo] TRANSPOSED: out[n, m] = acc + bias  (V^T for the
 *                           attention kernel; ldo >= M, ldo % 4 == 0).  Columns [M, ldo) of every row are
 *                           NOT written by any kernel family: a caller that hands the result to
 *                           wan_attention_fwd zeroes [M, roundup(M, 64)) once (that kernel needs them finite)
 * ------------------------------------------------------------------------- */
typedef enum {
    WAN_EPI_BF16 = 0,
    WAN_EPI_GELU_BF16 = 1,
    WAN_EPI_F32 = 2,
    WAN_EPI_RESID_F32 = 3,
    WAN_EPI_BF16_T = 4
} wan_epilogue_t;

wan_status_t wan_gemm_bf16(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                           void* out, int64_t ldo, int M, int N, int K, int epilogue,
                           const float* gate, int64_t rows_per_batch, void* stream);
/* Host arithmetic only: the kernel family wan_gemm_bf16 dispatches an [M, K] x [N, K]^T product to. */
int wan_gemm_plan(int M, int N, int K);
#define WAN_GEMM_VARIANT_128 0      /* gemm_bf16_kernel: 128 x 128 x 64 tile, 4 waves, two workgroups per CU (small / under-filled shapes) */
#define WAN_GEMM_VARIANT_256_W8 1   /* gemm256_kernel: 256 x 256 x 64 tile, 8 waves, phased K loop */
#define WAN_GEMM_VARIANT_256_W4 2   /* gemm_w4_kernel: the same tile, 4 waves of 128 x 128 outputs (K >= 4096 by default) */
#define WAN_GEMM_VARIANT_256_PK 3   /* gemm_pk_kernel: the 4-wave tile as ONE persistent workgroup per CU, stream-K remainder (wan_gemm_bf16_ws) */

/* The same product with a caller-provided workspace: every nn.Linear of the DiT blocks on the path
 * (wan_transformer3d.py:264-267 q/k/v/o, :457-459 ffn) runs through this entry in the Python host and in wan_dit_block_forward.
 *     With a workspace, shapes a 256^2 kernel would take (K % 128 == 0, K >= 1024) run on the PERSISTENT form: one resident workgroup per CU walks
 *     whole output tiles as one continuous K-tile stream (no per-tile pipeline fill) and the remainder tiles are cut stream-K
 *     fashion so that every CU does the same amount of work (no tail round); split tiles are combined in K order by the last
 *     arriver (bitwise reproducible, no spin waits).  Small shapes of the 128^2 kernel whose tiles do not fill the chip (M ~ 2 000
 *     tokens: BASELINE configs[0]) run that kernel SPLIT-K (ABI 8): the K range of every tile in wan_gemm_ws_splits(M, N, K) pieces,
 *     combined in split order by the last arriver -- the same guarantees.  Everything else -- and workspace == NULL -- is wan_gemm_bf16.
 *     workspace: >= wan_gemm_workspace_bytes(M, N, K) bytes (0 when the shape would not use one), 16-byte aligned, owned by the
 *     caller, not shared by launches that may run concurrently (one per stream); its contents need not survive between calls.
 *     wan_gemm_ws_plan: the kernel family wan_gemm_bf16_ws picks when given a workspace (host arithmetic only). */
wan_status_t wan_gemm_bf16_ws(const void* A, int64_t lda, const void* W, int64_t ldw, const float* bias,
                              void* out, int64_t ldo, int M, int N, int K, int epilogue,
                              const float* gate, int64_t rows_per_batch, void* workspace, int64_t workspace_bytes, void* stream);
int64_t wan_gemm_workspace_bytes(int M, int N, int K);
int wan_gemm_ws_plan(int M, int N, int K);
int wan_gemm_ws_splits(int M, int N, int K);      /* pieces per tile of the split-K form (1: not split); host arithmetic only */
/* Host arithmetic only (tests, curious hosts): the persistent kernel's plan.  wan_gemm_pk_grid: its grid (workers = one per CU,
 * a multiple of 8).  wan_gemm_pk_segment: segment `index` of worker `worker` -- evaluated by the SAME functions the kernel runs;
 * out[11] = tile m, tile n, first K tile, end K tile, partial?, workspace slot, arrival counter, first / last lane holding a piece of
 * the tile, my lane, stream-K tile index; returns 1 while the segment exists. */
int wan_gemm_pk_grid(int M, int N);
int wan_gemm_pk_segment(int M, int N, int K, int worker, int index, int* out);

/* ---------------------------------------------------------------------------
 * 8f-4  FP8 (OCP e4m3) projections -- an explicit, lossy option of the host model (`enable_fp8_linear`); never the default.
 *     replaces: the reference keeps e4m3 only as a STORAGE format and up-casts every weight to bf16 for the matmul
 *               (convert_weight_dtype_wrapper, videox_fun/utils/fp8_optimization.py:19-57).  Here both operands stay
 *               e4m3 into the matrix pipe: out = (A_q . W_q^T) * a_row_scale[m] * w_row_scale[n]  (+ bias, epilogue),
 *               A_q = e4m3(A / a_row_scale) per token row, W_q = e4m3(W / w_row_scale) per output channel.
 *     wan_gemm_fp8: same tile kernel, epilogues and argument meaning as wan_gemm_bf16; A [M,K] and W [N,K] are e4m3 bytes
 *               (lda / ldw in bytes = elements, multiples of 16), K % 128 == 0; products accumulate in fp32 on
 *               v_mfma_scale_f32_16x16x128_f8f6f4 with unit block scales (twice the bf16 MFMA rate).
 *     wan_quantize_rows_fp8: bf16 [rows, cols] -> e4m3 + one scale per row (max|x| / 448; round-to-nearest-even).
 *     wan_ln_modulate_fp8:  wan_ln_modulate with the quantisation fused into the row kernel (e4m3 out + row scales).
 * ------------------------------------------------------------------------- */
wan_status_t wan_gemm_fp8(const void* A_fp8, int64_t lda, const float* a_row_scale, const void* W_fp8, int64_t ldw,
                          const float* w_row_scale, const float* bias, void* out, int64_t ldo, int M, int N, int K,
                          int epilogue, const float* gate, int64_t rows_per_batch, void* stream);
/* wan_gemm_fp8_ws: wan_gemm_fp8 with a caller workspace (wan_gemm_fp8_workspace_bytes(M, N, K) bytes, 16-byte aligned, not shared
 * with another stream; w_row_scale 16-byte aligned).  Shapes whose bf16 product of the same TILE count would run on the persistent
 * stream-K kernel (wan_gemm_fp8_ws_plan == WAN_GEMM_VARIANT_256_PK: K % 256 == 0 and wan_gemm_ws_plan(M, N, K / 2) says so, or K >= 4096
 * and wan_gemm_ws_plan(M, N, K) does: the 8-way Ulysses shard) run its
 * e4m3 instantiation -- same segments, stream-K combine (bitwise reproducible) and epilogues, 128-element K tiles consumed by one
 * v_mfma_scale_f32_16x16x128_f8f6f4 per output tile in two phases ("schedule P", gemm_bf16_pk.hip); everything else, and a NULL
 * workspace, is wan_gemm_fp8.  wan_gemm_fp8_pk_segment: wan_gemm_pk_segment for that plan (K tiles of 128 elements). */
int wan_gemm_fp8_ws_plan(int M, int N, int K);
int64_t wan_gemm_fp8_workspace_bytes(int M, int N, int K);
wan_status_t wan_gemm_fp8_ws(const void* A_fp8, int64_t lda, const float* a_row_scale, const void* W_fp8, int64_t ldw,
                             const float* w_row_scale, const float* bias, void* out, int64_t ldo, int M, int N, int K,
                             int epilogue, const float* gate, int64_t rows_per_batch, void* workspace, int64_t workspace_bytes,
                             void* stream);
int wan_gemm_fp8_pk_segment(int M, int N, int K, int worker, int index, int* out);
wan_status_t wan_quantize_rows_fp8(const void* x_bf16, int64_t ldx, void* out_fp8, int64_t ldo, float* out_row_scale,
                                   int64_t rows, int cols, void* stream);
wan_status_t wan_ln_modulate_fp8(const float* x, const float* scale, const float* shift, int add_one, void* out_fp8,
                                 float* out_row_scale, int64_t rows, int dim, int64_t rows_per_batch, float eps, void* stream);

/* ---------------------------------------------------------------------------
 * a9  attention(): softmax(q k^T * scale) v, non-causal, head_dim 128, bf16 in/out,
 *     fp32 softmax and accumulation (flash-style, never materialises Lq x Lk).
 *     replaces: attention()/flash_attention() (attention_utils.py:43-211) as called from
 *               WanSelfAttention.forward (wan_transformer3d.py:294-299) and
 *               WanT2VCrossAttention.forward (wan_transformer3d.py:325-330).
 *     q   bf16 [B][Lq][H*128] (row stride ldq, sample stride q_bstride)
 *     k   bf16 [B][Lk][H*128]
 *     vt  bf16 [B][H*128][ldvt]  -- V TRANSPOSED: vt[h*128+d][key]; ldvt >= roundup(Lk,64),
 *         ldvt % 8 == 0, and columns [Lk, roundup(Lk,64)) must hold finite values (zeros)
 *     out bf16 [B][Lq][H*128]
 *     Keys >= Lk are masked (k_lens semantics of the flash-attn branch, attention_utils.py:95-100).
 *     flags: WAN_ATTN_Q_PRESCALED -- q already carries softmax_scale*log2(e) (written that way by
 *     wan_rmsnorm_rope's x0_scale); softmax_scale is then ignored and the softmax reference rides inside the MFMA
 *     accumulator (no per-score multiply-add).  0 = plain q: softmax_scale (> 0) is applied to the fp32 scores exactly.
 *     Numerics do not depend on the size of the scores: every form keeps a per-row softmax reference that is raised
 *     (O and the running sum rescaled) whenever a tile's row sums leave the fp32 / bf16 window.
 * ------------------------------------------------------------------------- */
wan_status_t wan_attention_fwd(const void* q, int64_t ldq, int64_t q_bstride,
                               const void* k, int64_t ldk, int64_t k_bstride,
                               const void* vt, int64_t ldvt, int64_t vt_bstride,
                               void* out, int64_t ldo, int64_t o_bstride,
                               int batch, int Lq, int Lk, int num_heads, int head_dim,
                               float softmax_scale, int flags, void* workspace, int64_t workspace_bytes,
                               void* stream);
/* The same product over a RAGGED batch in one launch: batch b attends keys [0, k_lens[b]) of its k / vt.
 *     replaces: the cu_seqlens packing of flash_attention() (attention_utils.py:95-146: k of every sample cut to k_lens[b],
 *               concatenated, one flash_attn_varlen_func call) -- here the samples stay where they are ([B][Lk][..], Lk = the
 *               padded length) and every workgroup reads ITS sample's key count: no packing copy, no host read of k_lens.
 *     k_lens  int32 [B] in DEVICE memory, read by the kernel (values are clamped to [1, Lk]; a caller that wants the
 *             reference's all-zero rows for an EMPTY sample zeroes them afterwards, as videocof_amd/attention_utils.py does)
 *     vt      columns [k_lens[b], roundup(k_lens[b], 64)) of sample b must be finite (zeros) -- the same contract per sample
 *     Everything else as wan_attention_fwd; the split-KV tail round is not used (it divides ONE key count), the max-free
 *     attempt and the XCD pinning are. */
wan_status_t wan_attention_fwd_varlen(const void* q, int64_t ldq, int64_t q_bstride,
                                      const void* k, int64_t ldk, int64_t k_bstride,
                                      const void* vt, int64_t ldvt, int64_t vt_bstride,
                                      void* out, int64_t ldo, int64_t o_bstride,
                                      int batch, int Lq, int Lk, const int32_t* k_lens, int num_heads, int head_dim,
                                      float softmax_scale, int flags, void* workspace, int64_t workspace_bytes,
                                      void* stream);
/* Optional scratch for wan_attention_fwd (16-byte aligned device memory whose first 16 bytes are ZERO when it is first used,
 * otherwise of irrelevant content; reusable across calls on one stream).  Header words (int32): [0] sticky "max-free attempt
 * off", [1] workgroups redone by the last call, [2] repair events of the lazy softmax reference since the caller last cleared
 * it (statistics).  With at least this many bytes (a) pre-scaled q first runs a max-free kernel (p = exp2(S) with reference 0;
 * rows whose sum leaves a checked window flag their workgroup in the scratch and are recomputed by the lazy-reference kernel
 * launched right behind -- same results for unflagged workgroups, ~2 % faster; once more than 1/8 of a launch had to be
 * recomputed word [0] turns the attempt off for later calls, which then cost one lazy-reference launch: 1.36 instead of
 * 1.40 PFLOP/s, no cliff), and (b) the last, partially filled round of workgroups of a long self-attention launch is split
 * over the key range so that it fills the chip (matters when few heads are local, e.g. the 5 heads per GPU of an 8-way
 * Ulysses shard: +15 %).  workspace = NULL is always valid (one lazy-reference launch). */
int64_t wan_attention_workspace_bytes(int batch, int Lq, int Lk, int num_heads, int head_dim);
/* Host arithmetic only (no GPU needed): what wan_attention_fwd will launch for this shape, flags and scratch size, as
 * WAN_ATTN_VARIANT_* bits (the value wan_get_tuning("last_attn_variant") reports after the call); 0 for an unsupported shape.
 * Lets a benchmark / test state the dispatched kernels without launching them.  No reference counterpart. */
int wan_attention_plan(int batch, int Lq, int Lk, int num_heads, int head_dim, int flags, int64_t workspace_bytes);
#define WAN_ATTN_Q_PRESCALED 1
#define WAN_ATTN_QK_FP8 2                   /* wan_attention_plan only: plan for wan_attention_fwd_qk8 */
#define WAN_ATTN_PV_FP8 4                   /* wan_attention_plan only, with WAN_ATTN_QK_FP8: plan for wan_attention_fwd_f8 */
#define WAN_ATTN_QSCALE(softmax_scale) ((softmax_scale) * 1.4426950408889634f)

/* a9s Local self-attention: every query block attends a LIST of key tiles (LOSSY by construction, opt-in; no reference counterpart:
 *     the reference's attention() is dense).  Query block qb = rows [256 qb, 256 qb + 256) attends exactly the keys of the physical
 *     64-key tiles tiles[row_ptr[qb] .. row_ptr[qb + 1]): dense attention over those keys (of the last physical tile only keys < Lk),
 *     no mask inside a listed tile.  One list serves every head and sample of a call.
 *     The lists (host memory, int32; n_qblocks = ceil(Lq / 256), n_ktiles = ceil(Lk / 64)) must satisfy, checked in this order:
 *       row_ptr[0] == 0; row_ptr non-decreasing; every row non-empty; every tile in [0, n_ktiles); every row strictly ascending.
 *     wan_attn_sparse_validate: host arithmetic only (no GPU needed); WAN_ERR_INVALID with wan_last_error() naming the first offence.
 *     wan_attn_sparse_create:   validates, then uploads once (synchronous copies: call it outside a stream capture).  The plan owns its
 *                               device copy and remembers Lq, Lk; it may serve any number of calls, on any stream, until destroyed --
 *                               the caller keeps it alive until the last launch that uses it has completed.
 *     wan_attn_sparse_listed:   total listed (query block, tile) pairs; listed / (n_qblocks * n_ktiles) is the density.
 *     wan_attention_fwd_sparse: q / k / vt / out / strides / softmax_scale / flags exactly as wan_attention_fwd.  Lq, Lk must be the
 *                               plan's (WAN_ERR_INVALID otherwise).  Every check happens on the host before anything is enqueued, so
 *                               every index the kernel reads lies inside its tensor by construction.  ONE launch of the lazy-reference
 *                               kernel (attn_fwd_w4_kernel<0,false,1|2,...,SPARSE>), no scratch; capturable.  With every tile listed
 *                               for every block the result equals wan_attention_fwd(workspace = NULL) bit for bit.
 *     wan_get_tuning("last_attn_variant") reports WAN_ATTN_VARIANT_W4_LAZY | WAN_ATTN_VARIANT_SPARSE (| _XCD_PINNED). */
typedef struct wan_attn_sparse wan_attn_sparse;
wan_status_t wan_attn_sparse_validate(const int32_t* row_ptr, const int32_t* tiles, int n_qblocks, int n_ktiles);
wan_status_t wan_attn_sparse_create(const int32_t* row_ptr, const int32_t* tiles, int Lq, int Lk, wan_attn_sparse** out);
void wan_attn_sparse_destroy(wan_attn_sparse* plan);
int64_t wan_attn_sparse_listed(const wan_attn_sparse* plan);
wan_status_t wan_attention_fwd_sparse(const void* q, int64_t ldq, int64_t q_bstride,
                                      const void* k, int64_t ldk, int64_t k_bstride,
                                      const void* vt, int64_t ldvt, int64_t vt_bstride,
                                      void* out, int64_t ldo, int64_t o_bstride,
                                      int batch, int Lq, int Lk, const wan_attn_sparse* plan, int num_heads, int head_dim,
                                      float softmax_scale, int flags, void* stream);

/* a9' Self-attention with the QK^T product on the fp8 matrix pipe (LOSSY, opt-in; the role of the reference's
 *     `sageattn` branch, attention_utils.py:152-211 with attention_type = "SAGE_ATTENTION": 8-bit QK^T, 16-bit P.V).
 *       q8  e4m3 [B][Lq][H*128] = e4m3( q * softmax_scale * log2(e) * 2^q_exp )      (strides in BYTES, rows 16-byte aligned)
 *       k8  e4m3 [B][Lk][H*128] = e4m3( k * 2^k_exp )
 *     both written by wan_rmsnorm_rope_fp8 (below); the power-of-two factors move typical post-RMSNorm magnitudes into e4m3's
 *     normal range (2^-6 .. 448) and are undone exactly by the MFMA's E8M0 operand scales, so the fp32 scores differ from the
 *     bf16 kernel's only by the 3-bit mantissas of q8 / k8 (a relative error of <= 2^-4 per element; |q| * 2^q_exp or
 *     |k| * 2^k_exp above 448 saturates).  Everything behind the scores -- lazy softmax reference, bf16 P, P.V, fp32 sums,
 *     split tail, XCD pinning, the scratch layout -- is wan_attention_fwd's lazy-reference form; vt / out as there.
 *     Measured error and speed: tests/test_gpu_fp8.py, DESIGN.md section 13. */
wan_status_t wan_attention_fwd_qk8(const void* q8, int64_t ldq8, int64_t q8_bstride, int q_exp,
                                   const void* k8, int64_t ldk8, int64_t k8_bstride, int k_exp,
                                   const void* vt, int64_t ldvt, int64_t vt_bstride,
                                   void* out, int64_t ldo, int64_t o_bstride,
                                   int batch, int Lq, int Lk, int num_heads, int head_dim,
                                   void* workspace, int64_t workspace_bytes, void* stream);
/* a9'' Both attention products on the fp8 matrix pipe (LOSSY, opt-in; SageAttention-2's operating point: 8-bit QK^T, fp8 P.V).
 *     q8 / k8 / vt / out / workspace as wan_attention_fwd_qk8 (the scratch is REQUIRED here: the softmax is the checked max-free form,
 *     a flagged workgroup is redone by the fp8-QK^T lazy-reference kernel with the bf16 vt).  v8 / v8_scales: V^T as MX e4m3, written by
 *     wan_vt_quantize_mx from the bf16 vt -- per channel row and per block of 32 consecutive keys one E8M0 scale (block max / scale in [128, 256)),
 *     the 64 keys of a tile stored in the order the kernel's P registers hold them; v8 [B][H*128][ldv8 bytes], ldv8 >= roundup(Lk, 64),
 *     % 16; v8_scales: wan_vt_mx_scale_bytes(batch, heads, Lk) bytes.  P is quantised inside the kernel, also as MX blocks (32 keys
 *     per query row, scale from the block's fp32 sum), so neither operand needs a bounded range.  Error / speed: DESIGN.md section 13. */
wan_status_t wan_attention_fwd_f8(const void* q8, int64_t ldq8, int64_t q8_bstride, int q_exp,
                                  const void* k8, int64_t ldk8, int64_t k8_bstride, int k_exp,
                                  const void* v8, int64_t ldv8, int64_t v8_bstride, const void* v8_scales,
                                  const void* vt, int64_t ldvt, int64_t vt_bstride,
                                  void* out, int64_t ldo, int64_t o_bstride,
                                  int batch, int Lq, int Lk, int num_heads, int head_dim,
                                  void* workspace, int64_t workspace_bytes, void* stream);
int64_t wan_vt_mx_scale_bytes(int batch, int num_heads, int Lk);
wan_status_t wan_vt_quantize_mx(const void* vt_bf16, int64_t ldvt, int64_t vt_bstride, int batch, int num_heads, int Lk,
                                void* v8, int64_t ldv8, int64_t v8_bstride, void* v8_scales, void* stream);
/* wan_rmsnorm_rope that leaves x0 / x1 untouched and writes e4m3 copies of the results, dense [rows][dim] bytes:
 * out0 = e4m3(bf16(result0 * x0_scale)), out1 = e4m3(bf16(result1 * x1_scale)) -- the bf16 rounding first, so that with
 * power-of-two extra factors the e4m3 value is a quantisation of exactly the number the bf16 path would have used. */
wan_status_t wan_rmsnorm_rope_fp8(const void* x0_bf16, const float* w0, const void* x1_bf16, const float* w1,
                                  int64_t ld, int64_t rows, int dim, int head_dim, float eps,
                                  const float* rope_cos, const float* rope_sin, const wan_rope_params* rp,
                                  float x0_scale, float x1_scale, void* out0_fp8, void* out1_fp8, void* stream);

/* K smoothing for a9' (what `sageattn(..., smooth_k=True)`, the default of the wheel behind attention_utils.py:173-185, does):
 * softmax_j(q_i . k_j) is unchanged when one vector is subtracted from every k_j, so the e4m3 copy of k is taken of
 * k - mean_over_tokens(k) -- a channel with a large common offset would otherwise spend its 3 mantissa bits on the offset.
 *   wan_col_mean_bf16:   mean[b][c] = mean over rows [0, valid_rows) of sample b of x (bf16 [batch * rows_per_batch][ld]); two-stage,
 *                        fixed summation order (bit-reproducible); workspace of wan_col_mean_workspace_bytes(batch, dim) bytes.
 *   wan_qk_quantize_fp8: q8 = e4m3(q * q_scale), k8 = e4m3((k - k_mean[b]) * k_scale), dense [rows][dim] bytes; q, k are the
 *                        bf16 results of wan_rmsnorm_rope (q already carries softmax_scale * log2(e)); k_mean = NULL: no smoothing.
 *                        Either operand may be left out (q_bf16 = q8 = NULL or k_bf16 = k8 = NULL; ABI 8): under Ulysses k is
 *                        quantised once when it has arrived, every head group of q when its own exchange has completed. */
int64_t wan_col_mean_workspace_bytes(int batch, int dim);
wan_status_t wan_col_mean_bf16(const void* x_bf16, int64_t ld, int64_t rows_per_batch, int valid_rows, int batch, int dim,
                               void* workspace, float* mean, void* stream);
wan_status_t wan_qk_quantize_fp8(const void* q_bf16, const void* k_bf16, int64_t ld, int64_t rows, int dim, int64_t rows_per_batch,
                                 const float* k_mean, float q_scale, float k_scale, void* q8, void* k8, void* stream);

/* ---------------------------------------------------------------------------
 * a9f  Cross-attention over a padded prompt with the text values folded into the output projection.
 *     replaces: WanT2VCrossAttention.forward (wan_transformer3d.py:313-333) + its `o` Linear for the usual case of a short prompt.
 *               The reference pads the prompt with zero rows to text_len BEFORE text_embedding and masks nothing (context_lens = None,
 *               :936): every text row behind the longest prompt of the call is one and the same row in every layer.  With `kept` rows
 *               scored one by one and row `kept` standing for the pad_count = text_len - kept identical ones (its exp2-domain score
 *               raised by log2(pad_count)), a head has kept + 1 <= 64 distinct keys and
 *                   att . W_co^T = sum_h (P_h V_h) W_co,h^T = sum_h P_h (V_h W_co,h^T) = P . V'
 *               -- the output projection contracts over num_heads * 64 probabilities instead of num_heads * 128 channels.
 *     wan_cross_probs:       probs bf16 [batch * rows_per_batch][ldp >= num_heads * 64]: column h * 64 + j = softmax weight of key j
 *                            of head h (the representative's includes all pad_count rows); columns j > kept are exact zeros.  q bf16
 *                            [batch * rows_per_batch][ldq] PRE-SCALED (softmax_scale * log2 e, as wan_rmsnorm_rope's x0_scale writes
 *                            it); k bf16 [batch][>= kept + 1 rows][ldk] (sample stride k_bstride).  fp32 scores (MFMA), softmax in the
 *                            exp2 domain against the row maximum, normalised in fp32, ONE rounding to bf16.  0 <= kept <= 63.
 *     wan_cross_fold_values: vfold bf16 [batch][dim][ldo >= num_heads * 64] = V'^T in nn.Linear layout (a weight of wan_gemm_bf16_ws):
 *                            vfold[b][n][h * 64 + j] = bf16( sum_d w_co[n][h * 128 + d] * vt[b][h * 128 + d][j] ), j <= kept, zeros
 *                            above; fp32 accumulation in a fixed order of d.  vt = the text V^T of wan_dit_block_forward.
 *     wan_cross_fold_plan:   THE RULE (host arithmetic only): 1 when `rows` (= batch * rows_per_batch) query rows should take the
 *                            folded branch -- tuning key "cross_fold" is not 0, bf16 weights, 1 <= kept, kept + 1 <= 64, kept <
 *                            text_len, and (unless "cross_fold" = 2) num_heads * 64 >= 1024, % 128 == 0 and rows >= the measured
 *                            crossover (cross_fold.hip).  kept = text_len means "prompt length not known": never folds.
 *     wan_cross_fold_workspace_bytes: bytes of vfold for a batch (batch * dim * num_heads * 64 * 2).
 *     All rows 16-byte aligned (ld* and strides % 8 == 0).  No scratch; the results do not depend on the launch.
 * ------------------------------------------------------------------------- */
wan_status_t wan_cross_probs(const void* q, int64_t ldq, const void* k, int64_t ldk, int64_t k_bstride, void* probs, int64_t ldp,
                             int batch, int64_t rows_per_batch, int num_heads, int kept, int pad_count, void* stream);
wan_status_t wan_cross_fold_values(const void* w_co, int64_t ldw, const void* vt, int64_t ldvt, int64_t vt_bstride, void* vfold,
                                   int64_t ldo, int64_t vfold_bstride, int batch, int dim, int num_heads, int kept, void* stream);
int wan_cross_fold_plan(int64_t rows, int num_heads, int text_len, int kept, int weights_bf16);
int64_t wan_cross_fold_workspace_bytes(int batch, int dim);

/* [rows, cols] bf16 (row stride ld) -> [cols, ldt] bf16 transposed; pad columns [rows, ldt) are zeroed.
 * Used when a caller hands attention() a row-major V (the reference's [B,L,N,D] layout). */
wan_status_t wan_transpose_bf16(const void* in, int64_t ld, void* out_t, int64_t ldt,
                                int64_t rows, int cols, void* stream);

/* ---------------------------------------------------------------------------
 * a1  patchify: latent [Cin,F,H,W] -> im2col tokens bf16 [L, Cin*pt*ph*pw], token order (f,h,w),
 *     K index (c,pt,ph,pw) c slowest = Conv3d(k=s=patch) weight.flatten(1) order
 *     (wan_transformer3d.py:662-663, 870-879).  in_dtype: 0 fp32, 1 bf16.
 * a14 unpatchify: head output fp32 [L, pt*ph*pw*Cout] (c fastest) -> [Cout, F*pt, H*ph, W*pw]
 *     (einsum 'fhwpqrc->cfphqwr', wan_transformer3d.py:1108-1131).  out_dtype: 0 fp32, 1 bf16.
 *     zero_frames: output frames [0, zero_frames) are written as 0 and their token rows are not read -- the
 *     VideoCoF mask `noise_pred[:, :, :condition_count] = 0` (pipeline_wan.py:736) folded into the store
 *     (exact also under classifier-free guidance: 0 + s * (0 - 0) = 0); 0 = plain unpatchify.
 * ------------------------------------------------------------------------- */
wan_status_t wan_patchify(const void* latent, int in_dtype, void* tokens_bf16, int64_t ldt,
                          int Cin, int F, int H, int W, int pt, int ph, int pw, void* stream);
wan_status_t wan_unpatchify(const float* tokens, int64_t ldt, void* out, int out_dtype,
                            int Cout, int F, int Hp, int Wp, int pt, int ph, int pw, int zero_frames, void* stream);
/* a14' unpatchify with `rep` copies of the result written by the same pass: copy k goes to out + k * rep_stride elements
 *     (rep_stride >= Cout*F*pt*Hp*ph*Wp*pw; for a batch of B samples the caller passes B * that, so the result reads
 *     [rep][B][Cout][...]).  16-byte stores when the rows and both strides allow it, element-wise otherwise; zero_frames applies
 *     to every copy.  rep = 1 writes what wan_unpatchify writes.
 *     replaces: `result = torch.cat([result, result], dim=0)` of the cfg_skip decorator
 *     (videox_fun/utils/cfg_optimization.py:34-36) -- no second read of the output, no concatenation launch. */
wan_status_t wan_unpatchify_rep(const float* tokens, int64_t ldt, void* out, int out_dtype,
                                int Cout, int F, int Hp, int Wp, int pt, int ph, int pw, int zero_frames,
                                int rep, int64_t rep_stride, void* stream);

/* ---------------------------------------------------------------------------
 * a21  Ulysses sequence parallelism: the wire layouts of the head all-to-all (replaces usp_attn_forward's packing,
 *      videox_fun/dist/wan_xfuser.py:68-111, and yunchang's SeqAllToAll4D; the collective itself is an RCCL
 *      all_to_all_single with equal splits issued by the host, videocof_amd/dist.py).  One rank holds T tokens of B samples;
 *      P ranks; Cl = dim / P channels (H / P heads) per rank after the exchange.
 *        token-major wire   [P][T][B][Cl]  (q, k, and the attention output)
 *        channel-major wire [P][Cl][B][T]  (V^T: exactly what wan_gemm_bf16(WAN_EPI_BF16_T, ldo = B*T) writes per sample)
 *      After the exchange a token-major wire buffer reads as [P*T][B][Cl] -- all tokens, this rank's heads, row stride B*Cl,
 *      sample stride Cl -- which wan_attention_fwd consumes and produces in place (no unpacking of q, k or o).
 *      wan_rmsnorm_rope_sp: wan_rmsnorm_rope that reads x0 / x1 (not modified) and writes the results straight into
 *                           token-major wire buffers (slabs = P, batch = B; rows = B * rp->rows_per_batch): the fused form
 *                           of "norm, rotate, then pack for the all-to-all".
 *      wan_sp_pack_heads / wan_sp_unpack_heads: [B][T][ldx >= P*Cl] <-> token-major wire (the o projection's input).
 *      wan_sp_unpack_vt: arrived channel-major wire -> vt [B][Cl][ldvt], column s*T + t (ldvt >= P*T; pad columns untouched).
 *      Cl % 8 == 0, T % 8 == 0.
 *      *_split (head-group pipelining): the same kernels on a wire buffer cut into TWO head groups -- channels
 *                           [0, split) of every slab, then channels [split, Cl) -- each a complete token-major wire buffer of its
 *                           own ([P][T][B][split], then [P][T][B][Cl - split] right behind it), so that each group travels in its own
 *                           all-to-all: the exchange of group 1 runs under the attention of group 0, the inverse exchange of group 0
 *                           under the attention of group 1.  split % 8 == 0, 0 <= split < Cl; split = 0 is the one-group layout.
 * ------------------------------------------------------------------------- */
wan_status_t wan_rmsnorm_rope_sp(const void* x0_bf16, const float* w0, const void* x1_bf16, const float* w1,
                                 int64_t ld, int64_t rows, int dim, int head_dim, float eps,
                                 const float* rope_cos, const float* rope_sin, const wan_rope_params* rp,
                                 float x0_scale, void* wire0, void* wire1, int slabs, int batch, void* stream);
wan_status_t wan_sp_pack_heads(const void* x_bf16, int64_t ldx, void* wire, int P, int T, int B, int Cl, void* stream);
wan_status_t wan_sp_unpack_heads(const void* wire, void* x_bf16, int64_t ldx, int P, int T, int B, int Cl, void* stream);
wan_status_t wan_sp_unpack_vt(const void* wire, void* vt_bf16, int64_t ldvt, int P, int B, int Cl, int T, void* stream);
wan_status_t wan_rmsnorm_rope_sp_split(const void* x0_bf16, const float* w0, const void* x1_bf16, const float* w1,
                                       int64_t ld, int64_t rows, int dim, int head_dim, float eps,
                                       const float* rope_cos, const float* rope_sin, const wan_rope_params* rp,
                                       float x0_scale, void* wire0, void* wire1, int slabs, int batch, int split, void* stream);
wan_status_t wan_sp_pack_heads_split(const void* x_bf16, int64_t ldx, void* wire, int P, int T, int B, int Cl, int split, void* stream);
wan_status_t wan_sp_unpack_heads_split(const void* wire, void* x_bf16, int64_t ldx, int P, int T, int B, int Cl, int split, void* stream);

/* a21' The collective itself, owned by the library (for a host without torch.distributed; the Python host may use either):
 *      one communicator = one RCCL comm + ONE side HIP stream + a small ring of events (one per exchange in flight).
 *      replaces: set_multi_gpus_devices / init_distributed_environment (dist/fuser.py:35-54) and the head all-to-all inside
 *                xFuserLongContextAttention (dist/wan_xfuser.py:68-111).
 *      wan_sp_unique_id: rank 0 creates the 128-byte rendezvous token; the host distributes it (MPI, a file, torchrun's store).
 *      wan_sp_init: collective over all ranks (ncclCommInitRank) on the CURRENT HIP device; wan_sp_init_from_comm adopts an
 *                existing ncclComm_t (not destroyed by wan_sp_destroy).
 *      wan_sp_a2a_scatter_heads / wan_sp_a2a_gather_heads: the same operation on the wire layouts above -- slab d of `send_wire`
 *                (bytes_total / world_size bytes) goes to rank d, slab s of `recv_wire` arrives from rank s; the first name is
 *                for q / k / V^T (token shards -> head shards), the second for o (back).  ASYNCHRONOUS: enqueued on the side
 *                stream behind everything already enqueued on `compute_stream`; the caller goes on enqueueing the next
 *                projection and calls
 *      wan_sp_wait before the kernel that reads the receive buffers: `compute_stream` then waits (on the device) for every
 *                exchange started so far.  The host is never synchronised.  send / receive buffers must be distinct and stay
 *                untouched between start and wait (persistent pairs, as videocof_amd/wan_transformer3d.py keeps them).
 *      wan_sp_ticket / wan_sp_wait_for: the finer form -- wan_sp_ticket right after a start names that exchange, wan_sp_wait_for
 *                makes `compute_stream` wait for it (and, the side stream being in order, for every EARLIER one) while exchanges
 *                started later stay in flight: the k exchange can be consumed while the q exchange behind it still runs.  A
 *                ticket is good for a wait at any later time (a recycled event marks a later point of the side stream).  One
 *                host thread drives a communicator.
 *      wan_sp_all_gather: recv[r] <- send of rank r (the head output, wan_transformer3d.py:1085-1086); also asynchronous.
 *      Stream capture: while `compute_stream` is being captured into a hipGraph the collectives are recorded ON it (no side stream,
 *                no events; tuning key "sp_inline" forces that form).  Verified with ONE rank only (capture + bit-identical replay);
 *                several ranks replaying RCCL collectives from graphs in lockstep are untested -- the Python host refuses to capture
 *                a sequence-parallel forward with world_size > 1 unless WAN_SP_GRAPH_MULTI_RANK=1 (videocof_amd/graph.py).
 *      wan_sp_destroy: destroys the RCCL comm, the side stream and the events -- EXCEPT for a communicator that was ever captured:
 *                instantiated graphs hold its RCCL kernels, so its comm is deliberately leaked (it lives until the process exits).
 *      RCCL is bound at run time (dlopen "librccl.so.1"): WAN_ERR_UNSUPPORTED if it cannot be loaded. */
typedef struct wan_sp_comm wan_sp_comm;
#define WAN_SP_UNIQUE_ID_BYTES 128
wan_status_t wan_sp_unique_id(void* id128);
wan_status_t wan_sp_init(wan_sp_comm** comm, const void* id128, int rank, int world_size);
wan_status_t wan_sp_init_from_comm(wan_sp_comm** comm, void* nccl_comm, int rank, int world_size);
int wan_sp_rank(const wan_sp_comm* comm);
int wan_sp_world_size(const wan_sp_comm* comm);
wan_status_t wan_sp_a2a_scatter_heads(wan_sp_comm* comm, const void* send_wire, void* recv_wire, int64_t bytes_total, void* compute_stream);
wan_status_t wan_sp_a2a_gather_heads(wan_sp_comm* comm, const void* send_wire, void* recv_wire, int64_t bytes_total, void* compute_stream);
wan_status_t wan_sp_all_gather(wan_sp_comm* comm, const void* send, void* recv, int64_t bytes_per_rank, void* compute_stream);
wan_status_t wan_sp_wait(wan_sp_comm* comm, void* compute_stream);
int64_t wan_sp_ticket(const wan_sp_comm* comm);
wan_status_t wan_sp_wait_for(wan_sp_comm* comm, int64_t ticket, void* compute_stream);
wan_status_t wan_sp_destroy(wan_sp_comm* comm);

/* a21'' MEASUREMENT ONLY: a device-local copy with the launch footprint of a collective (csrc/sp_emulate.hip).  It stands in for the
 *      RCCL all-to-all / all-gather kernel of ONE rank where there are no peers (videocof_amd.dist.EmulatedRank(concurrent=True) runs
 *      it on a side stream while the rank's projections run on the compute stream), so that what a communication kernel costs the
 *      resident GEMM / attention grids -- and what they cost it -- can be seen on one GPU.
 *      grid: exactly `channels` workgroups (1..32) of `threads` lanes (256 or 512); workgroup c copies the c-th contiguous share of
 *      `bytes` in 16-byte accesses (buffers misaligned against each other: byte accesses); any byte count, any alignment.  No LDS, no
 *      barrier, no atomics, nothing a workgroup waits for: it advances on a single free CU.  dst and src must not overlap.
 *      ASSUMED, NOT MEASURED: that an RCCL collective on this chip occupies "N channels = N workgroups of 256-512 threads" comes from
 *      RCCL's public channel model; no RCCL kernel was traced here.  It moves no byte between devices: no xGMI, no peer latency. */
wan_status_t wan_sp_channel_copy(void* dst, const void* src, int64_t bytes, int channels, int threads, void* stream);

/* ---------------------------------------------------------------------------
 * a11  One WanAttentionBlock as a single call (WanAttentionBlock.forward, wan_transformer3d.py:464-515) -- the
 *      composite a non-Python host drives: LN-modulate -> q|k GEMM -> RMSNorm+RoPE (q pre-scaled) -> V^T GEMM ->
 *      self-attention -> o GEMM (+gate, +residual) -> LN-affine -> q GEMM -> RMSNorm -> cross-attention over the text
 *      K / V^T -> o GEMM (+residual) -> LN-modulate -> ffn.0 (+GELU) -> ffn.2 (+gate, +residual); the kernels above,
 *      enqueued in that order on `stream` (host code only, no extra arithmetic).  Single device (no sequence parallelism).
 *      x      fp32 [batch * rows_per_batch, dim]   residual stream, updated IN PLACE
 *      emod   fp32 [6][batch][dim]                 modulation + time projection (`(self.modulation + e).chunk(6)`, :494)
 *      ctx_k  bf16 [batch][text_len][dim]          RMS-normed text keys   (cross_attn.norm_k(k(context)), :321)
 *      ctx_vt bf16 [batch][dim][text_len]          text values, transposed (cross_attn.v(context), :322)
 *      valid_tokens = F*Hp*Wp <= rows_per_batch: keys beyond it (sequence padding) are masked, V^T covers them only.
 *      Workspaces are caller-owned (sizes: wan_dit_block_workspace_bytes); vt's pad columns [valid_tokens, ldvt) must be
 *      finite (zero them once); the two attention scratches follow wan_attention_workspace_bytes and may be NULL.
 *      Cross-attention: when wan_cross_fold_plan(batch * rows_per_batch, num_heads, text_len, ws->text_kept, 1) says so and ws->vfold
 *      is there, `cross-attention -> o GEMM` runs as wan_cross_probs (into ws->att) -> wan_cross_fold_values (into ws->vfold) -> one
 *      o GEMM per sample over K = num_heads * 64 (a9f): the same sum with V' rounded to bf16 where the plain branch rounds the
 *      attention output -- equal within the kernels' tolerances, not bit for bit.  A zero-initialised vfold / text_kept keeps the plain branch.
 * ------------------------------------------------------------------------- */
typedef struct {
    int dim, ffn_dim, num_heads, text_len;
    float eps;
    const void *w_qk, *w_v, *w_o, *w_cq, *w_co, *w_ffn0, *w_ffn2;      /* bf16 [out, in]; w_qk = q rows then k rows */
    const float *b_qk, *b_v, *b_o, *b_cq, *b_co, *b_ffn0, *b_ffn2;
    const float *norm_q, *norm_k, *norm_cq;                           /* WanRMSNorm gains */
    const float *norm3_w, *norm3_b;                                   /* LayerNorm (affine) before cross-attention */
} wan_block_weights;

typedef struct {
    void *h, *qk, *att, *cq, *ff, *vt;        /* bf16: [M,dim] [M,2 dim] [M,dim] [M,dim] [M,ffn] [batch][dim][ldvt] */
    int64_t ldvt;
    void* attn_ws_self; int64_t attn_ws_self_bytes;
    void* attn_ws_cross; int64_t attn_ws_cross_bytes;
    void* gemm_ws; int64_t gemm_ws_bytes;      /* wan_gemm_bf16_ws workspace shared by the block's Linears (wan_gemm_workspace_bytes of the
                                                  largest one; NULL = the one-workgroup-per-tile kernels) */
    void* vfold; int64_t vfold_bytes;          /* the folded text values V'^T (a9f): wan_cross_fold_workspace_bytes(batch, dim) bytes, rewritten
                                                  by every layer of every call; NULL = never fold */
    int text_kept;                             /* longest prompt of the call in text rows (the host knows it: len(context[b])); rows behind it
                                                  are identical padding.  <= 0 or >= text_len = not known: never fold.
                                                  (vfold, vfold_bytes, text_kept were appended at the END of the struct under ABI 11: a host
                                                  compiled against the shorter struct must be recompiled; zero-initialised they change nothing) */
} wan_block_workspace;

wan_status_t wan_dit_block_forward(float* x, const float* emod, const void* ctx_k, const void* ctx_vt,
                                   const wan_block_weights* w, const wan_block_workspace* ws,
                                   const float* rope_cos, const float* rope_sin, const wan_rope_params* rp,
                                   int batch, int64_t rows_per_batch, int64_t valid_tokens, void* stream);
/* The token-local part of a block -- everything behind the self-attention output projection (wan_transformer3d.py:504-511:
 * norm3, cross-attention over the text tokens, FFN) -- as one call: the tail of wan_dit_block_forward, and what a
 * sequence-parallel host calls after its own self-attention part (it drives the exchanges itself; dist/wan_xfuser.py:68-111).
 * Uses ws->h, att, cq, ff, attn_ws_cross, gemm_ws only (qk / vt may be NULL).  ABI 8. */
wan_status_t wan_dit_block_tail_forward(float* x, const float* emod, const void* ctx_k, const void* ctx_vt,
                                        const wan_block_weights* w, const wan_block_workspace* ws,
                                        int batch, int64_t rows_per_batch, void* stream);
wan_status_t wan_dit_block_workspace_bytes(int dim, int ffn_dim, int batch, int64_t rows_per_batch, int64_t valid_tokens,
                                           int64_t* bytes /* [6]: h, qk, att, cq, ff, vt */, int64_t* ldvt);

/* ---------------------------------------------------------------------------
 * a11' The token path of WanTransformer3DModel.forward (wan_transformer3d.py:870-879, 1034-1083, 535-548, 1108-1131) as one
 *      call: patchify -> patch-embedding GEMM -> num_layers x wan_dit_block_forward -> head LN-modulate -> head GEMM ->
 *      unpatchify.  The embedding MLPs stay with the host and arrive as inputs:
 *      latent  [batch][in_dim][F][H][W] (latent_dtype 0 fp32 | 1 bf16); out the same shape with out_dim channels
 *      emod    fp32 [num_layers][6][batch][dim]   `modulation + time_projection(e)` of every block (:494, :899-901)
 *      ehead   fp32 [2][batch][dim]               `head.modulation + e` (shift, scale; :545)
 *      ctx_k / ctx_vt  host arrays of num_layers device pointers: the text K and V^T of each block (wan_dit_block_forward)
 *      rp      grid = (F/pt, H/ph, W/pw); rows_per_batch >= tokens (pad rows are zero on entry to the first block)
 *      zero_frames as wan_unpatchify.  Workspace: the block workspace plus x fp32 [batch*rows_per_batch, dim],
 *      tokens bf16 [tokens, in_dim*pt*ph*pw], head_out fp32 [batch*rows_per_batch, pt*ph*pw*out_dim].
 * ------------------------------------------------------------------------- */
typedef struct {
    int num_layers, in_dim, out_dim, pt, ph, pw;
    const wan_block_weights* blocks;                /* [num_layers] */
    const void* pe_w; const float* pe_b;            /* patch_embedding as a GEMM: bf16 [dim, in_dim*pt*ph*pw] */
    const void* head_w; const float* head_b;        /* head.head: bf16 [pt*ph*pw*out_dim, dim] */
} wan_dit_weights;

typedef struct {
    wan_block_workspace block;
    float* x;
    void* tokens;
    float* head_out;
} wan_dit_workspace;

wan_status_t wan_dit_forward(const void* latent, int latent_dtype, void* out, int out_dtype, const float* emod,
                             const float* ehead, const void* const* ctx_k, const void* const* ctx_vt,
                             const wan_dit_weights* w, const wan_dit_workspace* ws, const float* rope_cos,
                             const float* rope_sin, const wan_rope_params* rp, int batch, int F, int H, int W,
                             int64_t rows_per_batch, int zero_frames, void* stream);
/* The same call with the result written `rep` times along the batch axis (out = [rep][batch][out_dim][F][H][W]) by
 * wan_unpatchify_rep: a cfg_skip step (cfg_optimization.py:5-38) computes the conditional half and returns it twice.
 * rep = 1 enqueues exactly what wan_dit_forward enqueues. */
wan_status_t wan_dit_forward_rep(const void* latent, int latent_dtype, void* out, int out_dtype, const float* emod,
                                 const float* ehead, const void* const* ctx_k, const void* const* ctx_vt,
                                 const wan_dit_weights* w, const wan_dit_workspace* ws, const float* rope_cos,
                                 const float* rope_sin, const wan_rope_params* rp, int batch, int F, int H, int W,
                                 int64_t rows_per_batch, int zero_frames, int rep, void* stream);

/* a17  UniPC updates as one fused pass: out[i] = c0*x0[i] + c1*x1[i] + c2*x2[i] + c3*x3[i] (x1..x3 may be
 *      NULL), fp32 accumulate, all tensors of one dtype (0 fp32, 1 bf16).
 *      replaces: the elementwise chains of convert_model_output / multistep_uni_p_bh_update /
 *      multistep_uni_c_bh_update (fm_solvers_unipc.py:318-320, 458-470, 600-612); the scalar algebra
 *      stays on the host (float64). */
wan_status_t wan_lincomb(void* out, int dtype, const void* x0, const void* x1, const void* x2, const void* x3,
                         float c0, float c1, float c2, float c3, int64_t n, void* stream);

/* a17b  The flow DPM-Solver++ step as one fused pass, two outputs:
 *          x0_out[i]   = a_s*sample[i] + a_v*v[i]                          (stored in `dtype`: the scheduler's history entry)
 *          prev_out[i] = c_s*sample[i] + c_0*x0r[i] + c_1*m1[i] + c_2*m2[i] + c_n*noise[i]    (x0r = x0 as stored)
 *      sample, v, m1, m2 and both outputs are all fp32 (dtype 0) or all bf16 (dtype 1); `noise` is always fp32; m1, m2 and
 *      noise may be NULL (m2 only with m1).  fp32 accumulate; the x0 bits equal wan_lincomb's on the same two terms.
 *      replaces: convert_model_output's x0 prediction (fm_solvers.py:381-383) and the elementwise chains of
 *      dpm_solver_first_order_update / multistep_dpm_solver_second_order_update / multistep_dpm_solver_third_order_update
 *      (fm_solvers.py:465-482, 549-592, 666-676) incl. the sde-dpmsolver++ noise term; the scalar algebra stays on the host
 *      (float64, videocof_amd/fm_solvers.py). */
wan_status_t wan_solver_step(void* x0_out, void* prev_out, int dtype, const void* sample, const void* v, const void* m1,
                             const void* m2, const float* noise, float a_s, float a_v, float c_s, float c_0, float c_1,
                             float c_2, float c_n, int64_t n, void* stream);

/* a17c  Temporal context windows (DESIGN.md "Temporal context windows"): a clip of Fs latent frames is denoised as K overlapping
 *      windows of n frames each, window k starting at latent frame starts[k] (host array; ascending from 0, the last one at
 *      Fs - n, no gap: anything else is WAN_ERR_INVALID; K <= WAN_WINDOW_MAX).  The loop's state is ONE tensor
 *          state [B, C, Fs + K*G + Fs, h, w] = [source | ground_0 .. ground_{K-1} | target]      (G grounding frames, 0 = none)
 *      and a window is [C, n + G + n, h, w] = [source[a_k : a_k + n] | ground_k | target[a_k : a_k + n]].  hw = h * w elements per
 *      frame; dtype 0 fp32, 1 bf16 (state, windows and predictions alike).  16-byte accesses when a frame is a multiple of
 *      16 bytes and the bases (and rep_stride) are aligned, element-wise otherwise.
 *      wan_window_gather: out = [rep][k1 - k0][B] windows, the model's input batch of windows [k0, k1); rep in {1, 2} writes the
 *          doubled batch of a guided step in the same pass, copy r at out + r * rep_stride elements
 *          (rep_stride >= (k1 - k0) * B * C * (2n + G) * hw).
 *          replaces: per window two slices and a cat, a cat over the windows, and `torch.cat([latents] * 2)` (pipeline_wan.py:700).
 *      wan_window_blend: pred = [K][B] window predictions (after guidance) -> out, the prediction for the state:
 *          source frames   0                                        (the CoF mask, pipeline_wan.py:736)
 *          ground_k        window k's grounding block, bits unchanged
 *          target frame f  sum over the windows k that cover f, ascending, of alpha[k * Fs + f] * pred_k[f - a_k]
 *          in float32 with SEPARATE roundings -- round(alpha * p) first, then acc = round(acc + round(alpha * p)) per further
 *          window, one final rounding to `dtype`; never a fused multiply-add.  alpha: device float32 [K, Fs], the normalised
 *          weights of videocof_amd.window_plan (exactly 1.0f where one window covers f: that frame is the window's prediction
 *          unchanged). */
#define WAN_WINDOW_MAX 64
wan_status_t wan_window_gather(void* out, const void* state, int dtype, const int* starts, int K, int k0, int k1, int B, int C,
                               int Fs, int n, int G, int64_t hw, int rep, int64_t rep_stride, void* stream);
wan_status_t wan_window_blend(void* out, const void* pred, int dtype, const float* alpha, const int* starts, int K, int B, int C,
                              int Fs, int n, int G, int64_t hw, void* stream);

/* a17d  Spatial context windows: the same in three axes.  Each axis has its own plan in LATENT cells -- t_starts
 *      [Kt] windows of n frames over Fs, y_starts [Ky] of th rows over H, x_starts [Kx] of tw columns over W; each as a17c's
 *      `starts` (host array, ascending from 0, the last at extent - length, no gap, at most WAN_WINDOW_MAX) -- and the windows are
 *      the K = Kt * Ky * Kx tiles of one shape, tile k = (kt * Ky + ky) * Kx + kx.  The loop's state is
 *          state [B, C, Fs + Kt*G + Fs, H, W] = [source | ground_0 .. ground_{Kt-1} | target]
 *      (every TEMPORAL window owns a grounding block; the spatial tiles of one temporal window share it) and tile (kt, ky, kx) is
 *          [C, n + G + n, th, tw] = [source[a_t : a_t + n, tile] | ground_kt[:, tile] | target[a_t : a_t + n, tile]],
 *      tile = rows [y0, y0 + th) x columns [x0, x0 + tw).  dtype 0 fp32, 1 bf16.  A tile row is tw elements at pitch W: the access
 *      unit is the largest of 16, 8, 4 bytes or one element that divides (in bytes) the row length, the pitch, every x0, the frame
 *      and tile-frame sizes, rep_stride and the base addresses, so no unit straddles a tile edge.
 *      wan_tile_gather: out = [rep][k1 - k0][B] tiles, the model's input batch of tiles [k0, k1); rep and rep_stride as in
 *          wan_window_gather (rep_stride >= (k1 - k0) * B * C * (2n + G) * th * tw elements).
 *      wan_tile_blend: pred = [K][B] tile predictions (after guidance) -> out, the prediction for the state:
 *          source frames                       0
 *          grounding frame g of block kt and
 *          target frame f, at (y, x)           the sum over the covering tiles only, in ascending k, of w * p, with
 *                                              w = round(round(at * ay[ky * H + y]) * ax[kx * W + x]),
 *                                              at = at_tab[kt * Fs + f] for target frames and 1.0f for grounding frames
 *          in float32 with SEPARATE roundings -- the first term is round(w * p), every later one acc = round(acc + round(w * p)),
 *          one final rounding to `dtype`; never a fused multiply-add.  at_tab [Kt, Fs], ay [Ky, H], ax [Kx, W]: device float32,
 *          the three axes' videocof_amd.window_plan(...).alpha.  With Ky = Kx = 1 both entries compute what the a17c pair does.
 *      Everything is validated on the host before anything is enqueued (each axis' plan, [k0, k1) inside K, rep / rep_stride,
 *      row and frame counts below 2^31); a failure is WAN_ERR_INVALID. */
wan_status_t wan_tile_gather(void* out, const void* state, int dtype, const int* t_starts, const int* y_starts, const int* x_starts,
                             int Kt, int Ky, int Kx, int k0, int k1, int B, int C, int Fs, int H, int W, int n, int th, int tw,
                             int G, int rep, int64_t rep_stride, void* stream);
wan_status_t wan_tile_blend(void* out, const void* pred, int dtype, const float* at_tab, const float* ay, const float* ax,
                            const int* t_starts, const int* y_starts, const int* x_starts, int Kt, int Ky, int Kx, int B, int C,
                            int Fs, int H, int W, int n, int th, int tw, int G, void* stream);

/* a17e  Edit inside a mask: the denoising loop itself keeps the clip outside a caller's mask on its source.
 *      replaces: nothing in the reference, whose loop repaints the whole target segment; callers composite in pixels afterwards.
 *      wan_latent_mask_u8: alpha uint8 [B, T, H, W] (a pixel mask, any base alignment) -> weights uint8 [B, Fl, H/8, W/8],
 *          Fl = 1 + ceil((T - 1) / 4), in integers (videocof_amd/video_io.py: reference_latent_edit_mask restates it in numpy int64 and
 *          equals the kernels byte for byte):
 *              p = the maximum of alpha over the pixel frames of latent frame j (frame 0 for j = 0, frames 4j-3 .. min(4j, T-1) for
 *                  j >= 1) and over rows 8y .. 8y+7, columns 8x .. 8x+7
 *              g = the maximum of p over the (2 grow + 1)^2 cells and the latent frames j - grow_t .. j + grow_t around a cell;
 *                  positions outside the frame or outside the sample's Fl frames are ignored
 *              weights = (2 S + m) / (2 m),   S = sum of g over the (2 feather + 1)^2 cells with clamped indices, m = (2 feather + 1)^2
 *          (floor).  feather <= grow is what makes a cell that holds a 255 pixel keep weight 255.  ratio_s / ratio_t: the VAE's
 *          compression ratios, 8 and 4 (what the kernels are built for; anything else is WAN_ERR_INVALID).  grow <=
 *          WAN_LATENT_MASK_MAX_GROW, grow_t <= WAN_LATENT_MASK_MAX_GROW_T, feather <= grow, none negative; H % 8 == 0 and W % 8 == 0;
 *          at most 2^31 - 1 mask bytes; `workspace`: device memory of wan_latent_mask_workspace_bytes(B, T, H, W) bytes (the p and g
 *          planes) -> else WAN_ERR_INVALID before anything is enqueued.  Enqueues three kernels on `stream`; never synchronises.
 *      wan_masked_prediction: in place on `pred`, the prediction for the loop state.  pred, sample: [B, C, F, hw] of one dtype (0 fp32,
 *          1 bf16), sample = the state [source | grounding | target] the prediction was made for; weights uint8 [Bm, Fs, hw], Bm in
 *          {1, B}, shared by the channels.  For every b, c, f < Fs and cell, with a = the weight, v = pred[.., target_frame0 + f, ..],
 *          xt = sample[.., target_frame0 + f, ..], s = sample[.., f, ..], every operation rounded to float32 on its own:
 *              w = a / 255.0f,   d = xt - s,   r = d / sigma,   out = (w * v) + ((1 - w) * r)
 *          -- never a fused multiply-add, IEEE division, one final round-to-nearest-even to `dtype`.  r is the prediction whose
 *          x0 = xt - sigma * r is the source.  Where a == 255 the element is not written (v's bits stay); where a == 0 the result is
 *          round(r).  Frames of pred outside [target_frame0, target_frame0 + Fs) are never written.  sigma: this step's sigma_i > 0
 *          (host float).  The access unit is the largest of 16, 8, 4 bytes or one element that divides (in bytes) Fs * hw, F * hw,
 *          target_frame0 * hw and the bases (the weights' base by its count of elements).  A null tensor, another dtype, sigma <= 0 or
 *          not finite, Bm not in {1, B}, target_frame0 < Fs or target_frame0 + Fs > F, a count of 2^31 or more -> WAN_ERR_INVALID
 *          before anything is enqueued.  Enqueues one kernel on `stream`; never synchronises. */
#define WAN_LATENT_MASK_MAX_GROW 4
#define WAN_LATENT_MASK_MAX_GROW_T 2
int64_t wan_latent_mask_workspace_bytes(int B, int T, int H, int W);
wan_status_t wan_latent_mask_u8(const void* alpha_u8, void* weights_u8, int B, int T, int H, int W, int ratio_s, int ratio_t, int grow,
                                int grow_t, int feather, void* workspace, int64_t workspace_bytes, void* stream);
wan_status_t wan_masked_prediction(void* pred, const void* sample, int dtype, const void* weights_u8, int B, int Bm, int C, int F,
                                   int Fs, int target_frame0, int64_t hw, float sigma, void* stream);

/* a17f  Edit region: run the loop only on the part of the clip the edit mask touches.  Three passes, each once per
 *      call; videocof_amd/edit_region.py states each in plain torch (reference_mask_bounds, reference_region_crop,
 *      reference_region_restore) and the kernels equal them bit for bit.
 *      replaces: nothing in the reference, whose loop runs on whole frames.
 *      Common to all three: a row of a frame is W elements, a row of the region wr elements at column x0; the access unit is the
 *      largest of 16, 8, 4 bytes or one element that divides (in bytes) W, wr, x0 and the base addresses, so no unit straddles the
 *      region's edge.  Everything is validated on the host before anything is enqueued; each enqueues ONE kernel on `stream` and never
 *      synchronises.
 *      wan_mask_bounds: weights uint8 [Bm, Fs, h, w] (wan_latent_mask_u8's) -> bounds int32 [Fs, 4] = (y_lo, y_hi, x_lo, x_hi) per
 *          latent frame: the inclusive bounds of the non-zero weights over all Bm samples; a frame without one gives (h, -1, w, -1).
 *          One workgroup per latent frame, reduced in registers and LDS: no atomics, no init pass, every output word written exactly
 *          once.  A null tensor, a count below 1, 2^31 weights or more, bounds not 4-byte aligned -> WAN_ERR_INVALID.
 *      wan_region_crop: in [R, H, W] (contiguous, elements of elem_bytes = 1, 2 or 4) -> out [R, hr, wr], out[r, y, x] =
 *          in[r, y0 + y, x0 + x], bits unchanged.  Serves the loop state (R = B * C * F) and the weights (R = Bm * Fs, bytes).
 *      wan_region_restore: source [B, C, cc, H, W] (the full-frame source block), region [B, C, cc + G + cc, hr, wr] (the loop's final
 *          state on the region) -> out [B, C, cc + G + cc, H, W], bits unchanged:
 *              source frame f            source[f]
 *              grounding frame g         region[cc + g] inside the box, source[g] outside it       (hence 0 <= G <= cc)
 *              target frame f            region[cc + G + f] inside the box, source[f] outside it
 *          so outside the box the target IS the source, bit for bit.
 *      For the last two: a null tensor, another element size, a box that does not lie inside the frame (y0, x0 >= 0; hr, wr >= 1;
 *      y0 + hr <= H; x0 + wr <= W), G outside [0, cc], a frame count or H * W of 2^31 or more -> WAN_ERR_INVALID.
 *      The same two with a range of frames as well (`edit_region_time_margin`; reference_region_crop_frames and
 *      reference_region_restore_frames state them), the same kernels behind them:
 *      wan_region_crop_frames: in [R, F, H, W] -> out [R, Fo, hr, wr]: the box of the frames that `runs` lists.  `runs` is read on the
 *          HOST: n_runs (1 to 3) pairs (start, count) of input frames, ascending, not overlapping, count >= 1, inside [0, F); Fo is the
 *          sum of the counts and output frame k is the k-th listed frame.  The loop state takes R = B * C and the runs (t0, n),
 *          (cc, G), (cc + G + t0, n) (the second left out where G = 0), the weights R = Bm and the run (t0, n).  One run (0, F) is
 *          wan_region_crop on [R * F, H, W].  Also WAN_ERR_INVALID: null `runs`, n_runs outside 1..3, a run that is empty, descends,
 *          overlaps its predecessor or leaves [0, F).
 *      wan_region_restore_frames: source [B, C, cc, H, W], region [B, C, n + G + n, hr, wr] (the loop's final state on the source
 *          frames [t0, t0 + n) and the box) -> out [B, C, cc + G + cc, H, W]:
 *              source frame f            source[f]
 *              grounding frame g         region[n + g] inside the box, source[g] outside it                  (hence 0 <= G <= cc)
 *              target frame f            region[n + G + f - t0] where t0 <= f < t0 + n and inside the box, source[f] everywhere else
 *          so outside the range and outside the box the target IS the source, bit for bit; (t0, n) = (0, cc) is wan_region_restore.
 *          Also WAN_ERR_INVALID: t0 < 0, n < 1, t0 + n > cc. */
wan_status_t wan_mask_bounds(const void* weights_u8, void* bounds_i32, int Bm, int Fs, int h, int w, void* stream);
wan_status_t wan_region_crop(void* out, const void* in, int elem_bytes, int64_t R, int H, int W, int y0, int x0, int hr, int wr,
                             void* stream);
wan_status_t wan_region_restore(void* out, const void* source, const void* region, int elem_bytes, int B, int C, int cc, int G, int H,
                                int W, int y0, int x0, int hr, int wr, void* stream);
wan_status_t wan_region_crop_frames(void* out, const void* in, int elem_bytes, int64_t R, int F, int H, int W, const int* runs,
                                    int n_runs, int y0, int x0, int hr, int wr, void* stream);
wan_status_t wan_region_restore_frames(void* out, const void* source, const void* region, int elem_bytes, int B, int C, int cc, int G,
                                       int H, int W, int t0, int n, int y0, int x0, int hr, int wr, void* stream);

/* a17g  Edit region, a box that follows the mask from frame to frame (`edit_region_follow`): one size hr x wr for the
 *      clip and a corner per latent frame.  The frames forms of a17f with a table of corners; videocof_amd/edit_region.py states both
 *      in plain torch (reference_region_crop_track, reference_region_restore_track) and the kernels equal them bit for bit.
 *      replaces: nothing in the reference, whose loop runs on whole frames.
 *      `origins` is read on the HOST, like `runs`: int32 pairs (y0_f, x0_f), one per frame.  Every entry is validated before anything
 *      is enqueued, then the table travels BY VALUE in the kernel's arguments, two 16-bit values per frame, at most
 *      WAN_REGION_TRACK_MAX_FRAMES frames; a workgroup indexes it with its own frame, which is a scalar load of the argument segment.
 *      So: no device allocation, no host-to-device copy, no synchronisation, ONE kernel per call.  The access unit is a17f's over W, wr,
 *      the bitwise OR of every x0_f and the base addresses: a single odd x0_f lowers it for the whole launch.
 *      wan_region_crop_track: wan_region_crop_frames with the box of INPUT frame f at origins[f] (`origins`: [F, 2]): in [R, F, H, W]
 *          -> out [R, Fo, hr, wr], output frame k = the box of the k-th frame the runs list, at that frame's corner.  The kernel
 *          knows no layout: for the loop state [source | grounding | target] the caller passes a table over all F = 2 cc + G frames
 *          in which grounding g has source frame g's corner and target f source frame f's; the weights take the table of the cc
 *          source frames.
 *      wan_region_restore_track: wan_region_restore_frames with the box of source frame f at origins[f] (`origins`: [cc, 2]):
 *              source frame f            source[f]
 *              grounding frame g         region[n + g] inside box g, source[g] outside it                    (hence 0 <= G <= cc)
 *              target frame f            region[n + G + f - t0] where t0 <= f < t0 + n and inside box f, source[f] everywhere else
 *          so outside its frame's box, and outside the range, the target IS the source, bit for bit.
 *      WAN_ERR_INVALID: whatever the frames forms reject, a null `origins`, any box that does not lie inside the frame (of ALL F, or
 *      cc, entries, listed by a run or not), more than WAN_REGION_TRACK_MAX_FRAMES frames (F, or cc).  A corner must be below 65536.
 *      Constant origins give the bytes of the frames forms. */
#define WAN_REGION_TRACK_MAX_FRAMES 512
wan_status_t wan_region_crop_track(void* out, const void* in, int elem_bytes, int64_t R, int F, int H, int W, const int* runs,
                                   int n_runs, const int* origins, int hr, int wr, void* stream);
wan_status_t wan_region_restore_track(void* out, const void* source, const void* region, int elem_bytes, int B, int C, int cc, int G,
                                      int H, int W, int t0, int n, const int* origins, int hr, int wr, void* stream);

/* a17h  Edit region, a mask of separate objects split into boxes (`edit_region_split`): at most WAN_REGION_SPLIT_MAX
 *      bands along ONE axis, a box of ONE size hr x wr per band, the boxes run as samples of one forward.
 *      videocof_amd/edit_region.py states all three in plain torch (reference_mask_spans, reference_region_crop_split,
 *      reference_region_restore_split) and the kernels equal them bit for bit.
 *      replaces: nothing in the reference, whose loop runs on whole frames.
 *      wan_mask_spans: weights uint8 [Bm, Fs, h, w] -> spans int16 [Fs, h + w, 2].  Per latent frame the first h pairs are, per row,
 *          the inclusive (x_lo, x_hi) of the non-zero weights over all Bm samples, (w, -1) for a row without one; the next w pairs
 *          are, per column, (y_lo, y_hi), (h, -1) for a column without one.  A frame's bounds (wan_mask_bounds) are the min and max of
 *          its spans, so a call that splits copies these 4 (h + w) Fs bytes to the host INSTEAD of the bounds.  One workgroup per
 *          latent frame; a pair is one 32-bit word, every word written exactly once: no atomics, no init pass.  The reads follow
 *          wan_mask_bounds' access unit.  WAN_ERR_INVALID: what wan_mask_bounds rejects (the spans' address a multiple of 4), h or w
 *          of 32768 or more.
 *      The boxes: `origins` int32 [K, 2] = (y0_k, x0_k) and `cuts` int32 [K + 1], read on the HOST like `runs`; `axis` 1: the cuts are
 *          columns, 0: rows.  Band k OWNS [cuts[k], cuts[k + 1]) on the cut axis and everything on the other one; boxes may overlap and
 *          may reach past what their band owns.  Everything is validated before anything is enqueued, then the table (a corner and an
 *          owned interval per box) travels BY VALUE in the kernel's arguments: no device allocation, no copy, no synchronisation, ONE
 *          kernel per call.  The access unit is a17f's over W, wr, every x0_k, the base addresses and, for a column cut, every cut
 *          column: no unit straddles a box's edge or a cut.
 *      wan_region_crop_split: wan_region_crop_frames for every box at once: in [R, F, H, W] -> out [K, R, Fo, hr, wr], box-major, bits
 *          unchanged.  With clip != 0 every element outside what band k owns is written as ZERO in box k: the form for the mask's
 *          weights, which pins the cells of another band's object to the source inside this box.
 *      wan_region_restore_split: source [B, C, cc, H, W], region [K B, C, n + G + n, hr, wr] (box-major) -> out [B, C, cc + G + cc, H, W]:
 *              source frame f            source[f]
 *              grounding frame g         box k's region[n + g] where the cell lies inside box k AND inside what band k owns, else source[g]
 *              target frame f            box k's region[n + G + f - t0] where t0 <= f < t0 + n and the same holds, else source[f]
 *          Every output unit is written once, from one of K + 1 places.
 *      WAN_ERR_INVALID: whatever the frames forms reject, null `origins` or `cuts`, K outside 1..WAN_REGION_SPLIT_MAX, another axis, a
 *      box that does not lie inside the frame, cuts that do not ascend strictly from 0 to the axis' extent.
 *      K = 1 gives the bytes of the frames forms. */
#define WAN_REGION_SPLIT_MAX 8
wan_status_t wan_mask_spans(const void* weights_u8, void* spans_i16, int Bm, int Fs, int h, int w, void* stream);
wan_status_t wan_region_crop_split(void* out, const void* in, int elem_bytes, int64_t R, int F, int H, int W, const int* runs,
                                   int n_runs, const int* origins, const int* cuts, int K, int axis, int clip, int hr, int wr,
                                   void* stream);
wan_status_t wan_region_restore_split(void* out, const void* source, const void* region, int elem_bytes, int B, int C, int cc, int G,
                                      int H, int W, int t0, int n, const int* origins, const int* cuts, int K, int axis, int hr,
                                      int wr, void* stream);

/* ===========================================================================
 * WanVAE (videox_fun/models/wan_vae.py).  Activations are CHANNELS-LAST bf16 [T, H, W, C].
 * ------------------------------------------------------------------------- */

/* a18/a19  every convolution of the VAE through one entry (two kernels behind it: the causal 3x3x3 / stride-1 convolutions with
 *     Cin % 32 == 0 and Cout % 96 == 0 keep their input patch in LDS; everything else is an implicit GEMM with a gathered A tile):
 *     out[(to,ho,wo), n] = bias[n] + sum_{kt,kh,kw,ci} in[to*st+kt-pt, ho*sh+kh-ph, wo*sw+kw-pw, ci] * w[n,(kt,kh,kw,ci)]
 *                          (+ resid[(to,ho,wo), n])
 *     replaces: CausalConv3d.forward incl. the cache_x halo (wan_vae.py:21-40: frames with negative
 *               time index are read from `hist`, the last `hist_frames` (<= 2) frames of the previous
 *               chunk, CACHE_T :18; missing history = the zero padding of :38);
 *               Resample's Conv2d: upsample2x=1 fuses Upsample(nearest-exact, 2x) (:81-83) into the
 *               gather, ZeroPad2d((0,1,0,1)) + stride 2 (:92-94) is ph=pw=0, sh=sw=2 with zero fill;
 *               upsample3d's time_conv + the channel->time interleave (:132-141): time_interleave=1
 *               writes channel n of frame t to frame 2t + n/(Cout/2), channel n%(Cout/2);
 *               ResidualBlock's `x + h` (:224) through `resid`; all 1x1 convs (:203, 238-239, 509-510).
 *     x    bf16 [T_in, H_in, W_in, Cin], Cin % 8 == 0
 *     w    bf16 [Cout, ldw] with k = ((kt*KH + kh)*KW + kw)*Cin + ci, zero padded to ldw >= roundup(K, 64)
 *     out  bf16 [T_out*H_out*W_out, ldo]  (time_interleave: [2*T_out*H_out*W_out, ldo], Cout/2 channels)
 *          ldo: row stride in elements, ldo >= the channels of a row (Cout, or Cout/2 with time_interleave) and ldo % 4 == 0
 *          (8-byte stores).  Pixels are dense: row (to*H_out + ho)*W_out + wo.  Columns [channels, ldo) of a row are never
 *          written.  ldo % 8 == 0 with a 16-byte aligned out / resid is what the LDS-patch kernel's 16-byte stores need; any
 *          other ldo runs the same convolution on the gather kernel.
 *     resid bf16 or NULL: the layout of out, the SAME row stride ldo (read at the offsets out is written at)
 *     bias fp32 [Cout] or NULL, 16-byte aligned */
typedef struct {
    int T_in, H_in, W_in, Cin;
    int T_out, H_out, W_out, Cout;
    int KT, KH, KW;          /* each 1 or 3 */
    int st, sh, sw;          /* strides */
    int pt, ph, pw;          /* leading pads (time pad = causal front pad) */
    int upsample2x;          /* gather from a virtual nearest-exact 2x upsample of (H_in, W_in) */
    int time_interleave;
} wan_conv_params;

wan_status_t wan_conv_cl(const void* x, const void* hist, int hist_frames, const void* w, int64_t ldw,
                         const float* bias, const void* resid, void* out, int64_t ldo,
                         const wan_conv_params* p, void* stream);

/* a19  RMS_norm (F.normalize over channels * sqrt(C) * gamma, wan_vae.py:43-58) + optional SiLU,
 *      per pixel on channels-last rows.  C % 8 == 0, C <= 512. */
wan_status_t wan_rmsnorm_silu_cl(const void* x_bf16, const float* gamma, void* out_bf16, int64_t rows, int C,
                                 int silu, void* stream);

/* a19  row softmax for AttentionBlock (single head of dim C over h*w, wan_vae.py:256-260):
 *      probs[r, i] = softmax_i(scale * scores[r, i]) for i < n, 0 for n <= i < npad. */
wan_status_t wan_softmax_rows(const float* scores, int64_t lds, void* probs_bf16, int64_t ldp, int64_t rows,
                              int n, int npad, float scale, void* stream);

/* boundary layout: planar [Cv, npix] (the reference's [C,T,H,W]) <-> channels-last [npix, Cpad] bf16.
 * dtype: 0 fp32, 1 bf16.  cl_to_video optionally clamps to [-1, 1] (wan_vae.py:669). */
wan_status_t wan_video_to_cl(const void* video, int in_dtype, void* out_bf16, int Cv, int Cpad, int64_t npix, void* stream);
wan_status_t wan_cl_to_video(const void* x_bf16, int64_t ld, void* out, int out_dtype, int Cv, int64_t npix,
                             int clamp, void* stream);

/* ===========================================================================
 * Frames in, frames out: the uint8 frames of a video reader / writer on the device, on both sides of the VAE.
 * ------------------------------------------------------------------------- */

/* uint8 [B, T, H, W, 3] (interleaved, as read) -> [B, 3, T, H, W] planar in out_dtype (0 fp32, 1 bf16):
 *     out = cast(float32(u) * float32(2.0 / 255.0) - 1.0f), two float32 operations rounded one after the other (no FMA),
 *     then one round-to-nearest-even cast -- what AutoencoderKLWan.encode consumes, no further cast in between.
 * replaces: load_video_frames' host conversion `permute([3, 0, 1, 2]).unsqueeze(0).float()`, `x * (2.0 / 255.0) - 1.0`
 *           (fast_infer.py:88-90; inference.py the same) and the pipeline's `video.to(device, dtype)` (pipeline_wan.py:397).
 * Any H, W, T; B * T <= 65535.  H * W % 16 == 0 with 16-byte aligned tensors moves 16 bytes per access. */
wan_status_t wan_frames_u8_to_video(const void* frames_u8, void* out, int out_dtype, int B, int T, int H, int W,
                                    void* stream);

/* the decoder's output [B, 3, T, H, W] (in_dtype 0 fp32, 1 bf16), frames [t0, t0 + nt) -> uint8 [B, T_out, H, W, 3] from
 * frame t_dst on (so that the grounding and the edit segment of a CoF call land in their slices of one clip):
 *     u8 = trunc(float32(clamp(x / 2 + 0.5, 0, 1)) * 255.0f), `x / 2` and `+ 0.5` each rounded to in_dtype as a torch
 *     tensor op of that dtype rounds them.
 * replaces: decode_latents' `(frames / 2 + 0.5).clamp(0, 1)`, `.cpu().float().numpy()` (pipeline_wan.py:423-428) and
 *           save_videos_grid's `b c t h w -> t h w c` rearrangement and `(x * 255).numpy().astype(np.uint8)`
 *           (videox_fun/utils/utils.py:59-68; one video per call: make_grid is the identity).
 * Any H, W, T; B * nt <= 65535; nt == 0 enqueues nothing. */
wan_status_t wan_video_to_frames_u8(const void* video, int in_dtype, void* frames_u8, int B, int T, int H, int W,
                                    int t0, int nt, int T_out, int t_dst, void* stream);

/* The same two conversions on a rectangle of the frame (`edit_region_vae_halo`): the VAE encodes and decodes the BOX
 * only -- the edit region's rectangle widened by a halo -- and the frames that come back are the source's own bytes outside the
 * region's rectangle.  videocof_amd/edit_region.py states each in plain torch / numpy (reference_frames_box_to_video,
 * reference_video_box_stitch) and the kernels equal them bit for bit and byte for byte.
 * replaces: nothing in the reference, which encodes and decodes whole frames.
 * Common to both: the box is rows [by, by + bh), columns [bx, bx + bw) of the H x W frame, in pixels, any box inside the frame.  Streams
 * of rows at a pitch as wan_region_crop's; the access unit is the largest of 16, 8, 4, 2 or 1 pixels that divides W, bx, bw and the byte
 * tensors' base addresses and leaves the planes' words aligned, so no unit straddles the box's edge.  Everything is validated on the host
 * before anything is enqueued; each enqueues ONE kernel on `stream` and never synchronises.
 * wan_frames_u8_box_to_video (beside wan_frames_u8_to_video): frames uint8 [B, T, H, W, 3] -> out [B, 3, T, bh, bw] in out_dtype (0 fp32,
 *     1 bf16), out[b, c, t, y, x] = cast(float32(frames[b, t, by + y, bx + x, c]) * float32(2.0 / 255.0) - 1.0f): that kernel's
 *     arithmetic, and with the whole-frame box that kernel's bits.  A null tensor, a count below 1, another dtype, a box that does not
 *     lie inside the frame, B * T or H * W * 3 of 2^31 or more -> WAN_ERR_INVALID.
 * wan_video_box_stitch_u8 (beside wan_video_to_frames_u8 and wan_frames_u8_composite): video [B, 3, T, bh, bw] (the decoder's output on
 *     the box; in_dtype 0 fp32, 1 bf16), frames [t0, t0 + nt), and source uint8 [Bs, Ts, H, W, 3] (Bs = 1 or B), frames [src_t0,
 *     src_t0 + nt) -> frames uint8 [B, T_out, H, W, 3], frames [t_dst, t_dst + nt), every byte of them written exactly once.  With o the
 *     source's byte, e the decoder's sample converted exactly as wan_video_to_frames_u8 converts it, (ry, rx, rh, rw) the region's
 *     rectangle in frame pixels (inside the box) and f = feather:
 *         outside the rectangle   out = o
 *         inside it               d   = the least distance of the pixel to an edge of the rectangle that does NOT lie on the frame's
 *                                       border (top: y - ry if ry > 0; bottom: ry + rh - 1 - y if ry + rh < H; left and right likewise;
 *                                       no such edge: infinity)
 *                                 a   = 255 if f == 0 or d >= f else (255 * (d + 1)) / (f + 1)                 (floor)
 *                                 out = (a * e + (255 - a) * o + 127) / 255          (wan_frames_u8_composite's formula, floor, exact)
 *     feather 0 is the literal stitch; a rectangle that is the whole frame gives wan_video_to_frames_u8's bytes.  The decoder's samples
 *     outside the rectangle are never read.  `source_u8` and `frames_u8` must not overlap.  nt == 0 enqueues nothing.  A null tensor, a
 *     count below 1, Bs not 1 or B, another dtype, a box not inside the frame, a rectangle not inside the box, a negative feather,
 *     t0 + nt > T, src_t0 + nt > Ts, t_dst + nt > T_out, B * nt or H * W * 3 of 2^31 or more, a side above 2^24 -> WAN_ERR_INVALID. */
wan_status_t wan_frames_u8_box_to_video(const void* frames_u8, void* out, int out_dtype, int B, int T, int H, int W, int by, int bx,
                                        int bh, int bw, void* stream);
wan_status_t wan_video_box_stitch_u8(const void* video, int in_dtype, const void* source_u8, void* frames_u8, int B, int Bs, int T,
                                     int Ts, int T_out, int H, int W, int by, int bx, int bh, int bw, int ry, int rx, int rh, int rw,
                                     int feather, int t0, int nt, int src_t0, int t_dst, void* stream);

/* Fit a clip to another size: resample (antialiased triangle) and crop uint8 [B, T, H, W, 3] -> uint8 [B, T, Ho, Wo, 3] in one launch.
 * replaces: nothing in the reference's inference path, which hands the clip's own size to the pipeline (fast_infer.py:409-423), so its
 *           users resize per frame on the host; the geometry is the training loader's resize and centre crop
 *           (videox_fun/data/dataset_image_video.py:464-477), the filter Pillow's 8-bit BILINEAR resample, whose support widens with
 *           the downscale factor.
 * Two separable passes over bytes, horizontal first, the intermediate rounded to a byte; per axis and output index i
 *     out[i] = min(255, (2^21 + sum_{j < n[i]} in[xmin[i] + j] * k[i][j]) >> 22)           (32-bit integers, k >= 0, sum_j k = 2^22)
 * xtab / ytab: one table per axis in device memory, for the Wo / Ho output indices that are produced (a crop only selects them):
 *     int32 xmin[n_out] | int32 n[n_out] | int32 k[n_out][taps]       (taps = kx / ky = the axis' largest n, k zero from n[i] on)
 *     = wan_frames_resample_table_bytes(n_out, taps) bytes.  The host builds them in float64 (videocof_amd/video_io.py,
 *     resample_axis_table); the kernel does no floating point.  Windows are clamped to the source and to the tile's staging, so a
 *     malformed table gives wrong bytes, never an access outside the tensors.
 * taps <= WAN_RESAMPLE_MAX_TAPS per axis (24: a downscale of about 11x; 8x needs 17, 19 at a border) -> else WAN_ERR_UNSUPPORTED;
 * B * T <= 65535 -> else WAN_ERR_UNSUPPORTED; a frame below 2 GiB.  Any H, W, Ho, Wo and any alignment: source rows are read with
 * 16-byte loads from the 16-byte boundary below their first byte, output pieces are stored as dwordx4 where their address allows.
 * Enqueues one kernel on `stream`; never synchronises. */
#define WAN_RESAMPLE_MAX_TAPS 24
int64_t wan_frames_resample_table_bytes(int n_out, int taps);
wan_status_t wan_frames_u8_resample(const void* src_u8, void* dst_u8, int B, int T, int H, int W, int Ho, int Wo,
                                    const void* xtab, int kx, const void* ytab, int ky, void* stream);

/* The writer's grid and the side-by-side compare clip: n_src source clips placed into rectangles of ONE uint8 [T_out, Hc, Wc, 3]
 * canvas in one launch, each converted to bytes on the way; every canvas byte is written, what no source covers with the byte `pad`
 * (make_grid's border and empty cells are 0 BEFORE the writer's `rescale`: pad = 0, or trunc((0 + 1) / 2 * 255) = 127 with it).
 * replaces: save_videos_grid for more than one sample -- torchvision's make_grid(nrow=6, padding=2, pad_value=0) mosaic, `rescale`,
 *           `(x * 255).numpy().astype(np.uint8)` (videox_fun/utils/utils.py:59-68) -- and save_side_by_side (fast_infer.py:183-206):
 *           _normalize_to_01 of both clips, the crop to the common T/H/W from the start of each axis, torch.cat(dim=4), the writer.
 * A source (wan_compose_src) is a strided view: `base` = its element [0, 0, 0, 0], strides in elements, `extent` = the elements
 * addressable from `base` (the geometry is checked against it).  kind: uint8 interleaved [T, H, W, 3] (stride_c = 1 between the
 * channels of a pixel) or planar float32 / bf16 [3, T, H, W].  Frames [t0, t0 + nt), rows [y0, y0 + h), columns [x0, x0 + w) of it
 * go to the canvas frames [0, nt) at (dst_y, dst_x); canvas frames from nt on are pad there.  mode:
 *     COPY              (uint8)  the bytes as they are
 *     LOADER_ROUNDTRIP  (uint8)  what the reference's compare clip shows of a clip it loaded:  v = float32(u) * float32(2.0 / 255.0) - 1.0f
 *                                (fast_infer.py:88-90), _normalize_to_01(v), trunc(. * 255.0f) -- NOT the identity on bytes
 *     WRITER            (float)  trunc(x * 255.0f), of (x + 1.0f) / 2.0f when `rescale` is set (utils.py:65-67); no clamp, as there: outside
 *                                [0, 256) the reference's conversion is undefined, here it is the low byte of the truncated int32
 *     NORMALIZE         (float)  _normalize_to_01 (fast_infer.py:183-189), then the writer: trunc(clamp(r(x), 0, 1) * 255.0f) with
 *                                r(x) = (x + 1.0f) / 2.0f if the tensor's minimum is < 0 or its maximum > 1, else x
 * Every float32 operation is rounded on its own (no FMA); a bf16 source rounds `x + 1.0` and `/ 2.0` to bf16 as torch's tensor ops do.
 * The range rule is decided ON THE DEVICE: `rescale_flag` points to the int32 wan_video_range_flag wrote for the WHOLE tensor the
 * reference would hand to _normalize_to_01 (required for NORMALIZE; optional for LOADER_ROUNDTRIP, where NULL means the rescale is
 * taken -- true of every clip with a byte below 128; not allowed otherwise); the host never reads it.
 * Destination rectangles may not overlap; n_src <= WAN_COMPOSE_MAX_SRC (16), T_out <= 65535 -> else WAN_ERR_UNSUPPORTED.  A window
 * that leaves its tensor or a rectangle that leaves the canvas is WAN_ERR_INVALID before anything is enqueued.  Any H, W and
 * alignment: the canvas is stored in 16-byte pieces cut at 16-byte addresses (dwordx4 inside a row, bytes at its two ends); a piece
 * inside one interleaved uint8 source is read as two aligned 16-byte words, everything else element by element.
 * Enqueues one kernel on `stream`; never synchronises. */
#define WAN_COMPOSE_MAX_SRC 16
enum { WAN_COMPOSE_U8 = 0, WAN_COMPOSE_F32 = 1, WAN_COMPOSE_BF16 = 2 };
enum { WAN_COMPOSE_COPY = 0, WAN_COMPOSE_LOADER_ROUNDTRIP = 1, WAN_COMPOSE_WRITER = 2, WAN_COMPOSE_NORMALIZE = 3 };
typedef struct {
    const void* base;
    const int* rescale_flag; /* device int32 of wan_video_range_flag, or NULL */
    int64_t extent;
    int64_t stride_c, stride_t, stride_y, stride_x;
    int kind, mode, rescale;
    int t0, y0, x0, nt, h, w;
    int dst_y, dst_x;
} wan_compose_src;
wan_status_t wan_frames_u8_compose(const wan_compose_src* srcs, int n_src, void* canvas_u8, int T_out, int Hc, int Wc,
                                   int pad, void* stream);

/* _normalize_to_01's range rule (fast_infer.py:185-187) over n contiguous elements (kind as above; uint8 = the loader's float32 video
 * of those bytes) into one int32 in device memory: bit 0 = an element < 0 or > 1 was seen, bit 1 = a NaN was seen; the rule's
 * `vmin < 0.0 or vmax > 1.0` holds exactly when the word is 1 (torch's min / max of a tensor with a NaN are NaN, and both
 * comparisons with a NaN are false: no rescale).  Zeroes the word and enqueues one kernel on `stream`; never synchronises. */
wan_status_t wan_video_range_flag(const void* x, int kind, int64_t n, int* flag, void* stream);

/* 8-bit YCbCr planes <-> uint8 [T, H, W, 3] RGB frames: what a decoder yields (an ffmpeg pipe, an NV12 surface, a .y4m file) and what
 * an encoder takes, converted on the device -- 1.5 bytes per pixel cross the host link instead of 3, the host does no pixel arithmetic.
 * replaces: nothing in the reference, whose reader (imageio) converts to RGB on the host before load_video_frames sees a frame.
 * Planes (wan_yuv_planes): a base pointer each, `*_extent` = the bytes addressable from that base (the geometry is checked against
 * it and no load leaves it), strides in bytes.  Luma is H rows of W bytes; chroma is Ch x Cw samples, Cw = ceil(W / 2) if sub_x else
 * W, Ch = ceil(H / 2) if sub_y else H, `c_step` bytes from one sample of a plane to the next (1 planar; 2 for NV12-style interleaved
 * CbCr, where cr = cb + 1, or cb = cr + 1 for NV21).  cb = cr = NULL: mono (reading only; Cb = Cr = 128).  Any base alignment, any
 * row stride >= the row, any frame stride (writing: >= a frame).
 * Integer arithmetic only, all shifts arithmetic, every sum fits an int32 (videocof_amd/video_io.py: yuv_matrix builds the tables in
 * float64, reference_yuv_to_frames / reference_frames_to_yuv restate this in numpy and equal the kernels byte for byte):
 *   in   chroma up: per axis two samples with weights in quarters, indices clamped to the plane --
 *            not subsampled (c[i], 4);  centred: even i (c[i/2 - 1], 1), (c[i/2], 3), odd i (c[i/2], 3), (c[i/2 + 1], 1);
 *            left co-sited: even i (c[i/2], 4), odd i (c[i/2], 2), (c[i/2 + 1], 2)
 *        C = (sum over the 2 x 2 taps of wy * wx * c + 8) >> 4, one rounding; vertical always centred, horizontal by `cosited`;
 *        rgb[c] = clamp((k[3c] * (Y - yo) + k[3c + 1] * (Cb - 128) + k[3c + 2] * (Cr - 128) + 2^15) >> 16, 0, 255)
 *   out  (Y, Cb, Cr)[c] = clamp((k[3c] * R + k[3c + 1] * G + k[3c + 2] * B + (off[c] << 16) + 2^15) >> 16, 0, 255), off = (yo, 128, 128);
 *        4:2:0 (sub_x = sub_y = 1): (a + b + c + d + 2) >> 2 over each 2 x 2 block of those 8-bit chroma values, the last column / row
 *        repeated when W / H is odd (centre siting; `cosited` is not read); 4:4:4 (sub_x = sub_y = 0): the per-pixel values.  Other
 *        subsamplings are not written -> WAN_ERR_UNSUPPORTED.
 * wan_yuv_coef: the nine 16-bit fixed-point coefficients (|k| < 2^23) and the luma offset, by value from HOST memory.
 * A thread moves 16 pixels: 48 RGB bytes, 16 luma bytes, 8 or 16 chroma bytes per plane, each as dwordx4 / dwordx2 where its address
 * allows, as aligned dwords shifted with v_alignbyte_b32 elsewhere, byte by byte at the end of a row; no byte outside the described
 * rows is written.  T <= 65535 -> else WAN_ERR_UNSUPPORTED.  A geometry that leaves an extent, planes that overlap on the way out or
 * a null argument is WAN_ERR_INVALID before anything is enqueued.  Enqueues one kernel on `stream`; never synchronises. */
typedef struct {
    void* y;
    void* cb;
    void* cr;
    int64_t y_extent, cb_extent, cr_extent;
    int64_t y_row, y_frame, c_row, c_frame;
    int c_step, sub_x, sub_y, cosited;
} wan_yuv_planes;
typedef struct {
    int k[9];
    int yo;
} wan_yuv_coef;
wan_status_t wan_yuv_to_frames_u8(const wan_yuv_planes* planes, const wan_yuv_coef* inverse, void* frames_u8, int T, int H, int W,
                                  void* stream);
wan_status_t wan_frames_u8_to_yuv(const void* frames_u8, const wan_yuv_planes* planes, const wan_yuv_coef* forward, int T, int H, int W,
                                  void* stream);

/* Keep what the edit left alone: where did the edit change the frames the pipeline saw (a feathered uint8 mask), and the edit put back
 * over the ORIGINAL clip under that mask, the original's bytes kept wherever nothing was edited or the fit cropped the frame away.
 * replaces: nothing in the reference, which returns the whole clip as the VAE and the DiT left it; callers composite on the host in float.
 * Integer arithmetic only (videocof_amd/video_io.py: reference_change_mask / reference_composite_frames restate this in numpy int64 and
 * equal the kernels byte for byte).
 *
 * wan_change_mask: source, edit uint8 [B, T, H, W, 3] (any base alignment) -> alpha uint8 [B, T, H, W].  Per sample and frame:
 *     d     = max_c |edit - source|
 *     s     = (2 S + n) / (2 n),   S = sum of d over the (2 smooth + 1)^2 window with indices clamped to the frame, n = (2 smooth + 1)^2
 *     b     = s > threshold
 *     g     = max of b over the (2 grow + 1)^2 window and the frames t - grow_t .. t + grow_t; positions outside the frame or outside the
 *             sample's T frames are ignored (the maximum never crosses from one sample of a batch into the next)
 *     alpha = (2 * 255 * C + m) / (2 m),   C = count of g over the (2 feather + 1)^2 window with clamped indices, m = (2 feather + 1)^2
 * all divisions floor.  feather <= grow is what makes b = 1 imply alpha = 255: every pixel of the feather window around it has g = 1.
 * 0 <= threshold <= 254, smooth <= WAN_MASK_MAX_SMOOTH, grow <= WAN_MASK_MAX_GROW, grow_t <= WAN_MASK_MAX_GROW_T, feather <= grow, none
 * negative -> else WAN_ERR_INVALID before anything is enqueued.  B * T <= 65535 -> else WAN_ERR_UNSUPPORTED.  `workspace`: device memory of
 * wan_change_mask_workspace_bytes(B, T, H, W) bytes (the b and g planes).  Enqueues three kernels on `stream`; never synchronises. */
#define WAN_MASK_MAX_SMOOTH 7
#define WAN_MASK_MAX_GROW 32
#define WAN_MASK_MAX_GROW_T 4
int64_t wan_change_mask_workspace_bytes(int B, int T, int H, int W);
wan_status_t wan_change_mask(const void* source_u8, const void* edit_u8, void* alpha_u8, int B, int T, int H, int W, int threshold,
                             int smooth, int grow, int grow_t, int feather, void* workspace, int64_t workspace_bytes, void* stream);

/* wan_frames_u8_resample's two passes on one-channel planes (the alpha of wan_change_mask brought to the size of the source window):
 * uint8 [N, H, W] -> uint8 [N, Ho, Wo], horizontal pass first into `tmp_u8` (N * H * Wo bytes, rounded to bytes), then the vertical pass;
 * the same tables, the same arithmetic, the same limits on the tap counts.  Windows are clamped to the plane: a malformed table gives
 * wrong bytes, never an access outside the tensors.  N <= 65535 and Ho <= 65535 -> else WAN_ERR_UNSUPPORTED.  Enqueues two kernels on
 * `stream`; never synchronises. */
wan_status_t wan_plane_u8_resample(const void* src_u8, void* tmp_u8, void* dst_u8, int N, int H, int W, int Ho, int Wo, const void* xtab,
                                   int kx, const void* ytab, int ky, void* stream);

/* original uint8 [N, Ho, Wo, 3], edit uint8 [N, wh, ww, 3], alpha uint8 [N, wh, ww] -> out uint8 [N, Ho, Wo, 3] (N = B * T frames):
 *     inside the window rows [wy, wy + wh), columns [wx, wx + ww), per byte   out = (a * e + (255 - a) * o + 127) / 255   (floor, exact)
 *     outside it                                                              out = o
 * With the window the whole frame this is the same-size composite.  Any sizes and alignment: a thread moves 16 pixels, each of its runs
 * as dwordx4 where its address allows.  A window that leaves the frame is WAN_ERR_INVALID; N <= 65535 -> else WAN_ERR_UNSUPPORTED.
 * Enqueues one kernel on `stream`; never synchronises. */
wan_status_t wan_frames_u8_composite(const void* original_u8, const void* edit_u8, const void* alpha_u8, void* out_u8, int N, int Ho,
                                     int Wo, int wy, int wx, int wh, int ww, void* stream);

/* Clip statistics: how far is clip b from clip a, per frame, in exact integers, split by a mask.  a, b uint8 [N, H, W, 3] (N = B * T
 * frames, any base alignment), alpha uint8 [N, H, W] or NULL -> stats int64 [N][2][WAN_CLIP_STATS_WORDS].  A pixel's region r is 1 where
 * alpha != 0, else 0 (NULL: every pixel in region 0).  Per frame and region:
 *     [0, 256)    the byte histogram: the number of bytes (all three channels) of the region's pixels with |a - b| == v
 *     [256, 512)  the smoothed histogram: the number of the region's pixels with s == v, s of wan_change_mask above (d = max_c |a - b|,
 *                 s = (2 S + n) / (2 n) over the (2 smooth + 1)^2 window with clamped indices), 0 <= smooth <= WAN_MASK_MAX_SMOOTH
 *     [512]       the SSIM sum: the sum of q over the region's windows, signed
 *     [513]       the number of those windows
 * SSIM is the 8-bit form of x264 / ffmpeg's `ssim` filter on each colour plane by itself: h4 = H >> 2, w4 = W >> 2 (rows and columns from
 * 4 h4 and 4 w4 on are not read for it); per 4 x 4 block the sums of a, of b, of a^2 + b^2 and of a b; a window is 2 x 2 neighbouring
 * blocks (8 x 8 pixels at stride 4, (h4 - 1)(w4 - 1) of them per plane) with the blocks' sums added to s1, s2, ss, s12;
 *     vars = 64 ss - s1^2 - s2^2,  covar = 64 s12 - s1 s2
 *     q = rint((double)(2 s1 s2 + 416) * (double)(2 covar + 235963) / ((double)(s1^2 + s2^2 + 416) * (double)(vars + 235963)) * 2^20)
 * two rounded products, one IEEE division, round half to even; identical windows give exactly 2^20.  A window is in region 1 if any of
 * its 64 alpha bytes is non-zero.  h4 < 2 or w4 < 2: no windows, both words 0.
 * Every word of stats is overwritten, nothing is accumulated into; counts are exact and independent of the order of execution (integer
 * adds only; videocof_amd/video_io.py: reference_clip_stats restates this in numpy and equals the kernels word for word).  A null a, b or
 * stats, a size below 1, smooth out of range or a workspace below wan_clip_stats_workspace_bytes(N, H, W) bytes -> WAN_ERR_INVALID;
 * N > 65535 or a frame of 2 GiB or more -> WAN_ERR_UNSUPPORTED; both before anything is enqueued.  Enqueues four kernels on `stream`;
 * never synchronises. */
#define WAN_CLIP_STATS_WORDS 514          /* 256 + 256 + 2 */
int64_t wan_clip_stats_workspace_bytes(int N, int H, int W);
wan_status_t wan_clip_stats(const void* a_u8, const void* b_u8, const void* alpha_u8, void* stats_i64, int N, int H, int W, int smooth,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* Colour match: bring the edit's colours back to the source's with one gain and offset per frame and channel, estimated where the edit
 * left the frame alone, in exact integers (videocof_amd/video_io.py: reference_color_stats / reference_color_coefficients /
 * reference_frames_affine restate this in Python ints and numpy and equal the kernels word for word).
 * replaces: color_transfer_post_process of save_videos_grid (videox_fun/utils/utils.py:31-57) in PURPOSE only: that one is Reinhard's
 * transfer in OpenCV's 8-bit LAB; this one is the same mean / deviation transfer per RGB channel.  A hue rotation is not corrected, and
 * neither is a shift that varies over the frame.
 *
 * wan_color_stats: ref uint8 [B, ref_T, H, W, 3], edit uint8 [B, T, H, W, 3] (any base alignment), alpha uint8 [B, ref_T, H, W] or NULL
 * -> stats int64 [B * T][WAN_COLOR_STATS_WORDS].  ref_T is T, or 1: that one frame (and its alpha) is then paired with every frame of the
 * sample.  A pixel counts where its alpha == 0 (NULL: every pixel).  Per frame, over the counted pixels:
 *     [0]                 n   their number
 *     [1 + 4 c + 0]       A   the sum of ref's channel c          [1 + 4 c + 1]   E   the sum of edit's
 *     [1 + 4 c + 2]       AA  the sum of ref's squares            [1 + 4 c + 3]   EE  the sum of edit's squares
 *     [13, 16)            0
 * Every word is overwritten; integer adds only, so the result does not depend on the order of execution.  A null ref, edit or stats, a
 * size below 1, ref_T other than 1 or T, or a workspace below wan_color_stats_workspace_bytes(B * T, H, W) bytes -> WAN_ERR_INVALID;
 * B * T > 65535 or a frame of 2 GiB or more -> WAN_ERR_UNSUPPORTED; both before anything is enqueued.  Enqueues two kernels on `stream`
 * (both clips are read once); never synchronises.
 *
 * wan_color_coef: stats int64 [B * T][16] as above -> coef int32 [B * T][3][2] = (g, b) per frame and channel, ONE = WAN_COLOR_ONE:
 *     the sums of frame t are first replaced by the sums over frames t - pool_t .. t + pool_t of the SAME sample (0 <= pool_t <=
 *     WAN_COLOR_MAX_POOL_T; pool_t >= T - 1 gives one transform per sample)
 *     n < max(1, min_pixels):   g = ONE, b = 0
 *     else   Vs = n AA - A A,  Ve = n EE - E E   (128-bit)
 *            g = ONE                                          if gain == 0 or Ve == 0
 *            k = max(0, bit_length(max(Vs, Ve)) - 38),  vs = Vs >> k,  ve = Ve >> k
 *            g = 2 ONE if ve == 0, else floor(sqrt((vs << 24) / ve)) (floor division, integer square root), clamped to [ONE / 2, 2 ONE]
 *            b = floor((ONE A - g E + (n >> 1)) / n)
 * No floating point anywhere.  The sums have to be sums: Vs, Ve >= 0.  A null pointer, B or T below 1, B * T above 2^24, pool_t out of
 * range or min_pixels < 0 -> WAN_ERR_INVALID.  Enqueues one kernel on `stream`; never synchronises.
 *
 * wan_frames_u8_affine: frames uint8 [N, H, W, 3] (any alignment), coef int32 [N][3][2] -> out uint8 of the frames' shape, per byte x of
 * channel c (its index mod 3) of frame f:   out = clamp((g x + b + ONE / 2) >> 12, 0, 255)   with an arithmetic shift, computed in 32
 * bits: -2^21 <= g <= 2^21 and -2^30 <= b <= 2^30 are the caller's to keep (wan_color_coef's are far inside).  out may be frames (in
 * place): a thread reads its bytes before it writes them, and no thread writes another's.  N <= 65535 and a frame below 2 GiB -> else
 * WAN_ERR_UNSUPPORTED.  Enqueues one kernel on `stream`; never synchronises. */
#define WAN_COLOR_STATS_WORDS 16
#define WAN_COLOR_ONE 4096
#define WAN_COLOR_MAX_POOL_T 8
int64_t wan_color_stats_workspace_bytes(int N, int H, int W);
wan_status_t wan_color_stats(const void* ref_u8, const void* edit_u8, const void* alpha_u8, void* stats_i64, int B, int T, int ref_T,
                             int H, int W, void* workspace, int64_t workspace_bytes, void* stream);
wan_status_t wan_color_coef(const void* stats_i64, void* coef_i32, int B, int T, int pool_t, int gain, int min_pixels, void* stream);
wan_status_t wan_frames_u8_affine(const void* frames_u8, const void* coef_i32, void* out_u8, int N, int H, int W, void* stream);

/* ===========================================================================
 * the umT5 text encoder (videox_fun/models/wan_text_encoder.py:256-304), the step
 * before the denoising path.  Its Linear layers are wan_gemm_bf16; the rest:
 * ------------------------------------------------------------------------- */

/* Strided-batched nn.Linear-style product: for z in [0, batch):
 *     out_z[m, n] = sum_k A_z[m, k] * W_z[n, k],  X_z = X + z * strideX (elements)
 * replaces: torch.einsum('binc,bjnc->bnij', q, k) and einsum('bnij,bjnc->binc', attn, v)
 *           of T5Attention.forward (wan_text_encoder.py:102-105), one problem per head.
 * epilogue: WAN_EPI_BF16 or WAN_EPI_F32, no bias.  K % 64 == 0, N % 4 == 0, strides of A/W % 8 == 0. */
wan_status_t wan_gemm_bf16_batched(const void* A, int64_t lda, int64_t strideA, const void* W, int64_t ldw,
                                   int64_t strideW, void* out, int64_t ldo, int64_t strideO,
                                   int M, int N, int K, int batch, int epilogue, void* stream);

/* nn.Embedding gather (wan_text_encoder.py:286-287): out fp32 [rows, dim] = table_bf16[ids[r], :].
 * ids are clamped into [0, vocab) for memory safety; the caller validates the range. */
wan_status_t wan_embedding_rows(const int64_t* ids, const void* table_bf16, int64_t vocab, float* out,
                                int64_t rows, int dim, void* stream);

/* T5LayerNorm (wan_text_encoder.py:48-60): out = x * rsqrt(mean(x^2) + eps) * w, x fp32 [rows, dim],
 * w fp32 [dim]; out_dtype 0 fp32, 1 bf16.  dim % 4 == 0, dim <= 8192. */
wan_status_t wan_rmsnorm_rows(const float* x, const float* w, void* out, int out_dtype, int64_t rows, int dim,
                              float eps, void* stream);

/* T5Attention score softmax (wan_text_encoder.py:93-104) with the relative-position bias of
 * T5RelativeEmbedding (:226-260) evaluated in place:
 *     probs[h, i, j] = softmax_j(scores[h, i, j] + bucket_table[bucket_lut[j - i + Lq - 1], h]),  j < k_len
 * and 0 for k_len <= j < npad (attention_mask == 0 keys, :98-99, and the K padding of the P.V product).
 * scores fp32 [H*Lq, lds]; bucket_table fp32 [num_buckets, H] (pos_embedding.embedding.weight);
 * bucket_lut int32 [Lq + Lk - 1] = _relative_position_bucket(j - i) (:245-264); probs bf16 [H*Lq, ldp]. */
wan_status_t wan_t5_softmax_bias(const float* scores, int64_t lds, const float* bucket_table,
                                 const int* bucket_lut, void* probs_bf16, int64_t ldp, int num_heads,
                                 int Lq, int Lk, int k_len, int npad, void* stream);

/* gated-GELU feed-forward product fc1(x) * gelu(gate(x)) (wan_text_encoder.py:125-126): out = a * b, bf16, n % 8 == 0. */
wan_status_t wan_mul_bf16(const void* a, const void* b, void* out, int64_t n, void* stream);

/* ---------------------------------------------------------------------------
 * Box fingerprint for benchmarks (no reference counterpart: the reference has no benchmark harness).  A FIXED calibration
 * workload, independent of the product kernels: (a) ~target_ms of 32x32x16 bf16 MFMAs on random operands beside LDS fragment
 * reads and a softmax VALU stream (the instruction mix of a flash-attention tile), one 4-wave workgroup per CU -- what the
 * matrix pipes of THIS box hold at its power limit; (b) 40 passes of a 256 MiB -> 256 MiB copy.  Unlike every other entry
 * point this call SYNCHRONISES the stream (it reads HIP events) -- it is a measurement, never part of a timed region.
 * scratch: device memory of >= wan_box_probe_scratch_bytes(), caller-owned.  target_ms <= 0 selects 300.
 * bench.py runs it before and after the timed region (`box` object, `value_normalised`).
 * ------------------------------------------------------------------------- */
typedef struct {
    float mfma_mix_tflops;   /* issued MFMA FLOP / time of the last two of three equal launches */
    float copy_tbps;         /* (read + write) bytes / time */
    float mfma_ms, copy_ms;  /* the measured intervals */
} wan_box_probe_result;
int64_t wan_box_probe_scratch_bytes(void);
wan_status_t wan_box_probe(wan_box_probe_result* result, void* scratch, int64_t scratch_bytes, int target_ms, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WAN_HIP_H */
