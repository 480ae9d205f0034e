/* libsincformer_hip.so — C ABI of the MI355X (gfx950) hot path.
 *
 * The reference (pure Python / PyTorch) has no FFI layer: its operator boundary
 * for this path is the set of aten dispatch sites listed in SURVEY.md §2b
 * (K1..K17).  Each entry point below replaces the cited reference call site.
 * Conventions:
 *   - plain pointers to DEVICE memory + sizes; no torch types; `stream` is a
 *     hipStream_t passed as void* (0 = default stream).
 *   - enqueue-only: every call is asynchronous on `stream`, allocates nothing,
 *     keeps no global state (thread-safe per stream), never throws.
 *   - returns 0 (SFM_OK) or a negative error: -1 bad argument, -2 unsupported
 *     shape, -3 launch failure.
 *   - `dtype` selects the 16-bit MFMA operand / activation format:
 *       0 = bf16, 1 = fp16 (accumulation is always fp32).
 *   - "16-bit" tensors are raw uint16_t words of that format.
 */
#ifndef SINCFORMER_HIP_H
#define SINCFORMER_HIP_H
#ifdef __cplusplus
extern "C" {
#endif

#define SFM_OK 0
#define SFM_ERR_ARG (-1)
#define SFM_ERR_SHAPE (-2)
#define SFM_ERR_LAUNCH (-3)
#define SFM_DT_BF16 0
#define SFM_DT_F16 1

/* epilogues of sfm_gemm16 */
#define SFM_EPI_NONE 0
#define SFM_EPI_SWISH 1      /* x*sigmoid(x)           models/conformer.py:45          */
#define SFM_EPI_GELU 2       /* erf GELU               agents/msa.py:45,64,69          */
#define SFM_EPI_RESID 3      /* resid + alpha*v        models/conformer.py:49,71,128   */
#define SFM_EPI_GLU 4        /* a*sigmoid(g)           models/conformer.py:114         */
#define SFM_EPI_SIGMOID 5
#define SFM_EPI_TANH_SCALE 6
#define SFM_EPI_SIGMA 7      /* exp(.5*clamp(v,-10,10)) agents/perception.py:249       */
#define SFM_EPI_CPEA 8       /* sigmoid | alpha*tanh   agents/cpea.py:102-105          */

/* ---- shared constants: the tile sizes, limits and mode codes that the host wrappers must agree with the kernels on.  This is
 * their one statement: the kernels use these names (a number a kernel derives is tied to its name here by a static_assert), and
 * the Python side reads every `#define SFM_<NAME> <literal>` line of this header into lib.CONSTANTS.  Plain literals only. */
#define SFM_LAYERNORM_MAX_D 512        /* sfm_layernorm / sfm_layernorm_bwd_*: the widest row they normalise (and so the widest Conformer d_model) */
#define SFM_ATTN_QTILE 128             /* query rows of a workgroup of attn_fwd_hd64_kernel: the tile of sfm_attention_fwd_varlen's items */
#define SFM_XCDS 8                     /* workgroups are dealt round-robin over this many XCDs ... */
#define SFM_XCD_RUN 8                  /* ... and the head_dim-64 attention kernels give each XCD runs of this many consecutive logical items */
#define SFM_DWCONV_TILE 64             /* frames of a workgroup of the register-resident depthwise kernels: the tile of sfm_dwconv_folded_varlen's table */
#define SFM_SINC_FIR16_WS_WORDS 278528 /* 16-bit words of sfm_sinc_fir16's staging buffer wsh (8 shifts x (hi, lo) x 64 channels x 272 padded taps) */
#define SFM_SINC_FIR16_STREAM1 (-1)    /* sfm_sinc_fir16_ex's passes: one pass by the streaming kernel (taps in LDS), the bitwise reference of passes = 1 */
#define SFM_PSTOI_MAX_BANDS 32        /* sfm_pstoi_loss: NB, F and frame_len (2 ..) it takes */
#define SFM_PSTOI_MAX_BINS 257
#define SFM_PSTOI_MIN_FRAME_LEN 2
#define SFM_PSTOI_MAX_FRAME_LEN 32
#define SFM_MIX_CHUNK 4096             /* samples per workgroup of sfm_mix_scale / sfm_mix_apply */
#define SFM_QUANT_MAX_STEPS 16         /* sfm_mask_quantize, sfm_curriculum_mask, sfm_pso_*: M in 2 .. this */
#define SFM_MASK_NONE 0                /* sfm_curriculum_mask's kind */
#define SFM_MASK_IRM 1
#define SFM_MASK_PCIRM 2
#define SFM_MASK_OPT_PCIRM 3
#define SFM_PSO_CHUNK 4096             /* samples per workgroup of sfm_pso_split */
#define SFM_PSO_FRAMES 8               /* STOI frames per workgroup of sfm_pso_fitness */
#define SFM_PSO_MAX_PARTICLES 256
#define SFM_PSO_MAX_BINS 1024
#define SFM_GT_COLS 64                 /* channel columns of the tap and twiddle operands (C <= 64, zero beyond C) */
#define SFM_GT_ROWS 384                /* samples per workgroup of sfm_gammatone_fir / sfm_gammatone_tf */
#define SFM_GT_MAX_TAPS 2048
#define SFM_GT_LDS_MAX 163840          /* bytes of LDS sfm_gammatone_tf may ask for (160 KiB) */
#define SFM_FE_MAX_FILTERS 64          /* sfm_cepstral / sfm_rasta: filters or channels per row, bins per row, DCT rows */
#define SFM_FE_MAX_BINS 257
#define SFM_FE_MAX_COEFFS 16
#define SFM_CEP_POWER 0                /* sfm_cepstral's in_mode */
#define SFM_CEP_MAGNITUDE 1
#define SFM_CEP_BLOCKS 2
#define SFM_CEP_NONE 0                 /* its compress */
#define SFM_CEP_LOG 1
#define SFM_CEP_CBRT 2
#define SFM_HC_PARAMS 12               /* sfm_haircell*: par = {A, B, y, l, r, x, h, M, dt, q0, c0, w0}, fp64 */
#define SFM_ADV_MAX_WIDTH 512          /* AdversarialLoss: first-layer Cin after zero padding (257 bins -> 512) */
#define SFM_ADV_LO_SCALE 2048.0        /* adversarial.hip: a forward operand is hi + lo / 2048 */
#define SFM_CSII_BINS 129              /* rfft(., 256) bins of the coherence */
#define SFM_HE_ROWS 256                /* output samples per workgroup of the Hilbert kernel (its output tile) */
#define SFM_HE_KSTEP 64                /* input samples per staged k-step (one accumulation segment) */
#define SFM_DNN_ROW_TILE 128           /* rows of a workgroup of dnn_layer_kernel */
#define SFM_DNN_ACT_NONE 0             /* sfm_dnn_layer / sfm_dnn_act_bwd: act */
#define SFM_DNN_ACT_RELU 1
#define SFM_DNN_ACT_SIGMOID 2
#define SFM_DNN_CONTEXT_MAX_K 4096     /* context rows with statistics: mean and std sit in LDS beside the tiles */
#define SFM_MSE_GATHER_MAX_BLOCKS 1024 /* sfm_mse_gather_loss: workgroups at most, one fp64 partial each = its ws in doubles */
#define SFM_MOMENTS_CHUNK_ROWS 256     /* sfm_context_moments: rows of a chunk at least */
#define SFM_MOMENTS_MAX_CHUNKS 1024    /* chunks at most; ws = (SFM_MOMENTS_MAX_CHUNKS + 1) D (2 ctx + 1) doubles */
#define SFM_RESYNTH_TILE_FRAMES 64     /* frames a workgroup of sfm_mask_resynth computes; it owns one output hop fewer */
#define SFM_RESYNTH_BWD_TILE_FRAMES 64 /* frames, hence rows of dmask, a workgroup of sfm_mask_resynth_bwd computes */
#define SFM_RESYNTH_MAX_NFFT 256      /* the largest n_fft and frame its LDS layout holds */
#define SFM_RESYNTH_MAX_FRAME 256
#define SFM_RESYNTH_MAX_CHANNELS 64
#define SFM_RESYNTH_COL_ALIGN 32       /* operand columns (n_fft of Wf, frame of Wi) are zero padded to a multiple of this */
#define SFM_RBM_TILE 32                /* sfm_rbm_*: a workgroup's output tile is 32 x 32; ceil(n_visible / 32) fp64 error partials per step */
#define SFM_RBM_KCHUNK 256             /* k staged per pass of sfm_rbm_prob (sfm_rbm_update: half of it) */
#define SFM_RBM_MAX_UNITS 16384        /* n_visible, n_hidden in 1 .. this */
#define SFM_RBM_MAX_BATCH 65536        /* rows of one update */
#define SFM_RBM_SAMPLE_NONE 0          /* sfm_rbm_prob's sample_mode */
#define SFM_RBM_SAMPLE_REPLAY 1
#define SFM_RBM_SAMPLE_COUNTER 2

int sfm_abi_version(void);

/* Dense layer / channels-last Conv1d as implicit GEMM on 16-bit MFMA.
 * Replaces nn.Linear / nn.Conv1d call sites: models/conformer.py:44,47,113,122,
 * 209,222; in_proj/out_proj of nn.MultiheadAttention (:69); agents/msa.py:143,
 * 154-160; agents/perception.py:195,198,203 (conv_blocks), :168 (downsample),
 * :175,179 (real/imag proj), :185,187 (uncertainty head); agents/cpea.py:56-76.
 *   A   [B, Lin, Cin] 16-bit (position stride lda >= Cin, batch stride a_batch_stride; elements)
 *   W   [Npad, Kpad] 16-bit, row n = output channel, K order = (tap, cin);
 *       zero padded; Kpad % 64 == 0, Npad % 64 == 0
 *   out row (b, l) = epi( sum_{tap,ci} A[b, l*stride-pad+tap, ci] W[n,(tap,ci)] + bias[n] )
 *   gn_partial (optional): per (batch, row-half-tile, group) {sum, sumsq} of the
 *       pre-activation outputs, [B][2*ceil(Lout/128)][N/gn_group][2] floats.
 *   out_f32: 0 = 16-bit result in the operands' format `dtype`, 1 = fp32, 2 = 16-bit in the OTHER format (bf16 <-> fp16:
 *       a stage boundary of the host's precision policy; one rounding of the fp32 accumulators).
 */
int sfm_gemm16(const void* A, const void* W, const float* bias, void* out, const float* resid,
               float* gn_partial, int B, int Lout, int Lin, int Cin, int lda, int ksize, int stride, int pad,
               long long a_batch_stride, int Kpad, int N, int Npad, int ldo, long long o_batch_stride,
               int ldr, long long r_batch_stride, float alpha, int epi, int out_f32, int gn_group,
               int nsplit, int dtype, void* stream);

/* Same contract with an explicit kernel variant (A/B measurements): 0 auto, 2 = 128-row tiles with a 2-stage LDS-DMA ring,
 * 6 = persistent form, 9 = 256-row wide tiles, 10 = 512 x 128 tiles (gemm16v2.hip).  sfm_gemm16 == variant 0. */
int sfm_gemm16_ex(const void* A, const void* W, const float* bias, void* out, const float* resid,
                  float* gn_partial, int B, int Lout, int Lin, int Cin, int lda, int ksize, int stride, int pad,
                  long long a_batch_stride, int Kpad, int N, int Npad, int ldo, long long o_batch_stride,
                  int ldr, long long r_batch_stride, float alpha, int epi, int out_f32, int gn_group,
                  int nsplit, int dtype, int variant, void* stream);
/* sfm_gemm16_ex + residual-branch dropout in the EPI_RESID epilogue (training forward of models/conformer.py:48,70,127):
 * out = resid + alpha * keep(seed, m*N + n)/(1 - p_drop) * (A W^T + bias), the same counter-based keep as sfm_ew_train. */
int sfm_gemm16_train(const void* A, const void* W, const float* bias, void* out, const float* resid,
                  float* gn_partial, int B, int Lout, int Lin, int Cin, int lda, int ksize, int stride, int pad,
                  long long a_batch_stride, int Kpad, int N, int Npad, int ldo, long long o_batch_stride,
                  int ldr, long long r_batch_stride, float alpha, int epi, int out_f32, int gn_group,
                  int nsplit, int dtype, int variant, float p_drop, unsigned int seed,
                     void* stream);
/* Linear (A [M, Cin] 16-bit, row stride lda) with the FeedForwardModule's Swish and hidden dropout fused into the epilogue
 * (training; models/conformer.py:44-46 and its backward).  backward == 0: z = A W^T + bias; out 16-bit = keep/(1-p) * swish(z),
 * out2 [M, N] 16-bit = d = keep/(1-p) * swish'(z), the derivative factor kept for the backward;  backward != 0: out 16-bit =
 * (A W^T) * aux with aux = the saved d.  Dropout counters m * N + n, the same as sfm_ew_train modes 0 / 1.  N % 8 == 0,
 * 16-byte aligned rows. */
int sfm_gemm16_swish(const void* A, const void* W, const float* bias, void* out, const void* aux, void* out2, int M, int Cin,
                     int lda, int Kpad, int N, int Npad, int ldo, int backward, float p_drop, unsigned int seed, int dtype,
                     void* stream);
/* Conv1d (channels-last) whose INPUT is normalised while the operand is staged: replaces the
 * GroupNorm -> GELU -> Conv1d chains of the PerceptionAgent (agents/perception.py:192-206 `_make_block`, :121-129
 * `_ResidualBlock.forward`, :167-171 `downsample`) without materialising the normalised activation:
 *     x = GELU(sc1[b,c] * x1 + sh1[b,c]  [+ sc2[b,c] * x2 + sh2[b,c]]),   out = Conv1d(x; W, bias, ksize, stride, pad)
 *   x1, x2 [B, Lin, Cin] 16-bit raw outputs of the producing conv(s); sc / sh [B, Cin] fp32 from sfm_gn_finalize
 *   W [N][ksize * Cin] 16-bit tap-major (sfm_gemm16's layout), bias [N]; out [B, Lout, N] (out_f32 as sfm_gemm16)
 *   gn_partial: as sfm_gemm16 ([B][2 ceil(Lout/128)][N/gn_group][2]) or NULL
 *   Ws, bias_s, out_s, gn_partial_s: optional Conv1d(Cin -> N, 1, stride 2) of a residual block's skip branch on the same
 *   x, computed from the same staged input (N = 128, ksize 7 only)
 * Shapes: Cin % 64 == 0; (ksize, stride, pad, N, #inputs) in {(7,2,3,128 + skip,1|2), (7,2,3,256,2), (3,1,1,128|256,1),
 * (5,2,2,256,2), (1,2,0,256,2)}; anything else returns SFM_ERR_SHAPE (-2). */
int sfm_conv16p(const void* x1, const float* sc1, const float* sh1, const void* x2, const float* sc2, const float* sh2,
                const void* W, const float* bias, void* out, float* gn_partial, const void* Ws, const float* bias_s,
                void* out_s, float* gn_partial_s, int B, int Lin, int Cin, int N, int ksize, int stride, int pad,
                int out_f32, int gn_group, int dtype, void* stream);

/* out[b,m,n] = bias[n] + sum_k sig[b, m*hop + k - padl] * Wt[k][n], exact fp32 on
 * v_mfma_f32_32x32x2_f32.  Replaces F.conv1d of SincConv1d (agents/perception.py:117),
 * torch.stft (training/conformer_pipeline.py:199), the irfft stage of torch.istft
 * (:210) and fp32 matmuls.  mode 0: zero outside [0,Ls); 1: reflect.
 * Columns >= nsplit go to out2 (when non-NULL) at column n - nsplit.
 * gn_partial layout: [B][4*ceil(M/128)][N/gn_group][2]. */
int sfm_framed_gemm_f32(const float* sig, const float* Wt, const float* bias, void* out, void* out2,
                        float* gn_partial, int B, int M, int Ls, long long sig_batch_stride, int hop,
                        int padl, int K, int Kpad, int N, int Npad, int nsplit, long long o_batch_stride,
                        long long ldm, long long ldn, int mode, int out_f32, int gn_group, int dtype,
                        void* stream);

/* softmax(Q K^T * scale) V per (batch, head); replaces the attention core of
 * nn.MultiheadAttention (models/conformer.py:69).  qkv [B,T,ldqkv] 16-bit with
 * q at column h*hd, k at koff+h*hd, v at voff+h*hd; out [B,T,ldo] 16-bit at h*hd.
 * scale <= 0 means Q is pre-multiplied by softmax_scale*log2(e) (folded into W_q/b_q). */
int sfm_attention_fwd(const void* qkv, void* out, int B, int T, int H, int hd, int ldqkv, int ldo,
                      int koff, int voff, long long qkv_batch_stride, long long o_batch_stride,
                      float scale, int dtype, void* stream);
/* Same, with the result written in `out_dtype` (SFM_DT_BF16 / SFM_DT_F16) when it differs from the operands' `dtype`
 * (precision policy: a bf16 attention core behind fp16 projections; head_dim 64 kernels only), and with the head_dim-64
 * kernel chosen per call by `variant` (A/B measurements; the library keeps no selection state): 0 = by shape (the pipelined
 * persistent kernel attn_fwd_hd64p for T 400..512, 800..1024 and >= 1024 with 512-row query tiles, for T 231..256 with 256-row
 * tiles; 32 query rows per wave otherwise), 1 = always 32 query rows per wave, 3 (or 2) = the persistent ring kernel of
 * round 2, 4 / 5 = the pipelined persistent kernel with one 8-wave / two 4-wave workgroups per CU. */
int sfm_attention_fwd_ex(const void* qkv, void* out, int B, int T, int H, int hd, int ldqkv, int ldo,
                         int koff, int voff, long long qkv_batch_stride, long long o_batch_stride,
                         float scale, int dtype, int out_dtype, int variant, void* stream);

/* nn.LayerNorm (+ optional erf GELU when act==1): models/conformer.py:43,68,107,150;
 * agents/msa.py:44-47; training/conformer_pipeline.py:274,282.  D <= 512; ldx, and ld16 / ld32 of the outputs that are
 * written, >= D (else SFM_ERR_SHAPE); dtype SFM_DT_BF16 or SFM_DT_F16 (else SFM_ERR_ARG). */
int sfm_layernorm(const float* x, const float* w, const float* b, void* out16, float* out32, int M, int D,
                  int ldx, int ld16, int ld32, float eps, int act, int dtype, void* stream);

/* nn.GroupNorm split in (stats from GEMM epilogue) -> finalize -> apply
 * (agents/perception.py:157,169,176,180,196,199,204 and the residual add+GELU :129). */
int sfm_gn_finalize(const float* partial, const float* w, const float* b, float* scale, float* shift, int B,
                    int P, int G, int C, long long rows, float eps, void* stream);
int sfm_gn_apply(const void* x1, const float* sc1, const float* sh1, const void* x2, const float* sc2,
                 const float* sh2, void* out, int B, long long rows_per_batch, int C, int in_f32, int out_f32,
                 int act, int dtype, void* stream);

/* depthwise Conv1d + BatchNorm1d(eval) + Swish, channels-last: models/conformer.py:117-119 */
int sfm_dwconv_bn_swish(const void* x, const float* wdw, const float* bdw, const float* bnw,
                        const float* bnb, const float* bnm, const float* bnv, void* out, int B, int T,
                        int C, int KS, float eps, int dtype, void* stream);

/* same operation with host-folded operands (wT [KS][C], BatchNorm+bias folded into sc/sh), register-resident
 * taps for KS in {7, 31} and C in {32, 64, 128, 256, 512}; any other C > 0 and odd KS on a generic kernel */
int sfm_dwconv_folded(const void* x, const float* wT, const float* sc, const float* sh, void* out, int B, int T,
                      int C, int KS, int act, int out_f32, int dtype, void* stream);

/* ---- packed (variable-length) batches: B utterances of different lengths back to back, no padding ----------------------
 * Row matrices hold the frames of all utterances concatenated: utterance u owns rows [frame_off[u], frame_off[u + 1]),
 * frame_off = int32[B + 1] on the device, ascending from 0, frame_off[B] = sum_T; waveforms likewise with samp_off.  The offsets
 * are read on the device; the host passes B, the longest utterance max_T and sum_T, which it knows from the lengths.  Each
 * utterance's result is what the dense entry point gives for it alone.  Null pointers -> SFM_ERR_ARG, B <= 0 and the shape
 * rules of the dense twin -> SFM_ERR_SHAPE, before any HIP call. */
/* sfm_framed_gemm_f32 on packed signals: frame t of utterance u = its samples t * hop + k - padl, zero (mode 0) or reflected
 * at its own first / last sample (mode 1; every signal longer than padl).  A 128-row tile covers packed rows of any number of
 * utterances.  out / out2 rows at stride ldm, columns at stride ldn, columns >= nsplit go to out2 when given. */
int sfm_framed_gemm_f32_varlen(const float* sig, const float* Wt, void* out, void* out2, const int* samp_off,
                               const int* frame_off, int B, int sum_T, int hop, int padl, int K, int Kpad, int N, int Npad,
                               int nsplit, long long ldm, long long ldn, int mode, int out_f32, int dtype, void* stream);
/* sfm_framed_gemm_split16 on packed signals (same layout, fp32 result) */
int sfm_framed_gemm_split16_varlen(const float* sig, const void* Whi, const void* Wlo, float* out, float* out2,
                                   const int* samp_off, const int* frame_off, int B, int sum_T, int hop, int padl, int K,
                                   int Kpad, int N, int Npad, int nsplit, int col2_off, long long ldm, int mode, void* stream);
/* sfm_attention_fwd_ex on packed rows: every utterance attends to its own rows.  head_dim 64: the 4-wave MFMA kernel, one
 * workgroup per entry of items = int32[n_items][4] (utterance, head, 128-row query tile, 0), every existing tile exactly once;
 * other head_dim <= 256: one wave per row, items unused, operands' format only (SFM_ERR_SHAPE otherwise).  scale <= 0: Q
 * already carries softmax_scale * log2(e). */
int sfm_attention_fwd_varlen(const void* qkv, void* out, const int* frame_off, const int* items, int n_items, int B, int max_T,
                             int sum_T, int H, int hd, int ldqkv, int ldo, int koff, int voff, float scale, int dtype,
                             int out_dtype, void* stream);
/* sfm_dwconv_folded on packed rows [sum_T, C]: zero edge at every utterance's own first and last frame.  KS 7 / 31 with C in
 * {32, 64, 128, 256, 512}: one workgroup per entry of tiles = int32[n_tiles][2] (utterance, 64-frame tile of it); any other
 * C > 0 and odd KS: generic kernel, tiles unused. */
int sfm_dwconv_folded_varlen(const void* x, const float* wT, const float* sc, const float* sh, void* out, const int* frame_off,
                             const int* tiles, int n_tiles, int B, int max_T, int sum_T, int C, int KS, int act, int out_f32,
                             int dtype, void* stream);
/* sfm_istft_ola on packed frames [sum_T, ld_frames] -> packed samples [sum_L]: per-utterance frame range, envelope, length */
int sfm_istft_ola_varlen(const float* frames, const float* win2, float* out, const int* frame_off, const int* samp_off, int B,
                         int sum_L, int n_fft, int hop, int win, long long ld_frames, void* stream);

/* layout / packing */
int sfm_convert_rows(const float* src, void* dst, long long M, int C, int Cz, long long ld_src,
                     long long ld_dst, int dtype, void* stream);
int sfm_transpose(const void* src, void* dst, int B, int R, int C, long long src_batch, long long src_row,
                  long long dst_batch, long long dst_row, int src_f32, int dst_f32, int dtype, void* stream);
int sfm_pool_time(const float* src, void* dst16, float* dst32, int B, int Tin, int Tout, int C,
                  long long ld_src, long long ld_dst, int dtype, void* stream);
/* as sfm_pool_time with out = scale[b, c] * avg + shift[b, c]: pooled GroupNorm'd latents straight from the raw layer
 * output (glue G1 applied to agents/perception.py:244-246 without materialising the full-rate normalised tensor) */
int sfm_pool_time_affine(const float* src, const float* scale, const float* shift, void* dst16, float* dst32, int B,
                         int Tin, int Tout, int C, long long ld_src, long long ld_dst, int dtype, void* stream);
/* sfm_pool_time_affine on a 16-bit source [B, Tin, ld_src] in the format `src_dtype` (the fused path writes the raw latent
 * heads in the PerceptionAgent stage's operand format: agents/perception.py:244-246 + glue G1); dst16 in the format `dtype` */
int sfm_pool_time_affine16(const void* src16, int src_dtype, const float* scale, const float* shift, void* dst16, float* dst32,
                           int B, int Tin, int Tout, int C, long long ld_src, long long ld_dst, int dtype, void* stream);
/* mean over time (glue G2: episodic-memory key), src fp32 [B, T, ld_src] cols [0, C) -> dst fp32 [B, C]; deterministic
 * two-pass sum, scratch: sfm_mean_time_scratch_floats floats; ld_src < C is SFM_ERR_SHAPE (sfm_sum_time too) */
long long sfm_mean_time_scratch_floats(int B, int T, int C);
int sfm_mean_time(const float* src, float* dst, float* scratch, int B, int T, int C, long long ld_src, void* stream);
/* the same reduction without the 1/T (training: gradient of a per-utterance bias broadcast over the frames) */
int sfm_sum_time(const float* src, float* dst, float* scratch, int B, int T, int C, long long ld_src, void* stream);
/* adjoint of sfm_pool_time (training: gradient of the pooled latents back to the full-rate latents), fp32 */
int sfm_pool_time_bwd(const float* dout, float* dsrc, int B, int Tin, int Tout, int C, long long ld_dout,
                      long long ld_dsrc, void* stream);
/* agents/msa.py:134-137 */
int sfm_stft_lognorm_pack(const float* re, const float* im, void* dst, long long M, int F, int zpad,
                          long long ld_dst, int dtype, void* stream);
/* adjoint of sfm_stft_lognorm_pack: g [M, ld_g] fp32 holds d(real') in columns [0,F) and d(imag') in [F,2F) */
int sfm_stft_lognorm_bwd(const float* re, const float* im, const float* g, float* dre, float* dim_, long long M, int F,
                         long long ld_g, void* stream);
/* agents/msa.py:166-172, training/conformer_pipeline.py:287-296 */
int sfm_polar_mask(const float* lm, const float* lp, const float* mag_bias, const float* nr, const float* ni,
                   float* mr, float* mi, float* er, float* ei, float* mmag, int B, long long rows_per_batch,
                   int F, float phase_scale, long long ld_logits, long long ld_enh, void* stream);
/* models/conformer.py:243-244 */
int sfm_complex_mul(const float* sr, const float* si, const float* mr, const float* mi, float* er, float* ei,
                    long long total, void* stream);
/* overlap-add + envelope division of torch.istft: training/conformer_pipeline.py:210 */
int sfm_istft_ola(const float* frames, const float* win2, float* out, int B, int T, int L, int n_fft, int hop,
                  int win, long long ld_frames, void* stream);
int sfm_pack_spec(const float* re, const float* im, float* dst, long long M, int F, int ld, long long ld_src,
                  void* stream);
/* agents/perception.py:88-112 */
int sfm_sinc_filters(const float* low_hz, const float* band_hz, const float* window, const float* n_,
                     float* filt, float* Wt, int C, int K, int Npad, float sample_rate, float min_low_hz,
                     float min_band_hz, void* stream);
/* Whole FeedForwardModule in one launch (models/conformer.py:41-49, eval): out = x + alpha*(W2 swish(W1 LN(x)+b1)+b2).
 * x/out [M,256] fp32; W1 [FF,256], W2 [256,FF] 16-bit row-major (nn.Linear layout); D must be 256, FF % 64 == 0. */
int sfm_ffn_fused(const float* x, const float* lnw, const float* lnb, const void* W1, const float* b1,
                  const void* W2, const float* b2, float* out, int M, int D, int FF, float alpha, float eps,
                  int dtype, void* stream);
/* sfm_ffn_fused + the LayerNorm that follows the module inside the block (mhsa.layer_norm after ff1, final_norm after ff2;
 * models/conformer.py:66,151) applied to y in the epilogue: ln_out [M, 256] 16-bit (ln_out_f32 = 0) or fp32; out (y) may be
 * NULL when only the normalised rows are needed. */
int sfm_ffn_fused_ln(const float* x, const float* lnw, const float* lnb, const void* W1, const float* b1, const void* W2,
                     const float* b2, float* out, int M, int D, int FF, float alpha, float eps, const float* ln2w,
                     const float* ln2b, void* ln_out, int ln_out_f32, int dtype, void* stream);
/* SincConv1d FIR (agents/perception.py:117) on the 16-bit matrix cores with hi/lo split operands
 * (3 MFMA passes, ~fp32 accuracy).  filt [64,K] fp32 from sfm_sinc_filters; wsh = workspace of
 * SFM_SINC_FIR16_WS_WORDS uint16; out [B,L,64] channels-last; gn_partial [B][sfm_sinc_fir16_tiles(L)][8][2],
 * which the caller must zero-fill (tiles past L are not written). */
int sfm_sinc_fir16_tiles(int L);
int sfm_sinc_fir16(const float* wave, const float* filt, void* wsh, void* out, float* gn_partial, int B,
                   int L, int C, int K, int out_f32, int dtype, void* stream);
/* passes: 3 = split operands (hi x hi + hi x lo + lo x hi: 1e-7 / 1e-6 max error), 1 = one rounding of waveform and taps to the
 * operand format (the kernel that keeps a shift's taps in registers), 0 = auto (1 for fp16 operands with a 16-bit result,
 * else 3) - sfm_sinc_fir16 = passes 0; SFM_SINC_FIR16_STREAM1 = the result of passes 1, bit for bit (out and gn_partial), from
 * the streaming one-pass kernel that keeps the taps in LDS: kept as the reference and A/B partner of the resident one */
int sfm_sinc_fir16_ex(const float* wave, const float* filt, void* wsh, void* out, float* gn_partial, int B, int L, int C, int K,
                      int out_f32, int dtype, int passes, void* stream);
/* The same frames-x-matrix product on the 16-bit matrix cores with split bf16 operands (hi + lo, 3 MFMAs per k-step,
 * ~4e-6 relative error): the STFTs of the training objective (training/conformer_pipeline.py:74-108) and their adjoints.
 * Whi / Wlo: the constant matrix pre-split and n-major, [Npad (x256)][Kpad (x32)] uint16; out fp32 [b][m][n] with row
 * stride ldm; columns >= nsplit go to out2 at column n - nsplit + col2_off (when out2 != NULL). */
int sfm_framed_gemm_split16(const float* sig, const void* Whi, const void* Wlo, float* out, float* out2, int B, int M,
                            int Ls, long long sig_batch_stride, int hop, int padl, int K, int Kpad, int N, int Npad,
                            int nsplit, int col2_off, long long o_batch_stride, long long ldm, int mode, void* stream);
/* Forward of the training objective (training/conformer_pipeline.py:52-108, 539-572): reductions in fp64.
 * S buffers must be zero-filled by the caller (the kernels accumulate into them).
 * ORDERED REDUCTIONS (every entry point of the training step that sums over workgroups takes an optional workspace `ws`): with
 * it, each workgroup writes its partial into ws and a second pass folds the partials in workgroup order - the step is then
 * bit-reproducible, like the reference's CPU step (training/conformer_pipeline.py:496-532); ws == NULL selects fp32 / f64
 * atomics.  Sizes: sfm_*_ws_floats / sfm_*_ws_doubles (the element type is part of the name); ws contents are scratch
 * (destroyed), 16-byte aligned. */
long long sfm_wave_moments_ws_doubles(int B, int L);
int sfm_wave_moments(const float* est, const float* tgt, double* S, int B, int L, double* ws, void* stream);
/* packed form of sfm_wave_moments (atomics only): est / tgt = B signals back to back, signal b = samples
 * [samp_off[b], samp_off[b + 1]) (int32 [B + 1] on the device; an empty signal leaves its row zero); max_L = the longest.
 * The grid is min(ceil(max_L / 256), 64) x B workgroups along x: SFM_ERR_SHAPE when that exceeds 2^31 - 1. */
int sfm_wave_moments_varlen(const float* est, const float* tgt, double* S, const int* samp_off, int B, int max_L, void* stream);
long long sfm_spec_sums_ws_doubles(long long n);
int sfm_spec_sums(const float* pr, const float* pi, const float* tr, const float* ti, double* S, long long n, double* ws,
                  void* stream);
int sfm_enhancer_loss_finalize(const double* Sw, const double* Sm, const double* Sr, const long long* nr, int B,
                               int L, long long n_mag, int R, float* out, void* stream);
/* Backward of the objective and of the bounded polar mask (training/conformer_pipeline.py:52-108, 283-295, 539-572).
 * sisnr_bwd: dwave = scale * d(neg SI-SNR)/d est from the moments Sw of sfm_wave_moments.
 * spec_loss_bwd: mode 0 spectral-convergence + log-magnitude of one resolution (S = its sfm_spec_sums), mode 1 the
 *   L1 magnitude term; writes/accumulates d/d(real, imag) at dr/di[m*ld + f].
 * stft_adjoint_ola: adjoint of the reflect-padded framing of torch.stft: frames [B,T,win] -> dwave [B,L]
 *   (optionally accumulated, optionally multiplied by post[L] afterwards).
 * polar_mask_bwd: (d enh_real, d enh_imag) -> d logits [M, ld_dlog >= 2F] (magnitude | phase columns). */
int sfm_sisnr_bwd(const float* est, const float* tgt, const double* Sw, float* dwave, int B, int L, float scale,
                  void* stream);
int sfm_spec_loss_bwd(const float* pr, const float* pi, const float* tr, const float* ti, const double* S, float* dr,
                      float* di, long long n, int F, long long ld, int mode, int accumulate, float scale, void* stream);
int sfm_stft_adjoint_ola(const float* frames, float* dwave, const float* post, int B, int T, int L, int n_fft, int hop,
                         int win, int accumulate, void* stream);
/* mag_bias (or NULL): [M / rows_per_batch, F] added to the magnitude logit as in sfm_polar_mask; nr = ni = NULL: the mask itself
 * is the output (noisy = 1 + 0j, agents/msa.py:166-172) */
int sfm_polar_mask_bwd(const float* lm, const float* lp, const float* mag_bias, const float* nr, const float* ni,
                       const float* der, const float* dei, float* dlog, long long M, long long rows_per_batch, int F,
                       float phase_scale, long long ld_logits, long long ld_dlog, void* stream);
/* small-shape attention backward (any head_dim <= 256; the MFMA kernels of sfm_attention_bwd need head_dim 64):
 * dkv32 = zero-filled fp32 scratch [B*T, 2*H*hd]; dqkv gets dQ' | dK | dV like sfm_attention_bwd. */
int sfm_attention_bwd_generic(const void* qkv, const void* O, const void* dO, const float* lse, float* dkv32, void* dqkv,
                              int B, int T, int H, int hd, int ldqkv, int ldo, int koff, int voff, float p_drop,
                              unsigned int seed, int dtype, void* stream);
/* Batched quality metrics (evaluation/ssnr.py:26-92, fallback STOI evaluation/stoi.py:53-99).
 * ssnr_frames: acc [B][2] fp64 (zero-filled) += { sum of clipped frame SNRs over non-silent frames, their count }.
 * stoi_frames: spectra [B, nframes, F] of the raw signals, sc / se [B] fp64 = 1/(rms + 1e-10) of clean / enhanced,
 *   acc [B] fp64 (zero-filled) += sum over frames of the clipped spectral correlation. */
int sfm_ssnr_frames(const float* clean, const float* enh, double* acc, int B, int L, int frame, int hop, float upper,
                    float lower, void* stream);
int sfm_stoi_frames(const float* cr, const float* ci, const float* er, const float* ei, const double* sc, const double* se,
                    double* acc, int B, int nframes, int F, void* stream);
/* lsd_frames: the reference's PESQ fallback (evaluation/pesq_eval.py:66-78) per frame, from the two spectra [B, nframes, F] of
 *   a rectangular-window DFT: acc [B] fp64 (zero-filled) += sqrt(mean_f (log(|C_f| + 1e-10) - log(|E_f| + 1e-10))^2). */
int sfm_lsd_frames(const float* cr, const float* ci, const float* er, const float* ei, double* acc, int B, int nframes, int F,
                   void* stream);
/* Packed forms for utterances of different lengths (layout as sfm_framed_gemm_f32_varlen): samples of utterance u =
 * [samp_off[u], samp_off[u + 1]); its frames in the METRIC's framing (n_u = (L_u - frame) / hop + 1, or 0 when L_u < frame)
 * = packed frames / spectrum rows [frame_off[u], frame_off[u + 1]), both int32 [B + 1] on the device; an utterance may own
 * no frame (its acc entries stay zero).  sum_frames = frame_off[B]; 0 launches nothing.  One wave per packed frame; the
 * per-utterance sums are fp64 atomics as in the dense forms.  acc / sc / se indexed by utterance as above. */
int sfm_ssnr_frames_varlen(const float* clean, const float* enh, double* acc, const int* samp_off, const int* frame_off, int B,
                           int sum_frames, int frame, int hop, float upper, float lower, void* stream);
int sfm_stoi_frames_varlen(const float* cr, const float* ci, const float* er, const float* ei, const double* sc,
                           const double* se, double* acc, const int* frame_off, int B, int sum_frames, int F, void* stream);
int sfm_lsd_frames_varlen(const float* cr, const float* ci, const float* er, const float* ei, double* acc, const int* frame_off,
                          int B, int sum_frames, int F, void* stream);
/* Gradient of the SincConv1d FIR bank w.r.t. its taps (training of agents/perception.py:79-118):
 * dfilt [C, K] += sum_{b,l} dy[b, l, c] x[b, l + k - K/2]; x [B, L] fp32, dy [B, L, C] 16-bit or fp32; scratch:
 * sfm_sinc_wgrad_scratch_floats floats (need not be zeroed).  K <= 256. */
long long sfm_sinc_wgrad_scratch_floats(int B, int L, int C, int K);
int sfm_sinc_wgrad(const float* x, const void* dy, int dy_f32, float* dfilt, float* scratch, int B, int L, int C, int K,
                   int dtype, void* stream);
/* The same tap gradient on the matrix cores for a 16-bit dy (K = 251 taps, centre 125): sfm_sinc_shift_pack writes 8 copies
 * of every utterance, zero-padded and shifted by 0..7 samples, xs 16-bit [B][8][sfm_sinc_shift_len(L)], so that the 8-tap
 * chunk at any sample is one aligned 16-byte load; sfm_sinc_wgrad16: dW fp32 [C][256] += dy^T * Toeplitz(x) (columns
 * 251..255 are scratch), dW zeroed by the caller. */
long long sfm_sinc_shift_len(int L);
int sfm_sinc_shift_pack(const float* x, void* xs, int B, int L, int dtype, void* stream);
int sfm_sinc_wgrad16(const void* dy, const void* xs, float* dW, int B, int L, int C, int dtype, float* ws, long long ws_floats,
                     void* stream);                       /* ws: sfm_tn_ws_floats(B * L, C, 256) */
/* Backward of the PerceptionAgent's GroupNorm nodes out = act(GN(x1) [+ GN(x2)]) (agents/perception.py:121-129, 157,
 * 192-206), channels-last [B, L, C], C a power of two in [64, 2048].  sc / sh [B, C] fp32: the forward's scale and shift;
 * mean / rstd [B, G].  reduce: S [B][3][C] += { sum dp, sum dp xhat1, sum dp xhat2 } with dp = dout * act'(p) (S zeroed by
 * the caller);  coefs: coef = [3][B][C] (a, b, c) and dparam [3][C] += (dbeta, dgamma1, dgamma2) (zeroed by the caller);
 * apply: dx_i = a dp - b - xhat_i c. */
int sfm_gn_bwd_reduce(const void* dout, int dout_f32, const void* x1, int x1_f32, const float* sc1, const float* sh1,
                      const float* mean1, const float* rstd1, const void* x2, int x2_f32, const float* sc2,
                      const float* sh2, const float* mean2, const float* rstd2, float* S, int B, int L, int C, int G,
                      int act, int dtype, float* ws, void* stream);
long long sfm_gn_bwd_reduce_ws_floats(int B, int L, int C);
/* (S is DESTROYED: after the coefficient tables it is the scratch of the ordered fold over b that produces dparam) */
int sfm_gn_bwd_coefs(float* S, const float* gamma1, const float* rstd1, const float* gamma2, const float* rstd2,
                     float* coef1, float* coef2, float* dparam, int B, int L, int C, int G, void* stream);
int sfm_gn_bwd_apply(const void* dout, int dout_f32, const void* x1, int x1_f32, const float* sc1, const float* sh1,
                     const float* mean1, const float* rstd1, const float* coef1, void* dx1, int dx1_f32, const void* x2,
                     int x2_f32, const float* sc2, const float* sh2, const float* mean2, const float* rstd2,
                     const float* coef2, void* dx2, int dx2_f32, int B, int L, int C, int G, int act, int dtype,
                     void* stream);
/* SURVEY 8f N4.  MetacognitiveArbitrationAgent (agents/maa.py:70-135) on N = B * T uncertainty values; stats = (running_mean,
 * running_var) fp32 on the device; params = W1[64] b1[64] W2[64*64] b2[64] W3[4*64] b3[4] fp32 (the decision_net).
 * update_stats: train()-mode EMA (momentum 0.1, unbiased batch variance; acc = 2 zeroed doubles, re-zeroed on return);
 * forward: logits / probs [N,4], decisions int64 [N], confidence [N];  backward: dsigma [N] and the 16-bit operands of the
 * weight-gradient GEMMs (H1, H2, dZ1, dZ2 [N,64]; GL [N,8] = total logit gradient; XN [N,8], column 0 = normalised sigma). */
int sfm_maa_update_stats(const float* sigma, long long n, double* acc, float* stats, long long* num_updates, float momentum,
                         void* stream);
int sfm_maa_forward(const float* sigma, const float* stats, const float* params, float* logits, float* probs,
                    long long* decisions, float* confidence, long long n, void* stream);
int sfm_maa_backward(const float* sigma, const float* stats, const float* params, const float* g_logits, const float* g_probs,
                     const float* g_conf, float* dsigma, void* H1, void* H2, void* dZ1, void* dZ2, void* GL, void* XN,
                     long long n, int dtype, void* stream);
/* VectorQuantizer (models/vq.py:54-96), M <= 16 scalar centroids: q = nearest centroid (first minimum), idx int64,
 * acc[0] += sum (x - q)^2 (double, zeroed by the caller);  backward: dx = g_q + g_loss beta 2 (x - q) / n (straight-through +
 * commitment term), dcent[k] += g_loss 2 (q - x) / n over the elements assigned to k (codebook term; zeroed by the caller). */
int sfm_vq_forward(const float* x, const float* centroids, int M, float* q, long long* idx, double* acc, long long n,
                   void* stream);
int sfm_vq_backward(const float* x, const long long* idx, const float* centroids, int M, const float* g_q,
                    const float* g_loss, float beta, float* dx, float* dcent, long long n, void* stream);
/* Optimiser step (training/conformer_pipeline.py:424-429 AdamW, :509 NaN/Inf skip, :514 clip_grad_norm_) on flat fp32
 * buffers.  ctl = 8 doubles: [0] step count, [1] sum of squares (sfm_sumsq accumulates; zeroed by the step), [2] flag > 0
 * forces a skip, [3] applied gradient scale, [4] skipped (0/1), [5],[6] bias corrections, [7] gradient norm. */
long long sfm_sumsq_ws_doubles(long long n);
int sfm_sumsq(const float* g, long long n, double* out, double* ws, void* stream);        /* ws: sfm_sumsq_ws_doubles(n) */
int sfm_adamw_step(float* p, float* g, float* m, float* v, long long n, double* ctl, float lr, float beta1, float beta2,
                   float eps, float wd, float inv_scale, float max_norm, int write_back_grad, void* stream);
/* Same, leaving alone - p, m and v - the parameters that received no gradient in this step (torch.optim.AdamW skips a
 * parameter whose grad is None): spans[k] = first flat element of parameter k (n_params + 1 ascending entries, device),
 * touched[k] > 0 = stepped (device; in data-parallel runs the per-rank 0/1 masks summed by the gradient all-reduce, so
 * that every replica takes the same decision). */
int sfm_adamw_step_masked(float* p, float* g, float* m, float* v, long long n, double* ctl, float lr, float beta1, float beta2,
                          float eps, float wd, float inv_scale, float max_norm, int write_back_grad, const long long* spans,
                          const float* touched, int n_params, void* stream);
/* The same step under the reference's AMP recipe (training/conformer_pipeline.py:442 torch.amp.GradScaler, :504
 * scaler.scale(loss).backward(), :512-517 unscale_ / clip_grad_norm_ / scaler.step / scaler.update) with the loss scale kept on the
 * device: loss_scale = 4 floats {S, clean steps since S last changed, steps skipped for Inf / NaN gradients, steps skipped for a
 * non-finite loss}.  g holds S (x world; inv_world = 1 / world) times the gradient: the prepare thread unscales, takes the
 * clip / skip decision, halves S (backoff_factor) after a step with Inf / NaN gradients, multiplies it by growth_factor after
 * growth_interval clean steps - GradScaler.update() without a host round trip.  spans / touched may both be NULL. */
int sfm_adamw_step_scaled(float* p, float* g, float* m, float* v, long long n, double* ctl, float lr, float beta1, float beta2,
                          float eps, float wd, float inv_world, float max_norm, int write_back_grad, const long long* spans,
                          const float* touched, int n_params, float* loss_scale, float growth_factor, float backoff_factor,
                          int growth_interval, void* stream);
/* torch.optim.Adam(weight_decay = wd) behind clip_grad_norm_(max_norm) (training/pipeline.py:563-567, 664-669 of the reference) on
 * the same flat buffers, ctl layout, spans / touched mask and loss-scale state (loss_scale NULL: S = 1).  The norm (ctl[7]) and the
 * clip coefficient are those of the unscaled gradient WITHOUT the decay term; then g <- g + wd p, m <- beta1 m + (1 - beta1) g,
 * v <- beta2 v + (1 - beta2) g^2, p <- p - (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps).  A step skipped for a non-finite gradient or
 * for the flag ctl[2] leaves p, m, v and the step count alone and multiplies S by backoff_factor (counted in loss_scale[2] and
 * loss_scale[3]).  g is left as it was.  The betas are given as 1 - beta (in 0 .. 1]: 0.001f is 1 - 0.999 to 5e-8 relative, while
 * 1 - 0.999f is that only to 1.3e-5, which v would inherit. */
int sfm_adam_l2_step(float* p, float* g, float* m, float* v, long long n, double* ctl, float lr, float one_minus_beta1,
                     float one_minus_beta2, float eps, float wd, float inv_world, float max_norm, const long long* spans,
                     const float* touched, int n_params, float* loss_scale, float growth_factor, float backoff_factor,
                     int growth_interval, void* stream);
/* ---- training path of the ConformerBlock (backward of models/conformer.py:28-151) ---- */
/* dW[n,k] += sum_m G[m,n] X[m,k] (weight gradient; M is split over workgroups: with ws (>= sfm_tn_ws_floats(M, N, K) floats) every
 * split writes its partial [N][K] and the partials are added to dW in split order, without ws by fp32 atomics; zero dW first);
 * db (optional): db[n] += sum_m G[m,n] in the same launch; sfm_colsum = the stand-alone bias gradient */
long long sfm_tn_ws_floats(int M, int N, int K);
int sfm_gemm16_tn(const void* G, const void* X, float* dW, float* db, int M, int N, int K, int ldg, int ldx, int ldw,
                  int dtype, float* ws, long long ws_floats, void* stream);
/* Conv1d weight gradient (training of agents/perception.py:121-129, 160-188 convs): G = dY [B*Lout, N] 16-bit, x
 * [B, Lin, Cin] channels-last 16-bit, dW [N, ksize*Cin] tap-major fp32 += G^T im2col(x) with the im2col rows addressed
 * in place (zero padding by range check); db (optional) += column sums of G. */
int sfm_conv_wgrad16(const void* G, const void* x, float* dW, float* db, int B, int Lout, int Lin, int Cin, int N, int ksize,
                     int stride, int pad, long long x_batch_stride, int ldg, int ldw, int dtype, float* ws, long long ws_floats,
                     void* stream);                       /* ws: sfm_tn_ws_floats(B * Lout, N, ksize * Cin) */
long long sfm_colsum_ws_floats(int M, int N);
int sfm_colsum(const void* G, float* out, int M, int N, int ldg, int g_f32, int dtype, float* ws, void* stream);
/* LayerNorm backward; ws (optional, sfm_layernorm_bwd_ws_floats(M, D) floats): ordered dgamma / dbeta.  D <= 512 and every
 * row stride (ldx, ldy, ld) >= D, else SFM_ERR_SHAPE */
long long sfm_layernorm_bwd_ws_floats(int M, int D);
int sfm_layernorm_bwd(const float* x, const float* gamma, const float* dy, const float* dres, float* dx,
                      float* dgamma, float* dbeta, int M, int D, int ldx, int ld, float eps, float* ws, void* stream);
/* the same with dy in the 16-bit format `dtype` (dy_16 != 0) and its own row stride ldy; ld = row stride of dres and dx */
int sfm_layernorm_bwd_ex(const float* x, const float* gamma, const void* dy, int dy_16, const float* dres, float* dx,
                         float* dgamma, float* dbeta, int M, int D, int ldx, int ldy, int ld, float eps, int dtype,
                         float* ws, void* stream);
/* the same, also writing next16 [M, D] (format `dtype`, contiguous rows) = next_alpha * dropout(dx; next_p, next_seed) with the
 * counters of sfm_ew_train mode 4: the 16-bit operand the next backward node of the residual chain starts from */
int sfm_layernorm_bwd_next(const float* x, const float* gamma, const void* dy, int dy_16, const float* dres, float* dx,
                           float* dgamma, float* dbeta, int M, int D, int ldx, int ldy, int ld, float eps, int dtype,
                           void* next16, float next_alpha, float next_p, unsigned int next_seed, float* ws, void* stream);
/* mode 0 swish fwd, 1 swish bwd, 2 GLU fwd, 3 GLU bwd, 4 alpha*g*dropout; counter-based dropout (p, seed) */
int sfm_ew_train(const void* z, const void* g, void* out, long long M, int N, int mode, int g_f32, int out_f32,
                 float alpha, float p, unsigned int seed, int dtype, void* stream);
/* BatchNorm1d training statistics / backward (through the following Swish); ws (optional): sfm_col_stats_ws_floats(M, C) floats.
 * sfm_col_stats without aux gives the raw moments { sum y, sum y^2 }: kept for callers that want them; the training step forms
 * its statistics from sfm_col_stats_shifted */
long long sfm_col_stats_ws_floats(int M, int C);
int sfm_col_stats(const float* y, const float* aux, const float* mean, const float* rstd, float* S, int M, int C, float* ws,
                  void* stream);
/* the sums of the BatchNorm statistics, shifted: K[c] = mean of min(M, 128) rows of y spread evenly over the M; S[c] =
 * { sum (y - K[c]), sum (y - K[c])^2 } (S zero-filled; ws as above) */
int sfm_col_pilot(const float* y, float* K, int M, int C, void* stream);
int sfm_col_stats_shifted(const float* y, const float* K, float* S, int M, int C, float* ws, void* stream);
/* gradient fan-in: out[m, c] = a[m, c] + (c < Cb ? b[m, c] : 0), fp32 rows with strides lda / ldb / ldo (C, Cb multiples of 4) */
int sfm_add_cols(const float* a, const float* b, float* out, long long M, int C, int Cb, long long lda, long long ldb, long long ldo,
                 void* stream);
/* BiLSTM dW_hh operand: previous output of each chain, h fp32 [B, T, 2H] -> out 16-bit [B*T, 2H]
 * (out[b,t,:H] = h[b,t-1,:H], out[b,t,H:] = h[b,t+1,H:], zero at the chain's first step) */
int sfm_lstm_hprev16(const float* h, void* out, int B, int T, int H, int dtype, void* stream);
/* nn.BatchNorm1d training statistics from the shifted sums S of sfm_col_stats_shifted and their shift K (sfm_col_pilot):
 * mean = K + S0 / M, var = S1 / M - (S0 / M)^2, rstd, folded affine (sc, sh) and the in-place update of the running statistics
 * (unbiased variance; run_* may be NULL); eval_mode: statistics = run_mean / run_var, nothing updated (S, K may be NULL) */
int sfm_bn_finalize(const float* S, const float* K, const float* gamma, const float* beta, float* run_mean, float* run_var,
                    float* mean, float* rstd, float* sc, float* sh, int C, long long M, float eps, float momentum, int eval_mode,
                    void* stream);
int sfm_bn_swish_bwd(const void* g, const float* y, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, float* S, float* dy, int M, int C, int g_f32, int pass, int dtype,
                     float* ws, void* stream);             /* ws: as sfm_col_stats (pass 0 only) */
/* depthwise-conv weight/bias gradient: per-(utterance, span) partial sums go to `scratch`
 * (sfm_dwconv_wgrad_scratch_floats floats, need not be zeroed) and are reduced into dw [C, KS] / db [C] (accumulated). */
long long sfm_dwconv_wgrad_scratch_floats(int B, int T, int C, int KS);
int sfm_dwconv_wgrad(const void* x, const float* dy, float* dw, float* db, float* scratch, int B, int T, int C, int KS,
                     int dtype, void* stream);
/* attention forward for training (writes log2-domain LSE [B,H,T], applies attention dropout) and its backward */
int sfm_attention_fwd_train(const void* qkv, void* out, float* lse, int B, int T, int H, int hd, int ldqkv,
                            int ldo, int koff, int voff, long long qkv_batch_stride, long long o_batch_stride,
                            float scale, float p_drop, unsigned int seed, int dtype, void* stream);
int sfm_attention_bwd(const void* qkv, const void* O, const void* dO, const float* lse, float* delta, void* dqkv,
                      int B, int T, int H, int hd, int ldqkv, int ldo, int koff, int voff, float p_drop,
                      unsigned int seed, int dtype, void* stream);
/* The three training launches that see (B, T), on packed rows (utterance u = rows [frame_off[u], frame_off[u + 1]), int32[B + 1] on
 * the device).  Attention, head_dim 64 only: items = sfm_attention_fwd_varlen's table, one workgroup of each kernel per entry
 * (forward: 128 queries; backward: 128 queries for dQ, 128 keys for dK / dV); lse and the workspace delta are fp32 [H, sum_T]
 * (entry h * sum_T + packed row, log2 domain); the dropout hash row of (u, h, q) is H * frame_off[u] + h * T_u + q, which is the
 * dense launches' (b * H + h) * T + q when all lengths are equal. */
int sfm_attention_fwd_train_varlen(const void* qkv, void* out, float* lse, const int* frame_off, const int* items, int n_items,
                                   int B, int max_T, int sum_T, int H, int hd, int ldqkv, int ldo, int koff, int voff,
                                   float scale, float p_drop, unsigned int seed, int dtype, void* stream);
int sfm_attention_bwd_varlen(const void* qkv, const void* O, const void* dO, const float* lse, float* delta, void* dqkv,
                             const int* frame_off, const int* items, int n_items, int B, int max_T, int sum_T, int H, int hd,
                             int ldqkv, int ldo, int koff, int voff, float p_drop, unsigned int seed, int dtype, void* stream);
/* sfm_dwconv_wgrad on packed rows: spans = int32[n_spans][3] (utterance, first frame, frame count), every frame of every
 * utterance in exactly one span, no span across an utterance; the x window is zero outside the span's own utterance.  One
 * partial per span in scratch (sfm_dwconv_wgrad_varlen_scratch_floats floats; SFM_ERR_SHAPE when that count passes 2^31 - 1),
 * folded in table order into dw [C, KS] / db [C] (accumulated). */
int sfm_dwconv_wgrad_varlen_scratch_floats(int n_spans, int C, int KS);
int sfm_dwconv_wgrad_varlen(const void* x, const float* dy, float* dw, float* db, float* scratch, const int* frame_off,
                            const int* spans, int n_spans, int B, int sum_T, int C, int KS, int dtype, void* stream);
/* Linear layer with K = 256 inputs and a 16-bit result, one 8-wave workgroup per 128 rows for ALL output columns (A tile resident in
   registers, W streamed through an LDS-DMA ring, epilogue of a 64-row W chunk under the next chunk's MFMAs; csrc/lin256.hip):
     glu == 0: out[M, NW]     = A[M, 256] W^T + b                       (models/conformer.py:57-59, the Q | K | V projection)
     glu != 0: out[M, NW / 2] = GLU(A W^T + b), W rows in 64-row groups of 32 values | 32 gates
                                                                         (models/conformer.py:92-96, pointwise_conv1 + GLU)
   A rows have stride lda >= 256 (16-bit elements, multiple of 8), W is [NW, 256] row-major, NW % 64 == 0 (% 128 with glu),
   bias [NW] fp32 or NULL; out_dtype may be the other 16-bit format (one rounding of the fp32 accumulators) or, with glu == 0,
   2 = fp32 (ldo a multiple of 4; the BiLSTM input projections of agents/cpea.py:43-50).  The same contract as
   sfm_gemm16 on these shapes, and the same bits (same MFMA, same k order, same epilogue expressions). */
int sfm_lin256(const void* A, const void* W, const float* bias, void* out, int M, int NW, int lda, int ldo, int glu, int dtype,
               int out_dtype, void* stream);
/* The same with LayerNorm(X32[m, :256]; lnw, lnb, eps) as the operand rows (models/conformer.py:88 conv.layer_norm -> :92 pointwise_conv1):
   the workgroup that owns 128 rows for all output columns normalises them once, in its prologue, from the fp32 residual stream
   [M, ldx] - the arithmetic of sfm_layernorm on D = 256, bit for bit -, so sfm_layernorm + sfm_lin256 in one launch and without the
   16-bit normalised tensor in HBM.  16-bit results only. */
int sfm_ln_lin256(const float* X32, int ldx, const float* lnw, const float* lnb, float eps, const void* W, const float* bias,
                  void* out, int M, int NW, int ldo, int glu, int dtype, int out_dtype, void* stream);
/* PerceptionAgent latent heads (agents/perception.py:183-199, real_proj | imag_proj 1x1 convs stacked: NW = 2 * latent_dim rows of W) with
   the time pooling of the fused path (glue G1) in the same launch: pooled[b, i, :] = mean over the adaptive-average window of frame i
   of xd[b, t, :256] W^T + bias (16-bit, RAW: the GroupNorm that follows has no activation, is affine per (utterance, channel) and is
   applied to `pooled` afterwards - sfm_pool_time_affine16 with Tin == Tout), and the GroupNorm statistics of the FULL-RATE outputs:
   gn_partial [B, P, NW / gcols, 2] (sum, sum of squares per row tile; P = ceil(Tout / sfm_headpool_frames_per_tile(Tin, Tout)); reduce
   with sfm_gn_finalize(rows = Tin)).  The full-rate head outputs are never written.  gcols = 16; Tin >= Tout. */
int sfm_headpool_frames_per_tile(int Tin, int Tout);
int sfm_headpool(const void* xd, const void* W, const float* bias, void* pooled, float* gn_partial, int B, int Tin, int Tout, int NW,
                 int lda, int ldp, int gcols, int dtype, void* stream);

/* ---- The ragged front end: PerceptionAgent, pooling and CPEA on a zero-padded batch, one row per utterance,
   every buffer laid out for the LONGEST row, the valid length of each row in an int32 device table.  Each entry point is its
   dense one with a length per row.  Common contract: nothing beyond a row's length is READ (it is the dense kernel's own zero
   edge); what is WRITTEN for row b is, bit for bit, what the dense entry point writes for that utterance alone (B = 1); what
   lies beyond a row's length is either left untouched or written as ZEROS, as stated per entry point.  Tables are trusted to be
   consistent (the host builds them with the dense path's integer formulas); lengths are clamped to the buffers. ----
   sfm_sinc_fir16_varlen: the one-pass resident-tap kernel of sfm_sinc_fir16_ex.  wave [B, Lrow] fp32, lengths[b] <= Lrow valid
   samples; out [B, Lrow, 64]: rows < lengths[b] written, the others untouched; gn_partial [B][sfm_sinc_fir16_tiles(Lrow)][8][2]
   ZERO-FILLED by the caller: the slots of the tiles past lengths[b] stay zero, the others are those of the row alone (same slot
   indices).  passes: 1, or 0 where the auto rule picks 1 (fp16 operands, 16-bit result); else SFM_ERR_SHAPE. */
int sfm_sinc_fir16_varlen(const float* wave, const int* lengths, const float* filt, void* wsh, void* out, float* gn_partial, int B,
                          int Lrow, int C, int K, int out_f32, int dtype, int passes, void* stream);
/* sfm_conv16p with lin_tab[b] <= Lin input rows and lout_tab[b] = (lin_tab[b] + 2 pad - ksize) / stride + 1 output rows of
   utterance b.  x1, x2 [B, Lin, Cin]: rows >= lin_tab[b] never read.  out (out_s) [B, Lout, N]: rows < lout_tab[b] written, the
   others untouched.  gn_partial (_s) [B][2 ceil(Lout / 128)][N / gn_group][2] ZERO-FILLED by the caller: a workgroup whose tile
   starts at or past lout_tab[b] leaves before it stages anything.  Shapes as sfm_conv16p, skip and two-input forms included;
   fp16 operands only (SFM_DT_BF16: SFM_ERR_SHAPE). */
int sfm_conv16p_varlen(const void* x1, const float* sc1, const float* sh1, const void* x2, const float* sc2, const float* sh2,
                       const void* W, const float* bias, void* out, float* gn_partial, const void* Ws, const float* bias_s,
                       void* out_s, float* gn_partial_s, const int* lin_tab, const int* lout_tab, int B, int Lin, int Cin, int N,
                       int ksize, int stride, int pad, int out_f32, int gn_group, int dtype, void* stream);
/* sfm_gn_finalize with rows_tab[b] rows and p_tab[b] <= Pmax partial slots of utterance b: partial [B, Pmax, G, 2], of which the
   first p_tab[b] slots of row b are folded, in sfm_gn_finalize's order; the others are never read.  scale, shift [B, C]: all written. */
int sfm_gn_finalize_varlen(const float* partial, const float* w, const float* b, float* scale, float* shift, const int* rows_tab,
                           const int* p_tab, int B, int Pmax, int G, int C, float eps, void* stream);
/* sfm_gn_apply(act = 1, one input) on 16-bit rows with a 16-bit result: x1, out [B, L, C] in `dtype`, C a power of two in
   [64, 2048].  Rows < rows_tab[b]: GELU(x1 * sc1[b] + sh1[b]); rows >= rows_tab[b]: never read, written as ZEROS (the zero edge of
   the k 3 uncertainty conv that sfm_gemm16 then runs on out). */
int sfm_gn_apply_varlen(const void* x1, const float* sc1, const float* sh1, void* out, const int* rows_tab, int B, int L, int C,
                        int dtype, void* stream);
/* sfm_headpool with tab int32 [B][4] = (Tin_b, Tout_b, sfm_headpool_frames_per_tile(Tin_b, Tout_b), ceil(Tout_b / that)):
   xd [B, TinS, lda]: rows >= Tin_b never read; pooled [B, ToutS, ldp]: rows < Tout_b as sfm_headpool, rows >= Tout_b ZEROS (NW
   columns); gn_partial [B, PS, NW / gcols, 2] ZERO-FILLED by the caller: a tile at or past P_b leaves. */
int sfm_headpool_varlen(const void* xd, const void* W, const float* bias, void* pooled, float* gn_partial, const int* tab, int B,
                        int TinS, int ToutS, int PS, int NW, int lda, int ldp, int gcols, int dtype, void* stream);
/* sfm_bilstm_layer_rows16 with ttab[b] <= T steps of chain b: the forward chain walks 0 .. ttab[b] - 1, the reverse one starts at
   ttab[b] - 1.  xg [B, T, 2, 4H]: rows >= ttab[b] never read; out16 [B * T, ld16]: rows < ttab[b] as the dense kernel gives for
   the chain alone, rows >= ttab[b] ZEROS (2H columns).  A finished chain idles while the others of its workgroup go on.  H 128
   with w16 != 0 only (else SFM_ERR_SHAPE). */
int sfm_bilstm_layer_rows16_varlen(const float* xg, const float* whh, void* out16, long long ld16, const int* ttab, int B, int T,
                                   int H, int w16, int dtype, void* stream);
/* The hand-over to the packed back half, on 32-bit words: src [B, src_rows, ld_src] -> dst [sum_b rows_tab[b], ld_dst]; the first
   `width` words of row r < rows_tab[b] of utterance b go to row dst_off[b] + r (dst_off = exclusive prefix sums of rows_tab).
   Rows >= rows_tab[b] never read; every word of dst's `width` columns written. */
int sfm_rows_gather32(const void* src, void* dst, const int* rows_tab, const int* dst_off, int B, int src_rows, int width,
                      long long ld_src, long long ld_dst, void* stream);

/* one direction-pair of an nn.LSTM layer (agents/cpea.py:43-50,99), see lstm.hip */
int sfm_bilstm_layer(const float* xg, const float* whh, float* out, int B, int T, int H, int dtype, void* stream);
/* inference only: w16 != 0 runs the recurrent product W_hh h on fp16 operands (weights and h rounded once, fp32 accumulation, gates /
   cell state / output fp32).  H 128: four chains of one direction per workgroup, the product on v_mfma_f32_4x4x4_16b_f16
   (2.3 x the fp32 kernel at batch 256, 1.2 x at batch 64); a chain's result does not depend on B or on the other chains.  H 64:
   v_dot2_f32_f16, one chain per workgroup; H 32 keeps the fp32 kernel.  (agents/cpea.py:43-50,99: the same nn.LSTM recurrence) */
int sfm_bilstm_layer_ex(const float* xg, const float* whh, float* out, int B, int T, int H, int w16, void* stream);
/* the same recurrence with the result written as 16-bit rows out16 [B * T, ld16] (ld16 >= 2H elements) in `dtype` (SFM_DT_F16 /
   SFM_DT_BF16): bit for bit sfm_convert_rows of sfm_bilstm_layer_ex's fp32 result, which is then never written.  H 128 with
   w16 != 0 only (else SFM_ERR_SHAPE): the fused forward, whose next GEMM reads these rows. */
int sfm_bilstm_layer_rows16(const float* xg, const float* whh, void* out16, long long ld16, int B, int T, int H, int w16,
                            int dtype, void* stream);
/* sfm_bilstm_layer_train with the same fp16-operand recurrent product (the reference's LSTM runs under fp16 autocast in training:
   training/conformer_pipeline.py:504); `save` and the BPTT (sfm_bilstm_layer_bwd) stay fp32 */
int sfm_bilstm_layer_train_ex(const float* xg, const float* whh, float* out, float* save, int B, int T, int H, int w16, void* stream);
/* training: as sfm_bilstm_layer, also saving the activated gates and cell states [B, T, 2, 5, H] fp32; and the BPTT of
 * the layer: dout [B, T, 2H] -> dxg [B, T, 2, 4H] = gradient w.r.t. the input projection (dW_ih, dW_hh, biases and dx
 * are GEMMs / column sums of dxg afterwards). */
int sfm_bilstm_layer_train(const float* xg, const float* whh, float* out, float* save, int B, int T, int H, int dtype,
                           void* stream);
int sfm_bilstm_layer_bwd(const float* save, const float* whh, const float* dout, float* dxg, int B, int T, int H,
                         void* stream);
/* EpisodicMemory.forward eval (agents/memory.py:112-133) in one launch, see memory.hip */
int sfm_memory_fwd(const float* emb, const float* params, float* bias_out, float* gate_out, int* top_idx,
                   float* sim_out, int B, int key_dim, int value_dim, int slots, float temperature, void* stream);
/* Backward of sfm_memory_fwd (EpisodicMemory in train() mode): d_out = gradient of the gated bias [B, value_dim], d_gate = of
 * the gate [B] (or NULL); d_emb [B, key_dim] (or NULL) and dparams = a ZERO-FILLED blob with the layout of `params`
 * (gradients of key_proj, keys, values, value_proj, gate, accumulated over the rows: with ws - sfm_memory_bwd_ws_floats floats -
 * every row writes its own copy of the blob and the copies are folded in row order; ws == NULL: fp32 atomics). */
long long sfm_memory_param_floats(int key_dim, int value_dim, int slots);
long long sfm_memory_bwd_ws_floats(int B, int key_dim, int value_dim, int slots);
int sfm_memory_bwd(const float* emb, const float* params, const float* d_out, const float* d_gate, float* d_emb,
                   float* dparams, int B, int key_dim, int value_dim, int slots, float temperature, float* ws, void* stream);

/* Stage objectives of the curriculum (training/losses.py:22-143; curriculum_losses.hip).  Both write the scalar loss to loss[0]
 * and, when a gradient pointer is given, EVERY element of the gradient (callers need not zero it) in the same launch.  Sums over
 * workgroups go through `ws` (required; scratch, destroyed) and the ordered fold: no atomics, bit-reproducible.
 * sfm_pstoi_loss: loss = -mean over (B, NB, S = T / frame_len) of the correlation of the mean-removed, clipped band envelopes.
 *   layout 0: e0 / c0 = enhanced / clean magnitudes [B, F, T]; e1 = c1 = g1 = NULL; g0 (or NULL) [B, F, T].
 *   layout 1: (e0, e1) / (c0, c1) = (real, imag) of enhanced / clean, channels-last [B, T, F]; the magnitude is
 *     sqrt(re^2 + im^2 + 1e-8); (g0, g1) both or neither, [B, T, F].
 *   band_w [NB, F] dense (rows may overlap); beta_db = the clip level in dB (10^(beta / 20) x the clean energy).
 *   The clean side gets no gradient.  Frames t >= S * frame_len are unused and get gradient 0.
 *   ws: sfm_pstoi_loss_ws_doubles(B, T, frame_len) doubles.  SFM_ERR_SHAPE: NB > SFM_PSTOI_MAX_BANDS, F > SFM_PSTOI_MAX_BINS,
 *   frame_len outside SFM_PSTOI_MIN_FRAME_LEN .. SFM_PSTOI_MAX_FRAME_LEN, T < frame_len, B * S > 2^31 - 1.
 * sfm_mse_loss: loss = mean (pred - target)^2 over n elements, summed in double; grad (or NULL) = 2 (pred - target) / n.
 *   ws: sfm_mse_loss_ws_doubles(n) doubles. */
long long sfm_pstoi_loss_ws_doubles(int B, int T, int frame_len);
int sfm_pstoi_loss(const float* e0, const float* e1, const float* c0, const float* c1, const float* band_w, float* loss,
                   float* g0, float* g1, double* ws, int B, int T, int F, int NB, int frame_len, float beta_db, int layout,
                   void* stream);
long long sfm_mse_loss_ws_doubles(long long n);
int sfm_mse_loss(const float* pred, const float* target, float* loss, float* grad, double* ws, long long n, void* stream);

/* AdversarialLoss (training/losses.py:150-289; adversarial.hip): what a discriminator call needs around the convs, which run on
 * sfm_gemm16 / sfm_conv_wgrad16.  Activations are channels-last 16-bit rows; sums are ordered (no atomics).  `loss` is ONE double
 * that the forward entry points ADD their scaled term to, in stream order: the caller zeroes it once per objective.
 * Forward operands are PAIRS of 16-bit words, v = hi + lo / 2048 (hi = v rounded to `dtype`, lo = the rounding error x 2048, also
 *   rounded): the `*lo` / `packed_lo` arguments, laid out like their hi twins.  The caller runs hi x hi + (lo x hi + hi x lo) / 2048
 *   (three sfm_gemm16 launches, the last two accumulating with alpha = 1 / 2048), so a pre-activation carries ~2^-20 and the
 *   kinks of LeakyReLU and of the L1 term are decided as in fp32; the backward uses the hi words alone.
 * sfm_adv_sn_fwd: legacy torch.nn.utils.spectral_norm (one power iteration, dim 0) of the n_layers convs of a discriminator, one
 *   workgroup per row of `table` (device, 16 int64 words per layer): {weight_orig [N][Cin][k] fp32, bias [N], weight_u [N],
 *   weight_v [Cin k], N, Cin, k, Cp, Npad, Kpad, off16, off32}.  training != 0: v <- normalize(W^T u), u <- normalize(W v),
 *   both written back; else the buffers are only read.  sigma = u^T W v.  packed + off16 receives W / sigma as [Npad][Kpad]
 *   16-bit in sfm_gemm16's layout (column tap * Cp + ci, zero elsewhere); saved + off32 receives bias [Npad] | u [N] | v [Cin k]
 *   | W v [N] | sigma [1] of THIS call (its backward needs them; off16 % 8 == 0).
 * The backward entry points share (g, cnorm): g = the objective's incoming gradient (one float, on the device), cnorm = its
 *   largest static coefficient.  Each derives the same power of two S = 2^k, |g cnorm| S in [32, 64), and everything the pass
 *   rounds to 16 bits carries S (so fp16 dY tensors stay in the normal range whatever g is); S is divided out, exactly, where a
 *   gradient leaves in fp32.  g == NULL: S = 1.
 * sfm_adv_sn_bwd: d weight_orig [N][Cin][k] (= or +=) (G - <G, W / sigma> u v^T) / sigma / S for G = S dL/d(W / sigma)
 *   [N][k][Cp] tap-major as sfm_conv_wgrad16 leaves it; db (= or +=) db_in / S (both or neither); u, v, sigma from the forward
 *   call's `saved`.
 * sfm_adv_stage: pair == 0: x [B, F, T] fp32 magnitudes; pair != 0: (x, im) = (real, imag) [B, T, F], magnitude
 *   sqrt(re^2 + im^2 + 1e-8).  -> x16 [B, T, Cp] 16-bit, columns >= F zero, and x32 [B, T, F] fp32 (or NULL).
 * sfm_adv_stage_bwd: the adjoint: d [B, T, Cp] fp32 (carrying S) -> dx [B, F, T], or (dx, dx_im) [B, T, F]; every element written.
 * sfm_adv_leaky: a16 = LeakyReLU_0.2(z) for n fp32 pre-activations (n % 4 == 0); with z_real (the real pass's pre-activation
 *   of the same layer) also loss += scale * sum |leaky(z) - leaky(z_real)|; ws: sfm_adv_leaky_ws_doubles(n) doubles.
 * sfm_adv_leaky_bwd: dz16 = (incoming + S * w_fm * g[0] * sign(leaky(z) - leaky(z_real))) * (z > 0 ? 1 : 0.2): the 16-bit dY of the
 *   two gradient GEMMs; incoming or z_real may be NULL (not both).  g = the objective's incoming gradient, on the device.
 * sfm_adv_pool: AvgPool1d(4, 2, 1), padding counted: in32 [B, Tin, F] -> out32 [B, Tin / 2, F] (or NULL), out16 [B, Tin / 2, Cp].
 * sfm_adv_pool_bwd: dx [B, Tin, Cp] += its adjoint of dnext [B, Tin / 2, Cp].
 * sfm_adv_head: out [B, T] = Conv1d(C, 1, 3, pad 1) of a16 [B, T, C] with w16 [3][C] tap-major 16-bit and bias[0];
 *   loss += scale * sum (out - target)^2; ws: sfm_adv_head_ws_doubles(B, T) doubles.
 * sfm_adv_head_bwd: dout = g[0] * coef * (out - target); da [B, T, C] fp32 = S x its adjoint; dwb (or NULL) = dw [3][C] tap-major | db
 *   (not scaled), through ws: sfm_adv_head_bwd_ws_floats(B, T, C) floats. */
int sfm_adv_sn_fwd(const long long* table, int n_layers, void* packed, void* packed_lo, float* saved, int training, float eps,
                   int dtype, void* stream);
int sfm_adv_sn_bwd(const float* G, const float* W, const float* u, const float* v, const float* sigma, float* dW,
                   const float* db_in, float* db, const float* g, float cnorm, int N, int Cin, int ksize, int Cp, int accumulate,
                   void* stream);
int sfm_adv_stage(const float* x, const float* im, void* x16, void* x16lo, float* x32, int B, int F, int T, int Cp, int pair,
                  int dtype, void* stream);
int sfm_adv_stage_bwd(const float* d, const float* re, const float* im, float* dx, float* dx_im, const float* g, float cnorm, int B,
                      int F, int T, int Cp, int pair, void* stream);
long long sfm_adv_leaky_ws_doubles(long long n);
int sfm_adv_leaky(const float* z, const float* z_real, void* a16, void* a16lo, double* ws, double* loss, float scale, long long n,
                  int dtype, void* stream);
int sfm_adv_leaky_bwd(const float* incoming, const float* z, const float* z_real, const float* g, float w_fm, float cnorm,
                      void* dz16, long long n, int dtype, void* stream);
int sfm_adv_pool(const float* in32, float* out32, void* out16, void* out16lo, int B, int Tin, int F, int Cp, int dtype,
                 void* stream);
int sfm_adv_pool_bwd(const float* dnext, float* dx, int B, int Tin, int Cp, void* stream);
long long sfm_adv_head_ws_doubles(int B, int T);
int sfm_adv_head(const void* a16, const void* a16lo, const void* w16, const void* w16lo, const float* bias, float* out, double* ws,
                 double* loss, float target, float scale, int B, int T, int C, int dtype, void* stream);
long long sfm_adv_head_bwd_ws_floats(int B, int T, int C);
int sfm_adv_head_bwd(const void* a16, const void* w16, const float* out, const float* g, float coef, float cnorm, float target,
                     float* da, float* dwb, float* ws, int B, int T, int C, int dtype, void* stream);

/* Curriculum batches (masks.hip): the mask targets of masks/{irm,pcirm,opt_pcirm}.py on n contiguous fp32 elements per plane, the
 * SNR mix of training/conformer_pipeline.py:142-150 (the rule of training/pipeline.py:71-94) over a batch, and the two fused.
 * All planes fp32; 16-byte accesses where every plane is 16-byte aligned, scalar ones otherwise.  n, B * L and B * T * F are at
 * most 2^31 - 1 (SFM_ERR_SHAPE beyond).  No atomics anywhere: results are the same bits from run to run.
 * sfm_mask_irm: out = clip((c^2 / (c^2 + n^2 + eps))^p, 0, 1) of the magnitudes c, n; p = 0.5 takes a square root, any other
 *   p > 0 powf (p <= 0: SFM_ERR_ARG).
 * sfm_mask_corr: rho_s = clip(|y c| / (sqrt(y^2 + eps) sqrt(c^2 + eps)), 0, 1) of noisy y and clean c, rho_n likewise of y and
 *   the noise: the per-T-F-unit rule (masks/pcirm.py:49-57) at every element, whatever the rank of the caller's tensors.
 * sfm_mask_pcirm: out = clip(S / (S + N + eps), 0, 1), S = rho_s (c |cos phi1|)^2, N = rho_n (n |cos phi2|)^2.
 * sfm_mask_quantize: table = M + 1 ascending boundaries [0, s_2 .. s_M, 1] then the M assigned values, doubles on the device;
 *   out = the value of the step m with boundary[m] <= x < boundary[m + 1], the last value for x >= boundary[M], compared in
 *   double; 0 where no step holds x (a NaN, a negative value).  M in 2..16 (SFM_ERR_SHAPE outside).
 * sfm_mix_scale: clean [B, L]; bank = every noise signal back to back, bank_off int32 [n_noise + 1] ascending from 0;
 *   noise_ids int32 [B] (clamped to the bank); snr_db [B]; lengths int32 [B] or NULL (= L; clamped to 0..L).  Utterance b is
 *   mixed with noise[j mod Ln] at sample j (a shorter noise tiled, a longer one cut).  Two launches: fp64 sums of clean^2 and
 *   noise^2 over the first lengths[b] samples, one partial pair per workgroup of SFM_MIX_CHUNK samples; then ONE workgroup adds each
 *   utterance's partials in index order and writes scale[b] = sqrt(Pc / (Pn 10^(snr_db / 10))), P = mean + 1e-10.
 *   ws: sfm_mix_scale_ws_doubles(B, L) doubles.  B <= 65535.
 * sfm_mix_apply: noisy[b, j] = clean[b, j] + scale[b] * noise[j mod Ln] for j < lengths[b], 0 from there on; noise_rows
 *   (or NULL) [B, L] receives the unscaled noise[j mod Ln], 0 from lengths[b] on.  Every element is written.
 * sfm_curriculum_mask: (cr, ci), (nr, ni) = spectra [B, T, F] of the clean utterances and of sfm_mix_apply's noise rows.
 *   (yr, yi) = C + scale[b] N, the spectrum of the mix (the STFT is linear).  kind 0: no mask (mask may be NULL); 1: the IRM
 *   of |C| and |s N| with exponent p; 2: the PCIRM of |C|, |s N|, |Y| with rho_s, rho_n as sfm_mask_corr gives them for
 *   those magnitudes and phi1 = arg C - arg Y, phi2 = arg N - arg Y, whose cosines are taken as Re(C conj Y) / (|C| |Y|) (a zero
 *   counts as phase 0); 3: that PCIRM quantised by `table` (sfm_mask_quantize's, M steps).
 * sfm_mix_scale_varlen: sfm_mix_scale on packed utterances.  Utterance u is packed[utt_off[u] .. utt_off[u + 1]), utt_off int32
 *   [n_utt + 1] ascending from 0 (clamped to 0 .. total, the sample count of `packed`); its length is its own, any alignment.  The
 *   same chunk partials, ordered fold and formula; the grid is the chunks of max_len (the longest utterance) x n_utt, samples of
 *   an utterance beyond max_len are not summed.  ws: sfm_mix_scale_varlen_ws_doubles(n_utt, max_len) doubles - an int, which is
 *   SFM_ERR_SHAPE where the entry point refuses: n_utt outside 1 .. 65535, max_len < 1, more than 2^31 - 1 doubles.
 * sfm_wave_batch: out [2, B, L] from index int32 [B] into a packed set (packed, utt_off, noise_ids [n_utt], scale [n_utt]).  With
 *   u = index[b]: out[0, b, j] = packed[utt_off[u] + j] + scale[u] * noise[j mod Ln], out[1, b, j] = packed[utt_off[u] + j] for
 *   j < min(length of u, L), and 0 from there on; both rows are 0 where u is outside 0 .. n_utt - 1 (-1: an empty row).  Every
 *   element is written.  A mixed row has the bits sfm_mix_apply gives for the padded utterance with that scale.  2 B L <= 2^31 - 1,
 *   B <= 65535. */
int sfm_mask_irm(const float* clean_mag, const float* noise_mag, float* out, long long n, float p, float eps, void* stream);
int sfm_mask_corr(const float* noisy, const float* clean, const float* noise, float* rho_s, float* rho_n, long long n, float eps,
                  void* stream);
int sfm_mask_pcirm(const float* clean_mag, const float* noise_mag, const float* rho_s, const float* rho_n, const float* phi1,
                   const float* phi2, float* out, long long n, float eps, void* stream);
int sfm_mask_quantize(const float* pcirm, const double* table, float* out, long long n, int M, void* stream);
long long sfm_mix_scale_ws_doubles(int B, int L);
int sfm_mix_scale(const float* clean, const float* bank, const int* bank_off, const int* noise_ids, const float* snr_db,
                  const int* lengths, double* ws, float* scale, int B, int L, int n_noise, void* stream);
int sfm_mix_apply(const float* clean, const float* bank, const int* bank_off, const int* noise_ids, const int* lengths,
                  const float* scale, float* noisy, float* noise_rows, int B, int L, int n_noise, void* stream);
int sfm_mix_scale_varlen_ws_doubles(int n_utt, int max_len);
int sfm_mix_scale_varlen(const float* packed, const int* utt_off, const float* bank, const int* bank_off, const int* noise_ids,
                         const float* snr_db, double* ws, float* scale, int n_utt, int max_len, int total, int n_noise,
                         void* stream);
int sfm_wave_batch(const float* packed, const int* utt_off, const float* bank, const int* bank_off, const int* noise_ids,
                   const float* scale, const int* index, float* out, int B, int L, int n_utt, int total, int n_noise,
                   void* stream);
int sfm_curriculum_mask(const float* cr, const float* ci, const float* nr, const float* ni, const float* scale,
                        const double* table, float* yr, float* yi, float* mask, int B, int T, int F, int kind, float p, float eps,
                        int M, void* stream);

/* The PSO search of OPT-PCIRM's middle step with the STOI fallback as fitness (masks/opt_pcirm.py:101-202, optimizer/pso.py,
 * evaluation/stoi.py:53-99), one swarm of N particles per utterance (csrc/pso.hip).  B <= 65535, 1 <= N <= 256, M in 2..16,
 * max_iter >= 1 (SFM_ERR_SHAPE outside).  No atomics: the same bits from run to run and for an utterance alone or in a batch.
 * sfm_pso_frame_coef: pcirm [B, C, T] fp32, table as sfm_mask_quantize takes it -> a, b [B, T] doubles: the channel mean of
 *   the mask's frame n quantised with the middle value x is a[n] + x b[n] (bucket membership compared in double, assigned values
 *   rounded to fp32; M < 3: b = 0, the middle value is unused).
 * sfm_pso_split: noisy, clean [B, Lmax]; lengths int32 [B]; samp_off int32 [B + 1] = the running sum of the lengths.  Mask frames
 *   of `frame` samples every `hop` (frame >= hop), frame n < T covering [n hop, min(n hop + frame, length)), overlap-added and
 *   divided by max(count, 1) give the gains ga, gb.  Writes ya = noisy ga, yb = noisy gb and clean, each utterance's samples
 *   at samp_off[b] (packed, fp32), and S [B, 4] = {sum ya^2, sum ya yb, sum yb^2, sum clean^2}: one fp64 partial per
 *   SFM_PSO_CHUNK samples, folded in index order.  ws: sfm_pso_split_ws_doubles(B, Lmax) doubles.
 * sfm_pso_fitness: packed spectra rows [sum_frames, F] (F <= 1024) of clean, ya, yb; frame_off int32 [B + 1].  For each
 *   utterance whose stopped[b] is 0 and each of its N positions x (rounded to fp32): the clipped frame correlations of
 *   clean / rms against (ya + x yb) / rms, summed over chunks of 8 frames: partial [B, NC, N], NC >= ceil(frames / 8) of every
 *   utterance; only an utterance's own chunks are written.
 * sfm_pso_step: round `it` of the search (0: optimizer/pso.py:92-110; 1..max_iter: one iteration, :114-179) for every swarm
 *   whose stopped[b] is 0.  The fitness is clip(sum of the partials in chunk order / frames, 0, 1) (0 without a frame), or
 *   `fitness` [B, N] handed in (exactly one of partial / fitness is non-NULL).  params = {w, c1, c2, lb, ub}; draws [B, 2 N +
 *   2 N max_iter]: initial positions, initial velocities, then (r1, r2) per iteration and particle.  Updates pbest and gbest
 *   [B, 2] = {position, fitness}, writes row `it` of hist [B, max_iter + 1, 3 + 2 N] = {gbest fitness, gbest position, mean
 *   fitness, position[N], fitness[N]}, iters[b] = it, stopped[b] = 1 once np.std(positions) < 1e-6, and unless stopped or
 *   it == max_iter moves pos / vel to the next iteration's.  The caller sets pos / vel to the first 2 N draws before round 0.
 * sfm_pso_quantize: sfm_mask_quantize over [B, CT] with middle[b] (double, rounded to fp32) as step 2's value when M >= 3. */
int sfm_pso_frame_coef(const float* pcirm, const double* table, double* a, double* b, int B, int C, int T, int M, void* stream);
long long sfm_pso_split_ws_doubles(int B, int Lmax);
int sfm_pso_split(const float* noisy, const float* clean, const int* lengths, const int* samp_off, const double* a,
                  const double* b, float* ya, float* yb, float* clean_packed, double* ws, double* S, int B, int Lmax, int T,
                  int frame, int hop, void* stream);
int sfm_pso_fitness(const float* cr, const float* ci, const float* ar, const float* ai, const float* br, const float* bi,
                    const int* frame_off, const int* lengths, const double* S, const double* pos, const int* stopped,
                    double* partial, int B, int N, int F, int NC, void* stream);
int sfm_pso_step(const double* partial, const double* fitness, const int* frame_off, const double* draws, const double* params,
                 double* pos, double* vel, double* pbest_pos, double* pbest_fit, double* gbest, double* hist, int* iters,
                 int* stopped, int B, int N, int NC, int it, int max_iter, int maximize, void* stream);
int sfm_pso_quantize(const float* pcirm, const double* table, const double* middle, float* out, int B, long long CT, int M,
                     void* stream);

/* Gammatone T-F analysis (gammatone.hip; signal_processing/gammatone.py of the reference): a causal FIR bank of C <= 64 channels
 * and K <= 2048 taps on the fp32 matrix cores and the per-frame power / centre-bin phase of get_tf_magnitudes from five sums per
 * frame instead of an rfft.  sig [B, L] fp32; taps [K][64] fp32, tap-major, K a multiple of 8 (a bank is padded with zero rows), columns
 * from C on zero; lengths int32 [B] or NULL (= L): samples from lengths[b] on read as 0.  B <= 65535.  wave64, no atomics: the same bits
 * from run to run and for an utterance alone or in a batch.
 * sfm_gammatone_fir: out [B, C, L] = sum_k taps[k][c] sig[b, m - k] (0 from lengths[b] on).
 * sfm_gammatone_tf: the fused form.  nblocks = L / hop whole hop-blocks; tw [2][hop][64] = cos, sin of 2 pi (k_c t mod N) / N for
 *   the block-local t; partial [B, nblocks, C, 5] = {sum y^2, sum y, sum (-1)^t y, sum y cos, sum y sin} of each block, summed in
 *   fp64 in t order and rounded once.  hop even, 2..384, and (25344 + K + 128 hop) * 4 bytes of LDS <= 160 KiB (SFM_ERR_SHAPE
 *   otherwise): sfm_gammatone_tf_fits(K, hop) != 0 - the same rule as a predicate, for the caller's router (no device work).
 *   Blocks that start behind lengths[b] are not written.
 * sfm_gammatone_moments: y [B, C, L] (sfm_gammatone_fir's) -> partial [B, T, C, 5]: the same five sums over the first w <= frame
 *   samples of frame n = y[n hop .. n hop + frame), frame-local t; tw [2][w][64].  Frames that end behind lengths[b] are not written.
 * sfm_gammatone_tf_finish: partial [B, P, C, 5] -> mag, phase and (unless NULL) re, im [B, C, T].  two = 1: frame n is rows n and
 *   n + 1, the second times rot [2][64] = cos, sin of 2 pi (k_c hop mod N) / N; two = 0: row n alone.  mag = (N s2 + s1^2 + sp^2) / 2,
 *   phase = atan2(im, re), in fp64 from the fp32 partials; everything from T_b = (lengths[b] - frame) / hop + 1 on is 0. */
int sfm_gammatone_fir(const float* sig, const float* taps, const int* lengths, float* out, int B, int L, int C, int K, void* stream);
int sfm_gammatone_tf_fits(int K, int hop);
int sfm_gammatone_tf(const float* sig, const float* taps, const float* tw, const int* lengths, float* partial, int B, int L, int C,
                     int K, int hop, int nblocks, void* stream);
int sfm_gammatone_moments(const float* y, const float* tw, const int* lengths, float* partial, int B, int L, int C, int T, int w,
                          int frame, int hop, void* stream);
int sfm_gammatone_tf_finish(const float* partial, const float* rot, const int* lengths, float* mag, float* phase, float* re,
                            float* im, int B, int C, int T, int P, int two, int L, int frame, int hop, int N, void* stream);

/* Meddis inner hair cell (haircell.hip; signal_processing/haircell.py of the reference): x [N, L] fp32, one chain of L Euler steps in
 * fp64 per row, every operation one IEEE double operation in the reference's order (no fused multiply-add), the three clamps kept.
 * par fp64 [12] = {A, B, y, l, r, x, h, M, dt, q0, c0, w0}.  A wave stages 64 rows x 64 samples through LDS; no atomics.
 * sfm_haircell: out [N, L] fp64 = h c[t], bit for bit the reference's process on the same fp32-valued input.
 * sfm_haircell_frames: frames [N, T] fp64 = the mean of the firing rate over [n hop, n hop + frame), T = (L - frame) / hop + 1,
 *   frame <= 2 hop (SFM_ERR_SHAPE otherwise), summed in t order; the rate signal is not stored.  Row i belongs to utterance i / C;
 *   lengths int32 [N / C] or NULL (= L): a chain stops at lengths[b], frames from T_b = (lengths[b] - frame) / hop + 1 on are 0. */
int sfm_haircell(const float* x, const double* par, double* out, int N, int L, void* stream);
int sfm_haircell_frames(const float* x, const double* par, const int* lengths, double* frames, int N, int C, int L, int frame,
                        int hop, int T, void* stream);

/* The DNN front end (features.hip; signal_processing/features.py of the reference).  Rows are frames: row b T + n of utterance b,
 * T_b = (lengths[b] - frame) / hop + 1 of them live (lengths int32 [B] or NULL = L); rows from T_b on are neither read nor written by
 * sfm_cepstral / sfm_rasta (the caller zero-fills) and written as 0 by sfm_feature_context.  wave64, no atomics.
 * sfm_cepstral: out[row ld_out + col_off + j] = sum_m dct[j][m] v[m], j < NC (NC = 0: v itself, j < M), v = compress(fb p),
 *   fb [M][F] fp32 (NULL: p itself, M = F), M <= 64, F <= 257, NC <= 16, dct [NC][M] fp32.  in_mode 0: p = re^2 + im^2 of the spectrum row
 *   in[row ld_in + f], in[row ld_in + im_off + f]; 1: its square root; 2: in = partial [B, P, F, 5] of sfm_gammatone_tf,
 *   p[c] = (partial[b, bmul n + badd, c, 0] + partial[b, bmul n + badd + 1, c, 0]) / window.  compress 0: none, 1: log(v + 1e-10),
 *   2: sign(v) |v|^(1/3); logarithm, cube root and DCT in fp64, the filterbank an fmaf chain in bin order.
 * sfm_rasta: logb [B, T, M] fp32 -> lfilter([.2, .1, 0, -.1, -.2], [1, -.98]) per band along the utterance's T_b frames from a zero
 *   state, exp, times eql [M], cube root, mean over the T_b frames in frame order, DCT rows dct [NC][M]; eql, dct and all of it fp64;
 *   the NC coefficients go to out[row ld_out + col_off + k] of every live row of the utterance.
 * sfm_feature_context: feat [B, T, D] -> out [B, T, (2 ctx + 1) D]: row n = rows clamp(n - ctx .. n + ctx, 0, T_b - 1) side by side;
 *   with mean / std [(2 ctx + 1) D] fp32 (both or neither): nan / inf -> 0, then (f - mean) / std in fp64, then a clip to +-clip.  D even.
 * sfm_rows_mean: out [B, N] = sum over n < T_b of in[(b T + n) ld_in + col_off + j] / (den > 0 ? den : T_b), fp64 in frame order. */
int sfm_cepstral(const float* in, const float* fb, const float* dct, const int* lengths, float* out, int B, int T, int L, int frame,
                 int hop, int in_mode, long long ld_in, int im_off, int F, int M, int NC, int compress, int P, int bmul, int badd,
                 float window, long long ld_out, int col_off, void* stream);
int sfm_rasta(const float* logb, const double* eql, const double* dct, const int* lengths, float* out, int B, int T, int L, int frame,
              int hop, int M, int NC, long long ld_out, int col_off, void* stream);
int sfm_feature_context(const float* feat, const float* mean, const float* stdv, const int* lengths, float* out, int B, int T, int L,
                        int frame, int hop, int D, int ctx, float clip, void* stream);
int sfm_rows_mean(const float* in, const int* lengths, float* out, int B, int T, int L, int frame, int hop, long long ld_in,
                  int col_off, int N, int den, void* stream);

/* CSII and NCM (intelligibility.hip; evaluation/csii.py and evaluation/ncm.py of the reference).  wave64, no atomics, every
 * cross-thread sum in fp64 in a fixed order: the same bits from run to run and for an utterance alone or in any pack.
 * sfm_csii_frames_varlen: cr, ci, er, ei = the planes [sum_frames, F] sfm_framed_gemm_f32_varlen wrote for the clean and the enhanced
 *   pack with the Hamming rfft(., 256) operand, F = 129 (SFM_ERR_SHAPE otherwise); utterance b owns rows [frame_off[b], frame_off[b + 1]).
 *   Per bin, over the utterance's frames in frame order: Pxx, Pyy, Pxy, divided by the frame count; msc = |Pxy|^2 / (Pxx Pyy + 1e-10)
 *   clipped to [0, 1] -> msc [B, 129] (or NULL); score [B] = clip(sum_f weights[f] msc[f], 0, 1) in bin order, 0 without a frame.
 * sfm_hilbert_env: x [R, L] fp32 -> env [R, L] = sqrt(x^2 + y^2), y = h (*) x circularly, h the kernel of scipy.signal.hilbert(.).imag.
 *   table = 2 L floats.  Odd L: h twice back to back, y[n] = sum_m table[n - m + L] x[m].  Even L (every even lag of h is 0): two
 *   convolutions of L / 2 samples, y[2 i + p] = sum_j table[p L + i - j + L / 2] x[2 j + 1 - p], i.e. g_p[d] = h[(2 d + 2 p - 1) mod L]
 *   twice for p = 0, then for p = 1.  L >= 1, L < 2^30.
 * sfm_hilbert_env_moments: X [2, B, C, L] fp32 (clean and enhanced sfm_gammatone_fir planes, 0 from lengths[b] on), C <= 64 (2 C <= 128
 *   operand columns; SFM_ERR_SHAPE beyond); utterance b convolves over its own lengths[b] samples with the table at tables + tab_off[b]
 *   (2 lengths[b] floats, as above).  tiles int32 [n_tiles][2] = (utterance, output tile of 256 samples of a convolution), utterance-
 *   major, tiles ascending: ceil(L_b / 256) of an odd length, 2 ceil(L_b / 512) of an even one (p = 0, then p = 1);
 *   partial [n_tiles, C, 5] fp64 = {sum ec, sum ee, sum ec^2, sum ee^2, sum ec ee} of the two envelopes over the tile's samples.
 *   n_tiles = 0 launches nothing.
 * sfm_ncm_finish: folds utterance b's tiles [tile_off[b], tile_off[b + 1]) in tile order; ncc [B, C] = cov / sqrt(var var) of the
 *   envelopes (0 where that root is below 1e-10), clipped to [-1, 1]; score [B] = clip(sum_c weights[c] max(ncc, 0), 0, 1); an
 *   utterance without a tile gets zeros. */
int sfm_csii_frames_varlen(const float* cr, const float* ci, const float* er, const float* ei, const int* frame_off,
                           const double* weights, double* score, double* msc, int B, int sum_frames, int F, void* stream);
int sfm_hilbert_env(const float* x, const float* table, float* env, int R, int L, void* stream);
int sfm_hilbert_env_moments(const float* X, const float* tables, const int* tab_off, const int* lengths, const int* tiles,
                            double* partial, int B, int C, int L, int n_tiles, void* stream);
int sfm_ncm_finish(const double* partial, const int* tile_off, const int* lengths, const double* weights, double* ncc, double* score,
                   int B, int C, void* stream);

/* SpeechEnhancementDNN (dnn.hip; models/dnn.py of the reference: [Linear, ReLU, Dropout] x 3, Linear, Sigmoid).
 * sfm_dnn_layer: out[M, N] = act(A[M, K] W[N, Kpad]^T + bias) on the 16-bit MFMA of `dtype`, fp32 accumulation.
 *   W [Npad, Kpad] 16-bit, zero padded, Kpad % 64 == 0, Npad % 64 == 0 (ops.pack_linear); bias fp32 [>= N] or NULL.
 *   a_mode 0 (rows16): A 16-bit rows, row stride lda (elements), lda % 8 == 0, zero padded to a multiple of 8 columns.
 *   a_mode 1 (rows32): A fp32 rows [M, K], any K and any lda >= K, converted while staged; read with 8-byte loads when A and lda
 *     allow it and 4-byte loads otherwise; nothing is read past column K of a row.
 *   a_mode 2 (context): A = raw [B, T, D] fp32 (8-byte aligned, D even and >= 8: read in pairs) with M = B T and K = D (2 ctx + 1); frames int32 [B] = live frames T_b per utterance
 *     (NULL: T; 0 is legal).  Row (b, n), column j D + c = raw[b, clamp(n - ctx + j, 0, T_b - 1), c]; with mean / stdv [K] (both or
 *     neither; K <= 4096): nan / inf -> 0, (f - mean) (1 / std), clip to +-10, in fp32.  Rows n >= T_b are zero rows; nothing is read for them.
 *     frames, mean and stdv are NULL in the other modes; lda is ignored in this one, T, D and ctx in the others.
 *   act 0 none, 1 ReLU, 2 sigmoid.  p_drop > 0 (act 1 only): the result is multiplied by keep(seed, m N + n) in {0, 1 / (1 - p)}
 *     after the ReLU, the keep function of sfm_gemm16_train.
 *   out_f32 0: 16-bit rows of `dtype`, row stride ldo >= N, columns N .. ldo written as zeros; 1: fp32 rows, row stride ldo.
 *   The same bits from run to run, and for a row alone or inside any M.
 * sfm_dnn_act_bwd: dz[M, ldz] 16-bit of `dtype` (ldz % 8 == 0, columns N .. ldz written as zeros) = dy * act'(.), dy fp32 (dy_f32 = 1)
 *   or 16-bit rows of stride ldy.  act 1: saved = the layer's 16-bit OUTPUT h, dz = dy (h > 0 ? 1 / (1 - p_drop) : 0) - h is positive
 *   exactly where the unit was active and kept; act 2: saved = the fp32 output y, dz = dy y (1 - y); act 0: dz = dy (saved unused). */
int sfm_dnn_layer(const void* A, const int* frames, const float* mean, const float* stdv, const void* W, const float* bias, void* out,
                  int a_mode, int M, int N, int K, long long lda, int T, int D, int ctx, int Kpad, int Npad, long long ldo, int out_f32,
                  int act, float p_drop, unsigned int seed, int dtype, void* stream);
int sfm_dnn_act_bwd(const void* dy, int dy_f32, long long ldy, const void* saved, long long ld_saved, void* dz, long long ldz, int M,
                    int N, int act, float p_drop, int dtype, void* stream);

/* Training the DNN from a frame set kept at D columns (training/pipeline.py of the reference: SpeechEnhancementDataset :217-289,
 * _train_epoch :643-685).  raw [n_frames, D] fp32 are the packed frames of all utterances, bounds int32 [n_frames, 2] (8-byte
 * aligned) the first and the one-past-last packed row of each frame's utterance.  No atomics, the same bits from run to run.
 * sfm_context_moments: mean, stdv fp32 [K], K = D (2 ctx + 1), of the context rows of all n_frames frames - column j D + c of
 *   frame n = raw[clamp(n - ctx + j, lo_n, hi_n - 1), c], nan / inf read as 0 - without forming them: the mean, then the
 *   population standard deviation from the squares centred on it, both summed in fp64 (one partial per chunk of rows and column,
 *   folded in chunk order), rounded to fp32; stdv < 1e-6 -> 1.  ws: (SFM_MOMENTS_MAX_CHUNKS + 1) K doubles.
 * sfm_dnn_layer_indexed: sfm_dnn_layer's context mode on an index list: row m of the operand is the context row of packed frame
 *   index[m] (int32 [M]; a repeated index is legal; < 0 or >= n_frames: a zero row), its neighbours clamped to bounds[index[m]];
 *   mean / stdv [K] (both or neither; K <= SFM_DNN_CONTEXT_MAX_K) as there.  D even and >= 8, K = D (2 ctx + 1).  a16_out (or
 *   NULL): [M, ld16] 16-bit of `dtype`, ld16 = K rounded up to 64, 16-byte aligned: the staged operand rows, columns K .. ld16
 *   zeros, written by the workgroups of column tile 0 - what sfm_gemm16_tn reads for the layer's weight gradient.  W, bias, out,
 *   ldo, out_f32, act, p_drop, seed as sfm_dnn_layer.  A row's result has the same bits alone or inside any M, and the bits of
 *   the context mode on the frame's utterance alone.
 * sfm_mse_gather_loss: y fp32 [M, C] compact, mask fp32 [n_frames, C] compact, t = clip(nan_to_num(mask[index[m], c], nan 0, +inf 1,
 *   -inf 0), 0, 1); loss[0] (or NULL) = mean (y - t)^2 over the M C elements (fp64 partials per workgroup, folded in order by a
 *   one-workgroup kernel).  dz (or NULL: validation): [M, ldz] 16-bit of `dtype`, ldz % 8 == 0, columns C .. ldz zeros,
 *   = S 2 (y - t) / (M C) y (1 - y), S = loss_scale[0] (device, NULL: 1): the output layer's pre-activation cotangent under the
 *   loss scale.  rec (or NULL) 4 doubles, the epoch's record: [0] += loss and [1] += 1 when the loss is finite, else [2] += 1;
 *   [3] = loss.  ctl (or NULL): the optimiser's control block, ctl[2] = 1 when the loss is not finite (the step is skipped).
 *   A row whose index is outside 0 .. n_frames - 1 adds nothing and gets a zero dz row.  ws: SFM_MSE_GATHER_MAX_BLOCKS doubles. */
int sfm_context_moments(const float* raw, const int* bounds, float* mean, float* stdv, double* ws, int n_frames, int D, int ctx,
                        void* stream);
int sfm_dnn_layer_indexed(const float* raw, const int* bounds, const int* index, const float* mean, const float* stdv, const void* W,
                          const float* bias, void* out, void* a16_out, int M, int N, int K, int n_frames, int D, int ctx, int Kpad,
                          int Npad, long long ldo, long long ld16, int out_f32, int act, float p_drop, unsigned int seed, int dtype,
                          void* stream);
int sfm_mse_gather_loss(const float* y, const float* mask, const int* index, const float* loss_scale, void* dz, long long ldz,
                        float* loss, double* rec, double* ctl, double* ws, int M, int C, int n_frames, int dtype, void* stream);

/* Mask to waveform (resynth.hip; steps 2-4 of TrainingPipeline.enhance_signal, training/pipeline.py:877-934 of the reference) in one
 * launch, exact fp32 on v_mfma_f32_32x32x2_f32, no atomics.  noisy, out [B, L] fp32; mask [B, T_mask, C] fp32; lengths int32 [B] = the
 * sample counts L_b of the zero-padded batch, or NULL (= L).  Per utterance: T_b = (L_b - frame) / hop + 1 (0 below one frame), the
 * frames n < N_b = min(T_b, T_mask) are windowed, transformed (rfft(., n_fft)), multiplied per bin by the mask row interpolated onto
 * the bins, transformed back, cropped to `frame`, windowed and overlap-added; every sample is divided by the sum of the squared
 * window over the frames that cover it.  Every element of out is written: 0 where no frame n < N_b covers it.  Mask rows from N_b on
 * and samples from L_b on are not read.  The same bits from run to run and for an utterance alone or anywhere in a batch.
 * Host-built operands, NC = n_fft and FR = frame rounded up to SFM_RESYNTH_COL_ALIGN, F = n_fft / 2 + 1:
 *   Wf [FR, NC]: column j < F = w[n] cos(2 pi (n j mod n_fft) / n_fft), column F + k - 1 = -w[n] sin(..k..), 1 <= k <= F - 2 (the
 *     imaginary parts of DC and Nyquist are identically zero and have no column); zero beyond row `frame` and column n_fft.
 *   Wi [NC, FR]: the matching rows of irfft (coefficients 1, 2, .., 2, 1 over n_fft), columns n < frame, times w[n]; zero beyond.
 *   tab_idx int32 [NC], tab_wt [NC]: gain of column c = (1 - wt) mask[.., idx] + wt mask[.., idx + 1], 0 <= idx <= C - 2.
 *   inv_wsum [3, hop]: 1 / window sum of the utterance's first hop, of an interior hop, of its last covered hop (a sum below 1e-8
 *     counts as 1).
 * hop * 2 == frame, frame <= n_fft <= SFM_RESYNTH_MAX_NFFT, n_fft even, 2 <= C <= SFM_RESYNTH_MAX_CHANNELS, T_mask >= 1
 * (SFM_ERR_SHAPE otherwise). */
int sfm_mask_resynth(const float* noisy, const float* mask, const int* lengths, const float* Wf, const float* Wi, const int* tab_idx,
                     const float* tab_wt, const float* inv_wsum, float* out, int B, int L, int T_mask, int frame, int hop, int n_fft,
                     int C, void* stream);

/* The adjoint of sfm_mask_resynth with respect to the mask (resynth.hip), one launch, exact fp32 on v_mfma_f32_32x32x2_f32, no
 * atomics.  The forward is linear in the mask, so the mask itself is no operand.  noisy [B, L] fp32 and lengths as there; dout
 * [B, L] fp32 = the cotangent of out; dmask [B, T_mask, C] fp32, every element written: with N_b = min(T_b, T_mask),
 *   dy_n[j] = dout[n hop + j] * inv_wsum[row of hop n + (j >= hop)][j mod hop]  (row 0 for the utterance's hop 0, 2 for hop N_b, else 1),
 *   P_n = (frame_n(noisy) Wf) * (dy_n WiT) element by element, dg_n[k] = P_n[k] + P_n[F + k - 1] (the second for 1 <= k <= F - 2),
 *   dmask[b, n, c] = sum over the bins of channel c - 1 of tab_wt[k] dg_n[k] + sum over the bins of channel c of (1 - tab_wt[k])
 *   dg_n[k], each in ascending k, for n < N_b; rows n >= N_b are 0.
 * Samples of noisy from L_b on and of dout from min(L_b, (N_b + 1) hop) on are not read (they have no influence on the forward).
 * No gradient to noisy is offered.  The same bits from run to run and for an utterance alone or anywhere in a batch.
 * Host-built operands, NC, FR, F as above:
 *   Wf [FR, NC], tab_wt [NC] (its first F words, one per bin, are read), inv_wsum [3, hop]: those of sfm_mask_resynth.
 *   WiT [FR, NC]: Wi transposed, row n < frame = the irfft coefficients of sample n times w[n] per spectrum column; zero beyond row
 *     `frame` and column n_fft.
 *   chan_bins int32 [C + 1]: the bins k with tab_idx[k] == c are chan_bins[c] .. chan_bins[c + 1] - 1 (tab_idx ascends with k), so
 *     chan_bins[0] = 0 and chan_bins[C - 1] = chan_bins[C] = F; a channel that brackets no bin has an empty range.
 * Shapes as sfm_mask_resynth (SFM_ERR_SHAPE otherwise). */
int sfm_mask_resynth_bwd(const float* noisy, const float* dout, const int* lengths, const float* Wf, const float* WiT,
                         const float* tab_wt, const float* inv_wsum, const int* chan_bins, float* dmask, int B, int L, int T_mask,
                         int frame, int hop, int n_fft, int C, void* stream);

/* RBM pre-training (rbm.hip; models/rbm.py of the reference: CD-k).  Everything fp32 on the device, every product exact fp32 on
 * v_mfma_f32_32x32x2_f32; W [n_visible, n_hidden] row-major as there.  No atomics: the same bits from run to run.
 * sfm_rbm_prob: prob[M, N] = sigmoid(A[M, K] op(W) + bias[N]), sigmoid(x) = 1 / (1 + exp(-x)) (0 and 1 at the extremes, never NaN).
 *   down 0: K = n_visible, N = n_hidden, op(W) = W, bias = h_bias;  down 1: K = n_hidden, N = n_visible, op(W) = W^T, bias = v_bias.
 *   Row m of A = data[rows[m]] (rows int32 [M]; NULL: row m itself), data [n_rows, lda] fp32 with lda >= K and 4-byte aligned rows;
 *   an index outside 0 .. n_rows - 1 reads as a row of zeros.  prob [M, N] compact.  A row's result has the same bits alone or
 *   inside any M, and through `rows` or from a gathered copy.
 *   sample_mode SFM_RBM_SAMPLE_NONE: sample and u NULL.
 *   SFM_RBM_SAMPLE_REPLAY: sample[M, N] fp32 = ((double)prob > u[m N + n]) ? 1 : 0, u fp64 [M, N] (np.random.random of the reference).
 *   SFM_RBM_SAMPLE_COUNTER: u NULL; sample[m, n] = 1 iff word(seed, m N + n) < ceil(prob * 2^24), else 0, where for the element
 *     index e (64-bit) word is the 24-bit number that the dropout keep function sfm_keep_scale(seed, e, .) compares with its
 *     threshold: g = hash(seed, e >> 3) (the full counter hash of the 8-element group), x = g + (e & 7) * 0x9E3779B1,
 *     x ^= x >> 15, x *= 0x846CA68B, x ^= x >> 16, word = x >> 8 (32-bit arithmetic); ceil(prob * 2^24) is formed in fp32 (exact).
 * sfm_rbm_update: W[i, j] += (lr / B) sum_b (v[b, i] ph[b, j] - nv[b, i] nh[b, j]) as one accumulation over 2 B terms (term 2 b
 *   positive, 2 b + 1 negative), in place, every element read and written once; v_bias[i] += lr mean_b(v - nv), h_bias[j] += lr
 *   mean_b(ph - nh) (column sums in fp64); err_partial[t], t < ceil(n_visible / SFM_RBM_TILE), = sum over b and the tile's 32
 *   visible units of (v - nv)^2 in fp64.  v[b] = data[rows[b]] as above; ph, nh [B, n_hidden], nv [B, n_visible] compact.
 *   B = the rows of THIS batch (1 .. SFM_RBM_MAX_BATCH): the last batch of an epoch is shorter.
 * sfm_rbm_fold_error: partial [n_steps, n_tiles] of the batches of one epoch over num_samples rows (batch s has
 *   min(batch_size, num_samples - s batch_size) rows; n_steps = ceil(num_samples / batch_size), n_tiles = ceil(n_visible / SFM_RBM_TILE),
 *   SFM_ERR_SHAPE otherwise) -> out[0] = mean over s of (sum_t partial[s, t]) / (rows_s n_visible), summed in a fixed order. */
int sfm_rbm_prob(const float* data, const int* rows, const float* W, const float* bias, float* prob, float* sample, const double* u,
                 int M, int n_visible, int n_hidden, int n_rows, long long lda, int down, int sample_mode, unsigned int seed,
                 void* stream);
int sfm_rbm_update(const float* data, const int* rows, const float* ph, const float* nv, const float* nh, float* W, float* v_bias,
                   float* h_bias, double* err_partial, int B, int n_visible, int n_hidden, int n_rows, long long ldv, float lr,
                   void* stream);
int sfm_rbm_fold_error(const double* partial, double* out, int n_steps, int n_tiles, int num_samples, int batch_size, int n_visible,
                       void* stream);

/* STOI of Taal et al. (2011) and ESTOI of Jensen & Taal (2016) (stoi.hip): what evaluation/stoi.py:46-50 of the reference computes
 * when pystoi is installed.  wave64, no atomics, every cross-thread sum in fp64 in a fixed order: an utterance has the same bits
 * alone, in a batch and in any packed set.  Nothing waits for the device: an utterance's kept-frame count stays there, and every
 * table is sized for all frames kept.  The kernels behind the resampler work at SFM_STOI_FS.  Utterance u = samples
 * [sig_off[u], sig_off[u] + sig_len[u]) of sig; it owns the
 * n_u = (sig_len[u] - SFM_STOI_FRAME) / SFM_STOI_HOP + 1 (0 below one frame) rows [frame_off[u], frame_off[u + 1]) of energy, src
 * and the band rows; sig_off, sig_len int32 [B], frame_off int32 [B + 1], all on the device.  win fp32 [SFM_STOI_FRAME] =
 * hanning(SFM_STOI_FRAME + 2)[1:-1]. */
#define SFM_STOI_FS 10000
#define SFM_STOI_FRAME 256
#define SFM_STOI_HOP 128
#define SFM_STOI_NFFT 512
#define SFM_STOI_BANDS 15
#define SFM_STOI_SEG 30
#define SFM_STOI_FIRST_BIN 7
#define SFM_STOI_LAST_BIN 218
#define SFM_STOI_DFT_COLS 432
#define SFM_STOI_ROW_TILE 16
#define SFM_STOI_SEG_TILE 32
#define SFM_STOI_TAP_HALF 10
#define SFM_STOI_MAX_RATE 8
/* evaluation/stoi.py:46-50, step 0 (rate): the polyphase FIR resampler.  Utterance u of `in` = samples [in_off[u], in_off[u] + in_len[u]),
 * of `out` = [out_off[u], out_off[u] + out_len[u]), out_len[u] = ceil(in_len[u] up / down) (the host's figure; all four int32 [B] on the
 * device).  out[n = t up + p] = sum_k in[t down + k - padl] taps[k up + p], zeros beyond both ends of the utterance, taps fp32 [K, up]:
 * fp32 operands, the sum an fma chain in fp64 in k order, stored as fp32.  max_out_len = the largest out_len (0 launches nothing).
 * 1 <= up, down <= SFM_STOI_MAX_RATE, 1 <= K <= 2 SFM_STOI_TAP_HALF SFM_STOI_MAX_RATE + 1, 0 <= padl < K, B <= 65535
 * (SFM_ERR_SHAPE otherwise). */
int sfm_stoi_resample(const float* in, const float* taps, const int* in_off, const int* in_len, const int* out_off, const int* out_len,
                      float* out, int B, int max_out_len, int up, int down, int K, int padl, void* stream);
/* evaluation/stoi.py:46-50, step 1 (silent frames) on the CLEAN signal: energy[f] = 20 log10(||win x_f|| + eps) in fp64, eps = 2^-52;
 * frame f is kept when energy[f] > max_f energy[f] - 40; src[frame_off[u] + k] = the k-th kept frame of utterance u in order,
 * kept[u] = their count K_u (0 without a frame).  One workgroup per utterance: energies, maximum, mask, exclusive scan. */
int sfm_stoi_keep(const float* sig, const float* win, const int* sig_off, const int* sig_len, const int* frame_off, double* energy,
                  int* src, int* kept, int B, void* stream);
/* evaluation/stoi.py:46-50, steps 1 (overlap-add of the kept windowed frames), 2 (spectra) and 3 (bands) of nsig = 1 or 2 signals that
 * share the kept list: spectral frame m < K_u - 1 of utterance u is rebuilt from the source frames src[m - 1], src[m], src[m + 1]
 * (each half = two windowed source half-frames), windowed again (fp64) and multiplied on v_mfma_f64_16x16x4_f64 (fp64 sums) by dft
 * [SFM_STOI_FRAME, SFM_STOI_DFT_COLS] fp32: column c < 212 = cos(2 pi n (c + SFM_STOI_FIRST_BIN) / SFM_STOI_NFFT), column 212 + c the
 * negated sine, zero beyond 424 (fp32 values).  bands0 / bands1 [frame_off[B], SFM_STOI_BANDS] fp32: row frame_off[u] + m, band j = sqrt(sum of
 * |X|^2 over the bins [lo_j, hi_j)) of edges 7 9 11 14 17 22 27 34 43 55 69 87 109 138 174 219, summed in fp64 in bin order; rows from
 * K_u - 1 on are not written.  tiles int32 [n_tiles, 2] = (utterance, tile of SFM_STOI_ROW_TILE spectral frames), ceil((n_u - 1) /
 * SFM_STOI_ROW_TILE) per utterance; a tile beyond K_u - 1 does nothing.  sig1 / bands1 NULL when nsig = 1.  n_tiles = 0 launches
 * nothing, and tiles may then be NULL (no utterance has two frames: every score is 1e-5). */
int sfm_stoi_bands(const float* sig0, const float* sig1, const float* win, const float* dft, const int* sig_off, const int* frame_off,
                   const int* src, const int* kept, const int* tiles, float* bands0, float* bands1, int n_tiles, int nsig,
                   void* stream);
/* evaluation/stoi.py:46-50, steps 4 (too few frames) and 5 (segments): score[u] fp64 from the band rows xb (clean) and yb of
 * sfm_stoi_bands; M = K_u - 1 < SFM_STOI_SEG gives 1e-5.  Segment m = SFM_STOI_SEG .. M is the block of rows m - 30 .. m - 1, all in
 * fp64.  extended 0: per band alpha = ||x|| / (||y|| + eps), y' = min(alpha y, x (1 + 10^(15/20))), the correlation of the
 * mean-removed rows, averaged over bands and segments.  extended 1: rows, then columns, mean-removed and divided by (norm + eps); the
 * sum of x y over the block / 30, averaged over segments.  One workgroup per utterance; the rows go through a ring in LDS, each read
 * once, SFM_STOI_SEG_TILE segments per stage, the segment values added in segment order.  No row from K_u - 1 on is read. */
int sfm_stoi_segments(const float* xb, const float* yb, const int* frame_off, const int* kept, double* score, int B, int extended,
                      void* stream);
/* The measure as the fitness of the OPT-PCIRM search (masks/opt_pcirm.py:146-183 with evaluation/stoi.py:46-50; stoi.hip).  The
 * candidate x gives the enhanced signal ya + x yb (sfm_pso_split); the resampler, the kept list (the clean signal's), the
 * overlap-add and the windowed DFT are linear in it, so spectral frame m is A_m + x B_m and the energy of band j is
 *   E(x) = P + 2 x Q + x^2 R,  P = sum_k |A_k|^2,  Q = sum_k Re(A_k conj B_k),  R = sum_k |B_k|^2  over the band's bins.
 * sfm_stoi_bands_pair: sfm_stoi_bands' grid, tile and operands for siga = ya and sigb = yb at SFM_STOI_FS -> planes fp64
 *   [frame_off[B], SFM_STOI_PLANES, SFM_STOI_BANDS]: row frame_off[u] + m holds P | Q | R of spectral frame m; rows from K_u - 1 on
 *   are not written.  The products a a, a b, b b are formed from the fp64 accumulators (Q never by a difference of band rows).
 *   Dynamic LDS (two A tiles, 65792 B), granted by the launcher.  n_tiles = 0 launches nothing, tiles may then be NULL.
 * sfm_pso_fitness_taal: fitness [B, N] fp64 = sfm_stoi_segments' score of the clean rows xb (sfm_stoi_bands, fp32) against the rows
 *   sqrt(max(E(x), 0)) in fp64 at x = pos[u, p] rounded to fp32 (the mask array holds the middle value so), formed while the ring is
 *   filled; 1e-5 where K_u - 1 < SFM_STOI_SEG.  One workgroup per (particle, utterance), the segment arithmetic is the one function
 *   sfm_stoi_segments runs.  A swarm whose stopped[u] is set is skipped (its row of fitness is left as it is).
 *   B <= 65535, 1 <= N <= SFM_PSO_MAX_PARTICLES, extended 0 / 1 as sfm_stoi_segments. */
#define SFM_STOI_PLANES 3
int sfm_stoi_bands_pair(const float* siga, const float* sigb, const float* win, const float* dft, const int* sig_off,
                        const int* frame_off, const int* src, const int* kept, const int* tiles, double* planes, int n_tiles,
                        void* stream);
int sfm_pso_fitness_taal(const float* xb, const double* planes, const int* frame_off, const int* kept, const double* pos,
                         const int* stopped, double* fitness, int B, int N, int extended, void* stream);
/* The gradient of the measure with respect to the ENHANCED signal (stoi_bwd.hip), three kernels that walk the forward back; the
 * kept list and K_u belong to the clean signal and are constants, so the gradient is exact.  A norm at the zero vector and a band
 * value of exactly 0 pass nothing back.  fp32 operands and stored results, every sum fp64 in a fixed order, no atomics.
 * Step 5 back: dyb [frame_off[B], SFM_STOI_BANDS] fp32 = gscore[u] (fp64 [B], the cotangent of score[u]) times the derivative of
 * score[u] by the band rows yb, from the same stored rows the forward read (so a clip decision is the forward's: an element with
 * alpha y > x (1 + 10^(15/20)) passes nothing, neither directly nor through alpha).  A row lies in up to SFM_STOI_SEG segments; its
 * cotangent is their sum in segment order, kept in LDS until the last of them has passed, then written once.  EVERY row of
 * [frame_off[u], frame_off[u + 1]) is written: zeros from K_u - 1 on and for an utterance below SFM_STOI_SEG spectral frames.
 * One workgroup per SFM_STOI_BWD_ROWS rows of an utterance: it walks every segment that holds one of its rows (the up to
 * SFM_STOI_SEG - 1 that reach in from the rows below included) and adds to its own rows only, so no sum crosses a workgroup and
 * the bits do not depend on the split.  max_rows: the largest frame_off[u + 1] - frame_off[u] (the host's figure; 0 launches
 * nothing). */
#define SFM_STOI_BWD_ROWS 32
int sfm_stoi_segments_bwd(const float* xb, const float* yb, const int* frame_off, const int* kept, const double* gscore, float* dyb,
                          int B, int max_rows, int extended, void* stream);
/* Steps 3 and 2 back, per tile of SFM_STOI_ROW_TILE spectral frames of sig (the resampled enhanced signal): the windowed rebuilt
 * frames and their Re | Im exactly as sfm_stoi_bands forms them, each bin scaled by dyb / band of its band (band = sqrt(sum |X|^2),
 * 0 where that is 0), the scaled tile multiplied on the same matrix instruction by dft_t [SFM_STOI_DFT_COLS, SFM_STOI_FRAME] fp32 (the
 * transpose of dft), times the window: dframes [frame_off[B], SFM_STOI_FRAME] fp32, row frame_off[u] + m = the cotangent of the
 * rebuilt signal's samples [128 m, 128 m + 256) through spectral frame m.  Rows of utterances with K_u - 1 >= SFM_STOI_SEG only, and
 * of those the rows below K_u - 1; no other row is written or read by sfm_stoi_fold_bwd.  n_tiles = 0 launches nothing. */
int sfm_stoi_bands_bwd(const float* sig, const float* win, const float* dft, const float* dft_t, const int* sig_off,
                       const int* frame_off, const int* src, const int* kept, const int* tiles, const float* dyb, float* dframes,
                       int n_tiles, void* stream);
/* Step 1 back, the overlap-add adjoint as a gather: dsig[sig_off[u] + s], s < sig_len[u], = sum over the at most two kept source
 * frames src[k] that cover sample s (found by a search in the ascending list) of win times the at most two dframes terms of the
 * rebuilt sample 128 k + s - 128 src[k], in ascending frame order.  Every sample is written once: 0 where no kept frame covers it,
 * where only the last kept frame's second half does, and for an utterance below SFM_STOI_SEG spectral frames; samples
 * sig_len[u] <= s < pad_to are written as 0 as well (pad_to = the row length of a zero-padded batch at SFM_STOI_FS, else 0).
 * max_len = the largest of sig_len and pad_to (0 launches nothing), B <= 65535. */
int sfm_stoi_fold_bwd(const float* dframes, const float* win, const int* sig_off, const int* sig_len, const int* frame_off,
                      const int* src, const int* kept, float* dsig, int B, int max_len, int pad_to, void* stream);

#ifdef __cplusplus
}
#endif
#endif
