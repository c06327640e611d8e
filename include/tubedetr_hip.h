/* C ABI of libtubedetr_hip.so - the MI355X (gfx950) kernels behind the TubeDETR hot path.
 *
 * The reference (antoyang/TubeDETR) is pure Python: its hot path has no FFI of its own, it calls
 * torch / torchvision operators from nn.Modules.  Each entry below therefore names the reference
 * call site (file:line under the reference tree) whose arithmetic it replaces; the Python modules
 * in tubedetr_amd/models keep the reference's nn.Module surface and bind these symbols with ctypes
 * (tubedetr_amd/_hip.py; the stub a reference maintainer would add is in INTEGRATION.md).
 *
 * Conventions: raw device pointers borrowed for the call (never retained, never freed); caller
 * allocates outputs and workspaces; no hidden allocation, no synchronisation, every launch goes to
 * the `stream` argument (a hipStream_t passed as void*); re-entrant, callable from any thread
 * (autograd workers).  Return 0 or a negative TD_ERR_* code; td_last_error() gives a thread-local
 * message.  dtype: TD_F32 (exact fp32 MFMA, parity mode) or TD_BF16 (bf16 MFMA, fp32 accumulate).
 * Activations are NHWC / row-major [rows][channels]; "T" below = the dtype's element type.
 */
#ifndef TUBEDETR_HIP_H
#define TUBEDETR_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define TD_F32 0
#define TD_BF16 1
#define TD_U8 2 /* input pixels only (td_frame_source) */
#define TD_OK 0
#define TD_ERR_INVALID (-1)
#define TD_ERR_LAUNCH (-2)

typedef void* td_stream_t; /* hipStream_t */

const char* td_last_error(void);
int td_abi_version(void);

/* Deterministic parity mode: 1 = every reduction that is normally split over workgroups and combined with fp32 atomics (weight gradients,
 * LayerNorm dgamma / dbeta, bias column sums) runs as one sequential reduction per output element: two runs of a step are bit-identical.
 * Process-wide atomic flag, seeded once from TD_DETERMINISTIC=1 in the environment, read at LAUNCH time: grid and split choices are frozen
 * into a captured HIP graph, so a graph captured under the other setting must be re-captured. */
int td_set_deterministic(int on);
int td_get_deterministic(void);

/* Dropout RNG: counter-based, keep(seed, element index) = hash32(element index * golden + seed) >= p * 2^32.  Every
 * dropout-capable entry point takes an optional `dropout_counter`: a DEVICE pointer to one uint32 step counter.  When
 * non-NULL the kernels re-key the seed with a hash of (seed, *dropout_counter), read at execution time - a captured HIP
 * graph then draws fresh, statistically independent masks on each replay (the caller increments the counter between
 * replays); forward and backward of one step must see the same counter value.  NULL = the seed is used as passed.
 * There is no process-global dropout state. */

/* Optional per-kernel-family timing with HIP events recorded on the launch stream around every MFMA kernel
 * launch (bench.py's roofline leg).  td_prof_enable(1) starts collecting (records are kept under a mutex; off by
 * default and then one relaxed atomic load per launch), td_prof_collect synchronises the recorded events and returns, per family (TD_PROF_*), the number of
 * launches, the summed duration in ms and the summed ALGORITHMIC flops (2*M*N*K of the un-padded problem). */
#define TD_PROF_GEMM_128x128 0
#define TD_PROF_GEMM_128x64 1
#define TD_PROF_WGRAD 2
#define TD_PROF_GEMM_64x128 3
#define TD_PROF_PW_RESIDENT 4 /* persistent weight-stationary pointwise instance */
#define TD_PROF_GEMM_256 5    /* 256-row tiles, eight wavefronts (conv_gemm_big_kernel), spatial (3x3) layers: the MFMA-bound members */
#define TD_PROF_GEMM_256_PW 6 /* the same kernel on pointwise layers with K >= 512: HBM-bound (4.2 TB/s of algorithmic bytes) */
#define TD_PROF_FUSED 7       /* LDS-resident chains: fused stem (stem.hip), fused frozen bottlenecks (bottleneck.hip) */
#define TD_PROF_CROSS_Q1 8    /* time-aligned cross-attention frame core (cross_attn.hip): HBM-bound by the memory rows */
#define TD_PROF_WGRAD_SINGLE 9 /* one weight gradient per launch (td_conv_wgrad[_bias]); TD_PROF_WGRAD = the batched launches */
#define TD_PROF_CHAIN 10 /* chained conv3 -> next-block conv1 pairs of layer3 (chain.hip): HBM-bound, the block output never read back */
#define TD_PROF_FAMILIES 11
int td_prof_enable(int on);
int td_prof_collect(int family, int dtype, long long* launches, double* ms, double* flops);
/* Sum of the ALGORITHMIC HBM bytes of the same launches (each operand / result tensor counted once per launch). */
int td_prof_collect_bytes(int family, int dtype, double* bytes);
/* CSV (family,dtype,M,N,K,R,stride,mode|splits,ms) of every recorded launch since td_prof_enable(1). */
int td_prof_dump(const char* path);
/* Debug: when non-NULL, td_conv_gemm workgroups launched by THIS thread write 6 cycle stamps each into
 * buf[workgroup*8 + i] (thread-local setting). */
int td_debug_set_stamp_buffer(unsigned long long* buf);

/* Geometry of one implicit-GEMM convolution / linear layer.  rows m enumerate (n, ho, wo);
 * k enumerates (r, s, c) with c fastest; the gathered source is NHWC [N][Hs][Ws][C].
 * mode 0 (forward):  hs = ho*stride - pad + r
 * mode 1 (dgrad):    hs = (ho + pad - r) / stride when divisible (source = grad of conv output)
 * A linear layer is R=S=1, stride=1, pad=0, Hs=Ho, Ws=Wo.                                        */
typedef struct td_conv_desc {
  int N, Hs, Ws, C;
  int Ho, Wo;
  int R, S, stride, pad;
  int mode;
  int Nc;     /* output channels = rows of the weight matrix [Nc][R*S*C] */
  int ldc;    /* leading dimension (elements) of the output / residual / mask rows */
  int out_sp; /* 1 = dense rows; >1 = row (n,ho,wo) is written at (n, ho*out_sp, wo*out_sp) of an */
  int out_H, out_W; /*        [N][out_H][out_W][ldc] tensor (strided 1x1 dgrad scatter)           */
  int aniso;            /* 1: `stride` / `pad` describe the vertical direction only, the horizontal one uses the two fields  */
  int stride_w, pad_w;  /*    below (forward geometry only).  The pixel-pair form of the stem: a 7x7 stride-2 convolution of */
                        /*    3-channel pixels = a 7x4 convolution, stride (2,1), pad (3,2), of 8-channel pixel PAIRS        */
} td_conv_desc;

/* Fused epilogue: v = acc (+ bias[n]) (+ residual[m][n]); relu; sigmoid; mask (v if mask_src>0 else 0);
 * dropout (inverted, counter-based hash RNG on element index). */
typedef struct td_epilogue {
  const float* bias;
  const void* residual;
  const void* mask_src;
  int relu;
  int sigmoid;
  float dropout_p;
  uint32_t dropout_seed;
  float alpha; /* scales acc before bias; 0 is treated as 1 */
  const uint32_t* dropout_counter; /* optional device step counter (see "Dropout RNG" above) */
} td_epilogue;

/* out[m][n] = epilogue(sum_k gather(src)[m][k] * wmat[n][k]).
 * Replaces: torch Conv2d/Linear forward + FrozenBatchNorm2d + ReLU + residual
 * (models/backbone.py:60-70,97-98; torchvision resnet Bottleneck; models/transformer.py:643,748,
 * 769; models/tubedetr.py:39,80) and, in mode 1 / with transposed weights, their input gradients. */
int td_conv_gemm(const void* src, const void* wmat, void* out, const td_conv_desc* d, const td_epilogue* e,
                 int dtype, td_stream_t stream);

/* Linear layer whose input rows are formed on the fly:
 *   out[out_map[m]][n] = epilogue( sum_k X[m][k] * wmat[n][k] (+ residual[res_map[m]][n]) ),   X[m] = [ A1[a1_map[m]] | A2[a2_map[m]] ]
 * (K1 columns from A1, K2 from A2; every map is a device int32[M] or NULL = identity; res_map NULL = the output row).
 * With a shared weight (w_shared) the product is (A1 + A2) W^T: "src + pos" enters the Q / K projections as a second operand stream
 * instead of a materialised sum (with_pos_embed + in_proj of nn.MultiheadAttention, models/transformer.py:637-640,
 * 735-737), and the temporal replication of the clip memory to its frames (models/transformer.py:393-427) becomes a row
 * index inside its consumers: the slow-fast aggregation (:441-445) reads the clip rows through a1_map / res_map and writes
 * the frame rows through out_map.  a2 may be NULL (one source).  K1 must be a multiple of the K tile (64 bf16 / 32 fp32
 * elements) when a2 is given; lda / ldc / ldr are row strides in elements (ldr <= 0: ldc). */
typedef struct td_linear_ex_desc {
  int M, N, K1, K2;
  int lda1, lda2, ldc, ldr;
  int w_shared;           /* 1: wmat is [N][K1] and multiplies both sources (K2 == K1): out = (A1 + A2) W^T, no [W | W] copy; 0: wmat is [N][K1 + K2] */
  long long rows1, rows2; /* rows held by the A1 / A2 buffers (bounds of the gather) */
  const int* a1_map;
  const int* a2_map;
  const int* out_map;
  const int* res_map;
} td_linear_ex_desc;
int td_linear_ex(const void* a1, const void* a2, const void* wmat, void* out, const td_linear_ex_desc* x, const td_epilogue* e,
                 int dtype, td_stream_t stream);

/* dw[n][k] += sum_m g[m][n] * gather(src)[m][k]   (fp32 atomics, `splits` partitions of m).
 * Replaces: autograd weight gradients of Conv2d / Linear on the same call sites. */
int td_conv_wgrad(const void* g, const void* src, float* dw, const td_conv_desc* d, int ldg, int dtype, int splits,
                  td_stream_t stream);
/* Same, and dbias[n] += sum_m g[m][n] (the bias gradient of a Linear / Conv2d with bias, models/transformer.py:643,748,769)
 * from the gradient fragments the kernel already holds; dbias (fp32, zero-initialised by the caller) may be NULL. */
int td_conv_wgrad_bias(const void* g, const void* src, float* dw, float* dbias, const td_conv_desc* d, int ldg, int dtype,
                       int splits, td_stream_t stream);

/* Batched weight gradients: ONE call computes the weight gradients of many conv layers, in up to three launches per phase -
 * one per kernel its jobs need (general geometry, pointwise, wide tiles) - and two phases (the overwriting jobs, then the
 * `accumulate` jobs); td_conv_wgrad_batch_plan below returns the layout.  dW of every job is written in the parameter's own [Nc][ci_real][R][S] fp32 layout with `scale[co]`
 * (the FrozenBN factor, may be NULL) folded in - overwritten, not accumulated.  With thousands of output tiles in flight
 * a job needs no reduction splits (no atomics, no accumulator memset, no finalize pass) unless its M is very long.
 * A linear layer is a job with R=S=1 (dW = the parameter's [out][in]); its bias gradient rides along (`dbias`).  The
 * transformer's ~94 weight gradients of one step are deferred to the end of backward and run as ONE such launch.
 * `jobs` is a host array, consumed before the call returns.  The per-launch job table lives in caller-provided
 * memory of td_conv_wgrad_batch_table_bytes(n_jobs) bytes each: `table_host` (page-locked host memory, written by this
 * call) and `table_dev` (device memory, filled by ONE hipMemcpyAsync on `stream`).  Both must stay untouched until the
 * stream has passed this call - for a captured stream, for the lifetime of the graph (the copy node re-reads
 * table_host at every replay).  No allocation, no synchronisation inside.
 * Replaces the same autograd call sites as td_conv_wgrad,
 * for all convs of the trunk at once (torchvision resnet Bottleneck backward, models/backbone.py:94-98). */
typedef struct td_wgrad_job {
  const void* g;      /* [M][ldg] output gradient rows */
  const void* src;    /* the layer's input activation (NHWC) */
  float* dW;          /* [Nc][ci_real][R][S] fp32 */
  const float* scale; /* [Nc] or NULL */
  td_conv_desc d;     /* forward geometry (mode 0) */
  int ldg;
  int ci_real;        /* input channels of the parameter (d.C may be padded) */
  float* dbias;       /* optional [Nc] fp32: column sums of g (bias gradient of a Linear / Conv2d with bias), overwritten */
  int accumulate;     /* 1: dW += (instead of =), run behind the overwriting jobs of the same call: the second operand stream of a
                       * two-source layer (td_linear_ex: dW = g^T A1 + g^T A2, the positional operand of the Q / K projections); no dbias */
  int prezeroed;      /* 1: the caller zero-filled dW (and dbias) already - e.g. ONE fill over a flat buffer that holds the dW of all
                       * jobs: the library then enqueues no per-job fill for jobs it splits along M (fp32 atomics into dW) */
} td_wgrad_job;
size_t td_conv_wgrad_batch_table_bytes(int n_jobs);
int td_conv_wgrad_batch(const td_wgrad_job* jobs, int n_jobs, int dtype, void* table_host, void* table_dev, size_t table_bytes,
                        td_stream_t stream);

/* Input frames of the trunk: one or more sources of NCHW frames - fp32 (the reference's normalised samples.tensors /
 * samples_fast.tensors, engine.py:55-57) or uint8 pixels (normalised here: (x/255 - mean[c]) * inv_std[c], the
 * datasets' T.Normalize done on the device, so the host sends a quarter of the bytes) - concatenated in order into one
 * NHWC T tensor with channels zero-padded to Cpad (8 or 4 for bf16, 4 for fp32).  `index` (device int32[n], may be NULL) picks the
 * source frame of every contributed frame: the slow clip is video[::k] of the SAME buffer as the fast frames
 * (datasets/vidstg.py:250-251) - no second copy of the pixels, no concatenation.  mean / inv_std: host arrays of C floats
 * or NULL (no normalisation). */
typedef struct td_frame_source {
  const void* data; /* [n_src][C][H][W] */
  int dtype;        /* TD_F32 or TD_U8 */
  int n;            /* frames contributed */
  const int* index; /* device int32[n] or NULL (= 0..n-1) */
  const int* valid_hw; /* device int32[n_src][2] = (rows, columns) of every SOURCE frame that hold pixels, or NULL (= H x W): a
                        * ragged batch padded to a common H x W; pixels outside are written as exactly 0 (after normalisation), like
                        * NestedTensor.from_tensor_list pads the normalised frames, util/misc.py:158-170 */
} td_frame_source;
int td_frames_to_nhwc(const td_frame_source* srcs, int n_srcs, int C, int H, int W, int Cpad, const float* mean,
                      const float* inv_std, void* y, int dtype, td_stream_t stream);

/* Native executor of the bottleneck-ResNet trunk (replaces the module-graph execution of torchvision resnet101 through
 * IntermediateLayerGetter, models/backbone.py:94-98, and its autograd backward).  Conv order in every array: stem,
 * then per block conv1, conv2, conv3[, downsample] (td_resnet_num_convs entries).  srcs: the N = sum of srcs[i].n input
 * frames (td_frames_to_nhwc: fp32 or uint8 + normalisation, optional frame index lists);
 * w_fwd/bias: prepared (FrozenBN-folded) weights of td_weight_prep; ws: caller-allocated workspace.  save=1 keeps every
 * activation for td_resnet_bwd; save=0 (the no_grad "fast" pass, models/tubedetr.py:128-129) runs in a 6-slot ring.
 * *feat points into ws: layer4 output NHWC [N][feat_hw[0]][feat_hw[1]][feat_hw[2]]. */
size_t td_resnet_fwd_ws_bytes(int N, int H, int W, const int* nblocks, int dtype, int save);
int td_resnet_num_convs(const int* nblocks);
int td_resnet_fwd(const td_frame_source* srcs, int n_srcs, const float* mean, const float* inv_std, int N, int H, int W,
                  const int* nblocks, const void* const* w_fwd, const float* const* bias, int save, void* ws, size_t ws_bytes,
                  void** feat, int* feat_hw, int stem_pairs, int first_train_stage, int dtype, td_stream_t stream);
/* first_train_stage (0..4, as for td_resnet_bwd): the stages below it are frozen - td_resnet_bwd never reads their inner
 * activations, so with save = 1 they may still run fused (td_bottleneck_fused); with save = 0 everything may. */
/* One whole frozen 64-plane bottleneck (layer1 of the torchvision trunk, models/backbone.py:82-98) in one pass:
 * out[N][H][W][256] = relu(conv3(relu(conv2_3x3(relu(conv1(x))))) + identity), identity = x (Cin = 256, wd = NULL) or the
 * block's downsample 1x1 (Cin = 64, wd / bd given); prepared (FrozenBN-folded, K-contiguous) bf16 weights: w1 [64][Cin],
 * w2 [64][3*3*64], w3 [256][64], wd [256][64].  The 64-channel tensors between the three convolutions stay in LDS.
 * Used by td_resnet_fwd; exported for the parity test. */
int td_bottleneck_fused(const void* x, void* out, const void* w1, const float* b1, const void* w2, const float* b2, const void* w3,
                        const float* b3, const void* wd, const float* bd, int N, int H, int W, int Cin, int dtype, td_stream_t stream);
/* Chained pointwise pair across two consecutive bottlenecks of one stage (bf16, planes = 256: layer3):
 *   out[M][4P] = relu(y2[M][P] w3[4P][P]^T + b3 + residual[M][4P])   conv3 + FrozenBN + identity + ReLU of block j
 *   h1[M][P]   = relu(out w1[P][4P]^T + b1)                           conv1 + FrozenBN + ReLU of block j + 1
 * in ONE launch: `out` is written (it is the next identity and, in a saved pass, the saved activation) but never read back.
 * Bit-identical to td_conv_gemm(conv3, residual, relu) followed by td_conv_gemm(conv1, relu).  Replaces the two calls
 * torchvision's Bottleneck.forward makes on either side of a block boundary (models/backbone.py:97-98) in both trunk passes
 * (models/tubedetr.py:127-134).  Used by td_resnet_fwd; exported for the parity test. */
int td_pw_chain2(const void* y2, const void* w3, const float* b3, const void* residual, void* out, const void* w1, const float* b1,
                 void* h1, int M, int planes, int dtype, td_stream_t stream);
/* stem_pairs = 1 (bf16, even W): the stem runs in its pixel-pair form - the frames are laid down with 4 channels per
 * pixel (3 + one zero), two horizontally adjacent pixels form one 8-channel element, and the 7x7 stride-2 convolution
 * becomes a 7x4 convolution with stride (2, 1) and padding (3, 2) over them: K = 224 instead of 392 (3 channels padded to 8),
 * half the input bytes.  w_fwd[0] must then be the [64][7][4][8] weight td_stem_pair_weights derives from the prepared
 * [64][7][7][8] one. */
int td_stem_pair_weights(const void* w_fwd_8, void* w_pairs, int Co, int dtype, td_stream_t stream);
/* The whole frozen stem in one pass (torchvision resnet conv1 + bn1 + relu + maxpool, reached through models/backbone.py:94-98):
 * pooled[N][PH][PW][64] = maxpool3x3s2p1( relu( conv7x7s2p3(x) + bias ) ), x_pairs = the frames as 4-channel pixels (two per 16-byte
 * element: [N][H][W/2][8], what td_frames_to_nhwc writes with Cpad = 4), w_pairs = td_stem_pair_weights' [64][7][4][8], bf16.  The
 * 64-channel convolution output stays in LDS (it is 4 GB per 1 000 frames of res 352 otherwise, written once and read 1.5 times).
 * td_resnet_fwd uses it when stem_pairs = 1; exported for the parity test. */
int td_stem_pool(const void* x_pairs, const void* w_pairs, const float* bias, void* pooled, int N, int H, int W, int dtype,
                 td_stream_t stream);
/* Backward through the stages >= first_train_stage (0..3; the reference trains layer2-4 = 1, backbone.py:82-89):
 * dfeat = gradient of *feat; fwd_ws = the save=1 workspace of the forward; dW[i] receives the gradient of conv i in
 * the parameter's own [Co][Ci][R][S] fp32 layout (FrozenBN scale un-folded); entries of frozen convs are ignored.
 * The forward may have run over N_fwd >= N frames (slow frames first, then the no_grad "fast" frames in the same
 * launch sequence); only the first N frames are back-propagated. */
size_t td_resnet_bwd_ws_bytes(int N, int H, int W, const int* nblocks, int first_train_stage, int dtype);
/* bytes of the weight-gradient job table (see td_conv_wgrad_batch): table_host = page-locked host memory, table_dev =
 * device memory, both caller-allocated and left untouched until the stream has passed the call. */
size_t td_resnet_bwd_table_bytes(const int* nblocks, int first_train_stage);
/* dW_prezeroed = 1: every dW[i] was zero-filled by the caller (one fill over the flat buffer they are views of): no per-job fills. */
int td_resnet_bwd(const void* dfeat, int N, int N_fwd, int H, int W, const int* nblocks, int first_train_stage,
                  const void* const* w_dgrad, const float* const* scale, float* const* dW, const void* fwd_ws, void* ws,
                  size_t ws_bytes, void* table_host, void* table_dev, size_t table_bytes, int dW_prezeroed, int dtype, int only_stage, td_stream_t stream);
/* only_stage = -1: the whole pass (one batched weight-gradient launch at its end).  only_stage = s: only the launches of stage s (3 = layer4 ..
 * first_train_stage), its weight gradients in a batched launch of their own; the caller issues s = 3, 2, .. on one stream with the same
 * workspace.  A data-parallel caller can then start the exchange of layer4's gradients while layer3 / layer2 are still computed
 * (DistributedDataParallel's bucketed reducer does that for the reference, main.py:372-376). */

/* Fold FrozenBatchNorm2d (models/backbone.py:60-70) into a conv: w_fwd[co][r][s][ci] = W[co][ci][r][s]*scale[co]
 * (ci zero-padded to Cpad), w_dgrad[ci][r][s][co] likewise (may be NULL), bias_out[co] = b - rm*scale,
 * scale_out[co] = w*rsqrt(rv+eps).  bn_* may be NULL (plain layer: scale 1, bias copied from `bias`). */
int td_weight_prep(const float* W, const float* bn_w, const float* bn_b, const float* bn_rm, const float* bn_rv,
                   const float* bias, int Co, int Ci, int R, int S, int Cpad, void* w_fwd, void* w_dgrad,
                   float* bias_out, float* scale_out, int dtype, td_stream_t stream);

/* Batched form of td_weight_prep: ONE launch prepares every layer of a model.  `items_dev` is a device copy of an
 * array of n td_prep_item (the caller uploads it once; it only holds pointers and sizes, which are stable across
 * optimizer steps).  blk0 = exclusive prefix sum of the items' workgroup counts ceil(Co_alloc/16)*ceil(Cpad/32);
 * total_blocks = their sum.  Co_alloc >= Co rows are written (rows >= Co are zero: padded output layers). */
typedef struct td_prep_item {
  const float* W;
  const float *bn_w, *bn_b, *bn_rm, *bn_rv, *bias;
  void *w_fwd, *w_dgrad;
  float *bias_out, *scale_out;
  int Co, Ci, RS, Cpad, Co_alloc, blk0;
} td_prep_item;
int td_weight_prep_batch(const td_prep_item* items_dev, int n, int total_blocks, int dtype, td_stream_t stream);

/* dW[co][ci][r][s] (+)= dw_k[co][r][s][ci] * scale[co]  (scale may be NULL). */
int td_wgrad_finalize(const float* dw_k, const float* scale, float* dW, int Co, int Ci, int R, int S, int Cpad,
                      int accumulate, td_stream_t stream);

/* NCHW fp32 frames -> NHWC T with channels zero-padded to Cpad (engine.py:55 samples.tensors). */
int td_nchw_to_nhwc(const float* x, void* y, int N, int C, int H, int W, int Cpad, int dtype, td_stream_t stream);
/* NHWC T -> NCHW fp32 (features returned through the nn.Module boundary). */
int td_nhwc_to_nchw(const void* x, float* y, int N, int C, int H, int W, int dtype, td_stream_t stream);
/* NCHW fp32 gradient -> NHWC T. */
int td_cast(const void* x, void* y, size_t n, int src_dtype, int dst_dtype, td_stream_t stream);

/* 3x3 stride-2 pad-1 max pooling, NHWC (torchvision resnet stem; forward only: the stem is frozen,
 * models/backbone.py:82-89). */
int td_maxpool3x3s2(const void* x, void* y, int N, int H, int W, int C, int dtype, td_stream_t stream);

/* y = LayerNorm(x + r) * gamma + beta over the last dim (cols); s_out (optional) receives x + r;
 * mean/rstd fp32 per row.  models/transformer.py:641-645,721-722,744-750,581,771. */
int td_add_layernorm_fwd(const void* x, const void* r, const float* gamma, const float* beta, void* y, void* s_out,
                         float* mean, float* rstd, int rows, int cols, float eps, int dtype, td_stream_t stream);
/* ds = LN backward wrt (x + r) (+ extra, an optional additional upstream gradient of s);
 * dgamma/dbeta accumulated with fp32 atomics. */
int td_add_layernorm_bwd(const void* dy, const void* s, const float* mean, const float* rstd, const float* gamma,
                         const void* extra, void* ds, float* dgamma, float* dbeta, int rows, int cols, int dtype,
                         td_stream_t stream);

/* out[n] += sum_m g[m][n]  (bias gradients). */
int td_colsum(const void* g, float* out, int rows, int cols, int ld, int dtype, td_stream_t stream);
/* y = a + b (b may be NULL -> copy); elementwise on T. */
int td_add(const void* a, const void* b, void* y, size_t n, int dtype, td_stream_t stream);

/* g = dy * scale where y > 0 else 0   (ReLU / ReLU+dropout backward from the saved output y). */
int td_relu_bwd(const void* dy, const void* y, void* g, size_t n, float scale, int dtype, td_stream_t stream);

/* GELU, exact erf form (the intermediate activation of HF RobertaModel, models/transformer.py:130-135,252-263):
 * y = 0.5 x (1 + erf(x / sqrt 2));  backward dx = dy * (Phi(x) + x phi(x)) from the saved pre-activation x. */
int td_gelu_fwd(const void* x, void* y, size_t n, int dtype, td_stream_t stream);
int td_gelu_bwd(const void* dy, const void* x, void* dx, size_t n, int dtype, td_stream_t stream);

/* y[i] = keep(seed, i) ? x[i] / (1-p) : 0 - the same counter-based mask as the fused epilogues
 * (element index i = row*ld + col), used standalone and to re-apply the mask in backward. */
int td_dropout(const void* x, void* y, size_t n, float p, uint32_t seed, const uint32_t* dropout_counter, int dtype,
               td_stream_t stream);

/* PositionEmbeddingSine (models/position_encoding.py:71-94, normalize=True, scale=2pi) from a
 * (N,h,w) uint8 pad mask -> pos [N][rows_per_image][2*npf] T  (token-major, the layout the encoder consumes).
 * rows_per_image >= h*w (<= 0: h*w): the rows behind the h*w tokens are written as zeros - the positional operand of the
 * text tokens the reference appends with torch.cat([pos_embed, zeros_like(text)]) (models/transformer.py:323-326). */
int td_pos_sine(const uint8_t* mask, void* pos, int N, int h, int w, int npf, float temperature, int rows_per_image, int dtype,
                td_stream_t stream);

/* Row gather / scatter: dst[dst_map[i]][0:cols] = src[src_map[i]][0:cols] (+ add[i][0:cols]) for i < n_rows (maps: device
 * int32[n_rows] or NULL = i).  The temporal replication of clip rows to frame rows (models/transformer.py:393-427: the text
 * rows of every frame's memory; the whole memory under --no_fast) as ONE pass of 16-byte accesses instead of a Python loop
 * of slice assignments; with `add` the same pass forms gathered + plain rows (the slow-fast mix, :441, re-formed in backward
 * instead of stored).  ld_* = row strides in elements, cols a multiple of 8 (bf16) / 4 (fp32). */
int td_rows_copy(const void* src, const int* src_map, const void* add, void* dst, const int* dst_map, int n_rows, int cols, int ld_src,
                 int ld_add, int ld_dst, int dtype, td_stream_t stream);
/* Segment sums over rows (the backward of that replication): out[out_map[r]][0:cols] = sum_{j in [ptr[r], ptr[r+1])} in[idx[j]][0:cols],
 * fp32 accumulation, r < n_out (ptr: device int32[n_out + 1], idx: device int32[ptr[n_out]], out_map: device int32[n_out] or NULL = r). */
int td_rows_segment_sum(const void* in, const int* idx, const int* ptr, void* out, const int* out_map, int n_out, int cols, int ld_in,
                        int ld_out, int dtype, td_stream_t stream);

/* Multi-head attention core on already projected q,k,v (nn.MultiheadAttention internals,
 * models/transformer.py:613,638-640 encoder; 661,713-719 temporal self-attention; 662,734-740
 * time-aligned cross-attention with Lq=1).  Batch-major rows: q [B][Lq] rows of stride ldq, head h in
 * columns h*hd..h*hd+hd-1 (hd = 32: TubeDETR's transformer, MFMA kernels in bf16; hd = 64: RoBERTa's 12 x 64 heads, fp32-math
 * kernels in both dtypes); k,v [B][Lk] likewise; key_pad [B][Lk] uint8 (1 = ignore) or NULL.
 * scores = scale * q.k; probs [B][H][Lq][Lk] fp32 = softmax (pre-dropout, saved for backward);
 * out [B][Lq] rows of stride ldo = dropout(probs) @ v; wavg [B][Lq][Lk] fp32 = head average of the
 * post-dropout probabilities (what nn.MultiheadAttention returns) or NULL.  hd = 32: any Lq, Lk >= 1 in both dtypes (Lk <= 512
 * and, for the backward, Lq <= 640 on LDS-resident kernels; beyond, or at 2^32 elements and more, kernels that walk chunks of keys
 * / queries with a 64-bit probability and dropout index - the same mask below 2^32).  hd = 64: Lk <= 512 and B*H*Lq*Lk < 2^32,
 * else TD_ERR_INVALID.  bf16 callers that need no weights: td_mha_lean_fwd / _bwd below store nothing of size Lq x Lk. */
int td_mha_fwd(const void* q, const void* k, const void* v, const uint8_t* key_pad, void* out, float* probs,
               float* wavg, int B, int H, int Lq, int Lk, int hd, int ldq, int ldk, int ldv, int ldo, float scale,
               float dropout_p, uint32_t dropout_seed, const uint32_t* dropout_counter, int dtype, td_stream_t stream);
/* Backward of td_mha_fwd.  dwavg [B][Lq][Lk] fp32 = gradient of the head-averaged weights
 * (guided-attention loss, models/tubedetr.py:357-369) or NULL; ds_ws: fp32 workspace [B][H][Lq][Lk].
 * dq, dk, dv are written with the row strides of q, k, v (ldq, ldk, ldv); dout has row stride ldo. */
int td_mha_bwd(const void* q, const void* k, const void* v, const void* dout, const float* probs, const float* dwavg,
               void* dq, void* dk, void* dv, float* ds_ws, int B, int H, int Lq, int Lk, int hd, int ldq, int ldk,
               int ldv, int ldo, float scale, float dropout_p, uint32_t dropout_seed, const uint32_t* dropout_counter,
               int dtype, td_stream_t stream);

/* Time-aligned cross-attention of the decoder (models/transformer.py:725-745; nn.MultiheadAttention with ONE query per
 * frame, E = 256 channels in H = 8 heads) with both memory-side projections moved to the query side:
 *   score[h][s] = u[f][h] . (mem[f*S+s] + pos[f*S+s])      u[f][h] = scale * W_k,h^T q[f],  q.b_k is constant over s and cancels
 *   out[f]      = W_v,blk zext[f],  zext[f] = [ z[f][0..H) | sum_s pd[f][h][s] ],  z[f][h] = sum_s pd[f][h][s] mem[f*S+s]
 * (pd = probabilities after dropout; same mask index and the same `probs` / `wavg` outputs as td_mha_fwd with Lq = 1).  The key
 * and value projections of the memory rows, 93 % of the decoder's FLOPs in the reference formulation, do not exist; the two
 * remaining products with W_k / W_v are GEMMs over the F query rows against the block-structured weights below.
 * u [F][H*E] T, mem / pos [F*S][E] T (pos may be NULL), key_pad [F][S] uint8 or NULL, probs [F][H][S] fp32, wavg [F][S] fp32 or
 * NULL, zext [F][ldz] T with ldz >= H*E + H (a multiple of 8).
 * Any S >= 1 is taken by td_cross_q1_fwd / _bwd / _bwd_coef (F * H * S < 2^32: the dropout index).  Up to S = 320 a workgroup keeps the
 * frame's scores (bf16, S <= 256, no fp32 d_mem: the frame's rows too, on the matrix pipe) in LDS; above it the streaming instances walk
 * the frame twice in chunks of 128 rows - statistics first (forward: running max / sum per head; backward: delta), outputs second - with
 * LDS use independent of S: the VALU family in fp32 and wherever an fp32 d_mem is written, the matrix-pipe family for the other bf16
 * launches.  No atomics in either range: the same call returns the same bits. */
int td_cross_q1_fwd(const void* u, const void* mem, const void* pos, const uint8_t* key_pad, float* probs, float* wavg, void* zext,
                    int F, int S, int H, int E, int ldz, float dropout_p, uint32_t dropout_seed, const uint32_t* dropout_counter,
                    int dtype, td_stream_t stream);
/* Backward: d_zext [F][ldz] T, dwavg [F][S] fp32 or NULL  ->  d_u [F][H*E] T and d_mem [F*S][E] FP32, overwritten when
 * accumulate == 0, else added to (the memory is shared by the six layers: the first layer to run writes, the others add);
 * d_mem == NULL: the memory needs no gradient, nothing is formed or stored.
 * pos receives no gradient here (sine encodings; learned ones use the projected-memory path). */
int td_cross_q1_bwd(const void* u, const void* mem, const void* pos, const float* probs, const void* d_zext, const float* dwavg,
                    void* d_u, float* d_mem, int accumulate, int F, int S, int H, int E, int ldz, float dropout_p, uint32_t dropout_seed,
                    const uint32_t* dropout_counter, int dtype, td_stream_t stream);
/* bf16 mode: the memory gradient of ALL layers in one pass instead of an fp32 read-modify-write of [F*S][E] per layer.
 * td_cross_q1_bwd_coef = td_cross_q1_bwd without d_mem: row f*S + s of `coef` (bf16, row stride coef_ld, a multiple of 32)
 * receives this layer's sixteen coefficients [ds[0..H) | pd[0..H)] at column coef_col (a multiple of 16; one block per layer).
 * td_cross_q1_dmem then forms  d_mem[f*S + s] = sum over layers l, heads h of  ds_l[h][s] u_l[f][h] + pd_l[h][s] d_z_l[f][h]
 * as one [S][coef_ld] x [coef_ld][E] product per frame on the matrix pipe and writes it in T (bf16): u[l] / d_zext[l] are the
 * tensors layer l handed to td_cross_q1_bwd_coef with coef_col = 16 l (a layer that did not run: both NULL, its columns of a
 * zero-filled `coef` are never written).  models/transformer.py:725-745 (backward of the six layers' shared memory). */
int td_cross_q1_bwd_coef(const void* u, const void* mem, const void* pos, const float* probs, const void* d_zext, const float* dwavg,
                         void* d_u, void* coef, int coef_ld, int coef_col, int F, int S, int H, int E, int ldz, float dropout_p,
                         uint32_t dropout_seed, const uint32_t* dropout_counter, int dtype, td_stream_t stream);
int td_cross_q1_dmem(const void* coef, int coef_ld, const void* const* u, const void* const* d_zext, int n_layers, void* d_mem, int F, int S,
                     int H, int E, int ldz, int dtype, td_stream_t stream);
/* Block-structured forms of one [E][E] slice of nn.MultiheadAttention.in_proj_weight (fp32, [out][in]; out channel j belongs to
 * head j / (E/H)) for those GEMMs: w_n [E][H*E + nb] holds W[j][:] * alpha in column block head(j) of row j (zeros elsewhere)
 * and, if bias != NULL (nb = H, else 0), bias[j] in column H*E + head(j); w_t [H*E + nb][E] is its transpose.  Both in `dtype`.
 *   keys:   u = q w_t^T (alpha = 1/sqrt(E/H)),  d_q = d_u w_n^T          values: out = zext w_n^T,  d_zext = d_out w_t^T */
int td_head_blocks_expand(const float* W, const float* bias, float alpha, void* w_n, void* w_t, int E, int H, int dtype, td_stream_t stream);
/* ...and back: from the dense fp32 gradient G [E][H*E + nb] of w_n, dW[j][c] = G[j][head(j)*E + c] * alpha and (db != NULL: nb = H)
 * db[j] = G[j][H*E + head(j)]. */
int td_head_blocks_extract(const float* G, float alpha, float* dW, float* db, int E, int H, td_stream_t stream);

/* Lean form of the same attention core for callers that do not need the weights (the per-frame visual-text encoder,
 * models/transformer.py:638-640: `weights` is dead there, SURVEY.md 8a'): nothing of size Lq x Lk is stored.  The forward
 * writes two softmax statistics per (batch, head, query) into `stats` (td_mha_lean_stats_bytes(B, H, Lq) bytes: 4 floats per
 * row); the backward recomputes the probabilities from q, k, key_pad and those statistics, takes sum_k P dP from dout . out
 * (`out` = the forward's output), and uses the third float of each row as scratch.  bf16, hd = 32, 16-byte aligned rows, any
 * Lq >= 1 and Lk >= 1 (Lk <= 256 with Lq <= 448: one key block per row; beyond: streaming kernels that walk key blocks with an
 * online softmax, and query blocks for dK / dV; no float atomics, bit-reproducible); anything else returns TD_ERR_INVALID (use
 * td_mha_fwd / td_mha_bwd).  Same dropout mask as td_mha_fwd; the dropout element index (b*H + h)*Lq*Lk + q*Lk + k is 64-bit,
 * so B*H*Lq*Lk may exceed 2^32 (below 2^32 the mask is the 32-bit one). */
size_t td_mha_lean_stats_bytes(int B, int H, int Lq);
int td_mha_lean_fwd(const void* q, const void* k, const void* v, const uint8_t* key_pad, void* out, float* stats, int B, int H,
                    int Lq, int Lk, int hd, int ldq, int ldk, int ldv, int ldo, float scale, float dropout_p,
                    uint32_t dropout_seed, const uint32_t* dropout_counter, int dtype, td_stream_t stream);
int td_mha_lean_bwd(const void* q, const void* k, const void* v, const uint8_t* key_pad, const void* out, const void* dout,
                    float* stats, void* dq, void* dk, void* dv, int B, int H, int Lq, int Lk, int hd, int ldq, int ldk, int ldv,
                    int ldo, float scale, float dropout_p, uint32_t dropout_seed, const uint32_t* dropout_counter, int dtype,
                    td_stream_t stream);


/* ---- optimizer-side tail of a training step over FLAT fp32 buffers -------------------------------
 * All trainable parameters of the model lie back to back in one buffer (`param`), their gradients in the same order in
 * another (the flat buffer of the data-parallel exchange).  The buffers are tiled by at most TD_OPTIM_MAX_SEGMENTS
 * segments; a segment belongs to one parameter group (learning rate index: 0 = transformer + heads, 1 = backbone,
 * 2 = text encoder, main.py:381-405) and is `active` unless its parameters received no gradient (RoBERTa's pooler:
 * torch skips p.grad is None in clip_grad_norm_ and in optimizer.step()).  An inactive segment keeps param, exp_avg and
 * exp_avg_sq bit for bit and its gradients are never read into the norm; only its EMA moves,
 * ema = ema*ema_decay + (1-ema_decay)*param, as update_ema (util/optim.py:8-25) does for every state-dict entry. */
#define TD_OPTIM_MAX_SEGMENTS 32
#define TD_OPTIM_MAX_GROUPS 4
#define TD_OPTIM_NORM_BLOCKS 2048
typedef struct td_optim_segment {
  long long begin, end; /* element range [begin, end) */
  int group;            /* index into lr_dev[] */
  int active;           /* 0: no gradient - only the EMA is updated */
} td_optim_segment;
/* Replaces torch.nn.utils.clip_grad_norm_ (engine.py:149-150): norm_clip[0] = L2 norm of all active gradients,
 * norm_clip[1] = min(1, max_norm / (norm + 1e-6)) (1 when max_norm <= 0); *step (device int, may be NULL) += 1.
 * ws: td_grad_norm_ws_bytes() bytes of device scratch.  Two launches.
 * A non-finite active gradient is NOT detected here, and the step counter advances all the same.  A NaN element makes
 * the norm and the coefficient NaN (max_norm > 0), and the td_adamw_ema_step that follows multiplies every gradient by it:
 * every active param, both moments and the EMA are NaN after one launch.  An Inf element (or finite gradients whose fp32
 * norm overflows) makes the norm Inf and the coefficient 0: Inf * 0 = NaN lands in that element's param / moments / EMA,
 * every other element takes a zero-gradient step.  td_grad_norm_clip_guarded (below) is the call that notices. */
size_t td_grad_norm_ws_bytes(void);
int td_grad_norm_clip(const float* grad, size_t n, const td_optim_segment* segs, int n_segs, float max_norm, void* ws,
                      size_t ws_bytes, float* norm_clip, int* step, td_stream_t stream);
/* Replaces optimizer.step() of torch.optim.AdamW with three parameter groups (main.py:406-413, engine.py:151) and
 * update_ema (util/optim.py:8-25) in ONE launch: g = grad * norm_clip[1] (norm_clip may be NULL); param *= 1 - lr*wd;
 * exp_avg = lerp(exp_avg, g, 1-beta1); exp_avg_sq = beta2*exp_avg_sq + (1-beta2) g^2; param -= lr/(1-beta1^t) *
 * exp_avg / (sqrt(exp_avg_sq)/sqrt(1-beta2^t) + eps); ema = ema*ema_decay + (1-ema_decay)*param (ema may be NULL).
 * lr_dev: TD_OPTIM_MAX_GROUPS device floats (written by the host's adjust_learning_rate, util/optim.py:28-95);
 * step_dev: device int holding t (already incremented by td_grad_norm_clip). */
int td_adamw_ema_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, size_t n,
                      const td_optim_segment* segs, int n_segs, const float* lr_dev, const float* norm_clip,
                      const int* step_dev, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                      td_stream_t stream);
/* The same tail with a guard: a step whose gradient norm is not finite is skipped ON THE DEVICE, without a host
 * synchronisation, so the pair can be captured in a HIP graph (replaces the host-side `if not math.isfinite(loss_value):
 * sys.exit(1)` of engine.py:142-145, which a replayed graph never reaches).  Opt-in: the two calls above are unchanged.
 * guard: td_guard_bytes(history) bytes of device memory, 4-byte aligned, zero-filled ONCE by the caller and then owned by
 * these calls: a 16-byte header `int attempts, skipped, consecutive_skipped, applied_now`, followed by a ring of `history`
 * td_step_record (0 <= history <= TD_GUARD_HISTORY_MAX; 0: counters only).
 * td_grad_norm_clip_guarded: the total is accumulated exactly as td_grad_norm_clip accumulates it (same grid, same order,
 * same reductions), so on a finite buffer norm_clip[0..1] and *step are bit-identical to that call's; the per-group sums
 * are extra accumulators of the same pass.  ws: td_grad_norm_guard_ws_bytes() bytes, 8-byte aligned (per-workgroup
 * partial sums of the total and of each of the TD_OPTIM_MAX_GROUPS groups).  The decision is isfinite() of the fp32 norm
 * that is written to norm_clip[0]:
 *   finite:     norm_clip[1] as above, *step += 1, applied_now = 1, consecutive_skipped = 0;
 *   not finite: norm_clip[0] = the norm as computed (NaN / Inf), norm_clip[1] = 0, *step untouched, applied_now = 0,
 *               skipped += 1, consecutive_skipped += 1.
 * Either way attempts += 1 and, if history > 0, ring[(attempts - 1) % history] = {attempts, *step after the call (0 if
 * step is NULL), applied_now, norm, coefficient, loss[0] (NaN if loss is NULL), group_norm[g] = sqrt(sum of squares
 * over group g's active elements), 0 for a group without any}.  Stale NaN / Inf in inactive segments does not count,
 * as above.
 * `loss` (device float, may be NULL) is RECORDED and never decides: under data parallelism the loss is a per-rank value,
 * while the gradient buffer is the exchanged one and identical on every rank.  A decision taken from the loss could differ
 * between ranks - one applies the update, another skips it - and the replicas' weights would part for good; the norm of
 * the exchanged buffer gives every rank the same decision from the same bits.
 * td_adamw_ema_step_guarded: td_adamw_ema_step's kernel body behind one read of applied_now per workgroup.  applied_now
 * == 0: it returns before any load or store of param / exp_avg / exp_avg_sq / ema, all four stay bit-identical, the EMA
 * of inactive segments included (the batch counts as never seen); applied_now == 1: bit-identical to td_adamw_ema_step. */
#define TD_GUARD_HISTORY_MAX 4096
typedef struct td_step_record {
  int attempt;  /* 1-based number of the td_grad_norm_clip_guarded call that wrote the record */
  int step;     /* the step counter after that call: it counts applied updates only */
  int applied;  /* 1: the update ran; 0: skipped */
  float norm;   /* norm_clip[0] */
  float clip;   /* norm_clip[1] */
  float loss;   /* loss[0] as handed over, NaN if none */
  float group_norm[TD_OPTIM_MAX_GROUPS];
} td_step_record;
size_t td_grad_norm_guard_ws_bytes(void);
size_t td_guard_bytes(int history);
int td_grad_norm_clip_guarded(const float* grad, size_t n, const td_optim_segment* segs, int n_segs, float max_norm, void* ws,
                              size_t ws_bytes, float* norm_clip, int* step, const float* loss, void* guard, int history,
                              td_stream_t stream);
int td_adamw_ema_step_guarded(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, size_t n,
                              const td_optim_segment* segs, int n_segs, const float* lr_dev, const float* norm_clip,
                              const int* step_dev, float beta1, float beta2, float eps, float weight_decay, float ema_decay,
                              const void* guard, td_stream_t stream);

/* ---- SetCriterion as one launch ------------------------------------------------------------------
 * The 24 losses of models/tubedetr.py:270-372,397-460 (L1 + GIoU over the annotated frames' boxes, start / end KL
 * divergence against Gaussian targets, guided-attention loss) for the main output and the auxiliary decoder layers,
 * stacked on a leading layer axis, all fp32:
 *   boxes [nl][b*T][4] predicted cxcywh of EVERY frame; keep [n] = frame indices of the annotated frames (the
 *   keep-gather of engine.py:83-97), tgt [n][4] their target boxes; sted [nl][b][T][2] logits (or NULL);
 *   weights [nl][b][T][T] temporal self-attention weights (or NULL); time_mask / positive [b][T] uint8;
 *   inter [b][2] annotated (start, end); num_boxes: device scalar if non-NULL (kept by the data-parallel harness) else
 *   num_boxes_host; both are clamped to >= 1.
 * losses [nl][4] = (loss_bbox, loss_giou, loss_sted, loss_guided_attn) per layer.  The same launch stores the
 * derivative of every loss with respect to its inputs (g_l1, g_giou: [nl][b*T][4]; g_sted like sted; g_w like weights);
 * td_criterion_bwd combines them with the upstream gradient dlosses [nl][4] into d_boxes / d_sted / d_weights. */
int td_criterion_fwd(const float* boxes, const float* tgt, const long long* keep, const float* sted, const float* weights,
                     const uint8_t* time_mask, const uint8_t* positive, const int* inter, const float* num_boxes_dev,
                     float num_boxes_host, float sigma, int nl, int b, int T, int n, float* losses, float* g_l1, float* g_giou,
                     float* g_sted, float* g_w, td_stream_t stream);
int td_criterion_bwd(const float* dlosses, const float* g_l1, const float* g_giou, const float* g_sted, const float* g_w,
                     float* d_boxes, float* d_sted, float* d_weights, int nl, int b, int T, td_stream_t stream);

/* PostProcessSTVG (models/postprocessors.py:13-84): per video the (start, end) index pair with end > start that maximises
 * log_softmax(steds[:, :, 0])[start] + log_softmax(steds[:, :, 1])[end]; first index on ties, like torch.max.
 * steds [n_videos][T][2] fp32 logits (-inf on padded positions), start_end [n_videos][2] int64. */
int td_sted_decode(const float* steds, long long* start_end, int n_videos, int T, td_stream_t stream);

/* ---- Device-side clip augmentation -------------------------------------------------------------------------------
 * Resamples the decoded frames of many clips in ONE launch: the pixel work of the datasets' spatial transforms (random
 * horizontal flip, resize, size crop, second resize: datasets/video_transforms.py:70-118,135-232,235-324, applied
 * frame by frame on the host by cv2.resize in datasets/torch_videovision.py:125-161) and of the padding collate
 * (NestedTensor.from_tensor_list, util/misc.py:158-170).  Per job:
 *   src: uint8 rgb24, T frames of sh x sw pixels, 3 interleaved channels, `src_pitch` bytes per row and
 *        `src_frame_stride` bytes per frame; flip = 1 reads source column j as column sw - 1 - j;
 *   a virtual bilinear resize of the (flipped) source to rh x rw, of which the window (wy, wx, wh, ww) is produced;
 *   planar = 0: dst = interleaved uint8 [T][wh][ww][3] (the intermediate between the two resizes of the training
 *        transform, which rounds to uint8 in between);
 *   planar = 1: dst = the batch's padded uint8 video [n][3][H][W]; frame t goes to [frame_off + t]: pixels inside
 *        wh x ww are written, the rest of H x W is zero-filled, and mask [n][H][W] (bool bytes) gets 0 inside, 1 outside.
 * Sampling rule (cv2.INTER_LINEAR / F.interpolate(mode="bilinear", align_corners=False), no antialiasing): output pixel
 * (y, x) of the virtual image samples at cy = (y + 0.5) * sh / rh - 0.5 (cx alike), clamped to the source; coordinates
 * are exact integers ((2y + 1) sh - rh over 2 rh: quotient = row, remainder = weight); value = floor(blend + 0.5).
 * rh x rw = sh x sw is an exact copy.  `jobs` is a host array consumed before the call returns; the job table lives in
 * caller-provided memory like td_conv_wgrad_batch's (table_host page-locked, table_dev device memory, both of
 * td_clip_resample_table_bytes(n_jobs) bytes and untouched until the stream has passed the call).  No allocation, no
 * synchronisation inside.  Sizes up to 16384 per side; a source row of more than 8192 pixels is rejected. */
typedef struct td_resample_job {
  const void* src;
  long long src_frame_stride;
  int src_pitch;
  int T, sh, sw;
  int flip;
  int rh, rw;
  int wy, wx, wh, ww;
  void* dst;
  int planar;
  int frame_off;
  int H, W; /* planar = 1: the padded frame; planar = 0: ignored */
  void* mask; /* planar = 1 only */
} td_resample_job;
size_t td_clip_resample_table_bytes(int n_jobs);
int td_clip_resample(const td_resample_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* td_clip_resample with the decoder's native frames as the source (an addition WITHIN ABI 11: nothing above changed, and
 * td_abi_version() stays 11).  A job is a td_resample_job plus the source format; with fmt = TD_SRC_RGB24 it IS that job
 * (plane0 / pitch0 / frame_stride = src / src_pitch / src_frame_stride), so one launch may mix formats.
 *   TD_SRC_I420 (ffmpeg yuv420p; yuvj420p with full_range = 1): per frame a Y plane of sh x sw bytes, then U, then V,
 *        each ch x cw with ch = (sh + 1) / 2, cw = (sw + 1) / 2 (integer division);
 *   TD_SRC_NV12: the Y plane, then one plane of ch rows of cw interleaved (U, V) byte pairs (plane1; plane2 unused).
 * Every plane has its own pointer (of frame 0) and row pitch; frame t of each plane lies t * frame_stride bytes further.
 * An ffmpeg rawvideo pipe packs tightly: pitches sw, cw, cw (NV12: sw, 2 cw), plane1 = plane0 + sw sh,
 * plane2 = plane1 + cw ch, frame_stride = sw sh + 2 cw ch.  Odd sw, sh are legal: the last column / row shares its
 * chroma sample.  No byte outside a plane's rows of the job's T frames is read.
 * Conversion rule (exact integers, so results are reproducible to the bit): source pixel (y, x) uses chroma sample
 * (y >> 1, x >> 1) - replication, no interpolation - and, in int32, with yo = 16 (limited range) or 0 (full range),
 *   c = Y - yo, d = U - 128, e = V - 128,
 *   R = clamp((cy c + crv e + 32768) >> 16), G = clamp((cy c - cgu d - cgv e + 32768) >> 16),
 *   B = clamp((cy c + cbu d + 32768) >> 16)          (>> arithmetic = floor division; clamp to [0, 255]).
 * Coefficients are round(65536 x) of the textbook values; from Kr, Kb, Kg = 1 - Kr - Kb: crv = 2 (1 - Kr) s,
 * cbu = 2 (1 - Kb) s, cgu = 2 Kb (1 - Kb) / Kg s, cgv = 2 Kr (1 - Kr) / Kg s, with cy = 255 / 219, s = 255 / 224 for
 * limited range and cy = s = 1 for full range:
 *                      cy      crv     cbu     cgu    cgv
 *   BT.601 limited   76309  104597  132201   25675  53279
 *   BT.601 full      65536   91881  116130   22553  46802
 *   BT.709 limited   76309  117489  138438   13975  34925
 *   BT.709 full      65536  103206  121609   12276  30679
 * (within 0.502 of a level of the float64 formula over all (Y, U, V); |accumulator| < 3.6e7).  The job's output is, byte
 * for byte, what td_clip_resample produces from the rgb24 frames this rule makes of the source: flip reads converted
 * column sw - 1 - j; sampling rule, window, destinations, mask, zero fill and limits are td_clip_resample's.  Agreement
 * with any decoder library's own yuv -> rgb conversion (ffmpeg's swscale) is not claimed.  The job table is sized by
 * td_clip_resample_src_table_bytes (its records are larger than td_clip_resample's). */
#define TD_SRC_RGB24 0
#define TD_SRC_I420 1
#define TD_SRC_NV12 2
#define TD_MATRIX_BT601 0
#define TD_MATRIX_BT709 1
typedef struct td_resample_src_job {
  const void* plane0; /* rgb24 pixels, or Y */
  const void* plane1; /* I420: U; NV12: UV pairs; RGB24: ignored */
  const void* plane2; /* I420: V; else ignored */
  long long frame_stride;
  int pitch0, pitch1, pitch2;
  int fmt;
  int matrix, full_range; /* I420 / NV12 only */
  int T, sh, sw;
  int flip;
  int rh, rw;
  int wy, wx, wh, ww;
  void* dst;
  int planar;
  int frame_off;
  int H, W;
  void* mask;
} td_resample_src_job;
size_t td_clip_resample_src_table_bytes(int n_jobs);
int td_clip_resample_src(const td_resample_src_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* Every index vector of one durations pattern in ONE launch (an addition WITHIN ABI 11).  A batch of b videos of durations d_i
 * sampled with stride k has c_i = ceil(d_i / k) slow clips per video - any mix of clip counts - n = sum c_i clips in all, and
 * F = b t frames with t = max d_i (shorter videos are padded in time).  ``table`` is a DEVICE array of b records
 * (d_i, first_clip_i = sum_{j<i} c_j, c_i), int32; b <= 256.
 * Owner clip of frame (i, j): first_clip_i + min(j / k, c_i - 1) - for the frames of a video the reference's rule (models/transformer.py:393-427,
 * models/tubedetr.py:154-187: frame j belongs to clip j / k of its video, the last clip may be shorter); a time-padded frame takes its
 * video's last clip.  With equal clip counts this is i * n_clips + j / k, the reference's flat numbering.
 * Outputs (caller-allocated device buffers, each written completely; a NULL pointer leaves that vector out; the 14 maps are written
 * together or not at all).  S = hw + L rows per clip / frame (hw visual tokens, then L text tokens); clip rows are c S + s, frame rows f S + s.
 *   owner, vid_of_frame [F] int64; vid_of_clip [n] int64; query_mask [F] bytes, 1 = time padding (frame 0 of a video is never 1)
 *   frame_dest, clip_of [sum d_i] int64: padded frame number i t + j, and owner clip, of the valid frames in video order
 *   vis_src, vis_dst [F hw]; txt_src, txt_dst [F L]; all_src [F S]: clip row / frame row of every visual, text, any token
 *   iota_vis, clip_vis [n hw]; clip_txt [n L]: 0, 1, 2, ...; clip rows of the visual / the text tokens
 *   seg_X_idx, seg_X_ptr for X = vis (m = hw, first row 0), txt (m = L, first row hw), all (m = S, first row 0): CSR lists "frame
 *     rows summed into output row (c, col)", [F m] and [n m + 1].  Clip c owns the count_c frames from f0_c on, so
 *     ptr[c m + col] = m f0_c + col count_c and idx[ptr + q] = (f0_c + q) S + first row + col, frames ascending; ptr[n m] = F m.
 * int32 unless stated; F S < 2^31 is required.  n_clips must be sum c_i: the table is not readable from the host side of the call, and
 * the buffers' sizes follow from it. */
typedef struct td_replica_maps_out {
  long long* owner;
  long long* vid_of_frame;
  long long* vid_of_clip;
  unsigned char* query_mask;
  long long* frame_dest;
  long long* clip_of;
  int* vis_src;
  int* vis_dst;
  int* txt_src;
  int* txt_dst;
  int* all_src;
  int* iota_vis;
  int* clip_vis;
  int* clip_txt;
  int* seg_vis_idx;
  int* seg_vis_ptr;
  int* seg_txt_idx;
  int* seg_txt_ptr;
  int* seg_all_idx;
  int* seg_all_ptr;
} td_replica_maps_out;
int td_replica_maps(const int* table, int b, int t, int k, int hw, int L, int n_clips, const td_replica_maps_out* out, td_stream_t stream);

/* ---- Grounded tubes drawn into decoded frames (an addition WITHIN ABI 11: nothing above changed) -----------------------
 * Writes the answer to a grounding question - the box of every frame, the temporal span, the decoder's attention - into the
 * decoded frames of many clips in ONE launch, in the frames' own pixel format (the reference's demo re-opens every frame
 * as a JPEG in matplotlib: demo_stvg.py:152-194, server_stvg.py:218-257).  Per job:
 *   T frames of sh x sw in fmt = TD_SRC_RGB24 / TD_SRC_I420 / TD_SRC_NV12, planes, pitches and frame stride described as in
 *   td_resample_src_job (odd sizes are legal, chroma planes are (sh + 1) / 2 x (sw + 1) / 2), once for the source (src0..2)
 *   and once for the destination (dst0..2).  A destination plane may BE its source plane (same pointer, pitch and frame
 *   stride: in place); any other overlap of a destination plane with a source plane is an error.  Every byte of the rows of
 *   the job's destination frames gets the value defined below; no other byte is written (not the row padding between the row
 *   and the pitch), and no byte outside the source rows is read.
 * Inputs, device pointers, each nullable (NULL leaves its layer out):
 *   boxes      fp32 [n_tube][4], xyxy in source pixels (what PostProcess returns);
 *   span       int64 [2]: first and last tube row that contain the object, both inclusive (one row of td_sted_decode's
 *              output); NULL: every row does;
 *   frame_map  int32 [T]: the tube row r of frame t; NULL: r = t.  A frame whose r is outside [0, n_tube) is a plain copy;
 *   heat       uint8 [n_tube][mh][mw]: one attention map per tube row;
 *   box_color, heat_color, dim_color: three bytes IN THE FRAME'S OWN COLOUR SPACE (R, G, B or Y, U, V);
 *   thickness >= 1 (with boxes), heat_alpha and dim_alpha in [0, 256].
 * The rule (exact integers, reproducible to the bit).  A frame is a stack of up to three layers; a layer gives every luma
 * pixel (rgb24: every pixel) an alpha a in [0, 256] and a colour c, and a byte v becomes (v (256 - a) + c a + 128) >> 8.
 * In this order:
 *   1. dim, only when span is given and r lies outside it: a = dim_alpha everywhere, c = dim_color.
 *   2. heat, whenever heat is given: pixel (y, x) samples map r at gy = clamp(((2 y + 1) mh 128) / sh - 128, 0, 256 (mh - 1)),
 *      gx alike from x, mw, sw (integer division of a non-negative operand); i = g >> 8, f = g & 255, neighbour min(i + 1, n - 1);
 *      h = ((256 - fy) ((256 - fx) q00 + fx q01) + fy ((256 - fx) q10 + fx q11) + 32768) >> 16; a = (h heat_alpha + 127) / 255,
 *      c = heat_color.
 *   3. box, only when boxes is given and r lies inside the span: x0 = (int)floorf(bx0 + 0.5f), y0, x1, y1 alike, in fp32,
 *      finite values clamped to +-2^20 before the conversion; a box with a non-finite coordinate or with x1 <= x0 or y1 <= y0
 *      draws nothing.  a = 256 for a pixel in [x0, x1) x [y0, y1) that is not in [x0 + th, x1 - th) x [y0 + th, y1 - th),
 *      c = box_color; the parts of the outline outside the frame are simply absent.
 * A chroma sample (I420 / NV12) takes, per layer, the mean alpha of the luma pixels of its 2 x 2 block that exist,
 * (sum + n / 2) / n with n in {1, 2, 4}, and is blended with the U / V byte of the colour (NV12: both bytes of the pair).
 * Colours: tubedetr_amd.render.color_in_space makes the three bytes from an RGB colour by the forward of the conversion
 * above (exact integers): Y = clamp((yr R + yg G + yb B + 2^20 yo + 2^19) >> 20), U = clamp((ur R + ug G + ub B +
 * 2^20 128 + 2^19) >> 20), V alike (>> = floor division), coefficients round(2^20 x) of yr = Kr s_y, yg = Kg s_y,
 * yb = Kb s_y, ur = -Kr / (2 (1 - Kb)) s_c, ug = -Kg / (2 (1 - Kb)) s_c, ub = s_c / 2, vr = s_c / 2, vg = -Kg / (2 (1 - Kr)) s_c,
 * vb = -Kb / (2 (1 - Kr)) s_c, with s_y = 219 / 255, s_c = 224 / 255 for limited range and s_y = s_c = 1 for full range
 * (BT.601: Kr = 0.299, Kb = 0.114; BT.709: Kr = 0.2126, Kb = 0.0722): within 0.5004 of a level of the float64 formula
 * for every (R, G, B).  (20 fraction bits where the device rule above has 16: at 16 the three limited-range U coefficients
 * all round the same way and bright colours come out 0.5036 off; three bytes per job are converted on the host.)
 * Limits: sides 1..16384, mh and mw 1..256.  A violation returns an error whose message names the field; nothing is
 * launched.  `jobs` is a host array consumed before the call returns; the job table lives in caller-provided memory as
 * for td_clip_resample (table_host page-locked, table_dev device memory, both of td_tube_overlay_table_bytes(n_jobs)
 * bytes).  No allocation, no synchronisation inside. */
typedef struct td_overlay_job {
  const void* src0; /* rgb24 pixels, or Y */
  const void* src1; /* I420: U; NV12: UV pairs; RGB24: ignored */
  const void* src2; /* I420: V; else ignored */
  long long src_frame_stride;
  int src_pitch0, src_pitch1, src_pitch2;
  void* dst0;
  void* dst1;
  void* dst2;
  long long dst_frame_stride;
  int dst_pitch0, dst_pitch1, dst_pitch2;
  int fmt;
  int T, sh, sw;
  const float* boxes;
  const long long* span;
  const int* frame_map;
  const unsigned char* heat;
  int n_tube;
  int mh, mw;
  int thickness;
  int heat_alpha, dim_alpha;
  unsigned char box_color[3], heat_color[3], dim_color[3];
} td_overlay_job;
size_t td_tube_overlay_table_bytes(int n_jobs);
int td_tube_overlay(const td_overlay_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* ---- Scored K-best moments (an addition WITHIN ABI 11: nothing above changed) ------------------------------------------
 * Per video the K likeliest (start, end) pairs that are not near-copies of each other, with their log-probabilities:
 * td_sted_decode's arg-max continued by a greedy temporal NMS, with the window ensembling of PostProcessSTVG
 * (models/postprocessors.py:27-53) done by the kernel.  ONE launch, one workgroup per video, whatever K is; no
 * allocation, no synchronisation, no atomics: the result does not depend on scheduling.  This comment is the rule.
 *   steds   fp32 [n_windows][T][2] logits (start, end);
 *   valid   bytes [n_windows][T], 0 = padded position; NULL = every position is valid;
 *   win_ptr device int32 [n_videos + 1]: video v owns the windows win_ptr[v] .. win_ptr[v + 1] - 1; NULL = window v alone
 *           (then n_windows >= n_videos).  The caller guarantees a non-decreasing table that ends at n_windows and gives
 *           no video more than max_windows windows; the kernel clamps a video's window count to [0, max_windows] and
 *           every window index to [0, n_windows), so a wrong table cannot make it read outside steds / valid.
 * Positions.  Video v has P_v = n_w(v) T positions; position p = (w - win_ptr[v]) T + j is entry j of window w: the
 *   reference's concatenation.  Padded slots keep their place, so p indexes the video's frames_id list.  A padded position
 *   has logit -inf in both channels; a -inf logit in steds means the same.
 * Score.  ls = log_softmax of the start logits over the P_v positions, le alike of the end logits, in td_sted_decode's
 *   arithmetic order (maximum m, sum S of expf(x - m), then (x - m) - logf(S), all fp32, the sums partitioned as there, so
 *   ls and le are td_sted_decode's bit for bit); score(s, e) = ls[s] + le[e], one fp32 addition.
 * Picks.  For k = 0 .. K - 1 the pick is the pair of the largest score among the pairs with
 *     s < e,  a finite score (neither -inf nor NaN),  not an earlier pick and not suppressed by an earlier pick.
 *   Ties are exact (bit-equal fp32 scores) and go to the smallest e, then the smallest s: td_sted_decode's order, torch's.
 * Suppression, in 64-bit integers.  For an earlier pick (a, b): inter = max(0, min(e, b) - max(s, a) + 1),
 *   union = (e - s + 1) + (b - a + 1) - inter; (s, e) is suppressed iff inter * nms_den > nms_num * union.  A temporal IoU
 *   exactly equal to nms_num / nms_den is kept.  nms_num == nms_den suppresses nothing but the picks themselves (plain
 *   top-K); nms_num == 0 suppresses every pair that shares a frame with a pick.
 * Outputs.  count[v] = number of picks made (< K when no admissible pair is left; 0 for a video of fewer than two valid
 *   positions); pairs [n_videos][K][2] int64 and scores [n_videos][K] fp32 hold the picks in order, rows k >= count[v]
 *   hold (-1, -1) and -inf.  Row 0 is td_sted_decode's answer whenever an admissible pair exists.
 * Refused on the host (td_last_error, nothing launched): a null steds / pairs / scores / count; n_videos < 1, T < 1,
 *   max_windows < 1, n_windows < 1 (without win_ptr: n_windows < n_videos); K outside 1 .. 32; nms_den < 1, nms_num < 0 or
 *   nms_num > nms_den; max_windows * T > 3840 (the two log-probability vectors and the per-end best start of a video stay
 *   in LDS for all K rounds: td_sted_decode's bound). */
int td_sted_topk(const float* steds, const unsigned char* valid, const int* win_ptr, int n_videos, int n_windows, int T,
                 int max_windows, int K, int nms_num, int nms_den, long long* pairs, float* scores, int* count,
                 td_stream_t stream);

/* ---- Grounded tubes cropped out of decoded frames (an addition WITHIN ABI 11: nothing above changed) -------------------
 * Takes the object's pixels out of the decoded frames of many clips in ONE launch: per frame the window around the tube's
 * box, resized to a fixed oh x ow - a thumbnail strip, the input of a second-stage model, a mined track.  It is
 * td_clip_resample with the window read on the device, per frame, from the box: no boxes.cpu(), no per-frame job records.
 * Per job:
 *   Source.  T frames of sh x sw in fmt = TD_SRC_RGB24 / TD_SRC_I420 / TD_SRC_NV12: plane0..2, frame_stride, pitch0..2,
 *     matrix, full_range exactly as in td_resample_src_job (odd sizes are legal, chroma planes are (sh + 1) / 2 x (sw + 1) / 2).
 *   Tube.  Device pointers boxes (fp32 [n_tube][4], xyxy in source pixels, required), span (int64 [2], nullable) and
 *     frame_map (int32 [T], nullable), and n_tube: what they are in td_overlay_job.
 *   Geometry.  oh x ow: the output size; margin_num / margin_den: context added on every side as a fraction of the box
 *     side; keep_aspect 0 or 1.
 *   Outputs, device.  dst uint8 [T][3][oh][ow] (required); mask bytes [T][oh][ow], valid bytes [T], windows int32 [T][6]
 *     (each nullable: NULL leaves it out).
 * The rule (this comment is the specification; integers are 64-bit where a product could pass 2^31):
 *   1. Tube row of frame t: r = frame_map ? frame_map[t] : t.
 *   2. The frame is EMPTY when r is outside [0, n_tube), when span is given and r is outside [span[0], span[1]], when a
 *      coordinate of box r is not finite, or when a later step says so.
 *   3. Rounding is td_tube_overlay's: finite values clamped to +-2^20, then x0 = (int)floorf(bx0 + 0.5f), y0, x1, y1 alike, in
 *      fp32.  Empty if x1 <= x0 or y1 <= y0.
 *   4. Margin: bw = x1 - x0, bh = y1 - y0; mx = (bw margin_num) / margin_den, my = (bh margin_num) / margin_den (integer
 *      division); x0 -= mx, x1 += mx, y0 -= my, y1 += my.
 *   5. Clamp to the frame: wx0 = max(x0, 0), wx1 = min(x1, sw), wy0 = max(y0, 0), wy1 = min(y1, sh); cw = wx1 - wx0,
 *      ch = wy1 - wy0.  Empty if cw <= 0 or ch <= 0.
 *   6. Output size.  keep_aspect = 0: rh = oh, rw = ow.  keep_aspect = 1: if cw oh >= ch ow then rw = ow and
 *      rh = min(oh, max(1, (2 ch ow + cw) / (2 cw))), else rh = oh and rw = min(ow, max(1, (2 cw oh + ch) / (2 ch))).
 *   7. Pixels.  For y < rh and x < rw, dst[t][c][y][x] is, byte for byte, what td_clip_resample writes for the job whose
 *      source is the ch x cw sub-image at (wy0, wx0) of the frame (I420 / NV12 frames converted to rgb24 by the integer rule
 *      above first, the chroma sample of source pixel (y, x) being (y >> 1, x >> 1) OF THE FRAME, not of the sub-image), with
 *      flip = 0, virtual size rh x rw, the window all of it, planar = 1, H = oh, W = ow.  Every other byte of the frame's
 *      3 oh ow is 0; mask is 0 inside rh x rw and 1 outside: the collate's bottom / right padding, so the crops have the
 *      uint8 video + mask layout of a staged batch.
 *   8. A frame that is not empty has valid[t] = 1 and windows[t] = (wy0, wx0, ch, cw, rh, rw): the record that maps a
 *      second stage's results back into the frame.
 *   9. An empty frame has pixels all 0, mask all 1, valid[t] = 0 and a window of six zeros.
 * No byte outside the job's dst / mask / valid / windows extents is written; no byte outside the source rows of the job's T
 * frames is read.  One launch for any number of jobs; no allocation, no synchronisation, no atomics.
 * Limits: sh 1..16384; sw 1..8192 (the window can be the whole row: td_clip_resample_src's row bound); oh, ow 1..4096;
 * T >= 0; n_tube >= 1; margin_den 1..1024, margin_num 0..4 margin_den; and two staged rows of sw pixels plus the column table
 * of ow entries must fit 64 KiB of LDS (6 sw + 8 ow <= 65380 is enough: any ow at sw <= 5400, any sw at ow <= 2000; td_clip_resample
 * refuses the same whole-row window for the same reason).  A
 * violation returns an error whose message names the field; nothing is launched.  `jobs` is a host array consumed before the
 * call returns; the job table lives in caller-provided memory as for td_tube_overlay (table_host page-locked, table_dev
 * device memory, both of td_tube_crop_table_bytes(n_jobs) bytes). */
typedef struct td_crop_job {
  const void* plane0; /* rgb24 pixels, or Y */
  const void* plane1; /* I420: U; NV12: UV pairs; RGB24: ignored */
  const void* plane2; /* I420: V; else ignored */
  long long frame_stride;
  int pitch0, pitch1, pitch2;
  int fmt;
  int matrix, full_range; /* I420 / NV12 only */
  int T, sh, sw;
  const float* boxes;
  const long long* span;
  const int* frame_map;
  int n_tube;
  int oh, ow;
  int margin_num, margin_den;
  int keep_aspect;
  void* dst;
  void* mask;
  unsigned char* valid;
  int* windows;
} td_crop_job;
size_t td_tube_crop_table_bytes(int n_jobs);
int td_tube_crop(const td_crop_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* ---- Grounded tubes redacted in decoded frames (an addition WITHIN ABI 11: nothing above changed) ----------------------
 * Hides the answer to a grounding question - or everything but the answer - in the decoded frames of many clips in ONE
 * launch, in the frames' own pixel format: "blur the man in the red jacket", "pixelate the plate the caption describes",
 * or the inverse (a spotlight, bystander privacy).  One job takes the UNION of up to eight tubes.  Per job:
 *   Frames.  Source (src0..2, src_frame_stride, src_pitch0..2) and destination (dst0..2, dst_frame_stride, dst_pitch0..2),
 *     fmt, T, sh, sw exactly as in td_overlay_job: odd sizes are legal, chroma planes are (sh + 1) / 2 x (sw + 1) / 2.  A
 *     destination plane may BE its source plane (same pointer, pitch and frame stride: in place); any other overlap of a
 *     destination plane with a source plane is an error.
 *   Tube.  Device pointers boxes (fp32 [n_tube][K][4], xyxy in source pixels, required), span (int64 [K][2], nullable:
 *     first and last tube row of rectangle k, both inclusive) and frame_map (int32 [T], nullable); n_tube; K in 1..8
 *     rectangles per tube row.
 *   What to do.  mode = TD_REDACT_FILL / TD_REDACT_MOSAIC / TD_REDACT_BLUR; invert 0 or 1; margin_num / margin_den as in
 *     td_crop_job; cell (mosaic: even, 2..256); radius (blur: 1..64); color[3] (fill: three bytes IN THE FRAME'S OWN COLOUR
 *     SPACE, R, G, B or Y, U, V).  The ones the mode does not use are ignored.
 * The rule (this comment is the specification; exact integers, reproducible to the bit):
 *   1. Tube row of frame t: r = frame_map ? frame_map[t] : t.
 *   2. Rectangle k of frame t EXISTS when r is in [0, n_tube), span is NULL or span[k][0] <= r <= span[k][1], all four
 *      coordinates of boxes[r][k] are finite, and the steps below leave it non-empty.
 *   3. Rounding is td_tube_overlay's, in fp32: finite values clamped to +-2^20, then x0 = (int)floorf(bx0 + 0.5f), y0, x1, y1
 *      alike.  Absent if x1 <= x0 or y1 <= y0.
 *   4. Margin is td_tube_crop's step 4: bw = x1 - x0, bh = y1 - y0; mx = (bw margin_num) / margin_den, my = (bh margin_num) /
 *      margin_den (integer division); x0 -= mx, x1 += mx, y0 -= my, y1 += my.
 *   5. Clamp to the frame: wx0 = max(x0, 0), wx1 = min(x1, sw), wy0 = max(y0, 0), wy1 = min(y1, sh).  Absent if wx1 <= wx0
 *      or wy1 <= wy0.
 *   6. Snap outward, the same in all three formats, so that the redacted luma set does not depend on the format and every
 *      existing luma pixel of a 2 x 2 chroma block decides alike.
 *        FILL and BLUR: X0 = wx0 & ~1, X1 = min(wx1 + (wx1 & 1), sw); Y0, Y1 alike with sh.
 *        MOSAIC: X0 = (wx0 / cell) cell, X1 = min(((wx1 + cell - 1) / cell) cell, sw); Y0, Y1 alike with sh.  The grid is
 *        anchored at the frame's origin, not at the box: a moving box does not make the cells crawl.
 *   7. Selection.  Luma pixel (rgb24: pixel) (y, x) is SELECTED iff (it lies in [X0, X1) x [Y0, Y1) of at least one existing
 *      rectangle of its frame) XOR invert.  Chroma sample (i, j) is selected iff luma pixel (2 i, 2 j) is.  So a frame without
 *      a rectangle (r out of range, outside every span, absent boxes) is a plain copy with invert = 0 and selected everywhere
 *      with invert = 1: nothing is left in the clear by accident.
 *   8. Values, per plane and per channel (the three channels of rgb24 are independent, and so are the U bytes and the V bytes
 *      of an NV12 plane).  An unselected byte is the source byte.  A selected byte is
 *        FILL:   color[0] in the Y plane, color[1] for U, color[2] for V; color[c] for channel c of rgb24.
 *        MOSAIC: cp = cell (luma, rgb) or cell / 2 (chroma).  The sample's cell is the cp x cp block of the plane's
 *                origin-anchored grid, cut off at the plane's edge; the value is (sum of the SOURCE samples of the cell +
 *                n / 2) / n, n the number of samples in the cell.
 *        BLUR:   rp = radius (luma, rgb) or (radius + 1) / 2 (chroma).  The value is (sum of the SOURCE samples in
 *                [y - rp, y + rp] x [x - rp, x + rp] that lie in the plane + n / 2) / n, n their count: one exact
 *                two-dimensional sum, no rounding between a horizontal and a vertical pass.
 *   9. Every byte of the rows of the job's destination frames gets the value above; no other byte is written (not the row
 *      padding between the row and the pitch), and no byte outside the source rows is read.
 *  10. In place is legal for FILL and MOSAIC: a workgroup owns whole cells and reads them before it writes.  BLUR reads
 *      neighbours that another workgroup may already have rewritten, so BLUR with a destination plane that is its source
 *      plane is refused with an error that names dst0.
 * Limits: sides 1..16384; T >= 0; n_tube >= 1; K 1..8; cell even, 2..256 (MOSAIC); radius 1..64 (BLUR); margin_den 1..1024,
 * margin_num 0..4 margin_den; boxes non-null.  A violation returns an error whose message names the field; nothing is
 * launched.  `jobs` is a host array consumed before the call returns; the job table lives in caller-provided memory as for
 * td_tube_overlay (table_host page-locked, table_dev device memory, both of td_tube_redact_table_bytes(n_jobs) bytes).  One
 * launch for any number of jobs, which may differ in format, mode and size; no allocation, no synchronisation, no atomics. */
#define TD_REDACT_FILL 0
#define TD_REDACT_MOSAIC 1
#define TD_REDACT_BLUR 2
typedef struct td_redact_job {
  const void* src0; /* rgb24 pixels, or Y */
  const void* src1; /* I420: U; NV12: UV pairs; RGB24: ignored */
  const void* src2; /* I420: V; else ignored */
  long long src_frame_stride;
  int src_pitch0, src_pitch1, src_pitch2;
  void* dst0;
  void* dst1;
  void* dst2;
  long long dst_frame_stride;
  int dst_pitch0, dst_pitch1, dst_pitch2;
  int fmt;
  int T, sh, sw;
  const float* boxes;
  const long long* span;
  const int* frame_map;
  int n_tube;
  int K;
  int mode;
  int invert;
  int margin_num, margin_den;
  int cell;
  int radius;
  unsigned char color[3];
} td_redact_job;
size_t td_tube_redact_table_bytes(int n_jobs);
int td_tube_redact(const td_redact_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* ---- Which kernel a td_conv_gemm / td_linear_ex call would run on (an addition WITHIN ABI 11: nothing above changed) ----
 * The launching calls plan every launch with one host function and then launch the plan; these two run the same planner and
 * return the plan instead.  They touch no device (no HIP call; the epilogue's pointers are only tested for NULL), use the
 * process's dispatch knobs exactly as a launch in the same process would, and take the CU count as an argument (the launching
 * calls pass the current device's).  `routes` has room for 4 records; *n_routes becomes 1, or 4 for a stride-2 3x3 input
 * gradient split by output parity.  An argument the launching call refuses is refused here with the same code and message. */
#define TD_GEMM_KERNEL_TILED 0      /* conv_gemm_kernel */
#define TD_GEMM_KERNEL_PERSISTENT 1 /* pw_resident2_kernel */
#define TD_GEMM_KERNEL_BIG8 2       /* conv_gemm_big8_kernel: 256 x 256 tiles */
#define TD_GEMM_KERNEL_BIG8N 3      /* conv_gemm_big8n_kernel: 256 x 128 tiles */
#define TD_GEMM_WALK_POINTWISE 0
#define TD_GEMM_WALK_TAP_UNIFORM 1
#define TD_GEMM_WALK_GATHER 2
#define TD_GEMM_WALK_GX 3 /* td_linear_ex's two-source rows */
typedef struct td_gemm_route {
  int family;                  /* TD_PROF_* */
  int kernel;                  /* TD_GEMM_KERNEL_* */
  int bm, bn;                  /* tile: output rows x output channels */
  int stages;                  /* tiled kernel: 2 or 3; the others: 0 */
  int walk;                    /* TD_GEMM_WALK_* */
  unsigned grid, block;        /* workgroups, threads per workgroup */
  int dtype;                   /* with the six below: the launch's td_prof_dump record */
  int M, N, K, R, stride, mode;
} td_gemm_route;
int td_conv_gemm_route(const td_conv_desc* d, const td_epilogue* e, int dtype, int n_cu, td_gemm_route* routes, int* n_routes);
/* has_a2: whether the launching call would pass a second source */
int td_linear_ex_route(const td_linear_ex_desc* x, int has_a2, const td_epilogue* e, int dtype, int n_cu, td_gemm_route* routes, int* n_routes);

/* ---- How a td_conv_wgrad_batch call would be laid out on the device (an addition WITHIN ABI 11: nothing above changed) ----
 * td_conv_wgrad_batch plans the whole call with one host function - every argument check included - before it enqueues
 * anything, and then launches the plan; this runs the same planner and returns the plan instead.  It touches no device (no HIP
 * call; the jobs' pointers are only tested for NULL) and uses the process's TD_WGRAD_* knobs as a launch in the same process
 * would; the CU count and the deterministic mode are arguments (the launching call passes the current device's and
 * td_get_deterministic()).  plan_jobs[i] belongs to jobs[i]; `launches` has room for 6 records (3 kernels x 2 phases), in
 * launch order.  An argument the launching call refuses is refused here with the same code and message. */
#define TD_WGRAD_KERNEL_GENERAL 0   /* conv_wgrad_batch_kernel, any geometry */
#define TD_WGRAD_KERNEL_POINTWISE 1 /* conv_wgrad_batch_kernel, 1x1 / stride 1 / no padding */
#define TD_WGRAD_KERNEL_WIDE 2      /* conv_wgrad_wide_batch_kernel */
typedef struct td_wgrad_plan_job {
  int phase;               /* 0: overwriting, 1: accumulating (behind every launch of phase 0) */
  int kernel;              /* TD_WGRAD_KERNEL_* */
  int cls;                 /* wide tiles: bit 0 = 256 output channels per tile, bit 1 = 256 k columns, bit 2 = pointwise */
  int tn, tk;              /* tile grid of the job */
  int splits;              /* reduction splits: the job has tn * tk * splits work items */
  int mper;                /* reduction rows per split */
  int out_mode;            /* 2: plain stores (unsplit and overwriting), 1: fp32 atomics */
  int fill_dw, fill_dbias; /* the library zero-fills dW / dbias ahead of the launches */
  int xcd;                 /* the XCD whose workgroups run the job */
  int first;               /* its first slot (work-item index) inside that XCD */
  int launch;              /* index into `launches` */
  int pos;                 /* row of the job in that launch's table */
} td_wgrad_plan_job;
typedef struct td_wgrad_plan_launch {
  int phase, kernel, n_jobs;
  int start[9];         /* table rows of XCD x: [start[x], start[x + 1]) */
  int slots[8];         /* work items of XCD x */
  unsigned grid, block; /* workgroups (8 x the longest XCD's slots), threads per workgroup */
  int item_stages;      /* stages of 64 (bf16) / 32 (fp32) reduction rows a work item is bounded to */
  double flops, bytes;  /* of the launch's jobs; the profiler records one row per phase, the sums over its launches */
} td_wgrad_plan_launch;
int td_conv_wgrad_batch_plan(const td_wgrad_job* jobs, int n_jobs, int dtype, int n_cu, int deterministic, td_wgrad_plan_job* plan_jobs,
                             td_wgrad_plan_launch* launches, int* n_launches);

/* ---- Grounded tubes interpolated to every decoded frame (an addition WITHIN ABI 11: nothing above changed) -------------
 * The model answers at the sampled rate (one tube row per sampled frame); td_tube_overlay, td_tube_crop and td_tube_redact
 * run on clips decoded at the full rate, and their frame_map can only HOLD the box of one tube row.  This stage turns the
 * tube rows of many clips, in ONE launch, into one box per decoded frame - and optionally one attention map per decoded
 * frame - which the three kernels then take with frame_map = NULL.  Per job:
 *   Inputs, device pointers:
 *     boxes      fp32 [n_tube][K][4], xyxy, required;
 *     span       int64 [K][2]: first and last tube row of rectangle k, both inclusive (as in td_redact_job); NULL: every row;
 *     row_frame  int32 [n_tube]: the frame number at which tube row r was sampled, increasing; NULL: row r sits at
 *                first + r step.  Below, row_frame[r] means either;
 *     heat       uint8 [n_tube][mh][mw]: one attention map per tube row; nullable.
 *   Scalars: n_tube; K in 1..8; T dense frames; t0: dense frame i has frame number f = t0 + i (a long video can be done in
 *     chunks); first, step (used without row_frame); mode = TD_DENSE_HOLD / TD_DENSE_LERP / TD_DENSE_HULL; smooth: a radius
 *     in tube rows, 0..16; mh, mw (with heat).
 *   Outputs, device pointers, each nullable except dense:
 *     dense       fp32 [T][K][4];
 *     valid       bytes [T][K];
 *     dense_span  int64 [K][2];
 *     dense_heat  uint8 [T][mh][mw]: required iff heat is given.
 * The rule (this comment is the specification).  Every fp32 operation below is ONE IEEE operation rounded to nearest even,
 * never contracted into a fused multiply-add, so numpy float32 reproduces it bit for bit; integers are exact.
 *   1. Row r is PRESENT for rectangle k when span is NULL or span[k][0] <= r <= span[k][1], and the four coordinates of
 *      boxes[r][k] are finite.
 *   2. Smoothing.  With smooth = w > 0 the WORKING BOX of a present row r is, per coordinate, the fp32 sum over the present
 *      rows q of [r - w, r + w] that lie in [0, n_tube), added in ascending q to +0.0f, divided once by (float)count.  Absent
 *      rows stay absent.  With w = 0 the working box is the row's box, bits unchanged.
 *   3. For dense frame i, f = t0 + i.  a is the largest r with row_frame[r] <= f and b = a + 1.
 *        f < row_frame[0] or f > row_frame[n_tube - 1]: absent in every mode.
 *        f == row_frame[a]: the working box of row a if it is present, else absent.  No arithmetic.
 *        Otherwise fa = row_frame[a], fb = row_frame[b], num = f - fa, den = fb - fa; den <= 0 or den > 2^24 (a table that
 *        does not increase, or does not keep the promise below): absent.
 *      With a table, a is what this search returns, whatever the table holds: lo = 0, hi = n_tube - 1; while lo < hi:
 *      mid = (lo + hi + 1) >> 1; row_frame[mid] <= f ? lo = mid : hi = mid - 1; a = lo.  No index leaves [0, n_tube).
 *   4. Modes, for a frame strictly between row a and row b; A and B are their working boxes.
 *        HOLD: A if a is present, else absent: what frame_map does today.
 *        LERP: both present: wgt = (float)num / (float)den, v = A + wgt * (B - A) per coordinate: one division, one
 *              subtraction, one multiplication, one addition, each rounded to fp32.  Otherwise absent.
 *        HULL: both present: (min(A0, B0), min(A1, B1), max(A2, B2), max(A3, B3)), min(x, y) being y < x ? y : x and max(x, y)
 *              y > x ? y : x.  Exactly one present: that row's working box.  Neither: absent.  The conservative cover for a
 *              redaction: whatever moves in a straight line between two samples stays inside.
 *   5. An absent (i, k) writes four quiet NaNs of bit pattern 0x7FC00000 and valid = 0; td_tube_overlay, td_tube_crop and
 *      td_tube_redact treat a non-finite box as absent, so they need no span.  A computed box with a coordinate that is not
 *      finite (an overflow) is written as computed, a NaN among them as 0x7FC00000, with valid = 0.  Otherwise valid = 1.
 *   6. dense_span[k], in dense indices: s0 = max(span[k][0], 0), s1 = min(span[k][1], n_tube - 1) (NULL span: 0 and
 *      n_tube - 1).  s0 > s1: (0, -1).  HOLD and LERP: (row_frame[s0] - t0, row_frame[s1] - t0).  HULL covers the open
 *      intervals that its one-sided hold fills: the start is row_frame[s0 - 1] + 1 - t0 when s0 > 0, the end
 *      row_frame[s1 + 1] - 1 - t0 when s1 < n_tube - 1.  Not clamped to [0, T): it is what td_overlay_job takes as span.
 *   7. Heat, when given, for every byte of the map; it ignores span and smoothing.  Before the first or after the last row,
 *      or a refused den: 0.  f == row_frame[a]: row a's byte qa.  In between, with qb row b's byte: HOLD: qa; LERP:
 *      (qa (den - num) + qb num + den / 2) / den in integers; HULL: max(qa, qb).
 * Refused on the host with a message that names the field (nothing is launched): boxes or dense NULL; n_tube < 1; K outside
 * 1..8; T < 0 or T > 2^20; |t0| > 2^23; |first| > 2^23 and step outside 1..2^16 (both without row_frame only); smooth
 * outside 0..16; an unknown mode; heat without dense_heat or the reverse; mh, mw outside 1..256 (with heat).  The frame
 * numbers in row_frame are the caller's promise to lie within +-2^23: the int -> float conversions are then exact.  A job
 * with T = 0 is legal and writes only dense_span.  `jobs` is a host array consumed before the call returns; the job table
 * lives in caller-provided memory as for td_tube_overlay (table_host page-locked, table_dev device memory, both of
 * td_tube_densify_table_bytes(n_jobs) bytes).  One launch for any number of jobs of mixed modes; no allocation, no
 * synchronisation, no atomics: the same call returns the same bits.  No byte outside the job's outputs is written. */
#define TD_DENSE_HOLD 0
#define TD_DENSE_LERP 1
#define TD_DENSE_HULL 2
typedef struct td_dense_job {
  const float* boxes;
  const long long* span;
  const int* row_frame;
  const unsigned char* heat;
  int n_tube;
  int K;
  int T;
  int t0;
  int first, step;
  int mode;
  int smooth;
  int mh, mw;
  float* dense;
  unsigned char* valid;
  long long* dense_span;
  unsigned char* dense_heat;
} td_dense_job;
size_t td_tube_densify_table_bytes(int n_jobs);
int td_tube_densify(const td_dense_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* ---- K labelled tubes and a moment timeline drawn in one pass (an addition WITHIN ABI 11: nothing above changed) ---------
 * td_tube_overlay draws one tube in one colour, and two of its jobs cannot share destination frames.  This entry point draws
 * the K <= 8 tubes of a clip (K sentences, or the K best moments of one) into the frames in ONE pass: every tube in its own
 * colour with a label, and a timeline strip at the bottom that shows where the K spans lie and where the frame is.
 * The frames side of a job - src0..2, dst0..2, pitches, frame strides, fmt, T, sh, sw, in place or apart, odd sizes - is
 * td_overlay_job's, word for word: every byte of the rows of the job's destination frames gets the value defined below, no
 * other byte is written and no byte outside the source rows is read.
 * Inputs, device pointers, each nullable (NULL leaves its layers out):
 *   boxes      fp32 [n_tube][K][4], xyxy in source pixels (td_redact_job's layout);
 *   span       int64 [K][2]: first and last tube row of tube k, both inclusive; NULL: every row lies in every span;
 *   frame_map  int32 [T], heat uint8 [n_tube][mh][mw], heat_alpha, heat_color, dim_alpha, dim_color, thickness, n_tube:
 *              what they are in td_overlay_job;
 *   tube_color[k]: the colour of tube k, tag_text_color, bar_color, cursor_color: three bytes IN THE FRAME'S OWN COLOUR SPACE;
 *   tags       uint8 [K][tag_h][tag_w]: one alpha bitmap (a label) per tube, shared by all frames; needs boxes; with tag_h in
 *              1..32, tag_w in 1..256, tag_scale in 1..8 (a bitmap sample covers tag_scale x tag_scale pixels) and tag_alpha
 *              in [0, 256] (the plate under the label);
 *   lane_h     0: no timeline; else 1..64, the height of a tube's lane; needs 1 <= n_tube <= 2^20 and K lane_h <= sh; with
 *              bar_alpha and seg_alpha in [0, 256].
 * The rule (exact integers, reproducible to the bit).  As in td_tube_overlay a frame is a stack of layers; a layer gives every
 * luma pixel (rgb24: every pixel) an alpha a in [0, 256] and has ONE colour c, and a byte v becomes
 * (v (256 - a) + c a + 128) >> 8.  r is the tube row of frame t (frame_map[t], or t).  A frame whose r is outside [0, n_tube) is
 * a plain copy (no timeline either).  Else, in this order (a pixel outside a layer's area has a = 0 there):
 *   1. dim, only when span is given and r lies outside EVERY tube's span: a = dim_alpha everywhere, c = dim_color.
 *   2. heat, whenever heat is given: td_tube_overlay's step 2, word for word; c = heat_color.
 *   3. box k, for k = 0 .. K - 1 in this order, only when boxes is given, r lies in span k (no span: always) and box
 *      boxes[r][k] is present: its corners are rounded as in td_tube_overlay's step 3 (fp32, finite values clamped to +-2^20,
 *      x0 = (int)floorf(bx0 + 0.5f), y0, x1, y1 alike; a non-finite coordinate, x1 <= x0 or y1 <= y0: absent).  a = 256 for a
 *      pixel in [x0, x1) x [y0, y1) that is not in [x0 + th, x1 - th) x [y0 + th, y1 - th), c = tube_color[k].
 *   4. tag k, for k = 0 .. K - 1 in this order, after ALL boxes, only where box k was drawn in step 3 and tags is given.  The
 *      plate is PW = tag_w tag_scale pixels wide and PH = tag_h tag_scale high, at px0 = x0 and py0 = y0 - PH when that is
 *      >= 0, else py0 = y0 (above the box; inside it when there is no room above).  Two layers on the pixels of
 *      [px0, px0 + PW) x [py0, py0 + PH):
 *        a. the plate: a = tag_alpha, c = tube_color[k];
 *        b. the glyph: m = tags[k][(y - py0) / tag_scale][(x - px0) / tag_scale], a = (256 m + 127) / 255, c = tag_text_color.
 *   5. the timeline, last, only when lane_h > 0: the strip is rows [sh - K lane_h, sh), lane k is rows
 *      [sh - (K - k) lane_h, sh - (K - k - 1) lane_h), and column x stands for tube row i(x) = floor(x n_tube / sw) (64-bit).
 *        a. the bar: a = bar_alpha on the whole strip, c = bar_color;
 *        b. segment k, for k = 0 .. K - 1 in this order: a = seg_alpha on the pixels of lane k whose i(x) lies in span k (no
 *           span: all of them), c = tube_color[k];
 *        c. the cursor: a = 256 on columns [xc0, xc1) of the whole strip, xc0 = floor(r sw / n_tube),
 *           xc1 = max(floor((r + 1) sw / n_tube), xc0 + 1), c = cursor_color.
 * The parts of any layer outside the frame are simply absent.  A chroma sample (I420 / NV12) takes, PER LAYER, the mean alpha
 * of the luma pixels of its 2 x 2 block that exist, (sum + n / 2) / n with n in {1, 2, 4}, and is blended with the U / V byte
 * of that layer's colour - which is why the bar, each segment and the cursor are layers of their own.
 * Two identities follow.  With K = 1, no tags, lane_h = 0 and tube_color[0] = box_color the result is td_tube_overlay's, byte
 * for byte.  With no dim, heat, tags and timeline the result for K tubes is that of K in-place td_tube_overlay passes, k
 * ascending, each with tube k's boxes, span and colour.
 * Limits: td_overlay_job's, K in 1..8, and those named with the inputs above.  A violation returns an error whose message names
 * the field; nothing is launched.  `jobs` is a host array consumed before the call returns; the job table lives in
 * caller-provided memory as for td_tube_overlay (table_host page-locked, table_dev device memory, both of
 * td_tube_overlay_multi_table_bytes(n_jobs) bytes).  One launch for any number of jobs of mixed formats and K; no allocation,
 * no synchronisation inside. */
typedef struct td_overlay_multi_job {
  const void* src0; /* rgb24 pixels, or Y */
  const void* src1; /* I420: U; NV12: UV pairs; RGB24: ignored */
  const void* src2; /* I420: V; else ignored */
  long long src_frame_stride;
  int src_pitch0, src_pitch1, src_pitch2;
  void* dst0;
  void* dst1;
  void* dst2;
  long long dst_frame_stride;
  int dst_pitch0, dst_pitch1, dst_pitch2;
  int fmt;
  int T, sh, sw;
  const float* boxes;
  const long long* span;
  const int* frame_map;
  const unsigned char* heat;
  const unsigned char* tags;
  int n_tube;
  int K;
  int mh, mw;
  int thickness;
  int heat_alpha, dim_alpha;
  int tag_h, tag_w, tag_scale, tag_alpha;
  int lane_h, bar_alpha, seg_alpha;
  unsigned char tube_color[8][3];
  unsigned char heat_color[3], dim_color[3], tag_text_color[3], bar_color[3], cursor_color[3];
} td_overlay_multi_job;
size_t td_tube_overlay_multi_table_bytes(int n_jobs);
int td_tube_overlay_multi(const td_overlay_multi_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* ---- Shot cuts in decoded frames (an addition WITHIN ABI 11: nothing above changed) -------------------------------------
 * Every stage above takes a clip for one continuous take.  Across a hard cut td_tube_densify slides (LERP) or blows up (HULL)
 * a box between two unrelated scenes.  Three entry points make the cuts visible: td_frame_stats reads the pixels once,
 * td_shot_cuts decides on its statistics, td_tube_densify_shots stops at the result.  All of it is integers.
 *
 * td_frame_stats.  Per job (one clip):
 *   src0..2, src_pitch0..2, src_frame_stride, fmt, T, sh, sw: the source side of td_overlay_job, word for word (every plane of
 *     the format is described and checked, although the chroma planes are never read);
 *   step in 1..8;
 *   hist  uint32 [T][64], sad  uint32 [T]: device pointers, either nullable, not both.
 * The rule (this comment is the specification):
 *   The SAMPLED pixels are (y, x) with y % step == 0 and x % step == 0; N = ceil(sh / step) * ceil(sw / step) of them.
 *   The luma L of a sampled pixel: I420 and NV12: the Y byte as stored, no range conversion; RGB24: (77 R + 150 G + 29 B + 128) >> 8.
 *   hist[t][b] = the number of sampled pixels of frame t with L >> 2 == b.
 *   sad[t]     = the sum over the sampled pixels of |L_t - L_(t-1)|; sad[0] = 0.  sad[t] == 0: frame t repeats frame t - 1.
 * Refused on the host with a message that names the field (nothing is launched): an unknown fmt; T < 0; sh, sw outside
 * 1..16384; sh * sw > 2^24 (which keeps sad below 2^32); step outside 1..8; hist and sad both NULL; every violation of a plane
 * (null, pitch below the row, frame stride below the plane) in td_tube_overlay's words.  T = 0 is legal and writes nothing.
 * One launch serves any number of jobs of mixed formats, sizes and steps.  The outputs are zeroed inside the call, on the
 * stream, so the result does not depend on what they held; the sums are integer atomics, so the same call returns the same
 * bits.  No allocation, no synchronisation, no byte outside the outputs is written.  A long video done in chunks overlaps
 * them by ONE frame: sad of a chunk's first frame is 0 by definition, so the chunk behind starts at the last frame of the
 * chunk in front and drops its own row 0.  Job table: as for td_tube_overlay, td_frame_stats_table_bytes(n_jobs) bytes. */
typedef struct td_stats_job {
  const void* src0; /* rgb24 pixels, or Y */
  const void* src1; /* I420: U; NV12: UV pairs; RGB24: ignored */
  const void* src2; /* I420: V; else ignored */
  long long src_frame_stride;
  int src_pitch0, src_pitch1, src_pitch2;
  int fmt;
  int T, sh, sw;
  int step;
  unsigned* hist;
  unsigned* sad;
} td_stats_job;
size_t td_frame_stats_table_bytes(int n_jobs);
int td_frame_stats(const td_stats_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* td_shot_cuts consumes the statistics and touches no pixels.  Per job:
 *   hist  uint32 [T][64], sad  uint32 [T]: what td_frame_stats wrote, both required; T in 0..2^20; N in 1..2^24, the number
 *     of sampled pixels (every row of hist sums to it);
 *   thresholds as integer fractions, numerators in 0..2^20, denominators in 1..2^20: hist_num / hist_den (the Python layer's
 *     default: 1/4), sad_num / sad_den (8/1), peak_num / peak_den (3/1); w in 0..16 (4);
 *   outputs, device pointers: d uint32 [T] (nullable), cut bytes [T], shot int32 [T], n_shots int32 [1].
 * The rule.  d[0] = 0 and d[t] = sum_b |hist[t][b] - hist[t-1][b]| (uint32; at most 2 N).  Frame t >= 1 starts a new shot,
 * cut[t] = 1, iff all four hold, in 64-bit integers:
 *   1. d[t] * hist_den > hist_num * 2 N;
 *   2. sad[t] * sad_den > sad_num * N;
 *   3. d[t] is a local peak over the neighbours Q = {q != t : max(1, t - w) <= q <= min(T - 1, t + w)}: d[q] < d[t] for
 *      q < t and d[q] <= d[t] for q > t.  Of equal neighbours the earliest wins: at most one cut per w + 1 frames;
 *   4. Q is empty, or d[t] * peak_den * |Q| > peak_num * sum_{q in Q} d[q].
 * Else cut[t] = 0; cut[0] = 0.  shot[t] = the inclusive prefix sum of cut; n_shots = shot[T - 1] + 1, or 0 for T = 0.
 * Both gates are needed: the histogram gate alone fires on a fade, the difference gate alone on fast motion.  Known limit: a
 * one-frame flash gives ONE cut, at its first frame (the frame behind it has an equal or lower d, and the earliest wins).  Gradual transitions
 * are not cuts.  The defaults are starting values that were tried on synthetic clips only: no footage has validated them.
 * Refused on the host, naming the field: hist, sad, cut, shot or n_shots NULL; T, N, w, a numerator or a denominator outside
 * its range.  One workgroup per job, one launch for any number of jobs; no allocation, no synchronisation, no atomics. */
typedef struct td_cuts_job {
  const unsigned* hist;
  const unsigned* sad;
  int T;
  int N;
  int hist_num, hist_den;
  int sad_num, sad_den;
  int peak_num, peak_den;
  int w;
  unsigned* d;
  unsigned char* cut;
  int* shot;
  int* n_shots;
} td_cuts_job;
size_t td_shot_cuts_table_bytes(int n_jobs);
int td_shot_cuts(const td_cuts_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* td_tube_densify_shots: td_tube_densify that stops at shot cuts.  jobs[i] is a td_dense_job, unchanged; shots[i] says which
 * shot every frame number lies in:
 *   shot     int32 [shot_T] on the device (td_shot_cuts' `shot`); NULL: no shots for this job;
 *   shot_t0  the frame number of shot[0]; shot_T in 0..2^20.
 * Frame number f has shot id shot[f - shot_t0] when 0 <= f - shot_t0 < shot_T; outside that range, or with shot NULL, its
 * shot is UNKNOWN, which matches every shot.  So a caller densifying in chunks hands the whole video's array to every chunk,
 * and chunked equals unchunked.  Two frame numbers are IN ONE SHOT when their shots match.
 * The rule is td_tube_densify's, with these extensions (its step numbers):
 *   1'. Row r is USABLE for frame f when it is present (step 1) and row_frame[r] and f are in one shot.
 *   2'. The smoothing window of row r takes only the present rows q with row_frame[q] and row_frame[r] in one shot.
 *   3', 4'. A frame on a row (f == row_frame[a]) is as before.  Strictly between rows a and b:
 *        a and b both in one shot with f: step 4 as it stands (HULL's one-sided case included);
 *        exactly one of them in one shot with f - a cut lies between f and the other: that row's working box if the row is
 *          present, else absent, in EVERY mode (HOLD and LERP gain HULL's one-sided case at a cut);
 *        neither (two cuts inside one interval, f between them): absent.
 *      An absent row never becomes a one-sided hold in HOLD and LERP while its neighbour is in the same shot: with every
 *      shot unknown the result is td_tube_densify's, bit for bit.
 *   7'. Heat ignores presence as before: both rows in one shot with f: step 7; one: that row's byte; neither: 0.
 *   dense_span (step 6) is unchanged.
 * td_tube_densify IS this entry point with shots = NULL: one kernel.  `shots` may be NULL (then every job has none).  Refused:
 * what td_tube_densify refuses, in its words but under this name, and shot_T outside 0..2^20 or |shot_t0| > 2^23 with a shot
 * array.  The job table is td_tube_densify's: td_tube_densify_shots_table_bytes(n_jobs) == td_tube_densify_table_bytes(n_jobs) bytes. */
typedef struct td_dense_shots {
  const int* shot;
  int shot_t0;
  int shot_T;
} td_dense_shots;
size_t td_tube_densify_shots_table_bytes(int n_jobs);
int td_tube_densify_shots(const td_dense_job* jobs, const td_dense_shots* shots, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* ---- Boxes that follow the object's pixels between sampled frames (an addition WITHIN ABI 11: nothing above changed) -----
 * td_tube_densify fills the decoded frames between two sampled ones by arithmetic on the boxes alone; an object does not move
 * on a straight line between two samples.  td_tube_follow is the stage between td_tube_densify and td_tube_overlay /
 * td_tube_crop / td_tube_redact: it looks at the pixels and moves every in-between box onto the object by block matching
 * against the nearest sampled frame.  Per job (one clip):
 *   src0..2, src_pitch0..2, src_frame_stride, fmt, T, sh, sw: the source side of td_overlay_job, word for word (every plane of
 *     the format is described and checked, although the chroma planes are never read);
 *   K in 1..8;
 *   boxes   fp32 [T][K][4], xyxy in source pixels, one box per decoded frame and tube: what td_tube_densify writes (four NaNs:
 *           absent);
 *   anchor  bytes [T]: non-zero - the boxes of this frame are the model's own (a sampled frame);
 *   shot    int32 [T], nullable: td_shot_cuts' `shot` for these same T frames;
 *   radius  R in 0..16; reach in 1..64; accept_num in 0..2^20, accept_den in 1..2^20;
 *   outputs, device pointers: out fp32 [T][K][4] (required); offset int32 [T][K][2] as (dy, dx), cost uint32 [T][K] and status
 *           bytes [T][K], each nullable.  out may BE boxes: a unit (t, k) reads only its own box and anchor boxes, writes only
 *           its own, and an anchor box is never changed (it is written back with its own bits).
 * The luma L of pixel (y, x) is td_frame_stats': I420 and NV12: the Y byte as stored; RGB24: (77 R + 150 G + 29 B + 128) >> 8.
 * The rule for frame t and tube k, B = boxes[t][k] (this comment is the specification; all integers except step 8):
 *   1. COPIED (status 0) when anchor[t] != 0 or a coordinate of B is not finite: out gets B's bit patterns, offset (0, 0),
 *      cost 0, status 0.  Every later "copied" means the same.
 *   2. The anchor frame g: for d = 1 .. reach in this order, q = t - d and then q = t + d; the first q qualifies with
 *      0 <= q < T, anchor[q] != 0, every coordinate of boxes[q][k] finite and, with shot given, shot[q] == shot[t].  The nearer
 *      anchor wins, of two equally near the earlier.  None qualifies: copied.
 *   3. Rounding is td_tube_overlay's (finite values clamped to +-2^20, then (int)floorf(v + 0.5f) in fp32), applied to the anchor
 *      box, (ax0, ay0, ax1, ay1), and to B, (bx0, by0, bx1, by1).
 *   4. The template: x0 = max(ax0, 0), y0 = max(ay0, 0), x1 = min(ax1, sw), y1 = min(ay1, sh); w = x1 - x0, h = y1 - y0; w <= 0
 *      or h <= 0: copied.  The 16 x 16 sample points are px[j] = x0 + ((2 j + 1) w) / 32 and py[i] = y0 + ((2 i + 1) h) / 32
 *      (integer divisions; always inside the clamped box), and tem[i][j] = L of frame g at (py[i], px[j]).
 *   5. The predicted shift: ddx = ((bx0 + bx1) - (ax0 + ax1)) >> 1, ddy alike from the y's, on the UNCLAMPED rounded corners;
 *      >> is the arithmetic shift, which floors.
 *   6. The candidates are (dy, dx) with -R <= dy, dx <= R, and
 *      c(dy, dx) = sum_{i,j} | L_t(clamp(py[i] + ddy + dy, 0, sh - 1), clamp(px[j] + ddx + dx, 0, sw - 1)) - tem[i][j] |,
 *      at most 65 280.  Clamping to the frame's edge keeps every candidate defined.
 *   7. The best candidate has the smallest c; ties go to the smallest dy^2 + dx^2, then the smallest dy, then the smallest dx
 *      (so a flat picture answers (0, 0)).  cost = that c.
 *   8. ACCEPTED (status 1) iff c * accept_den <= accept_num * 256 in 64-bit integers (accept_num / accept_den grey levels per
 *      sample): offset = (dy, dx) and out = (B.x0 + (float)dx, B.y0 + (float)dy, B.x1 + (float)dx, B.y1 + (float)dy), each ONE
 *      fp32 addition; with dy = dx = 0 B's bits are copied.  REJECTED (status 2) otherwise: out gets B's bits, offset (0, 0),
 *      and cost keeps c.
 * Translation only: the template keeps the anchor's scale.  Every frame is matched against an anchor, never against its
 * neighbour: nothing drifts, and every (t, k) is independent of every other.  A long video done in chunks overlaps them by
 * `reach` frames.  A rejected match (an occlusion, the object leaving the frame) leaves the interpolated box.  The Python
 * layer's default for accept (24 / 1) is a starting value: nobody has tried it on real footage.
 * Refused on the host with a message that names the field (nothing is launched): every violation of a plane (null, pitch
 * below the row, frame stride below the plane) in td_tube_overlay's words; an unknown fmt; T < 0; sh, sw outside 1..16384; K,
 * radius, reach, accept_num or accept_den outside its range; boxes, anchor or out NULL.  T = 0 is legal and writes nothing.
 * One launch serves any number of jobs of mixed formats, sizes, K and radius.  Job table: as for td_tube_overlay,
 * td_tube_follow_table_bytes(n_jobs) bytes.  No allocation, no synchronisation, no atomics; the same call returns the same bits. */
typedef struct td_follow_job {
  const void* src0; /* rgb24 pixels, or Y */
  const void* src1; /* I420: U; NV12: UV pairs; RGB24: ignored */
  const void* src2; /* I420: V; else ignored */
  long long src_frame_stride;
  int src_pitch0, src_pitch1, src_pitch2;
  int fmt;
  int T, sh, sw;
  int K;
  const float* boxes;
  const unsigned char* anchor;
  const int* shot;
  int radius, reach;
  int accept_num, accept_den;
  float* out;
  int* offset;
  unsigned* cost;
  unsigned char* status;
} td_follow_job;
size_t td_tube_follow_table_bytes(int n_jobs);
int td_tube_follow(const td_follow_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

/* ---- Rendered frames exported: cut, downscaled, converted (an addition WITHIN ABI 11: nothing above changed) --------------
 * The last stage of the render chain: the frames that td_tube_overlay / td_tube_redact wrote become what an encoder or a browser
 * takes - only the frames of the answer, smaller, in another pixel format, padded to even sides (the reference's demo decodes
 * to rgb24 and writes yuv420p with pad=ceil(iw/2)*2:ceil(ih/2)*2: demo_stvg.py:95,193).  One pass, and it decides how many
 * bytes cross to the host.  Per job (this comment is the specification; everything is exact integers):
 *   Source: T frames of sh x sw in src_fmt = TD_SRC_RGB24 / TD_SRC_I420 / TD_SRC_NV12; src0..2, src_pitch0..2 and
 *     src_frame_stride as in td_overlay_job (odd sizes are legal, chroma planes are (sh + 1) / 2 x (sw + 1) / 2).
 *   Colour: matrix and full_range describe whichever side is yuv; with both sides yuv they describe both, so a yuv -> yuv job
 *     never changes matrix or range.  An rgb24 -> rgb24 job ignores them.
 *   Frames: To output frames.  take = NULL: To must equal T and output frame i is source frame i.  Else take is a device int32
 *     [To] and output frame i is source frame take[i]; an entry outside [0, T) makes output frame i a BLANK frame.  valid, device
 *     bytes [To], nullable: 1 for a taken frame, 0 for a blank one.
 *   Picture: oh x ow with 1 <= oh <= sh and 1 <= ow <= sw - the same size or smaller; nothing is enlarged.
 *   Destination: dst_fmt, dst0..2, dst_pitch0..2, dst_frame_stride describe To frames of dh x dw with dh >= oh, dw >= ow (chroma
 *     planes (dh + 1) / 2 x (dw + 1) / 2).  The picture sits at the top left; every other sample of a frame, and every sample of
 *     a blank frame, is pad: three bytes in the DESTINATION's colour space (R, G, B; or luma pad[0], U pad[1], V pad[2]).  A
 *     chroma sample (cy, cx) with cy < (oh + 1) / 2 and cx < (ow + 1) / 2 belongs to the picture, the others are pad.  The
 *     destination must not overlap the source: there is no export in place.
 * The rule is a composition of three stages.
 *   A. Area resize of a plane of n_y x n_x samples to m_y x m_x (m <= n), per channel.  Along one axis output sample j takes
 *      source sample i with weight w(j, i) = max(0, min((j + 1) n, (i + 1) m) - max(j n, i m)); the weights of one j sum to n.
 *      With D = n_y n_x and S = sum over y and x of wy wx v, the value is (S + (D >> 1)) / D (integer division).  Equal sizes
 *      give an exact copy; an exact 2:1 gives the rounded 2 x 2 mean (S' + 2) >> 2.
 *   B. yuv -> rgb of a pixel: td_clip_resample_src's rule, unchanged - chroma sample (y >> 1, x >> 1) and the 16-bit
 *      coefficient table above.
 *   C. rgb -> yuv of a picture of h x w pixels.  Luma of pixel (y, x): td_tube_overlay's colour rule (color_in_space),
 *      Y = clamp((yr R + yg G + yb B + 2^20 yo + 2^19) >> 20) with the round(2^20 x) coefficients given there.  Chroma sample
 *      (cy, cx) covers the n = 1, 2 or 4 pixels of its 2 x 2 block that exist (an odd last row or column has fewer: centre
 *      siting); with Rs, Gs, Bs their sums, U = clamp((ur Rs + ug Gs + ub Bs + n (2^20 128 + 2^19)) >> (20 + log2 n)), V alike
 *      (>> = floor division, clamp to [0, 255]).  Every accumulator lies in [0, 2^30]; a solid colour gives exactly
 *      color_in_space(colour); the result is within 0.5004 of a level of the float64 formula applied to the block's mean.
 * By format pair:
 *   rgb24 -> rgb24   A on the three channels (sh x sw -> oh x ow);
 *   yuv -> yuv       (I420 / NV12 in any combination) A on the Y plane (sh x sw -> oh x ow) and on the U and the V plane
 *                    independently ((sh + 1) / 2 x (sw + 1) / 2 -> (oh + 1) / 2 x (ow + 1) / 2); I420 <-> NV12 is only packing,
 *                    and at equal size the job repacks byte for byte;
 *   rgb24 -> yuv     A, rounded to bytes, then C on the oh x ow picture;
 *   yuv -> rgb24     B on every source pixel, then A.
 * Limits: sh 1..16384; sw 1..8192; dh, dw 1..16384; T >= 0, To >= 0 (To = 0 writes nothing; T = 0 makes every taken frame
 * blank).  A job that resizes (oh != sh or ow != sw) needs sh sw <= 2^24, so that S + (D >> 1) <= 255.5 x 2^24 < 2^32 fits
 * unsigned 32 bits; a same-size job has no such bound.  LDS: a workgroup stages, per source row, the columns under 256
 * output columns, and needs 9216 + 3 min(sw, ceil(256 sw / ow) + 1) + 24 <= 65536 bytes (rgb24; a yuv source needs less) - an
 * inequality that every sw <= 8192 satisfies, so the bound on sw is the only one: every resizing job with ow <= 4096 and every
 * same-size job up to sw = 8192 is admitted.  A violation returns an error whose message names the field (ow / oh for an
 * enlargement, "sh * sw", dh / dw, To, the plane fields in td_tube_overlay's words, "overlaps"); nothing is launched.
 * No byte outside the job's destination rows of its To frames and of valid is written (not the row padding between the row and
 * the pitch); no byte outside the source rows of the taken frames is read.  One launch serves any number of jobs of mixed
 * formats and sizes.  Job table: as for td_tube_overlay, td_frame_export_table_bytes(n_jobs) bytes.  No allocation, no
 * synchronisation, no atomics; the same call returns the same bits. */
typedef struct td_export_job {
  const void* src0; /* rgb24 pixels, or Y */
  const void* src1; /* I420: U; NV12: UV pairs; RGB24: ignored */
  const void* src2; /* I420: V; else ignored */
  long long src_frame_stride;
  int src_pitch0, src_pitch1, src_pitch2;
  int src_fmt;
  int matrix, full_range;
  int T, sh, sw;
  const int* take;
  int To;
  int oh, ow;
  void* dst0;
  void* dst1;
  void* dst2;
  long long dst_frame_stride;
  int dst_pitch0, dst_pitch1, dst_pitch2;
  int dst_fmt;
  int dh, dw;
  unsigned char pad[3];
  unsigned char* valid;
} td_export_job;
size_t td_frame_export_table_bytes(int n_jobs);
int td_frame_export(const td_export_job* jobs, int n_jobs, void* table_host, void* table_dev, size_t table_bytes, td_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
