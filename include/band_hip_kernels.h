/*
 * band_hip_kernels.h — thin C ABI between the host-side HIP backend
 * (band_amd/csrc/backend/hip/) and the hand-written gfx950 kernels.
 *
 * This is the "Thin C ABI (build-internal)" of SURVEY.md §8(b): plain
 * pointers, sizes and POD parameter blocks, no C++ or torch types.  Every
 * entry point returns 0 on success or a hipError_t value (>0), or BH_EINVAL
 * (-1) for a parameter block that fails host-side validation.  Launch entry
 * points are asynchronous on the given stream (nullptr = the calling
 * thread's current-device null stream is NOT used: pass a real stream).
 *
 * Each op launcher stands in for one TFLite 2.9.2 builtin kernel that
 * `tflite::Interpreter::Invoke` dispatches from the reference hot path
 * `TfLiteModelExecutor::ExecuteSubgraph` (band/backend/tfl/model_executor.cc:249-255):
 *   bh_conv2d_i8      <- CONV_2D            (reference_integer_ops::ConvPerChannel,
 *                                            reference_ops::Conv uint8)
 *   bh_conv2d_grouped_i8 <- CONV_2D whose filter has fewer input channels than the input
 *                                            (the same two kernels, groups = in_c / filter_in_c)
 *   bh_dwconv2d_i8    <- DEPTHWISE_CONV_2D  (reference_integer_ops::DepthwiseConvPerChannel)
 *   bh_fc_i8          <- FULLY_CONNECTED    (reference_integer_ops::FullyConnected)
 *   bh_eltwise_i8     <- ADD / SUB / MUL    (reference_integer_ops::Add / Mul, sub.cc)
 *   bh_pool_i8        <- AVERAGE_POOL_2D / MAX_POOL_2D (reference_integer_ops::{Average,Max}Pool)
 *   bh_irb_i8         <- [CONV_2D 1x1 ->] DEPTHWISE_CONV_2D 3x3 -> CONV_2D 1x1 [-> ADD], fused
 *   bh_chain_i8       <- DEPTHWISE_CONV_2D 3x3 -> CONV_2D 1x1 [-> ADD] [-> CONV_2D 1x1], fused
 *   bh_lut_u8         <- QUANTIZE (8-bit -> 8-bit), RELU / RELU6 / RELU_N1_TO_1, LOGISTIC
 *   bh_lut_f32        <- DEQUANTIZE (8-bit -> float32)
 *   bh_quantize_f32   <- QUANTIZE (float32 -> 8-bit, reference_ops::AffineQuantize)
 *   bh_concat         <- CONCATENATION      (reference_ops::Concatenation[WithScaling])
 *   bh_pad            <- PAD / PADV2        (reference_ops::Pad)
 *   bh_resize_nearest <- RESIZE_NEAREST_NEIGHBOR (reference_ops::ResizeNearestNeighbor)
 *   bh_resize_bilinear_i8 <- RESIZE_BILINEAR int8 (reference_ops::ResizeBilinearInteger)
 *   bh_resize_bilinear_u8 <- RESIZE_BILINEAR uint8 (optimized_ops::ResizeBilinear, float path)
 *   bh_softmax_i8     <- SOFTMAX 8-bit      (optimized_ops::Softmax, lookup-table path)
 *   bh_mean           <- MEAN               (optimized_integer_ops::Mean / optimized_ops::Mean)
 *   bh_mean_rows      <- MEAN 8-bit over the last axis (reference_ops::Mean / QuantizedMeanOrSum)
 *   (SQUARED_DIFFERENCE int8 runs through bh_eltwise_i8, BH_ELT_SQDIFF; RSQRT int8 and
 *    GELU 8-bit as bh_lut_u8 tables; GELU float32 through bh_unary_f32)
 *   bh_argminmax      <- ARG_MAX / ARG_MIN  (reference_ops::ArgMinMax: first extreme, strict compare)
 *   bh_resize_bilinear_argminmax_i8 <- RESIZE_BILINEAR int8 -> ARG_MAX / ARG_MIN over channels, fused
 *   bh_reindex        <- TRANSPOSE, STRIDED_SLICE, SLICE, SPLIT, SPLIT_V, SPACE_TO_DEPTH,
 *                        DEPTH_TO_SPACE, UNPACK, TILE (one launch per output; numpy's indexing
 *                        semantics; PACK runs through bh_concat)
 *   bh_gather         <- GATHER (np.take along one axis; the indices may be a runtime tensor)
 *   bh_batch_matmul_i8 / bh_batch_matmul_f32 <- BATCH_MATMUL int8 / float32 (the arithmetic of
 *                        reference_integer_ops::FullyConnected without a bias, per batch slice)
 *   bh_dynquant_rows + bh_fc_hybrid <- FULLY_CONNECTED float32 with int8 weights (fully_connected.cc
 *                        EvalHybrid: each input row quantised at run time, int8 product, float epilogue)
 *   bh_dynquant_items + bh_conv2d_hybrid / bh_dwconv2d_hybrid <- CONV_2D / DEPTHWISE_CONV_2D float32
 *                        with an int8 filter (conv.cc / depthwise_conv.cc EvalHybrid[PerChannel]: each
 *                        batch item quantised at run time; executors built with BAND_HIP_HYBRID_CONV=1)
 *   bh_detection_postprocess <- TFLite_Detection_PostProcess (custom; detection_postprocess.cc,
 *                        fast NMS, one class per detection)
 *   (HARD_SWISH 8-bit runs as a bh_lut_u8 table of reference_ops::HardSwish)
 *   bh_zero_insert + bh_conv2d_i8 <- TRANSPOSE_CONV int8 (reference_integer_ops::TransposeConv)
 *   bh_conv2d_f32 / bh_fc_f32 / bh_eltwise_f32 / bh_pool_f32 / bh_unary_f32 / bh_softmax_f32
 *                     <- the float32 forms of CONV_2D, DEPTHWISE_CONV_2D, FULLY_CONNECTED,
 *                        ADD/SUB/MUL, AVERAGE/MAX_POOL_2D, LOGISTIC/RELU*, SOFTMAX
 *                        (reference_ops float kernels) for fp16-weight models
 *
 * Quantised tensors live on the device as raw bytes in their TFLite type
 * (int8 or uint8).  Kernels work in the "int8 domain": a uint8 input is
 * mapped to int8 by XOR 0x80 on load (x - 128), and every zero point handed
 * to a kernel is already expressed in that domain.  Outputs are clamped to
 * [act_min, act_max] of the OUTPUT tensor's own type and stored as bytes, so
 * uint8 and int8 outputs are both bit-exact with TFLite.
 */
#ifndef BAND_HIP_KERNELS_H_
#define BAND_HIP_KERNELS_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BH_EINVAL (-1)

typedef void* bh_stream_t;
typedef void* bh_graph_exec_t;
typedef void* bh_event_t;

/* ---- device / memory / stream (runtime plumbing) ------------------------ */
int bh_device_count(int* count);
int bh_set_device(int ordinal);
int bh_get_device(int* ordinal);
/* arch name of `ordinal` (e.g. "gfx950:sramecc+:xnack-"), NUL-terminated */
int bh_device_arch(int ordinal, char* buf, size_t cap);
/* PCI bus id of `ordinal` ("0000:75:00.0", hipDeviceGetPCIBusId), NUL-terminated; cap >= 13 */
int bh_device_pci_bus_id(int ordinal, char* buf, int cap);
int bh_stream_create(bh_stream_t* stream);
int bh_stream_destroy(bh_stream_t stream);
int bh_stream_sync(bh_stream_t stream);
/* 0 when all work on the stream is done, BH_ENOTREADY while some is not */
int bh_stream_query(bh_stream_t stream);
int bh_malloc(void** ptr, size_t bytes);
int bh_free(void* ptr);
int bh_host_alloc(void** ptr, size_t bytes); /* pinned, portable */
int bh_host_free(void* ptr);
int bh_memcpy_h2d_async(void* dst, const void* src, size_t bytes, bh_stream_t s);
int bh_memcpy_d2h_async(void* dst, const void* src, size_t bytes, bh_stream_t s);
int bh_memcpy_d2d_async(void* dst, const void* src, size_t bytes, bh_stream_t s);
/* the same copy as a kernel launch (bh_copy_kernel), not a runtime blit */
int bh_copy_d2d(void* dst, const void* src, size_t bytes, bh_stream_t s);

/* CAST (cast_kernel): `count` elements of in_type as out_type, types among
 * uint8, int32, int64 and float32 (equal types: a copy).  One elementwise
 * launch, four elements per lane through the widest units where both pointers
 * are aligned to four elements (at most 16 bytes), one element per lane
 * otherwise; no host step, capturable.  float32 -> integer truncates toward
 * zero, NaN gives 0 and a value outside the range saturates; integer ->
 * integer keeps the low bits; integer -> float32 rounds to nearest
 * (band_hip_cast_shared.h holds the conversion, shared with the host twin).
 * Refused (BH_EINVAL, bh_last_error names the reason): null pointers, a
 * negative count, another type, a pointer not aligned to its element (4 bytes
 * for the 4- and 8-byte types). */
#define BH_CAST_U8 1
#define BH_CAST_I32 2
#define BH_CAST_I64 3
#define BH_CAST_F32 4
typedef struct bh_cast_params {
  int in_type, out_type; /* BH_CAST_* */
  long count;
  const void* input;
  void* output;
} bh_cast_params;
int bh_cast(const bh_cast_params* p, bh_stream_t s);
int bh_memset_async(void* dst, int value, size_t bytes, bh_stream_t s);
int bh_memcpy_h2d(void* dst, const void* src, size_t bytes);
int bh_memcpy_d2h(void* dst, const void* src, size_t bytes);

/* ---- stream capture -> hipGraph (one graph per prepared subgraph) ------- */
int bh_capture_begin(bh_stream_t s);
int bh_capture_end(bh_stream_t s, bh_graph_exec_t* exec);
int bh_graph_launch(bh_graph_exec_t exec, bh_stream_t s);
/* capture end that also returns the captured graph (free: bh_graph_free),
 * whose memcpy nodes bh_graph_memcpy_nodes lists (handle, dst, src, bytes;
 * up to max, *n = the count) and bh_graph_exec_set_memcpy retargets in the
 * instance (a 1-D host<->device copy of the same size) */
int bh_capture_end_keep(bh_stream_t s, bh_graph_exec_t* exec, void** graph);
int bh_graph_free(void* graph);
int bh_graph_memcpy_nodes(void* graph, void** nodes, void** dsts, const void** srcs, size_t* bytes, int max, int* n);
int bh_graph_exec_set_memcpy(bh_graph_exec_t exec, void* node, void* dst, const void* src, size_t bytes, int h2d);
int bh_graph_destroy(bh_graph_exec_t exec);

/* ---- events (timing) ---------------------------------------------------- */
int bh_event_create(bh_event_t* ev);
/* an event whose bh_event_sync sleeps until the GPU signals it (no
 * timing); replaces bh_stream_sync's spin-wait */
int bh_event_create_blocking(bh_event_t* ev);
/* an event with no timing whose waits spin (for bh_event_query polling) */
int bh_event_create_untimed(bh_event_t* ev);
int bh_event_destroy(bh_event_t ev);
int bh_event_record(bh_event_t ev, bh_stream_t s);
int bh_event_sync(bh_event_t ev);
/* 0 when the work before the event's record has finished, BH_ENOTREADY while
 * it is still running, else an error (non-blocking: hipEventQuery) */
#define BH_ENOTREADY (-2)
int bh_event_query(bh_event_t ev);
int bh_event_elapsed_ms(bh_event_t start, bh_event_t end, float* ms);
/* hold the stream for `us` microseconds (<= 100 ms): lets a profiler enqueue
 * a launch sequence before the GPU starts it, so events time execution */
int bh_spin_us(bh_stream_t s, int us);
/* one empty single-wave launch (profilers time chains of them to measure
 * the dispatch + gap an event pair adds around a real launch) */
int bh_empty_launch(bh_stream_t s);
/* this thread's next kernel launches carry dispatch timestamps: the first
 * kernel records `start` at its begin, every kernel records `stop` at its end
 * (hipExtLaunchKernel); bh_profile_events(NULL, NULL) turns it off.
 * Returns the number of kernels the previous setting timed. */
int bh_profile_events(bh_event_t start, bh_event_t stop);

/* ---- op parameter blocks ------------------------------------------------ */

/* CONV_2D.  Input NHWC [batch,in_h,in_w,in_c] bytes; output NHWC
 * [batch,out_h,out_w,out_c] bytes.  `weights` is the packed operand made by
 * bh_pack_conv_weights: int8-domain B^T [n_pad][k_pad] with
 * k = (ky*k_w + kx)*in_c + ci, zero padded.  bias_eff[c] already folds the
 * int32 bias and every zero-point cross term that does not depend on the
 * activations (see bh_pack_conv_weights); when w_zp != 0 (uint8 weights) the
 * kernel subtracts w_zp * sum_k x'[m][k] per output pixel. */
typedef struct bh_conv_params {
  int batch, in_h, in_w, in_c;
  int out_h, out_w, out_c;
  int k_h, k_w;
  int stride_h, stride_w, dil_h, dil_w;
  int pad_h, pad_w;               /* top / left padding (TFLite padding.h) */
  int k_pad, n_pad;               /* packed weight geometry */
  int in_xor;                     /* 0x80 when the input tensor is uint8 */
  int32_t in_zp;                  /* int8-domain input zero point (pad value) */
  int32_t w_zp;                   /* int8-domain weight zero point (0 if symmetric) */
  int32_t out_zp;                 /* output tensor zero point (own domain) */
  int32_t act_min, act_max;       /* output tensor domain */
  const void* input;
  void* output;
  const int8_t* weights;
  const int32_t* bias_eff;        /* [out_c] */
  const int32_t* mult;            /* [out_c] Q31 multipliers */
  const int32_t* shift;           /* [out_c] TFLite exponent (>0 = left) */
  /* Optional fused residual ADD (TFLite ADD applied to this conv's
   * requantised 8-bit output y and `residual`, same shape as the output):
   *   out = ADD(y, residual) with add.cc's left_shift-20 arithmetic.
   * Enabled when residual != NULL; y itself is then never stored. */
  const void* residual;
  int32_t add_y_off, add_r_off, add_o_off;    /* negated zps of y / residual, output zp */
  int32_t add_left_shift;
  int32_t add_y_mult, add_y_shift, add_r_mult, add_r_shift, add_o_mult, add_o_shift;
  int32_t add_act_min, add_act_max;
  /* optional 256-entry byte table applied to every stored output byte: a
   * following 8-bit unary op (QUANTIZE / RELU family / LOGISTIC) folded into
   * this epilogue (NULL = none) */
  const void* out_table;
  /* 1 when bh_conv_requant_fast_ok() holds for this layer's multipliers:
   * the kernels may then evaluate TFLite's two-step requantisation with one
   * 64-bit multiply-add and shifts (same results, fewer instructions) */
  int32_t requant_fast;
  /* kernel choice: BH_CONV_AUTO (by shape), or force one form where the
   * layer allows it (parity tests cover every form; A-B timing) */
  int32_t kernel_hint;
  /* 0: dense NHWC output.  Else output image n starts at output +
   * n * out_img_stride bytes (its out_h*out_w*out_c bytes contiguous): the
   * conv writes its slice of a CONCATENATION along a non-batch axis directly
   * (the concat launch is elided).  Such a layer runs conv_mfma_kernel. */
  int64_t out_img_stride;
} bh_conv_params;

/* Grouped launch of independent CONV_2D layers that each route to the
 * general MFMA kernel (bh_conv_group_ok): one dispatch runs every member's
 * workgroups (conv_group_kernel), each member computing exactly what its own
 * bh_conv2d_i8 launch would.  The members must not read each other's
 * outputs, and share one window type (all 1x1 unpadded, or none).
 * bh_conv_group_plan fills `host_table` (bh_conv_group_table_bytes(n)
 * bytes, n <= 32) and *g; the caller copies the table to device memory and
 * sets g->table before bh_conv_group_i8. */
typedef struct bh_conv_group {
  int n, blocks, is1x1;
  const void* table; /* device copy of the member table */
} bh_conv_group;
int bh_conv_group_ok(const bh_conv_params* p);
size_t bh_conv_group_table_bytes(int n);
int bh_conv_group_plan(const bh_conv_params* members, int n, void* host_table, bh_conv_group* g);
int bh_conv_group_i8(const bh_conv_group* g, bh_stream_t stream);
#define BH_CONV_AUTO 0
#define BH_CONV_MFMA 1 /* conv_mfma_kernel: per-wave fragments from L2, split-K deep layers */
#define BH_CONV_GEMM 2 /* conv_gemm_kernel: LDS-staged GEMM (1x1 s1, int8 in, symmetric filters) */
#define BH_CONV_GEMM_BIG 3 /* conv_gemm_big_kernel: 256-row tiles on 32x32x32 MFMA (same layers, large M) */
#define BH_CONV_STEM_VALU 4 /* RGB stems: conv_stem_kernel (VALU dot4) instead of conv_stem_mfma_kernel */
#define BH_CONV_STEM_MFMA 5 /* RGB stems: conv_stem_mfma_kernel (the routed form wherever its shape rules allow) */
#define BH_CONV_STEM_SCALAR 6 /* RGB stems: conv_stem_kernel with filters read through the scalar cache (round-4 form) */
#define BH_CONV_ROWS 7 /* conv_rows_kernel: 1x1 s1 layers of any K with N % 4 == 0 and K % 4 == 0 (never routed by shape) */
/* the tile configuration conv_gemm_big_kernel takes for an M x N layer when
 * routed automatically (2: 256x128, 3: 128x256), 0 when the layer is too
 * small for it (conv_gemm_kernel then) */
int bh_conv_gemm_big_config(long M, int N);

/* Grouped CONV_2D (TFLite filter [out_c][k_h][k_w][in_c / groups]).  `conv`
 * is the dense block with in_c / out_c the TOTAL channel counts; output
 * channel c belongs to group c / (out_c / groups) and reads input channels
 * [g * in_c / groups, (g + 1) * in_c / groups) only.  `weights` / bias_eff are
 * bh_pack_conv_weights(w, signed, out_c, K_g, ...) on the geometry
 * bh_conv_packed_geometry(out_c, K_g) with K_g = k_h * k_w * in_c / groups
 * (one row per output channel; group g owns rows [g * ocg, (g + 1) * ocg)).
 * groups must divide in_c and out_c.  Residual ADD, out_table, requant_fast
 * and out_img_stride are the dense epilogue's.  conv.kernel_hint takes the
 * BH_CONV_GROUPED_* values (anything else routes by shape). */
typedef struct bh_conv_grouped_params {
  bh_conv_params conv;
  int32_t groups;
} bh_conv_grouped_params;
#define BH_CONV_GROUPED_AUTO 0
#define BH_CONV_GROUPED_MFMA 1 /* conv_grouped_mfma_kernel, one 16-pixel tile per wave: the routed form */
#define BH_CONV_GROUPED_MFMA_2 2 /* the same kernel, two 16-pixel tiles per wave (never routed by shape) */

/* DEPTHWISE_CONV_2D.  weights: int8-domain [k_h][k_w][out_c] (TFLite layout
 * [1,kh,kw,oc] with XOR applied for uint8 filters).  Exact int32 math
 * (x'-in_zp)*(w'-w_zp) per tap, taps outside the image skipped. */
typedef struct bh_dwconv_params {
  int batch, in_h, in_w, in_c;
  int out_h, out_w, out_c, depth_multiplier;
  int k_h, k_w;
  int stride_h, stride_w, dil_h, dil_w;
  int pad_h, pad_w;
  int in_xor;
  int32_t in_zp, w_zp, out_zp;
  int32_t act_min, act_max;
  const void* input;
  void* output;
  const int8_t* weights;
  const int32_t* bias;            /* [out_c] raw int32 bias (zeros if absent) */
  const int32_t* mult;
  const int32_t* shift;
  /* optional 256-entry byte table applied to every stored output byte: a
   * following 8-bit unary op (QUANTIZE / RELU family / LOGISTIC) folded into
   * this epilogue (NULL = none) */
  const void* out_table;
  /* optional [out_c][4] int32 tap table from bh_pack_dw_taps (3x3, depth
   * multiplier 1, out_c % 4 == 0): the dot4 kernel then replaces the
   * per-tap one (weights / bias are not read).  NULL = per-tap kernel */
  const int32_t* taps;
  /* 1 when bh_conv_requant_fast_ok(mult, shift, out_c, 9, max|bias|) holds */
  int32_t requant_fast;
  /* kernel choice: BH_DW_AUTO (by shape), or force one form where the
   * shape allows it (parity tests cover every form; A-B timing) */
  int32_t kernel_hint;
} bh_dwconv_params;
#define BH_DW_AUTO 0
#define BH_DW_RUN 1   /* dwconv3x3_run_kernel: 4 pixels x 4 channels per thread */
#define BH_DW_DOT 2   /* dwconv3x3_dot_kernel: one pixel per thread */
#define BH_DW_MFMA 3  /* dwconv3x3_mfma_kernel: block-diagonal MFMA, C % 16 == 0 */

/* FULLY_CONNECTED.  input [rows][depth] bytes, weights int8-domain
 * [units][depth_pad] (depth_pad multiple of 16, zero padded); bias_eff as
 * for conv (folds bias - in_zp*sum(w') + depth*in_zp*w_zp). */
typedef struct bh_fc_params {
  int rows, depth, depth_pad, units;
  int in_xor;
  int32_t in_zp, w_zp, out_zp;
  int32_t act_min, act_max;
  const void* input;
  void* output;
  const int8_t* weights;
  const int32_t* bias_eff;
  const int32_t* mult;            /* [units] */
  const int32_t* shift;
  /* optional 256-entry byte table applied to every stored output byte: a
   * following 8-bit unary op (QUANTIZE / RELU family / LOGISTIC) folded into
   * this epilogue (NULL = none) */
  const void* out_table;
} bh_fc_params;

/* ADD / SUB / MUL with TFLite 4-D broadcasting.  Shapes are extended to 4-D
 * (leading 1s); a dimension of 1 in an input broadcasts.  Offsets are the
 * NEGATED zero points in each tensor's own domain (TFLite input*_offset). */
#define BH_ELT_ADD 0
#define BH_ELT_MUL 1
/* SQUARED_DIFFERENCE int8 (squared_difference.cc, left_shift 7): both inputs
 * scaled as ADD's, out = MBQMSmallerThanOneExp((a' - b')^2, o_mult, o_shift) +
 * o_off, clamped to act_min / act_max (the type's range: no fused activation).
 * bh_eltwise_i8 runs it through eltwise_sqdiff_kernel, an instantiation apart
 * from the ADD / MUL kernels. */
#define BH_ELT_SQDIFF 2
typedef struct bh_eltwise_params {
  int kind;                       /* BH_ELT_ADD (also SUB), BH_ELT_MUL or BH_ELT_SQDIFF */
  int in_signed;                  /* 1 int8, 0 uint8 (both inputs, output) */
  int shape_a[4], shape_b[4], shape_o[4];
  int32_t a_off, b_off, o_off;
  int32_t left_shift;             /* ADD: 20 */
  int32_t a_mult, a_shift;        /* ADD: input1 (shift <= 0) */
  int32_t b_mult, b_shift;        /* ADD: input2 (negated mult for SUB) */
  int32_t o_mult, o_shift;        /* ADD: output; MUL: the only multiplier */
  int32_t act_min, act_max;
  const void* a;
  const void* b;
  void* out;
} bh_eltwise_params;

/* AVERAGE_POOL_2D / MAX_POOL_2D (no rescale: in/out share scale). */
#define BH_POOL_AVG 0
#define BH_POOL_MAX 1
typedef struct bh_pool_params {
  int kind;
  int in_signed;
  int batch, in_h, in_w, channels;
  int out_h, out_w;
  int f_h, f_w, stride_h, stride_w, pad_h, pad_w;
  int32_t act_min, act_max;
  const void* input;
  void* output;
} bh_pool_params;

/* Fused MobileNet inverted-residual block (int8 per-channel models):
 *   [CONV_2D 1x1 expand ->] DEPTHWISE_CONV_2D 3x3 -> CONV_2D 1x1 project [-> ADD x]
 * exactly as the 3-4 TFLite ops compute it (each intermediate is requantised
 * to its own 8-bit tensor), but one launch: a workgroup owns a tile of
 * output pixels, stages the input region (tile + halo) in LDS, computes the
 * expanded activation for the region into LDS (MFMA), the depthwise output
 * into LDS (VALU), then the projection (MFMA) + residual epilogue to HBM.
 * Intermediates never touch HBM. */
typedef struct bh_irb_params {
  int batch, in_h, in_w, in_c;        /* x: NHWC int8 */
  int exp_c;                          /* expanded channels (== in_c when no expand) */
  int out_h, out_w, out_c;            /* y: NHWC int8 */
  int stride, pad_h, pad_w;           /* depthwise 3x3 */
  int has_expand;
  int tile_h, tile_w;                 /* output pixels per workgroup */
  /* expand 1x1 (packed like bh_pack_conv_weights: [n_pad][k_pad]) */
  const int8_t* exp_w; int exp_k_pad;
  const int32_t* exp_bias_eff; const int32_t* exp_mult; const int32_t* exp_shift;
  int32_t x_zp;                       /* x zero point */
  int32_t e_zp, e_act_min, e_act_max; /* expanded tensor quantisation */
  /* depthwise [3][3][exp_c] */
  const int8_t* dw_w;
  const int32_t* dw_bias; const int32_t* dw_mult; const int32_t* dw_shift;
  int32_t d_zp, d_act_min, d_act_max;
  /* project 1x1 ([n_pad][k_pad], bias_eff folds d_zp) */
  const int8_t* proj_w; int proj_k_pad;
  const int32_t* proj_bias_eff; const int32_t* proj_mult; const int32_t* proj_shift;
  int32_t p_zp, p_act_min, p_act_max;
  /* optional residual ADD(p, x) (has_residual: stride 1, in_c == out_c) */
  int has_residual;
  int32_t add_p_off, add_x_off, add_o_off, add_left_shift;
  int32_t add_p_mult, add_p_shift, add_x_mult, add_x_shift, add_o_mult, add_o_shift;
  int32_t add_act_min, add_act_max;
  const void* input;
  void* output;
  /* diagnostics: when non-NULL, wave 0 of each workgroup writes 8 uint64
   * s_memrealtime stamps (100 MHz) at phase boundaries to
   * debug_stamps[16 * workgroup] (slots 0-7 used); NULL in production */
  void* debug_stamps;
  /* single-step requantisation allowed (bh_conv_requant_fast_ok) per stage:
   * bit 0 expand, bit 1 depthwise, bit 2 project */
  int32_t requant_fast;
} bh_irb_params;

/* LDS bytes one workgroup of bh_irb_i8 needs for a tile (0 if unsupported) */
size_t bh_irb_lds_bytes(const bh_irb_params* p);
int bh_irb_i8(const bh_irb_params* p, bh_stream_t s);

/* Fused pointwise chain across a block boundary (int8 per-channel models):
 *   DEPTHWISE_CONV_2D 3x3 -> CONV_2D 1x1 [-> ADD residual] [-> CONV_2D 1x1]
 * i.e. a MobileNetV2 block's depthwise + project (+ its residual ADD) and the
 * NEXT block's expand, or a MobileNetV1 depthwise + pointwise pair, exactly
 * as the 2-3 TFLite ops compute them (every intermediate requantised to its
 * own 8-bit tensor), in one launch.  No halo recompute: the 1x1 layers map
 * pixel m to pixel m, so a workgroup owns px_blocks x 16 consecutive output
 * pixels, computes their depthwise output for every channel into LDS
 * (block-diagonal MFMA), the first 1x1 GEMM from LDS (MFMA) with its
 * residual epilogue, and the second 1x1 GEMM from that result in LDS.
 * Parameter blocks are the unfused launches' own (same packed operands):
 *   dw.output and pw1.input are ignored (the depthwise result stays in LDS);
 *   pw1.output may be NULL (the block output is private to pw2) or the
 *   tensor to store; pw2 is read only when has_pw2.
 * Supported: dw 3x3, depth multiplier 1, tap table, out_c % 16 == 0, any
 * stride / dilation; all stages int8 in / symmetric filters (in_xor == 0,
 * w_zp == 0), no out_table; pw1 / pw2 1x1 stride 1 with out_c % 4 == 0;
 * pw2 without residual and with K = pw1.out_c <= 320.  px_blocks in {1, 2, 4};
 * 16 waves (px_blocks 1) spread few-pixel layers' channel work wider; the
 * dense form holds more waves per SIMD on the large-grid layers. */
typedef struct bh_chain_params {
  bh_dwconv_params dw;
  bh_conv_params pw1;
  bh_conv_params pw2;
  int has_pw2;
  int px_blocks;
  int waves;  /* waves per workgroup: 4 (0 = 4), or 8 / 16 with px_blocks == 1 */
  /* 1: persistent form - both 1x1 filters, the depthwise filter and all
   * tables staged in LDS once per workgroup, which then walks a contiguous
   * range of 64-pixel blocks (px_blocks 4, 4 waves; filters must fit LDS) */
  int persist;
  /* 1: 2-D tile form (chain_tile_kernel) - a workgroup owns an 8 x 8 tile of
   * output pixels and stages its depthwise input patch (tile + halo), the
   * residual tile, both 1x1 filters and every table in LDS with one burst of
   * LDS-DMA; stride / dilation 1 or 2, pw2 K <= 320.  px_blocks, waves and
   * persist are ignored.  3 / 4: runs of 2 / 4 consecutive tiles per
   * workgroup through ONE buffer (the constant block staged once per run) */
  int tile;
  /* tile form: the chain's constant block (both 1x1 filters swizzled for
   * LDS, every table, the depthwise filter) built once by
   * bh_chain_tile_pack into bh_chain_tile_blob_bytes() of device memory */
  const void* tile_blob;
  /* tile form, diagnostics: when non-NULL each workgroup writes 8 shader-
   * clock stamps (s_memtime) at its phase boundaries to
   * debug_stamps[8 * workgroup]; NULL in production */
  void* debug_stamps;
  /* 1: deep-issue form - each wave issues the loads of 6 depthwise channel
   * groups per round (instead of 2) and the x-stationary 1x1 GEMMs take 3-6
   * channel tiles per round; px_blocks 1 (4 or 8 waves) or 2 (4 waves) */
  int deep;
  /* raster forms with a second 1x1 (0 / 1: off): the second 1x1's channel
   * tiles are split over c_split workgroups per pixel block (grid.y); each
   * recomputes the depthwise and first 1x1 for its pixels and stores its
   * channel slice - more, shorter workgroups for the few-pixel 14x14 / 7x7
   * layers.  2..4 */
  int c_split;
  /* 1: raster form with staged filters (chain_stage_kernel) - a workgroup of
   * px_blocks (1 / 2) x 16 pixels and `waves` (4 / 8) waves starts with one
   * burst of LDS-DMA of the first 1x1's filter and tables, its c_split slice
   * (0 / 1 .. 8, grid.y) of the second 1x1's and the residual rows from
   * tile_blob (bh_chain_tile_pack), runs the depthwise from global memory
   * and both 1x1 GEMMs from LDS; has_pw2 only, pw2 K <= 320.  2: the same
   * with the burst issued by the upper half of the waves while the lower
   * half runs the depthwise phase */
  int stage;
  /* 1: dense raster form (chain_dense_kernel) for chains whose grid gives
   * every CU several workgroups - 64 pixels per 4-wave workgroup, a wave
   * keeping its 16 pixels in LDS of its own through all three phases (no
   * workgroup barrier between them), one item per load round, compiled for
   * 6 - 8 waves per SIMD; px_blocks 4, 4 waves, no persist / tile / deep /
   * c_split / stage, at most 64 KB of LDS */
  int dense;
} bh_chain_params;

/* LDS bytes one workgroup of bh_chain_i8 needs (0 if unsupported) */
size_t bh_chain_lds_bytes(const bh_chain_params* p);
/* the stage form's share of bh_chain_lds_bytes / bh_chain_i8 (stage != 0) */
size_t bh_chain_stage_lds_bytes(const bh_chain_params* p);
int bh_chain_stage_launch(const bh_chain_params* p, bh_stream_t s);
/* the dense form's share of bh_chain_lds_bytes / bh_chain_i8 (dense != 0) */
size_t bh_chain_dense_lds_bytes(const bh_chain_params* p);
int bh_chain_dense_launch(const bh_chain_params* p, bh_stream_t s);
/* the tile form's share of bh_chain_lds_bytes / bh_chain_i8 (tile != 0) */
size_t bh_chain_tile_lds_bytes(const bh_chain_params* p);
int bh_chain_tile_launch(const bh_chain_params* p, bh_stream_t s);
/* the tile / stage forms' constant block: its size for these parameters (as
 * if tile == 1, or for the stage form when stage != 0; 0 if the form does not
 * apply) and a device pass that builds it from the params' filter / table
 * pointers into `blob` */
size_t bh_chain_tile_blob_bytes(const bh_chain_params* p);
int bh_chain_tile_pack(const bh_chain_params* p, void* blob, bh_stream_t s);
int bh_chain_i8(const bh_chain_params* p, bh_stream_t s);

/* MEAN over one contiguous run of axes (TFLite 2.9.2 reduce.cc EvalMean ->
 * optimized_integer_ops::Mean int8 / optimized_ops::Mean uint8 / float):
 * the input viewed as [outer][reduce][inner]; out[o][i] = for 8-bit types
 * clamp(MultiplyByQuantizedMultiplier(sum_r x, multiplier, shift) + bias),
 * for float32 (sum_r x in order) / reduce.  One thread per output. */
typedef struct bh_mean_params {
  long outer, reduce, inner;
  int type;                       /* 0 float32, 1 int8, 2 uint8 */
  int32_t multiplier, shift, bias;
  const void* input;
  void* output;
} bh_mean_params;
int bh_mean(const bh_mean_params* p, bh_stream_t s);

/* MEAN of an int8 / uint8 tensor over its last axis (reduce.cc EvalMean, the
 * two branches the 4-D {1, 2} form above does not take), the input viewed as
 * [rows][depth] with an int32 sum per row:
 *   exact != 0 (input and output share scale and zero point,
 *     reference_ops::Mean): out = (T)(sum / depth), C++ integer division;
 *   exact == 0 (reference_ops::QuantizedMeanOrSum, compute_sum false), every
 *     step a float32 operation of its own:
 *     out = clamp((int)roundf((float)sum / (float)depth * scale + bias) + out_zp)
 *     with scale = s_in / s_out and bias = -zp_in * scale + 0.5f from the caller.
 * mean_rows_kernel: one wave per row, 4 rows per workgroup, dword reads where
 * the row is 4-byte aligned, a cross-lane sum.  Refused (BH_EINVAL,
 * bh_last_error names the reason): null pointers, rows or depth < 1, type not
 * 1 / 2, depth * 255 >= 2^31, rows >= 2^31. */
typedef struct bh_mean_rows_params {
  long rows;
  int depth;
  int type;                       /* 1 int8, 2 uint8 */
  int exact;
  float scale, bias;
  int32_t out_zp;
  const void* input;
  void* output;
} bh_mean_rows_params;
int bh_mean_rows(const bh_mean_rows_params* p, bh_stream_t s);
/* "mean_rows_kernel", or "" for parameters bh_mean_rows refuses; static storage */
const char* bh_mean_rows_kernel(const bh_mean_rows_params* p);
/* the launcher's parameter check alone; pure host */
int bh_mean_rows_check(const bh_mean_rows_params* p);

/* The ten ops a converter makes of an int8 LayerNormalization over the last
 * axis of x [rows][depth], as one launch (layernorm_i8_kernel):
 *   m = MEAN(x)  d = SQUARED_DIFFERENCE(x, m)  v = MEAN(d)  e = ADD(v, eps)
 *   r = RSQRT(e)  g = MUL(r, gamma)  a = MUL(x, g)  b = MUL(m, g)
 *   c = SUB(beta, b)  y = ADD(a, c)
 * with the operand order as written.  Every op's requantisation is performed
 * in that order with the device functions of the single-op kernels, each
 * intermediate rounded and clamped to its own int8 value, so y is byte for
 * byte what the ten launches store; the intermediates are not stored.  One
 * wave per row, 4 rows per workgroup, the row in registers: 16 values per lane
 * x 64 lanes, so depth <= BH_LAYERNORM_MAX_DEPTH = 1024.  The RSQRT table and
 * the gamma / beta rows are staged in LDS once per workgroup.
 * The parameter blocks are the single ops' own (lower.cc fills them the same
 * way); their pointers and shapes are ignored, the tensors are:
 *   input [rows][depth], gamma [depth], beta [depth], rsqrt_table [256],
 *   eps_q the one byte of the eps constant, output [rows][depth].
 * Refused (BH_EINVAL, bh_last_error names the reason): null pointers, rows or
 * depth < 1, depth above the limit, rows >= 2^31, a MEAN block that disagrees
 * on depth or is not int8, a binary block that is not int8 or of the wrong
 * kind. */
#define BH_LAYERNORM_MAX_DEPTH 1024
typedef struct bh_layernorm_params {
  long rows;
  int depth;
  bh_mean_rows_params mean_x, mean_d;
  bh_eltwise_params sqdiff, add_eps, mul_gamma, mul_x, mul_m, sub_beta, add_out;
  int32_t eps_q;
  const void* rsqrt_table;
  const void* input;
  const void* gamma;
  const void* beta;
  void* output;
} bh_layernorm_params;
int bh_layernorm_i8(const bh_layernorm_params* p, bh_stream_t s);
/* "layernorm_i8_kernel", or "" for parameters bh_layernorm_i8 refuses; static storage */
const char* bh_layernorm_i8_kernel(const bh_layernorm_params* p);
int bh_layernorm_i8_check(const bh_layernorm_params* p);

/* The ten float32 ops a converter makes of a LayerNormalization over the last
 * axis of x [rows][depth], as one launch (layernorm_f32_kernel), optionally
 * followed in the same launch by the row quantisation of a hybrid
 * FULLY_CONNECTED (bh_dynquant_rows below).  The rule is the ten ops in their
 * order and operand order, each one IEEE float32 operation on a row x[0..C),
 * no contraction, the divisions and the square root correctly rounded:
 *   m = S(x) / C                      d_i = (x_i - m)^2  (two roundings)
 *   v = S(d) / C      e = v + eps     r = 1 / sqrt(e)    (sqrt, then divide, as unary_f32_kernel's RSQRT)
 *   g_i = r * gamma_i   a_i = x_i * g_i   b_i = m * g_i   c_i = beta_i - b_i   y_i = a_i + c_i
 * The two-pass form is the rule; E[x^2] - m^2 is not.  Only the two sums S are
 * reassociated, and their order is part of the rule - there is ONE order,
 * whatever the number of rows, the row's place in its workgroup or the
 * alignment of any pointer:
 *   lane l of 64 owns elements 256 j + 4 l + k, j = 0 .. 3, k = 0 .. 3 (those
 *   below C).  It starts from +0 and adds its own elements in ascending index
 *   order (j outer, k inner).  The 64 lane sums then meet in an xor butterfly
 *   over offsets 32, 16, 8, 4, 2, 1: at each offset o lane l replaces its value
 *   by value[l] + value[l ^ o].  Float addition commutes, so every lane ends
 *   with the same bits.
 * (MEAN op by op sums a row in index order in one lane, so the fused result
 * is not bit for bit the ten launches'; both lie within the same error bound
 * of the real LayerNorm, tests/layernorm_f32_models.py derives it.)
 * A wave owns a row and keeps it in registers from load to store: 16 values
 * per lane, so depth <= BH_LAYERNORM_F32_MAX_DEPTH = 1024.  A 16-byte aligned
 * row of a depth that is a multiple of 4 is read as float4; any other row is
 * read element by element into the same lanes.
 *   input [rows][depth], gamma [depth], beta [depth], eps the value of the ADD's constant;
 *   output [rows][depth] float32, or NULL: y is not stored;
 *   q [rows][depth], scale [rows], offset [rows], all set or all NULL: the
 *   hybrid row rule (symmetric, or asymmetric when `asymmetric`) applied to
 *   the float32 values y, through the device functions bh_dynquant_rows uses -
 *   the bytes bh_dynquant_rows writes when run on the stored y.
 * Refused (BH_EINVAL, bh_last_error names the reason): a null input, gamma or
 * beta; neither output nor q set; q, scale, offset only partly set; rows or
 * depth < 1; depth above the limit; rows >= 2^31; a float / int32 operand off
 * its 4-byte boundary.  No LDS, no scratch, no atomics. */
#define BH_LAYERNORM_F32_MAX_DEPTH 1024
typedef struct bh_layernorm_f32_params {
  long rows;
  int depth;
  float eps;
  const float* input;
  const float* gamma;
  const float* beta;
  float* output;    /* [rows][depth] or NULL */
  int8_t* q;        /* [rows][depth] or NULL (then scale and offset are NULL too) */
  float* scale;     /* [rows] */
  int32_t* offset;  /* [rows] */
  int asymmetric;
} bh_layernorm_f32_params;
int bh_layernorm_f32(const bh_layernorm_f32_params* p, bh_stream_t s);
/* "layernorm_f32_kernel", or "" for parameters bh_layernorm_f32 refuses; static storage */
const char* bh_layernorm_f32_kernel(const bh_layernorm_f32_params* p);
/* the launcher's parameter check alone; pure host */
int bh_layernorm_f32_check(const bh_layernorm_f32_params* p);

/* ---- host-side operand packing (pure CPU, no device calls) -------------- */

/* Pack OHWI conv weights ([out_c][k_h*k_w*in_c] bytes, signed or unsigned)
 * into the int8-domain padded B^T operand and compute bias_eff:
 *   bias_eff[c] = bias[c] - in_zp*S_c + K*in_zp*w_zp,  S_c = sum_k w'[c][k]
 * where w' = w (int8) or w-128 (uint8) and in_zp/w_zp are int8-domain.
 * packed must hold n_pad*k_pad bytes; bias may be NULL. */
int bh_pack_conv_weights(const void* w, int w_signed, int out_c, int k,
                         int k_pad, int n_pad, const int32_t* bias,
                         int32_t in_zp, int32_t w_zp, int8_t* packed,
                         int32_t* bias_eff);

/* Tile geometry the conv launcher expects for a layer (k_pad, n_pad). */
int bh_conv_packed_geometry(int out_c, int k, int* k_pad, int* n_pad);
/* DEPTHWISE_CONV_2D 3x3 / depth multiplier 1 tap table: for channel c,
 * taps[4c..4c+3] = {w[0..3][c] as bytes, w[4..7][c] as bytes,
 * w[8][c] << 8*(c%4), bias[c] - in_zp*sum_t w[t][c] + 9*in_zp*w_zp}.
 * w: int8-domain [9][c]; in_zp / w_zp int8-domain; c % 4 == 0. */
int bh_pack_dw_taps(const int8_t* w, int c, const int32_t* bias, int32_t in_zp, int32_t w_zp, int32_t* taps);
/* Whether a conv layer may use the single-step requantisation identity
 *   rdbypot(srdhm(x, M), e) + zp == (((x*M + c0) >> 31) + s + (zp << e)) >> e
 *   c0 = 2^30 + (e > 0 ? 2^(30+e) : 0),  s = (e > 0 && x < 0) ? -1 : 0
 * (TFLite MultiplyByQuantizedMultiplier with shift = -e <= 0).  Holds when
 * every multiplier is in (2^30, 2^31), every shift <= 0 and the int32
 * accumulators are small enough that nothing overflows:
 *   K * 2^16 + max|bias| + 255 * 2^e < 2^30.  Returns 1 / 0. */
int bh_conv_requant_fast_ok(const int32_t* mult, const int32_t* shift, int n, int k, int64_t max_abs_bias);

/* ---- launchers ---------------------------------------------------------- */
int bh_conv2d_i8(const bh_conv_params* p, bh_stream_t s);
/* Symbol of the kernel bh_conv2d_i8 dispatches these parameters to
 * ("conv_mfma_kernel", "conv_xs_kernel", "conv_rows_kernel",
 * "conv_direct_kernel"); static storage.  Profiling attribution only. */
const char* bh_conv2d_i8_kernel(const bh_conv_params* p);
/* grouped CONV_2D (bh_conv_grouped_params); BH_EINVAL with bh_last_error set
 * when groups does not divide the channel counts or a pointer is missing */
int bh_conv2d_grouped_i8(const bh_conv_grouped_params* p, bh_stream_t s);
/* Symbol bh_conv2d_grouped_i8 dispatches to ("conv_grouped_mfma_kernel"), ""
 * for a block it would refuse; static storage */
const char* bh_conv2d_grouped_i8_kernel(const bh_conv_grouped_params* p);
int bh_dwconv2d_i8(const bh_dwconv_params* p, bh_stream_t s);
/* Symbol of the kernel bh_dwconv2d_i8 dispatches these parameters to
 * ("dwconv3x3_run_kernel", "dwconv3x3_dot_kernel", "dwconv3x3_kernel",
 * "dwconv_generic_kernel"); static storage.  Profiling attribution only. */
const char* bh_dwconv2d_i8_kernel(const bh_dwconv_params* p);
int bh_fc_i8(const bh_fc_params* p, bh_stream_t s);
int bh_eltwise_i8(const bh_eltwise_params* p, bh_stream_t s);
int bh_pool_i8(const bh_pool_params* p, bh_stream_t s);

/* ---- glue ops (whole-model residency) ------------- */

/* out[i] = table[in[i]]: every 8-bit unary op whose result depends only on
 * the input byte.  The host fills the 256-entry device table (indexed by the
 * raw byte) with TFLite's own formula: QUANTIZE between 8-bit types
 * (Requantize), RELU / RELU6 / RELU_N1_TO_1 (ReluX), LOGISTIC (the 8-bit
 * lookup table of activations.cc).  bh_lut_f32: 256 float entries
 * (DEQUANTIZE: float(double(scale) * (q - zp))). */
int bh_lut_u8(const void* in, void* out, long n, const void* table, bh_stream_t s);
int bh_lut_f32(const void* in, void* out, long n, const float* table, bh_stream_t s);
/* float32 -> 8-bit: clamp((int)roundf(x / scale) + zp) */
int bh_quantize_f32(const float* in, void* out, long n, float scale, int32_t zp, int out_signed,
                    bh_stream_t s);

/* ---- float32 graphs ------------------------------------------------------
 * TFLite fp16 models (post-training float16 quantization) compute in float32
 * with fp16 constant weights behind DEQUANTIZE ops; the host folds those
 * DEQUANTIZEs and hands these kernels float32 operands.  Float results match
 * the reference within a stated tolerance (summation order differs), not
 * bit-exactly.  act_min / act_max are the fused activation's float bounds
 * (+-inf for NONE). */
typedef struct {
  int batch, in_h, in_w, in_c, out_h, out_w, out_c, k_h, k_w;
  int stride_h, stride_w, dil_h, dil_w, pad_h, pad_w;
  int depthwise, depth_multiplier;   /* depthwise: out_c = in_c * depth_multiplier */
  float act_min, act_max;
  const float* input;
  float* output;
  const float* weights; /* conv: [k_h*k_w*in_c][out_c]; depthwise: [k_h*k_w][out_c] */
  const float* bias;    /* [out_c] or NULL */
} bh_conv_f32_params;
int bh_conv2d_f32(const bh_conv_f32_params* p, bh_stream_t s);
/* Split-K factor (1, 2, 4, 8 or 16 slices of the filter taps per workgroup)
 * bh_conv2d_f32 runs conv_f32_kernel with for these parameters; 0 for a
 * depthwise or invalid block.  Pure host, no device call. */
int bh_conv2d_f32_split(const bh_conv_f32_params* p);

typedef struct {
  int rows, depth, units;
  float act_min, act_max;
  const float* input;   /* [rows][depth] */
  float* output;        /* [rows][units] */
  const float* weights; /* [units][depth] */
  const float* bias;    /* [units] or NULL */
} bh_fc_f32_params;
int bh_fc_f32(const bh_fc_f32_params* p, bh_stream_t s);

#define BH_ELTF_ADD 0
#define BH_ELTF_SUB 1
#define BH_ELTF_MUL 2
#define BH_ELTF_SQDIFF 3 /* SQUARED_DIFFERENCE: (a - b)^2 */
typedef struct {
  int kind;
  int shape_a[4], shape_b[4], shape_o[4]; /* 4-D, broadcast dims are 1 */
  float act_min, act_max;
  const float* a;
  const float* b;
  float* out;
} bh_eltwise_f32_params;
int bh_eltwise_f32(const bh_eltwise_f32_params* p, bh_stream_t s);

typedef struct {
  int kind; /* BH_POOL_AVG / BH_POOL_MAX */
  int batch, in_h, in_w, channels, out_h, out_w, f_h, f_w, stride_h, stride_w, pad_h, pad_w;
  float act_min, act_max;
  const float* input;
  float* output;
} bh_pool_f32_params;
int bh_pool_f32(const bh_pool_f32_params* p, bh_stream_t s);

#define BH_UNARY_CLAMP 0    /* RELU / RELU6 / RELU_N1_TO_1: min(max(x, lo), hi) */
#define BH_UNARY_LOGISTIC 1 /* 1 / (1 + exp(-x)) */
#define BH_UNARY_RSQRT 2    /* RSQRT: 1 / sqrt(x) */
#define BH_UNARY_GELU 3     /* GELU: 0.5 x (1 + erf(x / sqrt 2)) */
#define BH_UNARY_GELU_TANH 4 /* GELU, approximate: 0.5 x (1 + tanh(sqrt(2 / pi) x (1 + 0.044715 x^2))) */
/* 5 is no kind: tests/test_layernorm_gpu.py pins that bh_unary_f32 refuses it, so TANH could not take the next
 * value and the range checks name two constants (0 .. BH_UNARY_GELU_TANH, and BH_UNARY_TANH).  A constraint to
 * revisit in a change that may edit that test: the kinds should be contiguous. */
#define BH_UNARY_TANH 6      /* tanhf(x) */
int bh_unary_f32(int kind, const float* in, float* out, long n, float lo, float hi, bh_stream_t s);

/* reference_ops::Softmax (float): per row exp((x - max) * beta) / sum */
int bh_softmax_f32(const float* in, float* out, long rows, int depth, float beta, bh_stream_t s);

#define BH_CONCAT_MAX_INPUTS 16
typedef struct {
  int n_inputs;
  long outer;                              /* product of the dims before the axis */
  long row[BH_CONCAT_MAX_INPUTS];          /* bytes per outer index of input k */
  const void* input[BH_CONCAT_MAX_INPUTS];
  const void* table[BH_CONCAT_MAX_INPUTS]; /* optional 256-B rescale table (uint8
                                              ConcatenationWithScaling), NULL = copy */
  void* output;                            /* row of outer index o: sum_k row[k] bytes */
} bh_concat_params;
int bh_concat(const bh_concat_params* p, bh_stream_t s);

typedef struct {
  int elem_bytes;                 /* 1 or 4 */
  int in_shape[4];                /* NHWC (lower ranks padded with leading 1s) */
  int pad_before[4], pad_after[4];
  uint32_t value;                 /* bit pattern of the pad element */
  const void* input;
  void* output;
  /* 0: constant fill (PAD / PADV2); MIRROR_PAD: 1 REFLECT, 2 SYMMETRIC
   * (mirror_pad.cc GetInputDimension; pads < dim for REFLECT, <= dim) */
  int32_t mode;
} bh_pad_params;
int bh_pad(const bh_pad_params* p, bh_stream_t s);

typedef struct {
  int batch, in_h, in_w, out_h, out_w;
  int row_bytes;                  /* channels * element bytes */
  const int32_t* y_index;         /* [out_h] source row (host-computed, TFLite float formula) */
  const int32_t* x_index;         /* [out_w] source column */
  const void* input;
  void* output;
} bh_resize_nearest_params;
int bh_resize_nearest(const bh_resize_nearest_params* p, bh_stream_t s);

typedef struct {
  int batch, in_h, in_w, channels, out_h, out_w;
  const int32_t* y_tab;           /* [out_h][3]: lower row, upper row, 10-bit scaled y */
  const int32_t* x_tab;           /* [out_w][3] */
  const void* input;              /* int8 */
  void* output;
} bh_resize_bilinear_params;
int bh_resize_bilinear_i8(const bh_resize_bilinear_params* p, bh_stream_t s);

/* ARG_MAX / ARG_MIN (TFLite arg_min_max.cc -> reference_ops::ArgMinMax): the
 * input viewed as [outer][axis_len][inner]; out[o][i] = the index along the
 * axis of the extreme, found as the sequential loop finds it: start at
 * element 0 and replace only on > (< for min), so the FIRST extreme wins, a
 * float NaN is selected only as element 0, and -0.0 == +0.0.  Output int32
 * (out_bytes 4) or int64 (8, high word zero).  inner == 1 and axis_len < 64:
 * a thread per row (argminmax_kernel); inner == 1 and axis_len >= 64: a wave
 * per row with a cross-lane reduction that prefers the smaller index
 * (argminmax_row_kernel); inner > 1: a thread per position walking the axis
 * at stride `inner` (argminmax_kernel).  No scratch, no atomics. */
#define BH_ARG_I8 0
#define BH_ARG_U8 1
#define BH_ARG_F32 2
typedef struct {
  long outer, axis_len, inner;
  int in_type;                    /* BH_ARG_I8 / BH_ARG_U8 / BH_ARG_F32 */
  int is_min;                     /* 0 ARG_MAX, 1 ARG_MIN */
  int out_bytes;                  /* 4 (int32) or 8 (int64) */
  const void* input;
  void* output;                   /* [outer][inner], aligned to out_bytes */
} bh_argminmax_params;
int bh_argminmax(const bh_argminmax_params* p, bh_stream_t s);
/* the kernel bh_argminmax dispatches to for these sizes */
const char* bh_argminmax_kernel(const bh_argminmax_params* p);

/* The re-indexing ops - TRANSPOSE, STRIDED_SLICE, SLICE, SPLIT, SPLIT_V,
 * SPACE_TO_DEPTH, DEPTH_TO_SPACE: every output element is one input element.
 * The output is dense row-major over out_dims[0 .. rank); element
 * (i_0, .., i_{rank-1}) is input element in_offset + sum_d i_d * in_stride[d]
 * (strides and offset in elements; a stride may be negative).  The caller guarantees every such element lies inside the input.
 * bh_reindex_canonical drops unit dims and merges dims d, d + 1 when
 * in_stride[d] == in_stride[d + 1] * out_dims[d + 1] (rank >= 1 afterwards; a
 * map that is the identity comes out as rank 1, stride 1); pure host.  The
 * launcher canonicalises, refuses rank > 6 and more than 2^31 - 1 elements
 * (FastDiv index math), and runs one of
 *   reindex_rows_kernel    innermost stride 1: runs of out_dims[last] *
 *                          elem_bytes contiguous bytes on both sides, moved 16 /
 *                          8 / 4 / 1 bytes per lane (the widest that divides
 *                          the run, both addresses and every outer stride in
 *                          bytes); short runs share a wave
 *   reindex_tile_kernel    another dim has input stride 1 (a true transpose)
 *                          and that dim and the last are both >= 64 long:
 *                          64 x 64 tiles through LDS, loads coalesced along the
 *                          input-contiguous dim, stores along the output's last
 *   reindex_gather_kernel  the rest (negative / non-unit innermost stride, a
 *                          transpose with an edge shorter than a tile - measured
 *                          faster there): a thread per 4 output bytes, dword stores
 * No scratch, no atomics. */
#define BH_REINDEX_MAX_RANK 6
typedef struct {
  int elem_bytes;                 /* 1 or 4 */
  int rank;                       /* 0 .. BH_REINDEX_MAX_RANK */
  int out_dims[BH_REINDEX_MAX_RANK];
  int64_t in_stride[BH_REINDEX_MAX_RANK]; /* elements */
  int64_t in_offset;              /* elements */
  const void* input;              /* aligned to elem_bytes */
  void* output;                   /* aligned to elem_bytes */
  /* GATHER as a map: with `indices` set (null: a plain map, everything above)
   * the map is [outer][n_idx][inner] with in_stride {index_range * inner, inner,
   * 1} and in_offset 0, and coordinate j of dim 1 reads input row indices[j]
   * instead of row j: bh_reindex, bh_reindex_kernel and CpuReindex hand it to
   * bh_gather / CpuGather (bh_gather_params below, where the out-of-range rule
   * is); bh_reindex_canonical and bh_reindex_as(gather != 0) refuse it. */
  const void* indices;            /* n_idx int32 / int64 values on the device, aligned to index_bytes */
  int index_bytes;                /* 4 or 8 */
  int64_t index_range;            /* axis_size: an index outside [0, index_range) gives a zero row */
} bh_reindex_params;
int bh_reindex(const bh_reindex_params* p, bh_stream_t s);
/* the kernel bh_reindex dispatches to for this map ("" for a refused one) */
const char* bh_reindex_kernel(const bh_reindex_params* p);
int bh_reindex_canonical(const bh_reindex_params* p, bh_reindex_params* canonical);
/* bh_reindex with the form chosen by the caller: gather != 0 runs
 * reindex_gather_kernel, which takes any map, whatever bh_reindex would pick
 * (tools/reindex_profile.py times the forms side by side); 0 is bh_reindex. */
int bh_reindex_as(const bh_reindex_params* p, int gather, bh_stream_t s);

/* GATHER (batch_dims 0): params viewed as [outer][axis_size][inner] elements,
 * `indices` a flat list of n_idx int32 / int64 values in device memory (a
 * constant or an activation), output dense [outer][n_idx][inner] =
 * np.take(params, indices, axis).  One kernel, gather_rows_kernel: a lane moves
 * V = 16 / 8 / 4 / 1 bytes, the widest that divides inner * elem_bytes and both
 * base addresses; no scratch, no atomics.  An index outside [0, axis_size)
 * reads nothing and its output slice is zero bytes (TFLite fails the invoke on
 * a negative index and leaves a too large one undefined; a replayed graph can
 * do neither); the range check is band_hip_gather_shared.h's, shared with the
 * host twin.  Refused (BH_EINVAL, bh_last_error names bh_gather and the
 * reason): null pointers, elem_bytes not 1 or 4, index_bytes not 4 or 8, a
 * count < 1, params / output not aligned to elem_bytes, indices not aligned to
 * index_bytes, more than 2^31 - 1 output bytes (FastDiv index math). */
typedef struct {
  int elem_bytes;                 /* 1 or 4 */
  int index_bytes;                /* 4 or 8 */
  int64_t outer, axis_size, n_idx;
  int64_t inner;                  /* elements */
  const void* params;             /* aligned to elem_bytes */
  const void* indices;            /* aligned to index_bytes */
  void* output;                   /* aligned to elem_bytes */
} bh_gather_params;
int bh_gather(const bh_gather_params* p, bh_stream_t s);
/* the kernel bh_gather dispatches to ("" for refused parameters) */
const char* bh_gather_kernel(const bh_gather_params* p);
/* the refusals above alone; pure host */
int bh_gather_check(const bh_gather_params* p);

/* BATCH_MATMUL: out[b0, b1] = lhs[b0, b1] x rhs[b0, b1], an [m, k] by [k, n]
 * product per batch index; both operands may be activations.  The output is
 * dense [batch[0], batch[1], m, n].  An operand is given by strides (in
 * elements), so a transposed (adj_x / adj_y) or broadcast (batch stride 0)
 * operand is data: exactly one of an operand's two matrix strides is 1 (both
 * may be when one of its extents is 1).
 *   int8 (bh_batch_matmul_i8, bmm_mfma_kernel):
 *     out = clamp(MBQM(sum_k (lhs - lhs_zp)(rhs - rhs_zp), mult, shift) + out_zp, -128, 127)
 *     with one per-tensor (mult, shift); k <= 32767.  requant_fast: 0 the
 *     two-step form, 1 / -1 the single-step form where
 *     bh_conv_requant_fast_ok(&mult, &shift, 1, k, 0) holds (else two-step).
 *   float32 (bh_batch_matmul_f32, bmm_f32_kernel): the plain float32 sum; the
 *     quantisation fields are ignored.
 * Refused (BH_EINVAL, bh_last_error names the launcher and the reason): null
 * pointers, non-positive extents, a batch dim above 65535, k above the limit,
 * negative strides, an operand without exactly one unit stride, 2^31 or more
 * elements in a tensor.  No scratch, no atomics. */
#define BH_BMM_AUTO 0
/* kernel_hint bits (parity tests, A-B timing) */
#define BH_BMM_BYTES 1 /* 1-byte fragment units whatever the alignment */
#define BH_BMM_NT1 2   /* one 16-column tile per wave whatever the grid */
#define BH_BMM_NT4 4   /* four 16-column tiles per wave whatever the grid */
/* the transposed read of a K-strided (staged) operand */
#define BH_BMM_READ_B128 8    /* transposing LDS writes, one ds_read_b128 */
#define BH_BMM_READ_GATHER 16 /* row-major LDS image, 16 byte reads */
#define BH_BMM_READ_TR8 32    /* row-major LDS image, two ds_read_b64_tr_b8 */
typedef struct bh_batch_matmul_params {
  int32_t batch[2], m, n, k;
  int64_t lhs_bstride[2], rhs_bstride[2]; /* 0 = broadcast */
  int64_t lhs_row_stride, lhs_k_stride;
  int64_t rhs_k_stride, rhs_col_stride;
  int32_t lhs_zp, rhs_zp, out_zp, mult, shift, requant_fast, kernel_hint;
  const void* lhs;
  const void* rhs;
  void* out;
} bh_batch_matmul_params;
int bh_batch_matmul_i8(const bh_batch_matmul_params* p, bh_stream_t s);
/* "bmm_mfma_kernel", or "" for parameters bh_batch_matmul_i8 refuses; static storage */
const char* bh_batch_matmul_i8_kernel(const bh_batch_matmul_params* p);
int bh_batch_matmul_f32(const bh_batch_matmul_params* p, bh_stream_t s);
/* the launchers' parameter checks alone (elem_bytes 1: int8, 4: float32); pure host */
int bh_batch_matmul_check(const bh_batch_matmul_params* p, int elem_bytes);

/* RESIZE_BILINEAR (int8) followed by ARG_MAX / ARG_MIN over the channel axis
 * as one launch (resize_bilinear_argminmax_kernel): the resized tensor is
 * never stored.  Per output pixel the channel values are the same integer
 * expression as bh_resize_bilinear_i8's column form, walked c = 0 .. C-1 with
 * the first extreme kept.  output: [batch][out_h][out_w] indices.  A
 * workgroup stages the vertically blended input rows (int32, one padded row
 * of in_w * (channels | 1) words per output row) and the column tables in
 * LDS; geometries needing more than 64 KB of it, or more than 1024 output
 * columns, are refused (BH_EINVAL, bh_last_error names the reason) and the
 * caller runs the two launches.  bh_resize_bilinear_argminmax_i8_ok: the
 * same check without a launch (0 = would run). */
typedef struct {
  bh_resize_bilinear_params rz;   /* rz.output: the index map */
  int is_min;
  int out_bytes;                  /* 4 / 8 */
} bh_resize_argminmax_params;
int bh_resize_bilinear_argminmax_i8(const bh_resize_argminmax_params* p, bh_stream_t s);
int bh_resize_bilinear_argminmax_i8_ok(const bh_resize_argminmax_params* p);

/* RESIZE_BILINEAR uint8 (TFLite 2.9.2 optimized_ops::ResizeBilinear for
 * uint8 -> ResizeBilinearGenericSmallChannel<uint8>): float interpolation.
 * Host tables from ComputeInterpolationValues (float scale, floor / ceil):
 * y_idx [2*out_h] = {y0, y1}, y_frac [out_h] = input_y - y0 (float), same
 * for x.  Per output byte, in float with no contraction:
 *   (uint8)(v00*(1-dy)(1-dx) + v01*(1-dy)dx + v10*dy(1-dx) + v11*dy*dx + 0.5f)
 * summed left to right as the reference's expression. */
typedef struct {
  int batch, in_h, in_w, channels, out_h, out_w;
  const int32_t* y_idx;
  const int32_t* x_idx;
  const float* y_frac;
  const float* x_frac;
  const void* input;
  void* output;
} bh_resize_bilinear_u8_params;
int bh_resize_bilinear_u8(const bh_resize_bilinear_u8_params* p, bh_stream_t s);

typedef struct {
  long rows;
  int depth;                      /* softmax over the last dim */
  int is_signed;                  /* int8 (1) or uint8 (0), input and output */
  const float* table;             /* [256] device: table[255 - v] = expf(-in_scale * beta * v) */
  float out_scale;
  int32_t out_zp;
  const void* input;
  void* output;
} bh_softmax_params;
int bh_softmax_i8(const bh_softmax_params* p, bh_stream_t s);

/* The int8 attention core as one launch (attention_i8_kernel):
 *   out[b0, b1] = BATCH_MATMUL(SOFTMAX(BATCH_MATMUL(q[b0, b1], k[b0, b1]^T)), v[b0, b1])
 * on q [rows, head_dim], k [keys, head_dim], v [keys, out_dim] and out
 * [rows, out_dim] per batch index.  The stored bytes are those of
 * bh_batch_matmul_i8 (both operands K-contiguous) -> bh_softmax_i8 (int8) ->
 * bh_batch_matmul_i8 (rhs K-strided): the scores are requantised and clamped
 * to int8 before the softmax, the probabilities are int8 before the second
 * product, and the softmax's row sum is the float32 sum over the keys in
 * order.  Scores and probabilities live in LDS only.
 *   Operands by strides in elements (two batch strides, 0 = broadcast, a row
 * stride and an inner stride that must be 1), so [B, T, H, D] tensors are
 * read and written as [B, H, T, D] without a TRANSPOSE.
 *   qk / pv: each product's quantisation as bh_batch_matmul_params carries it
 * (pv.lhs_zp is the probabilities' zero point); table / sm_out_scale /
 * sm_out_zp as bh_softmax_params carries them.
 *   A workgroup holds 64 query rows' scores in an LDS strip of 64 x
 * (roundup(keys, 64) + 16) bytes, hence keys <= BH_ATTENTION_MAX_KEYS, and
 * each wave keeps its q fragments in registers, hence head_dim <= 128; out_dim
 * <= 128 (eight accumulator tiles per wave).
 * Refused (BH_EINVAL, bh_last_error names the reason): null pointers,
 * non-positive extents, keys / head_dim / out_dim above their limits, a batch
 * dim above 65535, negative strides, a non-unit inner stride, 2^31 or more
 * elements in a tensor (a batch or row stride of 2^31 or more counts as
 * that, whatever its extent, for the masked and the unmasked form alike:
 * the check's span sums then stay inside 64 bits), a multiplier / shift out
 * of range.  No scratch, no
 * atomics.
 *   The masked form (attention_bias_i8_kernel, bias != NULL): an int8 tensor
 * is ADDed to the scores before the softmax,
 *   out = BATCH_MATMUL(SOFTMAX(ADD(BATCH_MATMUL(q, k^T), bias)), v)
 * and the stored bytes are those of bh_batch_matmul_i8 -> bh_eltwise_i8
 * (BH_ELT_ADD) -> bh_softmax_i8 -> bh_batch_matmul_i8.  It is a padding mask
 * [b0, 1, 1, keys], a causal mask [1, 1, rows, keys] or a position bias
 * [1, b1, rows, keys] alike: the bias is read at bias_bstride[0] b0 +
 * bias_bstride[1] b1 + bias_row_stride row + bias_key_stride key (elements; 0
 * broadcasts that extent; bias_key_stride is 0 or 1) and is only read.  `add`
 * holds the ADD's constants as bh_eltwise_params carries them, a / b being
 * the ADD's first / second operand; add_scores_operand says which of the two
 * is the scores (0: a, 1: b), the other is the bias.  `table` is then the
 * softmax table of the ADD output's scale.  The new fields all zero: no bias.
 * Refused in addition: a negative bias stride, a bias_key_stride other than 0
 * or 1, a bias span of 2^31 or more elements, an ADD input shift above 0 (any
 * of the three shifts outside -31 .. 0), a left_shift outside 0 .. 31,
 * act_min > act_max, add_scores_operand other than 0 or 1.  (left_shift: TFLite's
 * int8 ADD uses 20; with 8-bit operands (q + off) << left_shift stays inside 32
 * bits up to 22, and above that the product wraps on the device exactly as
 * bh_eltwise_i8's does, so the four launches' bytes are still what is stored,
 * but they are not an ADD's any more.) */
#define BH_ATTENTION_MAX_KEYS 1024
#define BH_ATTENTION_MAX_DIM 128
/* kernel_hint bits (parity tests) */
#define BH_ATTN_BYTES 1 /* 1-byte fragment units whatever the alignment */
typedef struct bh_attention_quant {
  int32_t lhs_zp, rhs_zp, out_zp, mult, shift, requant_fast;
} bh_attention_quant;
/* the constants of an int8 ADD, in bh_eltwise_params' order: the negated zero
 * points of a and b, the output zero point, ... */
typedef struct bh_attention_add {
  int32_t a_off, b_off, o_off, left_shift, a_mult, a_shift, b_mult, b_shift, o_mult, o_shift, act_min, act_max;
} bh_attention_add;
typedef struct bh_attention_params {
  int32_t batch[2], rows, keys, head_dim, out_dim;
  int64_t q_bstride[2], k_bstride[2], v_bstride[2], out_bstride[2];
  int64_t q_row_stride, k_row_stride, v_row_stride, out_row_stride;
  int64_t q_inner_stride, k_inner_stride, v_inner_stride, out_inner_stride; /* 1 */
  bh_attention_quant qk, pv;
  const float* table; /* [256] device: bh_softmax_params.table of the scores' scale */
  float sm_out_scale;
  int32_t sm_out_zp;
  int32_t kernel_hint;
  const void* q;
  const void* k;
  const void* v;
  void* out;
  /* the masked form; all zero = no bias */
  const void* bias; /* int8, NULL = none */
  int64_t bias_bstride[2], bias_row_stride, bias_key_stride;
  bh_attention_add add;
  int32_t add_scores_operand; /* 0: the scores are the ADD's a, 1: its b */
} bh_attention_params;
int bh_attention_i8(const bh_attention_params* p, bh_stream_t s);
/* "attention_i8_kernel" ("attention_bias_i8_kernel" with a bias), or "" for parameters bh_attention_i8 refuses;
 * static storage */
const char* bh_attention_i8_kernel(const bh_attention_params* p);
/* the launcher's parameter checks alone; pure host, 0 = would run */
int bh_attention_i8_check(const bh_attention_params* p);
/* bytes of LDS a launch of these extents takes (0 for refused parameters) */
size_t bh_attention_i8_lds_bytes(const bh_attention_params* p);

/* Dynamic-range ("hybrid") FULLY_CONNECTED: float32 input, constant int8
 * weights [units][depth] with one scale and zero point 0, float32 output.
 * Restated from memory of TFLite's fully_connected.cc EvalHybrid and
 * tensor_utils::{Symmetric,Asymmetric}QuantizeFloats (DESIGN 4 holds the rule
 * and what is pinned).  Every float operation is one IEEE float32 operation
 * (float64 where marked), no contraction; round is half away from zero.
 *
 * bh_dynquant_rows (dynquant_rows_kernel, one wave per row) quantises each
 * row x of input [rows][depth] on its own:
 *   symmetric   r = max |x|; r == 0: q = 0, s = 1; else s = r / 127,
 *               inv = 127 / r, q = clamp(round(x inv), -127, 127); off = 0.
 *   asymmetric  rmin = min(0, min x), rmax = max(0, max x); equal: q = 0,
 *               s = 1, off = 0; else in float64 scale = (rmax - rmin) / 255
 *               (the difference in float32), off = the zero point nudged from
 *               the end with the smaller error, clamped to [-128, 127];
 *               s = (float)scale, inv = 1 / s,
 *               q = clamp(round((float)off + x inv), -128, 127).
 * into q [rows][depth], scale [rows], offset [rows].  Any depth.
 *
 * bh_fc_hybrid (fc_hybrid_kernel, v_mfma_i32_16x16x64_i8):
 *   dot = sum_k w[u][k] q[k] - off * w_row_sum[u]           (int32, exact)
 *   y = bias[u] + (float)dot * (s * w_scale), clamped to [act_min, act_max]
 * (a missing bias adds 0).  weights are packed [units][depth_pad] with
 * depth_pad a multiple of 16 and the padding zero, 16-byte aligned;
 * w_row_sum [units] = sum_k w[u][k], built once by the caller.  Rows <= 16
 * (the classifier head) spread a workgroup's 4 waves over unit tiles or over
 * K slices whose partial sums are added as integers.
 * Refused (BH_EINVAL, bh_last_error names the launcher and the reason): null
 * pointers, non-positive extents, depth > 65,535 (bh_fc_hybrid: the int32
 * dot), 2^31 or more elements in a tensor, a bad depth_pad, misaligned
 * operands.  No scratch, no atomics. */
typedef struct bh_dynquant_params {
  long rows;
  int depth;
  int asymmetric;
  const float* input;   /* [rows][depth] */
  int8_t* q;            /* [rows][depth] */
  float* scale;         /* [rows] */
  int32_t* offset;      /* [rows] */
} bh_dynquant_params;
int bh_dynquant_rows(const bh_dynquant_params* p, bh_stream_t s);
/* "dynquant_rows_kernel", or "" for parameters bh_dynquant_rows refuses; static storage */
const char* bh_dynquant_rows_kernel(const bh_dynquant_params* p);
/* the launcher's parameter check alone; pure host */
int bh_dynquant_rows_check(const bh_dynquant_params* p);

typedef struct bh_fc_hybrid_params {
  int rows, depth, depth_pad, units;
  float w_scale, act_min, act_max;
  const int8_t* q;            /* [rows][depth] */
  const float* in_scale;      /* [rows] */
  const int32_t* in_offset;   /* [rows] */
  const int8_t* weights;      /* [units][depth_pad] */
  const int32_t* w_row_sum;   /* [units] */
  const float* bias;          /* [units] or NULL */
  float* output;              /* [rows][units] */
} bh_fc_hybrid_params;
int bh_fc_hybrid(const bh_fc_hybrid_params* p, bh_stream_t s);
/* "fc_hybrid_kernel", or "" for parameters bh_fc_hybrid refuses; static storage */
const char* bh_fc_hybrid_kernel(const bh_fc_hybrid_params* p);
/* the launcher's parameter check alone; pure host */
int bh_fc_hybrid_check(const bh_fc_hybrid_params* p);

/* Dynamic-range ("hybrid") CONV_2D / DEPTHWISE_CONV_2D: float32 input,
 * constant int8 filter (OHWI; [1][kh][kw][out_c] depthwise) with zero points
 * 0, float32 output.  Restated from memory of TFLite's conv.cc EvalHybrid /
 * EvalHybridPerChannel, depthwise_conv.cc EvalHybridPerChannel and the
 * reference hybrid kernels - their source was not at hand (DESIGN 4 holds the
 * rule and says what is pinned).  Every float operation is one IEEE float32
 * operation (float64 where the row rule above marks it), no contraction.
 *
 * bh_dynquant_items quantises each batch item - the item_size = H W C floats
 * of one image - on its own by exactly the row rule of bh_dynquant_rows with
 * the item as the row, into q [items][item_size], scale [items], offset
 * [items].  Two forms.  One launch (dynquant_item_kernel): a workgroup per
 * item takes the item's min and max, derives (s, inv, off) and quantises.
 * Two launches: dynquant_minmax_kernel writes one (min, max) pair per
 * BH_DYNQUANT_CHUNK floats into `pairs` [items][chunks][2]; in
 * dynquant_items_kernel every workgroup reduces its item's pairs (min and max
 * are exact in any order), derives the same three values and quantises its
 * chunk, and the item's first workgroup stores s and off.  No atomics, no
 * waiting across workgroups.  form 0 picks by item_size (one launch up to
 * BH_DYNQUANT_ONE_LAUNCH_MAX floats), 1 / 2 force a form.  `pairs` may be
 * null where the one-launch form is taken.
 *
 * bh_conv2d_hybrid (conv_hybrid_kernel, v_mfma_i32_16x16x64_i8, the implicit
 * im2col GEMM M = batch out_h out_w, N = out_c, K = k_h k_w in_c):
 *   acc = sum over the in-bounds taps of w (q - off[b])       (int32, exact)
 *   one filter scale (per_channel 0; the input quantised symmetrically, off 0):
 *     y = bias[c] + (float)acc * (s[b] * ws)
 *   out_c filter scales (per_channel 1; the input quantised asymmetrically):
 *     y = ((float)acc * ws[c]) * s[b] + bias[c]
 * the kernel fills a padded tap with the byte off[b] and subtracts
 * off[b] * w_row_sum[c] (the sum over all taps), the same integer.
 * bh_dwconv2d_hybrid (dwconv_hybrid_kernel, VALU, a lane per 4 output
 * channels of a pixel; out_c scales):
 *   y = (float)acc * (ws[c] * s[b]) + bias[c]
 * All clamp to [act_min, act_max]; a missing bias adds 0.  weights: conv
 * [out_c][k_pad], k_pad = K rounded up to 16, zero padding, 16-byte aligned;
 * depthwise [k_h k_w][out_c] as the flatbuffer holds them.  w_scale is
 * [out_c] in every form (one scale: repeated).  w_row_sum [out_c] is read by
 * bh_conv2d_hybrid only.
 * Refused (BH_EINVAL, bh_last_error names the launcher and the reason): null
 * pointers, non-positive extents, K > 65,535 (the int32 sum), 2^31 or more
 * elements in a tensor, a bad k_pad or depth multiplier, an output shape that
 * reads outside the padded input, misaligned operands. */
#define BH_DYNQUANT_CHUNK 4096
#define BH_DYNQUANT_ONE_LAUNCH_MAX 16384
typedef struct bh_dynquant_items_params {
  int items, item_size;
  int asymmetric;
  int form;             /* 0: by item_size; 1: one launch; 2: two launches */
  const float* input;   /* [items][item_size] */
  int8_t* q;            /* [items][item_size] */
  float* scale;         /* [items] */
  int32_t* offset;      /* [items] */
  float* pairs;         /* [items][ceil(item_size / BH_DYNQUANT_CHUNK)][2]; two-launch form */
} bh_dynquant_items_params;
int bh_dynquant_items(const bh_dynquant_items_params* p, bh_stream_t s);
/* "dynquant_item_kernel" or "dynquant_minmax_kernel+dynquant_items_kernel", or "" when refused; static storage */
const char* bh_dynquant_items_kernel(const bh_dynquant_items_params* p);
int bh_dynquant_items_check(const bh_dynquant_items_params* p);

typedef struct bh_conv_hybrid_params {
  int batch, in_h, in_w, in_c, out_h, out_w, out_c;
  int k_h, k_w, stride_h, stride_w, dil_h, dil_w, pad_h, pad_w;
  int k_pad;             /* bh_conv2d_hybrid: K padded to 16 */
  int depth_multiplier;  /* bh_dwconv2d_hybrid: out_c / in_c */
  int per_channel;       /* bh_conv2d_hybrid: which epilogue */
  float act_min, act_max;
  const int8_t* q;            /* [batch][in_h][in_w][in_c] */
  const float* in_scale;      /* [batch] */
  const int32_t* in_offset;   /* [batch] */
  const int8_t* weights;
  const int32_t* w_row_sum;   /* [out_c]; conv only */
  const float* w_scale;       /* [out_c] */
  const float* bias;          /* [out_c] or NULL */
  float* output;              /* [batch][out_h][out_w][out_c] */
} bh_conv_hybrid_params;
int bh_conv2d_hybrid(const bh_conv_hybrid_params* p, bh_stream_t s);
const char* bh_conv2d_hybrid_kernel(const bh_conv_hybrid_params* p);  /* "conv_hybrid_kernel" or "" */
int bh_conv2d_hybrid_check(const bh_conv_hybrid_params* p);
int bh_dwconv2d_hybrid(const bh_conv_hybrid_params* p, bh_stream_t s);
const char* bh_dwconv2d_hybrid_kernel(const bh_conv_hybrid_params* p);  /* "dwconv_hybrid_kernel" or "" */
int bh_dwconv2d_hybrid_check(const bh_conv_hybrid_params* p);

/* TRANSPOSE_CONV support: U[y*sh][x*sw][:] = in[y][x][:], every other
 * position of U (out_h x out_w = (in-1)*stride+1) holds `fill` (the input
 * zero point, so it contributes 0).  A transpose conv is then a stride-1
 * CONV_2D over U with spatially flipped filters and padding k-1-pad. */
typedef struct {
  int batch, in_h, in_w, channels, stride_h, stride_w, out_h, out_w;
  uint32_t fill;                  /* byte */
  const void* input;
  void* output;
} bh_zero_insert_params;
int bh_zero_insert(const bh_zero_insert_params* p, bh_stream_t s);

/* TFLite_Detection_PostProcess, fast (class-agnostic) NMS with one class per
 * detection (detection_postprocess.cc DecodeCenterSizeBoxes +
 * MultiClassFastNMS), for `batch` images that share one anchor table.
 * Two kernels: detection_score_kernel (per anchor the first maximum over the
 * non-background classes, keyed as score descending / anchor ascending) and
 * detection_nms_kernel (one workgroup per image: candidates compacted in
 * anchor order, their boxes decoded in double, then at most max_detections
 * rounds of "take the largest active key, suppress every active candidate
 * whose IoU with it is > iou_threshold").  Outputs per image: boxes
 * [max_detections][4] (ymin xmin ymax xmax), classes, scores, num (float);
 * rows past num are zero.
 * box_type / score_type: 0 float32, 1 int8, 2 uint8; an 8-bit input is
 * dequantised as scale * (q - zero_point) (a DEQUANTIZE folded into the op:
 * the maximum is taken over the bytes, scale > 0 required).
 * scratch: bh_detection_scratch_bytes(batch, num_boxes) device bytes, fully
 * rewritten by every call (no state survives a call). */
typedef struct bh_detection_params {
  int batch, num_boxes, num_classes, num_classes_with_background, max_detections;
  float score_threshold, iou_threshold;
  float scale_y, scale_x, scale_h, scale_w;
  int box_type, score_type;
  float box_scale, score_scale;
  int32_t box_zp, score_zp;
  const void* box_encodings;      /* [batch][num_boxes][4] */
  const void* class_scores;       /* [batch][num_boxes][num_classes_with_background] */
  const float* anchors;           /* [num_boxes][4] ycenter xcenter h w */
  float* out_boxes;
  float* out_classes;
  float* out_scores;
  float* out_num;                 /* [batch] */
  void* scratch;
} bh_detection_params;
size_t bh_detection_scratch_bytes(int batch, int num_boxes);
int bh_detection_postprocess(const bh_detection_params* p, bh_stream_t s);

/* human-readable name of the last error set on this thread */
const char* bh_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* BAND_HIP_KERNELS_H_ */
