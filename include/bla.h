/*
 * bla.h -- C-ABI of the MI355X (gfx950) backend for the dense linear-algebra hot
 * path of damians13/big-linear-algebra.
 *
 * Plain C: pointers, ints and floats only -- no HIP, torch or C++ types.  The
 * host side (big-linear-algebra_amd/lib/ *.c, compiled by gcc, API-identical to
 * the reference's lib/matrix.h, lib/conv.h, lib/norm.h, lib/util.h, lib/layer.h)
 * and the Python tests/bench bind exactly these symbols.
 *
 * Conventions
 *   - every matrix is dense row-major fp32, element (r,c) at p[r*ld + c]
 *     (the reference's Matrix layout, lib/matrix.h:6-11, with ld = cols);
 *   - pointers named d_* / "device" are device pointers (bla_malloc or any HIP
 *     allocation, e.g. a torch tensor's data_ptr());
 *   - `stream` is a hipStream_t passed as void*; NULL = the library's own stream;
 *   - every entry point returns a bla_status (0 = BLA_OK); bla_last_error()
 *     gives the text.  Nothing here ever falls back to a CPU implementation:
 *     without a usable device every compute call fails with BLA_ERR_NO_DEVICE.
 *   - launches are asynchronous on `stream`; call bla_stream_sync to wait.
 *
 * Each compute entry point cites the reference function it replaces.
 */
#ifndef BLA_H
#define BLA_H

#include <stddef.h>
#include <stdint.h>

#if defined(BLA_BUILDING)
#define BLA_API __attribute__((visibility("default")))
#else
#define BLA_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef int bla_status;
enum {
	BLA_OK = 0,
	BLA_ERR_INVALID = 1,   /* bad argument (null pointer, negative size, ld too small) */
	BLA_ERR_SHAPE = 2,     /* operand shapes do not conform */
	BLA_ERR_NO_DEVICE = 3, /* no usable gfx950 device / runtime not initialised */
	BLA_ERR_HIP = 4,       /* a HIP runtime call failed; see bla_last_error() */
	BLA_ERR_UNDEFINED = 5, /* the reference itself is undefined here (e.g. col2im with stride != 1) */
	BLA_ERR_TIMEOUT = 6    /* a rank of the gradient exchange never arrived (bla_dp_check) */
};

/* ---- runtime -------------------------------------------------------------- */
BLA_API bla_status bla_init(int device);            /* select device, create stream + workspace; idempotent */
BLA_API bla_status bla_shutdown(void);
BLA_API int bla_is_initialized(void);
BLA_API int bla_device_count(void);          /* 0 when no device / no driver */
BLA_API const char* bla_last_error(void);
BLA_API const char* bla_status_string(bla_status s);
BLA_API const char* bla_version(void);
BLA_API bla_status bla_device_name(char* buf, int buflen);   /* gcnArchName of the active device */

/* Further contexts beside the default one bla_init creates: a context = {device, stream, split-K workspace, arrival counters}.
 * A host that drives several GPUs -- or several replicas on one GPU -- from ONE process ("single-process multi-device,
 * one host thread or one stream per device") creates one context per rank and makes it current on the calling thread before it issues
 * that rank's bla_* calls; NULL = back to the default context.  Objects (trainers, exchange objects, device memory) belong to the
 * device of the context that was current when they were created. */
typedef struct bla_context bla_context;
BLA_API bla_status bla_context_create(bla_context** out, int device);
BLA_API bla_status bla_context_set_current(bla_context* c);
BLA_API bla_status bla_context_destroy(bla_context* c);   /* BLA_ERR_INVALID while the context is current on another thread (set NULL there first, also before that thread ends) */

/* libc rand() belongs to the calling program (the reference's programs seed it once and draw from it between library calls: sampler
 * lib/mnist_csv2.c:36-62, dropout model/cifar_unet.c:1032-1042), but HIP runtime start-up and RCCL set-up draw from it too.  Every library
 * entry that reaches them parks the caller's stream by itself; a host program that makes such calls ITSELF brackets them with this pair.
 * Process-wide and nestable: the first enter (any thread) parks the stream, the last leave puts it back.  While a guard is open other threads
 * must not draw from rand() and expect the program's stream. */
BLA_API void bla_rand_guard_enter(void);
BLA_API void bla_rand_guard_leave(void);

BLA_API bla_status bla_malloc(void** d_ptr, size_t bytes);
BLA_API bla_status bla_free(void* d_ptr);
BLA_API bla_status bla_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes, void* stream);
BLA_API bla_status bla_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes, void* stream);
BLA_API bla_status bla_memcpy_d2d(void* d_dst, const void* d_src, size_t bytes, void* stream);
BLA_API bla_status bla_memset(void* d_dst, int byte, size_t bytes, void* stream);
BLA_API bla_status bla_stream_sync(void* stream);
BLA_API void* bla_default_stream(void);

/* Wall-clock free device timers (HIP events on `stream`) for bench.py's roofline leg. */
BLA_API bla_status bla_event_create(void** ev);
BLA_API bla_status bla_event_destroy(void* ev);
BLA_API bla_status bla_event_record(void* ev, void* stream);
BLA_API bla_status bla_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* syncs on ev_stop */

/* Launch-bound sequences (one image through a U-Net block is a dozen launches of a few microseconds): record any sequence of
 * bla_* calls issued on `stream` between begin and end into a hipGraph and replay it with one launch.  Run the sequence once
 * eagerly first -- scratch buffers and gather tables are created on first use, and allocating is not allowed while recording.
 * The recorded calls are not executed during recording; pointers and sizes are frozen into the graph. */
/* diagnostics: `blocks` workgroups of `waves` wavefronts each issue iters x 8 independent fp32 MFMAs (32x32x2) and nothing else --
 * the practical ceiling of the matrix pipe (tools/mfma_peak.py) */
BLA_API bla_status bla_diag_mfma_rate(void* stream, int blocks, int waves, int iters, float* d_sink);
BLA_API bla_status bla_graph_begin(void* stream);
BLA_API bla_status bla_graph_end(void* stream, void** graph);
BLA_API bla_status bla_graph_launch(void* graph, void* stream);
BLA_API bla_status bla_graph_destroy(void* graph);

/* ---- GEMM: replaces matrix_multiply_inplace / matrix_multiply (lib/matrix.c:35-57)
 * and every matrix_transpose + multiply + transpose-back sandwich around it
 * (model/mnist_nn.c:267-292, lib/conv.c:221-227) via transa/transb.
 *
 *   C[m x n] = epilogue( alpha * op(A)[m x k] . op(B)[k x n] )
 *   op(A) = A (m x k, lda >= k) if !transa, else A^T with A stored k x m (lda >= m)
 *   op(B) = B (k x n, ldb >= n) if !transb, else B^T with B stored n x k (ldb >= k)
 *
 * Arithmetic: fp32 MFMA (v_mfma_f32_32x32x2_f32), one fp32 rounding per product,
 * fp32 accumulation; summation order over k differs from the reference's
 * k-ascending scalar chain (documented tolerance: DESIGN.md).
 *
 * Epilogue, applied in this order to v = alpha*acc (all optional, NULL/0 = off):
 *   v += bias_row[r]          bias per output ROW  (matrix_add_tile_columns with an m x 1 b, lib/matrix.c:189-195)
 *   v += bias_col[c]          bias per output COLUMN (matrix_add_tile_rows, lib/matrix.c:199-205)
 *   pre_act[r*ld_pre + c] = v   (keeps Z next to A = act(Z), model/mnist_nn.c:221-224)
 *   act == BLA_ACT_RELU: v = v < 0 ? 0 : v        (lib/util.c:7-13)
 *   relu_mask: v *= (relu_mask[r*ld_mask + c] > 0 ? 1 : 0)   (relu_ddx + hadamard, model/mnist_nn.c:276-278)
 *   beta != 0: v += beta * C[r*ldc + c]
 * A NULL epilogue means alpha = 1 and nothing else.  When passing a struct, zero-initialise it and set alpha.
 */
enum { BLA_ACT_NONE = 0, BLA_ACT_RELU = 1 };

typedef struct bla_gemm_epilogue {
	float alpha;               /* 0 is NOT treated specially; use 1.0f for a plain product */
	float beta;
	const float* bias_row;     /* device, length m, or NULL */
	const float* bias_col;     /* device, length n, or NULL */
	float* pre_act;            /* device m x n (ld_pre), or NULL */
	int ld_pre;
	int act;                   /* BLA_ACT_* */
	const float* relu_mask;    /* device m x n (ld_mask), or NULL */
	int ld_mask;
	/* by-products fused into the latency-bound kernels (run as separate passes elsewhere):
	 *   row_sum_a[r] = sum_k A[r][k] (needs !transa): with A = dZ this is the bias gradient "sum over the batch
	 *   columns", the documented intent of matrix_col_sum (model/mnist_nn.c:271,282,293);
	 *   softmax_y/softmax_grad (m <= 32, no other post-op than bias_row/pre_act): C = column softmax of the result,
	 *   softmax_grad = (C - softmax_y) * softmax_scale, both with leading dimension ldc (model/mnist_nn.c:234,260-268). */
	float* row_sum_a;
	const float* softmax_y;
	float softmax_scale;
	float* softmax_grad;
	/* row_sum_a[r] = row_sum_beta * row_sum_a[r] + row_sum_alpha * sum_k A[r][k]; both 0 (a zero-initialised struct) = plain store of the
	 * sum.  With alpha = learn rate, beta = 1 the bias update b += lr * db rides along the weight-gradient product (latency-bound kernels only). */
	float row_sum_alpha, row_sum_beta;
	/* with the fused softmax tail: per-COLUMN accumulators (length n) of the reference's loss / accuracy bookkeeping, model/mnist_nn.c:237-257:
	 *   softmax_loss_acc[c]    += -sum_r y[r][c] * log(p[r][c] + 1e-15)            (double, LOSS_EPSILON of :15)
	 *   softmax_correct_acc[c] += y[pred][c] == 1, pred = first row with the largest probability (> 0)
	 * both NULL = off.  Summed over the columns they are the batch totals the reference adds into its epoch averages. */
	double* softmax_loss_acc;
	unsigned* softmax_correct_acc;
} bla_gemm_epilogue;

BLA_API bla_status bla_gemm_f32(void* stream, int transa, int transb, int m, int n, int k,
                        const float* d_a, int lda, const float* d_b, int ldb,
                        float* d_c, int ldc, const bla_gemm_epilogue* ep /* NULL = plain product */);
/* Two independent products (neither reads what the other writes) issued together: when both are latency-bound shapes they
 * share one launch and overlap -- dW_l = dZ_l.A^T beside dZ_{l-1} = W_l^T.dZ_l in model/mnist_nn.c:267-289, which the
 * reference runs one after the other.  Otherwise identical to two bla_gemm_f32 calls. */
typedef struct bla_gemm_desc {
	int transa, transb, m, n, k;
	const float* A; int lda;
	const float* B; int ldb;
	float* C; int ldc;
	const bla_gemm_epilogue* ep;   /* may be NULL */
} bla_gemm_desc;
BLA_API bla_status bla_gemm_pair_f32(void* stream, const bla_gemm_desc* p, const bla_gemm_desc* q);
/* Up to three independent products; three latency-bound ones with K-contiguous operands on both sides (transa = 0, transb = 1: the three
 * weight gradients of one MNIST-NN step, model/mnist_nn.c:267-292) share ONE launch.  Otherwise identical to separate calls. */
BLA_API bla_status bla_gemm_group_f32(void* stream, const bla_gemm_desc* descs, int count);

/* Tuning/diagnostics: force a tile configuration (-1 = automatic) and split-K factor (0 = automatic).  Configurations
 * (csrc/bla_gemm.hip): 0-2 register-staged tiles (any shape); 3/4/5/7 direct-to-LDS 128x128x16, 64x64x16, 128x128x32, 128x64x16
 * (16-byte aligned operands, k a multiple of the slab depth); 6 wave-split-K 32x32 for latency-bound shapes (16: its 16x16-tile form, which the automatic
 * choice takes when the 32x32 tiling would leave CUs idle); 8/9 256x128-class
 * three-buffer tiles; 10 persistent 128x128; 11/12/13 the one-workgroup-per-CU half-slab kernels 256x256x16, 256x256x32, 128x512x16
 * and 14 / 15 / 17 their 128x128, 128x256 and 192x192 forms (whole tiles, plain alpha epilogue only; the automatic choice takes the one whose tile count
 * is a whole number of rounds over the CUs); 18: 64x64 tiles on 32-deep slabs with two wave groups along K (1024^3-class products, one or two tiles
 * per CU).  A forced configuration that cannot take the call fails with
 * BLA_ERR_INVALID; the automatic choice never does. */
BLA_API bla_status bla_gemm_set_config(int config, int split_k);
/* Name of the kernel variant the last bla_gemm_f32 / _pair / _group / _batched call launched (for profiles/); where such a call made several
 * launches, the last one it issued (products of a pair or group that wait for a shared launch and then go alone are issued after the others). */
BLA_API const char* bla_gemm_last_kernel(void);

/* ---- mixed precision: bf16 operands, fp32 accumulation, on the bf16 matrix instructions (csrc/bla_gemm_bf16.hip) ------------------------------
 * A bf16 value is its 16-bit pattern in a uint16_t: the upper half of the IEEE fp32 encoding.
 *
 * Conversions over a 2-D window (rows x cols, pitches in elements; rows = 1 is the flat form).  fp32 -> bf16 rounds to nearest even: a NaN gives a NaN
 * (pattern (u >> 16) | 0x40), +-inf, +-0 and subnormals keep their value (nothing is flushed), a finite value above the largest bf16 rounds to inf, and
 * everything else is (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the fp32 bit pattern u.  bf16 -> fp32 is the exact widening u16 << 16.  Only the window is
 * written.  16-byte accesses when bases and pitches allow them (fp32 side: 16-byte base, pitch % 4 == 0; bf16 side: 16-byte base, pitch % 8 == 0). */
BLA_API bla_status bla_f32_to_bf16(void* stream, const float* d_src, int ld_src, uint16_t* d_dst, int ld_dst, int rows, int cols);
BLA_API bla_status bla_bf16_to_f32(void* stream, const uint16_t* d_src, int ld_src, float* d_dst, int ld_dst, int rows, int cols);
/* dst (cols x rows, ld_dst >= rows) = src^T for src (rows x cols, ld_src >= cols) of 16-bit elements, out of place, bit-exact: 64 x 64 tiles through
 * LDS, 16-byte accesses on either side whose base is 16-byte aligned with a pitch that is a multiple of 8 (2-byte accesses otherwise and at the edges). */
BLA_API bla_status bla_transpose_b16(void* stream, const uint16_t* d_src, int ld_src, uint16_t* d_dst, int ld_dst, int rows, int cols);

/*   C[m x n] = epilogue( alpha * op(A)[m x k] . op(B)[k x n] ),  A and B bf16, accumulation and epilogue in fp32
 * op(), the pitches, transa and transb mean exactly what they mean for bla_gemm_f32.  C is fp32 (BLA_C_F32: d_c is a float*) or bf16 (BLA_C_BF16: d_c is a
 * uint16_t*, rounded to nearest even ONCE, after the whole epilogue); ldc in elements of C's type.  Of the epilogue, alpha, beta, bias_row, bias_col and act
 * are honoured, in bla_gemm_f32's order; with beta != 0, C is read in its own type.  Any other field non-NULL or non-zero: BLA_ERR_INVALID, nothing is
 * launched.  NULL = a plain product.  Products of two bf16 values are exact in fp32, so the only error is that of the fp32 accumulation.
 *
 * Dispatch.  The fast path is a 128 x 128 x 64 tile kernel on v_mfma_f32_32x32x16_bf16 that reads both operands K-contiguous (the nt form: A stored m x k,
 * B stored n x k); it takes any m and n, and a k that is not a whole number of 64-deep slabs, when
 *     both bases are 16-byte aligned, lda and ldb are multiples of 8, and k is a multiple of 8 (k > 0).
 * For nn, tn and tt the operand that is not K-contiguous is first copied transposed (bla_transpose_b16) into the context workspace.  Every other call
 * (odd k, an operand off alignment, an odd pitch) goes to a bounds-checked kernel with 2-byte loads that is correct, not fast.
 * bla_gemm_last_kernel() names what the last call launched:
 *     gemm_bf16_mfma128x128x64_<nn|nt|tn|tt>_<f32|bf16>[_tcopyA][_tcopyB]     the fast path (tcopyX: operand X went through the transposed copy)
 *     gemm_bf16_general_<nn|nt|tn|tt>_<f32|bf16>                              the general path
 * Workspace: the transposed copies (and bla_gemm_f32_as_bf16's bf16 operands) live in the context workspace, which grows on demand.  As for every entry of
 * this library that may grow a workspace, a call must have run once eagerly, with shapes at least as large, before it is captured into a graph. */
enum { BLA_C_F32 = 0, BLA_C_BF16 = 1 };
BLA_API bla_status bla_gemm_bf16(void* stream, int transa, int transb, int m, int n, int k, const uint16_t* d_a, int lda, const uint16_t* d_b, int ldb,
                                 void* d_c, int ldc, int c_type, const bla_gemm_epilogue* ep /* NULL = plain product */);
/* bla_gemm_f32's own argument list, fp32 A, B and C in memory: both operands are rounded to bf16 (bla_f32_to_bf16) into the context workspace and
 * multiplied by bla_gemm_bf16 with BLA_C_F32 -- exactly that composition, bit for bit, with the bf16 operands in their fp32 layout at 16-byte aligned
 * bases and pitches rounded up to a multiple of 8 (so the product is on the fast path whenever k % 8 == 0).  The entry for a caller with fp32 data who
 * trades 16 mantissa bits of the operands for the bf16 matrix rate.  Epilogue and workspace rules: bla_gemm_bf16's. */
BLA_API bla_status bla_gemm_f32_as_bf16(void* stream, int transa, int transb, int m, int n, int k, const float* d_a, int lda, const float* d_b, int ldb,
                                        float* d_c, int ldc, const bla_gemm_epilogue* ep);
/* K-split of the fast path: for a product with few 128 x 128 output tiles and a long contraction (every weight gradient), which the unsplit
 * kernel runs on tiles_m tiles_n workgroups however many compute units there are.  An addition: bla_gemm_bf16 never splits.
 *
 * Partition rule.  slabs = ceil(k / 64).  The requested S is clamped to [1, slabs]; sps = ceil(slabs / S) slabs per split; S_eff = ceil(slabs / sps), so
 * no split is empty.  Split s takes k in [s sps 64, min(k, (s + 1) sps 64)).  A grid of tiles x S_eff workgroups runs the unsplit slab loop over its range
 * and stores its fp32 accumulator tile to partial [s][tile][128][128] in the context workspace, behind the transposed copies; a second kernel then computes
 * acc = P[0]; acc += P[1]; ... acc += P[S_eff - 1] per element (fp32, ascending s) and runs bla_gemm_bf16's epilogue on it.  No atomics and no arrival
 * order: the same call gives the same bits every time.  The error bound of the unsplit product holds unchanged.
 * S_eff == 1 IS bla_gemm_bf16's launch (same kernel, same name, no partials).  A call off the fast path (odd k, misaligned operand, odd pitch) runs the
 * general kernel unsplit.  With S_eff > 1 bla_gemm_last_kernel() answers the fast path's name with the suffix _splitk<S_eff>, e.g.
 * gemm_bf16_mfma128x128x64_nt_f32_splitk6.
 *
 * Automatic rule (splits = 0), a pure function of tiles = tiles_m tiles_n, slabs and the number of compute units cus (cus <= 0: 256):
 *     slots = 3 cus                        three workgroups share a compute unit at the kernel's registers and LDS
 *     S = 1                                when tiles >= slots, or when slabs < 2 BLA_GEMM_BF16_SPLITK_MIN_SLABS
 *     S = min(floor(slots / tiles), floor(slabs / BLA_GEMM_BF16_SPLITK_MIN_SLABS))   otherwise; then the partition rule.
 * BLA_GEMM_BF16_SPLITK_MIN_SLABS is the number of slabs below which a partial tile's 128 KB of write-and-read traffic is no longer paid for
 * (DESIGN 3.20 has the sweep that chose it).
 *
 * bla_gemm_bf16_splitk_plan (host only, needs no device): what a fast-path call with these extents launches.  splits >= 1: the partition rule;
 * splits == 0: the automatic rule for cus compute units.  partial_bytes = S_eff > 1 ? S_eff tiles_m tiles_n 65536 : 0.  Any out pointer may be NULL.
 * BLA_ERR_INVALID: a negative m, n, k or splits.  m, n or k of 0: S_eff 1, no partials. */
#define BLA_GEMM_BF16_SPLITK_MIN_SLABS 8
BLA_API bla_status bla_gemm_bf16_splitk_plan(int m, int n, int k, int splits, int cus, int* eff_splits, int* slabs_per_split, size_t* partial_bytes);
/* bla_gemm_bf16's argument list, checks and epilogue, plus splits: >= 1 the requested S, 0 the automatic rule with the context's compute units.
 * splits < 0: BLA_ERR_INVALID before anything is launched, C untouched.  Workspace: bla_gemm_bf16's plus the plan's partial_bytes (the capture rule of
 * bla_gemm_bf16 applies). */
BLA_API bla_status bla_gemm_bf16_splitk(void* stream, int transa, int transb, int m, int n, int k, const uint16_t* d_a, int lda, const uint16_t* d_b, int ldb,
                                        void* d_c, int ldc, int c_type, const bla_gemm_epilogue* ep, int splits);

/* ---- MXFP8: OCP microscaling fp8 operands, fp32 accumulation, on v_mfma_scale_f32_32x32x64_f8f6f4 (csrc/bla_gemm_mxfp8.hip) -----------
 * An addition beside the fp32 and bf16 entries: no existing entry, kernel or dispatcher decision changes.
 *
 * Element.  OCP e4m3fn in a uint8_t: 1 sign, 4 exponent (bias 7), 3 mantissa bits; largest finite value 448 (0x7E); 0x7F / 0xFF are NaN; no infinities;
 * subnormals are multiples of 2^-9.  This is NOT MI300's fnuz encoding.
 * Scale.  E8M0 in a uint8_t: byte s means 2^(s - 127); 0xFF is NaN.
 * MX operand of rows x k values, k % 32 == 0: elements [rows][ld] bytes with the contraction contiguous (ld >= k) and scales [rows][ld_s] bytes, byte
 * [r][g] scaling elements [r][32 g .. 32 g + 31] (ld_s >= k / 32).  Both GEMM operands are stored this way (A is m x k, B is n x k: bla_gemm_bf16's nt
 * form); other storage orders are the quantiser's business (trans), not the product's.
 *
 * Quantisation of a block of 32 fp32 values v (OCP MX v1.0 section 6.3, with the choices it leaves open fixed):
 *     e = clamp(floor(log2(max|v|)) - 8, -127, 127), scale byte e + 127;  max|v| == 0: byte 127.
 *     element = v 2^-e (exact in fp32 barring underflow) rounded to nearest even onto the e4m3 grid; a magnitude above 448 after rounding SATURATES to
 *     +-448; the sign of zero is kept; nothing is flushed on the fp32 side.
 *     A block that contains a NaN or an infinity: scale byte 0xFF and all 32 elements 0x7F.
 *     A partial last block (cols % 32 != 0) is completed with +0 VALUES, which are quantised with the block and written up to the next multiple of 32.
 * Dequantisation: decode(elem) 2^(s - 127), one fp32 multiplication (2^-127 is the fp32 subnormal; 448 2^127 overflows to inf as that multiplication
 * does); NaN with the bits 0x7FC00000 if either byte is NaN.
 *
 * bla_f32_to_mxfp8: trans = 0: the source is [rows][cols] fp32 (ld_src >= cols) and the blocks run along a source row.  trans = 1: the source is stored
 * [cols][rows] (ld_src >= rows), the contraction index is the slow one and the blocks run down a source column (through an LDS tile).  The output is
 * the MX operand above in both cases: this is how nn / tn / tt products reach the one nt kernel.  Only the window is written: elements up to cols
 * rounded up to 32 (ld at least that), ceil(cols / 32) scale bytes per row.  16-byte loads / 4- or 16-byte stores where bases and pitches allow.
 * bla_mxfp8_to_f32: the dequantisation over a rows x cols window (ld >= cols, ld_s >= ceil(cols / 32), ld_dst >= cols; cols need not be a multiple of 32). */
BLA_API bla_status bla_f32_to_mxfp8(void* stream, const float* d_src, int ld_src, int trans, int rows, int cols, uint8_t* d_elems, int ld, uint8_t* d_scales, int ld_s);
BLA_API bla_status bla_mxfp8_to_f32(void* stream, const uint8_t* d_elems, int ld, const uint8_t* d_scales, int ld_s, float* d_dst, int ld_dst, int rows, int cols);
/*   C[m x n] = epilogue( alpha * A[m x k] . B[n x k]^T )  on the dequantised values, accumulation and epilogue in fp32
 * c_type and ep are bla_gemm_bf16's (BLA_C_F32 / BLA_C_BF16; alpha, beta, bias_row, bias_col, act) and the same fields are refused in the same way.
 * k % 32 != 0, a negative extent, a NULL operand or scale array, a pitch below its window: BLA_ERR_INVALID before any launch, C untouched.
 * Dispatch.  The fast path is a 128 x 128 x 128 tile kernel on the scaled MFMA; it takes any m, n and k (k % 32 == 0, k > 0) when
 *     d_a and d_b are 16-byte aligned with lda % 16 == 0 and ldb % 16 == 0, and d_sa and d_sb are 4-byte aligned with ldsa % 4 == 0 and ldsb % 4 == 0.
 * It reads the scales as aligned dwords: the up to 3 bytes of pitch padding behind a row's k / 32 scale bytes may be read (never past the aligned dword
 * of a valid byte) and are replaced by 127 before use, whatever they hold.  Every other call goes to a bounds-checked kernel that decodes in software
 * and accumulates a k-ascending fmaf chain of dequantised values: correct, not fast.  bla_gemm_last_kernel() answers
 *     gemm_mxfp8_mfma128x128x128_<f32|bf16>     the fast path
 *     gemm_mxfp8_general_<f32|bf16>             the general path
 * Error.  Products of two dequantised values are exact in fp32 unless they leave its range, so the error is that of the accumulation.
 * NaN elements and 0xFF scales in a GEMM operand are UNSPECIFIED beyond "no fault, and only the affected rows or columns of C": the conversions define
 * them, the product documents what was observed (NaN in exactly those rows / columns, on both paths). */
BLA_API bla_status bla_gemm_mxfp8(void* stream, int m, int n, int k, const uint8_t* d_a, int lda, const uint8_t* d_sa, int ldsa, const uint8_t* d_b, int ldb,
                                  const uint8_t* d_sb, int ldsb, void* d_c, int ldc, int c_type, const bla_gemm_epilogue* ep /* NULL = plain product */);
/* bla_gemm_f32_as_bf16's argument list, fp32 A, B and C in memory: both operands are quantised (bla_f32_to_mxfp8, trans chosen so that each comes out
 * contraction-contiguous: A with trans = transa, B with trans = !transb) into the context workspace at 16-byte aligned bases, an element pitch of k rounded
 * up to 32 and a scale pitch rounded up to 4, and multiplied by bla_gemm_mxfp8 with k rounded up to 32 and BLA_C_F32 -- exactly that composition, bit
 * for bit, always on the fast path.  Any k >= 1 (and k = 0) is accepted.  Epilogue: bla_gemm_mxfp8's.  Workspace: bla_gemm_bf16's capture rule. */
BLA_API bla_status bla_gemm_f32_as_mxfp8(void* stream, int transa, int transb, int m, int n, int k, const float* d_a, int lda, const float* d_b, int ldb,
                                         float* d_c, int ldc, const bla_gemm_epilogue* ep);

/* ---- elementwise / broadcast / transpose / reductions: lib/matrix.c:59-205, lib/util.c:7-55 -------------
 * All operate in place on device memory exactly like their reference counterparts operate on host
 * memory; n = rows*cols.  HBM-bound; sums accumulate in fp64 and are rounded to fp32 once. */
BLA_API bla_status bla_scale_f32(void* stream, float* d_m, size_t n, float f);                 /* matrix_scale, lib/matrix.c:59-63 */
BLA_API bla_status bla_add_f32(void* stream, float* d_a, const float* d_b, size_t n);          /* matrix_add: a += b, lib/matrix.c:65-69 */
BLA_API bla_status bla_hadamard_f32(void* stream, float* d_a, const float* d_b, size_t n);     /* matrix_multiply_elementwise, lib/matrix.c:95-103 (shape check is the caller's) */
BLA_API bla_status bla_axpy_f32(void* stream, float* d_y, const float* d_x, float alpha, size_t n); /* y += alpha*x: matrix_scale+matrix_add pair, model/mnist_nn.c:303-315 */
BLA_API bla_status bla_relu_f32(void* stream, float* d, size_t n);                             /* relu, lib/util.c:7-13 */
BLA_API bla_status bla_relu_ddx_f32(void* stream, float* d, size_t n);                         /* relu_ddx, model/mnist_nn.c:47-51 */
BLA_API bla_status bla_add_tile_columns_f32(void* stream, float* d_a, int a_rows, int a_cols, const float* d_b, int b_cols); /* lib/matrix.c:189-195 */
BLA_API bla_status bla_add_tile_rows_f32(void* stream, float* d_a, int a_rows, int a_cols, const float* d_b);                /* lib/matrix.c:199-205 */
BLA_API bla_status bla_transpose_f32(void* stream, const float* d_in, float* d_out, int rows, int cols);  /* out (cols x rows) = in^T; matrix_transpose, lib/matrix.c:105-118 */
BLA_API bla_status bla_row_sum_f32(void* stream, const float* d_m, int rows, int cols, float* d_out);     /* 1 x cols, matrix_row_sum, lib/matrix.c:123-133 */
/* matrix_col_sum, lib/matrix.c:138-148.  AS_WRITTEN reproduces out[i] = sum_{j<cols} flat[i*rows+j] and returns
 * BLA_ERR_UNDEFINED where the reference reads out of bounds (rows > cols); INTENDED gives true row sums. */
enum { BLA_COLSUM_AS_WRITTEN = 0, BLA_COLSUM_INTENDED = 1 };
BLA_API bla_status bla_col_sum_f32(void* stream, const float* d_m, int rows, int cols, float* d_out, int mode);
BLA_API bla_status bla_frobenius_f32(void* stream, const float* d_m, size_t n, float* d_out);  /* d_out[0] = sqrt(sum x^2), lib/matrix.c:150-158 */
BLA_API bla_status bla_max_f32(void* stream, const float* d_m, size_t n, float* d_out);        /* d_out[0] = max (-inf when empty), lib/matrix.c:160-168 */
BLA_API bla_status bla_zscore_f32(void* stream, float* d_m, size_t n);                         /* matrix_z_score_normalize, lib/matrix.c:170-185 */
BLA_API bla_status bla_softmax_cols_f32(void* stream, float* d, int rows, int cols);           /* softmax per column, lib/util.c:15-34 */
BLA_API bla_status bla_softmax_rows_f32(void* stream, float* d, int rows, int cols);           /* softmax_row_wise, lib/util.c:36-55 */
/* softmax per column, then d_grad = (softmax - y) * scale in the same pass (model/mnist_nn.c:234,263-268) */
BLA_API bla_status bla_softmax_cols_grad_f32(void* stream, float* d, int rows, int cols, const float* d_y, float scale, float* d_grad);

/* ---- the matrix.h path in the reference's own element type (lib/matrix.h:4: double) for the -DBLA_FP64 build of the host layer
 * (SURVEY 7.0(1)): same meaning as the _f32 entries above, GEMM on v_mfma_f64_16x16x4_f64.  This is the <= 1e-12 comparison mode against the
 * reference's CPU results (only the order of additions differs), not a performance path. */
BLA_API bla_status bla_gemm_f64(void* stream, int transa, int transb, int m, int n, int k, const double* d_a, int lda, const double* d_b, int ldb,
                                double* d_c, int ldc, double alpha, double beta);                             /* lib/matrix.c:35-57 */
BLA_API bla_status bla_scale_f64(void* stream, double* d_m, size_t n, double f);                             /* :59-63 */
BLA_API bla_status bla_add_f64(void* stream, double* d_a, const double* d_b, size_t n);                      /* :65-69 */
BLA_API bla_status bla_hadamard_f64(void* stream, double* d_a, const double* d_b, size_t n);                 /* :95-103 */
BLA_API bla_status bla_add_tile_columns_f64(void* stream, double* d_a, int a_rows, int a_cols, const double* d_b, int b_cols);   /* :189-195 */
BLA_API bla_status bla_add_tile_rows_f64(void* stream, double* d_a, int a_rows, int a_cols, const double* d_b);                  /* :199-205 */
BLA_API bla_status bla_transpose_f64(void* stream, const double* d_in, double* d_out, int rows, int cols);   /* :105-118 */
BLA_API bla_status bla_row_sum_f64(void* stream, const double* d_m, int rows, int cols, double* d_out);      /* :123-133 */
BLA_API bla_status bla_col_sum_f64(void* stream, const double* d_m, int rows, int cols, double* d_out, int mode);   /* :138-148 */
BLA_API bla_status bla_frobenius_f64(void* stream, const double* d_m, size_t n, double* d_out);              /* :150-158 */
BLA_API bla_status bla_max_f64(void* stream, const double* d_m, size_t n, double* d_out);                    /* :160-168 */
BLA_API bla_status bla_zscore_f64(void* stream, double* d_m, size_t n);                                      /* :170-185 (sigma through sqrtf, as there) */
/* conv.h / norm.h / util.h in the same element type (csrc/bla_f64_conv.hip): the index maps of lib/conv.c, conv() / conv_ddx() with their two
 * products on the f64 GEMM, group norm and its gradient, relu, the two softmaxes -- argument meaning as the _f32 entries of the same name. */
BLA_API bla_status bla_im2col_f64(void* stream, const double* d_x, double* d_out, int h, int w, int k, int c_in, int stride);                 /* lib/conv.c:8-77 */
BLA_API bla_status bla_col2im_f64(void* stream, const double* d_cols, double* d_out, int h, int w, int k, int c_n, int stride);              /* :80-135 */
BLA_API bla_status bla_kernels_to_matrix_f64(void* stream, const double* d_kern, double* d_mat, int f_n, int c_n, int k);                     /* :138-153 */
BLA_API bla_status bla_matrix_to_kernels_f64(void* stream, const double* d_mat, double* d_kern, int f_n, int c_n, int k);                     /* :156-171 */
BLA_API bla_status bla_reshape_channels_matrix_f64(void* stream, double* d_channels, const double* d_matrix, int c_n, int hw);                /* :174-187, as written */
BLA_API bla_status bla_reshape_matrix_channels_f64(void* stream, double* d_matrix, const double* d_channels, int c_n, int hw);                /* :190-203, as written */
BLA_API bla_status bla_conv_forward_f64(void* stream, const double* d_x, const double* d_kern, double* d_im2col, double* d_kmat, double* d_product, double* d_output,
                                        int h, int w, int k, int c_in, int f_n, int stride);                                                  /* :205-212 */
BLA_API bla_status bla_conv_backward_f64(void* stream, const double* d_del_y, const double* d_im2col, const double* d_kmat, double* d_del_q, double* d_del_kmat,
                                         double* d_del_kern, double* d_del_col, double* d_del_x, int h, int w, int k, int c_in, int f_n, int stride);   /* :214-229 */
BLA_API bla_status bla_group_norm_f64(void* stream, const double* d_in, double* d_out, double* d_stdevs, double* d_means, int channels, int group_size, int hw);   /* lib/norm.c:5-50 */
BLA_API bla_status bla_group_norm_ddx_f64(void* stream, const double* d_source, double* d_dest, const double* d_data, const double* d_means, const double* d_stdevs,
                                          int channels, int group_size, int hw);                                                               /* :52-93 */
BLA_API bla_status bla_relu_f64(void* stream, double* d, size_t n);                                                                            /* lib/util.c:7-13 */
BLA_API bla_status bla_softmax_cols_f64(void* stream, double* d, int rows, int cols);                                                          /* :15-34 */
BLA_API bla_status bla_softmax_rows_f64(void* stream, double* d, int rows, int cols);                                                          /* :36-55 */

/* ---- convolution stages, lib/conv.c.  Images are contiguous [C][H][W]; kernels [F][C][k][k]; workspaces are
 * the reference's ConvData members (lib/conv.h:6-11): im2col [Ho*Wo][k*k*C], kernel_matrix [k*k*C][F],
 * product [Ho*Wo][F], output [F][Ho][Wo].  TF "SAME" padding, Ho = ceil((float)H/stride) (lib/conv.c:13-28,55-56). */
BLA_API bla_status bla_conv_out_hw(int h, int w, int stride, int* ho, int* wo);
BLA_API bla_status bla_im2col_f32(void* stream, const float* d_x, float* d_out, int h, int w, int k, int c_in, int stride);       /* _im2col, lib/conv.c:8-77 */
/* _col2im, lib/conv.c:80-135: the reference is defined for stride 1 only (it walks the image grid instead of the output grid).
 * Other strides give the INTENDED operation, the adjoint of _im2col (d_cols is [Ho*Wo][k*k*C], d_out [C][h][w]); with BLA_STRICT_REFERENCE=1
 * in the environment they return BLA_ERR_UNDEFINED instead. */
BLA_API bla_status bla_col2im_f32(void* stream, const float* d_cols, float* d_out, int h, int w, int k, int c_n, int stride);
BLA_API bla_status bla_kernels_to_matrix_f32(void* stream, const float* d_kern, float* d_mat, int f_n, int c_n, int k);          /* _reshape_kernels_matrix, lib/conv.c:138-153 */
BLA_API bla_status bla_matrix_to_kernels_f32(void* stream, const float* d_mat, float* d_kern, int f_n, int c_n, int k);          /* _reshape_matrix_kernels, lib/conv.c:156-171 */
/* The two channel reshapes keep the reference's names, argument order AND as-written direction:
 * reshape_channels_matrix(channels, matrix) writes channels <- matrix; reshape_matrix_channels(matrix, channels) writes matrix <- channels. */
BLA_API bla_status bla_reshape_channels_matrix_f32(void* stream, float* d_channels, const float* d_matrix, int c_n, int hw);     /* lib/conv.c:174-187 */
BLA_API bla_status bla_reshape_matrix_channels_f32(void* stream, float* d_matrix, const float* d_channels, int c_n, int hw);     /* lib/conv.c:190-203 */
/* conv(), lib/conv.c:205-212, intended composition (GEMM result reaches output; as written the last step overwrites product
 * from the stale output and never writes output -- the host layer offers that literal mode too). */
BLA_API bla_status bla_conv_forward_f32(void* stream, const float* d_x, const float* d_kern, float* d_im2col, float* d_kmat, float* d_product,
                                        float* d_output, int h, int w, int k, int c_in, int f_n, int stride);
/* conv_ddx(), lib/conv.c:214-229, intended composition.  h, w are the INPUT's size; del_y is [F][Ho][Wo].  Stride 1 is the reference's only
 * defined case; other strides use the adjoint _col2im above (BLA_STRICT_REFERENCE=1: BLA_ERR_UNDEFINED). */
BLA_API bla_status bla_conv_backward_f32(void* stream, const float* d_del_y, const float* d_im2col, const float* d_kmat, float* d_del_q,
                                         float* d_del_kmat, float* d_del_kern, float* d_del_col, float* d_del_x, int h, int w, int k, int c_in,
                                         int f_n, int stride);
/* Implicit-GEMM convolution for device-resident callers: the im2col matrix is gathered inside the MFMA kernel and
 * never written (no ConvData workspaces).  Values equal conv()'s `output` / conv_ddx()'s del_kernels and del_input
 * (lib/conv.c:205-229, intended composition).  Any stride.  The data gradient at stride != 1 (undefined in the reference) is
 * the adjoint of the forward map -- the stride-1 convolution of the zero-dilated del_y with the flipped kernels -- as the U-Net's three
 * down-convolutions need it (model/cifar_unet.c:1105,1111,1115; backward :1412,1420,1430); BLA_STRICT_REFERENCE=1 refuses it
 * (BLA_ERR_UNDEFINED).  d_scratch: F*C*k*k floats, needed only when d_del_x != NULL. */
BLA_API bla_status bla_conv2d_forward_f32(void* stream, const float* d_x, const float* d_kern, float* d_out, int h, int w, int k, int c_in, int f_n, int stride);
BLA_API bla_status bla_conv2d_backward_f32(void* stream, const float* d_del_y, const float* d_x, const float* d_kern, float* d_del_kern,
                                           float* d_del_x, float* d_scratch, int h, int w, int k, int c_in, int f_n, int stride);
/* `batch` images through the same kernels in one launch (the reference has no batch dimension: one conv() / conv_ddx() call
 * per image, model/cifar_unet.c:1105-1165).  x [B][C][H][W], out / del_y [B][F][Ho][Wo], del_x [B][C][H][W];
 * del_kern = SUM over the images of the per-image weight gradient, folded in image order. */
BLA_API bla_status bla_conv2d_forward_batched_f32(void* stream, const float* d_x, const float* d_kern, float* d_out, int batch, int h, int w, int k,
                                                  int c_in, int f_n, int stride);
BLA_API bla_status bla_conv2d_backward_batched_f32(void* stream, const float* d_del_y, const float* d_x, const float* d_kern, float* d_del_kern,
                                                   float* d_del_x, float* d_scratch, int batch, int h, int w, int k, int c_in, int f_n, int stride);
/* ---- mixed-precision convolution: bf16 operands, fp32 accumulation, on the bf16 matrix instructions (csrc/bla_conv_bf16.hip) -------------
 * An addition beside the fp32 entries above: no fp32 entry, plan or dispatcher decision changes.  bf16 = uint16_t bit patterns rounded as bla_f32_to_bf16
 * rounds; Cp = the channel count rounded up to a multiple of 8; every base address 16-byte aligned.
 *
 * Padded channel-last activations  P [B][Hp][Wp][Cp]:  P[b][top + y d][left + x d][c] = rne(src[b][c][y][x]); every other element -- the halo, the holes of
 * a dilation d > 1, the channels from C up to Cp -- is +0.  The 8 channels of one tap of one output pixel are then one aligned 16-byte chunk for any
 * stride, kernel and map size, and the product's gather needs no bounds checks.
 * Kernel matrices, tap-major:  forward  A [F][k k Cp]:  A[f][(p k + q) Cp + c] = rne(kern[f][c][p][q]);
 *                              data gradient, flipped and transposed  A [C][k k Fp]:  A[c][((k-1-p) k + (k-1-q)) Fp + f] = rne(kern[f][c][p][q]);
 * padding columns are +0.
 *
 * bla_conv_bf16_layout (host only): the padded extents of an h x w map.  data_gradient = 0, the operand of the forward pass and of nothing else here:
 * TF-SAME top / left as lib/conv.c:13-28 computes them, hp = h + vertical padding, wp = w + horizontal padding, dilate = 1.  data_gradient = 1, h x w being
 * the convolution's INPUT size: the layout of del_y [Ho][Wo] dilated by the stride: dilate = stride, top = k-1-pt, left = k-1-pl, hp = h+k-1, wp = w+k-1. */
BLA_API bla_status bla_conv_bf16_layout(int h, int w, int k, int stride, int data_gradient, int* hp, int* wp, int* top, int* left, int* dilate);
/* The copy described above, fp32 [batch][c][h][w] -> P [batch][hp][wp][Cp]: a convert-and-transpose through an LDS tile that writes EVERY element of d_dst
 * (16-byte stores; 16-byte loads when d_src is 16-byte aligned and w % 4 == 0).  The map must fit: top + (h-1) dilate < hp, left + (w-1) dilate < wp. */
BLA_API bla_status bla_conv_bf16_pad(void* stream, const float* d_src, uint16_t* d_dst, int batch, int c, int h, int w, int hp, int wp, int top, int left, int dilate);
/* kern fp32 [f_n][c_n][k][k] -> the forward matrix [f_n][k k Cp] (data_gradient = 0) or the data gradient's [c_n][k k Fp] (1), every element written */
BLA_API bla_status bla_conv_bf16_prepare_kernels(void* stream, const float* d_kern, uint16_t* d_dst, int f_n, int c_n, int k, int data_gradient);
/* The same for MANY kernel tensors in ONE launch: job i is bla_conv_bf16_prepare_kernels(kern, dst, f_n, c_n, k, data_gradient), and every
 * destination gets exactly the bits that call writes (one chunk body behind both kernels), every element in 16-byte stores.  d_jobs is a DEVICE array of
 * n_jobs jobs; max_chunks = the largest job's count of 8-element destination chunks, rows k k round8(inner) / 8 with (rows, inner) = (f_n, c_n) forward and
 * (c_n, f_n) for the data gradient: it sizes the grid (ceil(max_chunks / 256), n_jobs), and the threads past a job's own extent do nothing.
 * The jobs live in device memory, so the library cannot look at them: every field is the CALLER'S responsibility -- kern holds f_n c_n k k floats, dst is
 * 16-byte aligned and holds the whole matrix, extents > 0, no job needs more than max_chunks chunks (a larger one is left partly unwritten), destinations
 * do not overlap.  n_jobs == 0 does nothing.  BLA_ERR_INVALID, before the device is asked for: n_jobs < 0, a NULL table or max_chunks == 0 with n_jobs > 0,
 * more than 65535 jobs. */
typedef struct bla_conv_bf16_prep_job { const float* kern; uint16_t* dst; int f_n, c_n, k, data_gradient; } bla_conv_bf16_prep_job;
BLA_API bla_status bla_conv_bf16_prepare_kernels_table(void* stream, const bla_conv_bf16_prep_job* d_jobs, int n_jobs, size_t max_chunks);
/*   out[b][r][i][j] = sum_{p,q,c} A[r][(p k + q) cp + c] * P[b][i stride + p][j stride + q][c]  (+ ep_bias[b * ep_bias_stride + r], in fp32, if ep_bias)
 * A [rows][k k cp], P [batch][hp][wp][cp], out fp32 [batch][rows][ho][wo] (the project's layout).  One product for the forward pass (A = the forward matrix,
 * P = the padded input) and for the data gradient (A = the flipped matrix, P = the dilated padded del_y, stride 1, ho x wo = the input's h x w).
 * The kernel is bla_gemm_bf16's 128 x 128 x 64 fast kernel with the B operand gathered from P (columns = (image, output pixel)); the error is that of the
 * fp32 accumulation alone (DESIGN 3.18's bound with K = k k cp).  bla_gemm_last_kernel() then answers conv_bf16_gather128x128x64_s<stride>.
 * BLA_ERR_INVALID, before the device is asked for: a NULL A, P or out, an extent <= 0, stride < 1, cp % 8 != 0, an operand off 16-byte alignment, an
 * output whose taps reach past the padded map ((ho-1) stride + k > hp or (wo-1) stride + k > wp), or sizes past 32-bit indexing (one padded image
 * hp wp cp, or batch ho wo, at 2^31 or more).  No workspace. */
BLA_API bla_status bla_conv2d_gathered_bf16(void* stream, const uint16_t* d_a, int rows, const uint16_t* d_p, int batch, int hp, int wp, int cp, int k, int stride,
                                            int ho, int wo, float* d_out, const float* ep_bias, int ep_bias_stride);
/* The same product with a CHANNEL-LAST bf16 OUTPUT: it writes the padded map the next product reads, so consecutive bf16 convolutions chain
 * with no fp32 round trip and no bla_conv_bf16_pad between them.  An addition: bla_conv2d_gathered_bf16 above keeps its kernel and its bits.
 * A map is a padded channel-last bf16 tensor [batch][hp][wp][cp]: pixel (y, x), channel c of the tensor it carries sits at
 * d[((b hp + top + y dilate) wp + left + x dilate) cp + c] -- bla_conv_bf16_layout's forward layout of the next convolution (dilate 1), or the
 * data-gradient layout of the layer below (dilate = its stride).
 * Per output element (b, r, i, j), all in fp32 and in this order:  t = the accumulator;  t += bias[b bias_stride + r] (one add, as above);
 * relu: t = t > 0 ? t : +0;  gate.d: t = gate(b, i, j, r) > 0 ? t : +0 (ReLU's derivative, read from the bf16 activations of the layer's input map);
 * out_f32[b][r][i][j] = t (if given);  dst(b, i, j, r) = rne(t), bla_f32_to_bf16's rounding (if dst.d is given).
 * In dst, for every output pixel ALL dst.cp channels of position (top + i dilate, left + j dilate) are written -- channels rows .. dst.cp - 1 as +0, never
 * a rounded accumulator -- in 16-byte stores of whole 8-channel chunks, and nothing else is touched: halo rows and columns and the holes of a dilation keep
 * their bits.  A caller zero-fills a map once; its halo stays valid for every later pass that writes the same map.  dst.d and gate.d must not overlap d_p.
 * bla_gemm_last_kernel() answers conv_bf16_gather128x128x64_s<stride>_cl when dst.d is given, conv_bf16_gather128x128x64_s<stride> otherwise.
 * BLA_ERR_INVALID, before the device is asked for and with both outputs untouched: a NULL ep; out_f32 and dst.d both NULL; anything
 * bla_conv2d_gathered_bf16 refuses; dst.cp != rows rounded up to 8; gate.cp % 8 != 0 or gate.cp < rows; a map base off 16-byte alignment; top or left < 0,
 * dilate < 1; a map the output does not fit (top + (ho-1) dilate >= hp, left + (wo-1) dilate >= wp); a map of 2^31 elements or more.  No workspace. */
typedef struct bla_conv_bf16_map { uint16_t* d; int hp, wp, cp, top, left, dilate; } bla_conv_bf16_map;
typedef struct bla_conv_bf16_epilogue {
    const float* bias; int bias_stride;   /* ep_bias / ep_bias_stride of bla_conv2d_gathered_bf16; NULL = none */
    int relu;                              /* t = t > 0 ? t : +0 */
    bla_conv_bf16_map gate;                /* gate.d != NULL: t = gate(b, i, j, r) > 0 ? t : +0 */
    float* out_f32;                        /* optional: fp32 [batch][rows][ho][wo], the existing output */
    bla_conv_bf16_map dst;                 /* optional (dst.d == NULL: none): the next product's operand */
} bla_conv_bf16_epilogue;
BLA_API bla_status bla_conv2d_gathered_bf16_chained(void* stream, const uint16_t* d_a, int rows, const uint16_t* d_p, int batch, int hp, int wp, int cp, int k,
                                                    int stride, int ho, int wo, const bla_conv_bf16_epilogue* ep);
/* fp32 in memory, the argument meaning of bla_conv2d_forward_batched_f32 / bla_conv2d_backward_batched_f32 (no d_scratch): exactly the composition of the
 * three entries above in the context workspace, bit for bit -- what bla_gemm_f32_as_bf16 is to bla_gemm_bf16.
 *   forward:        pad(x) and prepare_kernels(kern, 0), then the gathered product with the optional bias.
 *                   Workspace: B Hp Wp Cp * 2 + F k k Cp * 2 bytes (each part rounded up to 256).
 *   data gradient:  pad(del_y) in the data-gradient layout and prepare_kernels(kern, 1), then the gathered product at stride 1.  At stride != 1 this is the
 *                   dilated form (the adjoint of the forward map); BLA_STRICT_REFERENCE=1 refuses it with BLA_ERR_UNDEFINED as the fp32 entry does.
 *                   Workspace: B (H+k-1) (W+k-1) Fp * 2 + C k k Fp * 2 bytes.
 *   weight gradient: MATERIALISED.  With Np = B Ho Wo rounded up to 8: one kernel writes the bf16 im2col G [(c,p,q)][(b,i,j)] at pitch Np straight from x,
 *                   one writes dY16 [f][(b,i,j)] at pitch Np from del_y (tails zero), and del_kern [F][C k k] = dY16 . G^T is bla_gemm_bf16's fast nt
 *                   product with m = F, n = C k k, k = Np (bla_gemm_last_kernel() names it).  Workspace: (F + C k k) Np * 2 bytes.
 * Either output of the backward entry may be NULL; its workspace is the larger of the two gradients' (they run one behind the other on the stream).
 * Pure argument errors (NULL pointers, extents <= 0, stride < 1) answer BLA_ERR_INVALID before the device is asked for; outputs are untouched after any
 * refusal.  These calls may grow the workspace: run once eagerly, with shapes at least as large, before capturing into a graph. */
BLA_API bla_status bla_conv2d_forward_batched_f32_as_bf16(void* stream, const float* d_x, const float* d_kern, float* d_out, int batch, int h, int w, int k,
                                                          int c_in, int f_n, int stride, const float* ep_bias, int ep_bias_stride);
BLA_API bla_status bla_conv2d_backward_batched_f32_as_bf16(void* stream, const float* d_del_y, const float* d_x, const float* d_kern, float* d_del_kern,
                                                           float* d_del_x, int batch, int h, int w, int k, int c_in, int f_n, int stride);
/* The weight gradient alone, its product K-split: the two operand passes of the backward entry above (dY16 and G at pitch Np, unchanged) into the context
 * workspace, then del_kern [F][C k k] = dY16 . G^T through bla_gemm_bf16_splitk's nt launch with m = F, n = C k k, k = Np and `splits` (0 = the automatic
 * rule, 1 = exactly the backward entry's weight gradient) -- that composition, bit for bit; bla_gemm_last_kernel() names the product, with _splitk<S_eff>
 * when it was split.  The product has ceil(F / 128) ceil(C k k / 128) output tiles over a contraction of B Ho Wo, so unsplit it occupies a handful of
 * compute units; the backward entry is not changed, and a caller who wants the fast backward pass calls this entry, then the backward entry with
 * d_del_kern = NULL.  Workspace: (F + C k k) Np * 2 bytes plus the plan's partial_bytes.  BLA_ERR_INVALID before the device is asked for: a NULL del_y,
 * x or del_kern, splits < 0, an extent <= 0, stride < 1; del_kern is untouched after any refusal. */
BLA_API bla_status bla_conv2d_weight_gradient_batched_f32_as_bf16(void* stream, const float* d_del_y, const float* d_x, float* d_del_kern, int batch, int h, int w,
                                                                  int k, int c_in, int f_n, int stride, int splits);
/* The IMPLICIT weight gradient, on the caller's padded copies -- the two a bf16 backward pass has anyway -- with no operand pass of its own:
 *   del_kern[f][c][p][q] = sum_{b,i,j} Q[b][top + i dilate][left + j dilate][f] * P[b][i stride + p][j stride + q][c],   i < ho, j < wo
 * Q [batch][hq][wq][fp] is del_y [batch][f_n][ho][wo] in bla_conv_bf16_layout(.., data_gradient = 1)'s layout (the data gradient's operand), P
 * [batch][hp][wp][cp] is x in the forward layout; del_kern is fp32 [f_n][c_n][k][k].  Only Q's positions (top + i dilate, left + j dilate) and channels
 * below f_n, and P's channels below c_n, reach a written element: the holes of the dilation and the padding channels may hold anything.  P's halo is read.
 * The product contracts over the N = batch ho wo pixels, so both operands are pixel-major with contiguous channels; the kernel is the 128 x 128 x 64 tile
 * with both operands k-major, its fragments read from LDS transposed (ds_read_b64_tr_b16).  K-split exactly as bla_gemm_bf16_splitk: the partition rule
 * and the automatic rule on m = f_n, n = k k cp, k = N (bla_gemm_bf16_splitk_plan(f_n, k k cp, N, splits, cus) answers S_eff and the slabs per split);
 * a grid of tiles x S_eff workgroups stores partial [s][tile][128][128] to the context workspace and a second kernel folds
 * acc = P[0]; acc += P[1]; ... ascending per element of del_kern, permuting (tap, channel) to [c][p][q].  S_eff = 1 runs the same two launches.  No
 * atomics, no arrival order: the same call gives the same bits every time.  The error is that of the fp32 accumulation alone: DESIGN 3.20's bound with
 * k = N.  bla_gemm_last_kernel() answers conv_bf16_wgrad128x128x64_s<stride>_splitk<S_eff> (S_eff = 1 included).
 * BLA_ERR_INVALID, before the device is asked for and with del_kern untouched: a NULL Q, P or del_kern, splits < 0, an extent <= 0, stride or dilate < 1,
 * top or left < 0, fp % 8 != 0 or cp % 8 != 0, fp < f_n or cp < c_n, an operand off 16-byte alignment, taps that reach past the padded map
 * ((ho-1) stride + k > hp or (wo-1) stride + k > wp), a gradient that does not fit Q (top + (ho-1) dilate >= hq or left + (wo-1) dilate >= wq), or sizes
 * past 32-bit indexing (batch hq wq fp, batch hp wp cp, N + 128 or k k cp + 128 at 2^31 or more).  Workspace: S_eff tiles 65536 bytes. */
BLA_API bla_status bla_conv2d_weight_gradient_gathered_bf16(void* stream, const uint16_t* d_q, int hq, int wq, int fp, int top, int left, int dilate,
                                                            const uint16_t* d_p, int hp, int wp, int cp, int batch, int k, int stride, int ho, int wo, int f_n,
                                                            int c_n, float* d_del_kern, int splits);
/* bla_conv2d_backward_batched_f32_as_bf16's arguments, input requirements and refusals (either output may be NULL; BLA_STRICT_REFERENCE=1 refuses a stride
 * != 1 data gradient with BLA_ERR_UNDEFINED), plus splits (< 0: BLA_ERR_INVALID).  Exactly this composition in the context workspace
 * [P | Q | A | partials], bit for bit: (1) pad(x) in the forward layout, when d_del_kern is given; (2) pad(del_y) ONCE in the data-gradient layout;
 * (3) bla_conv2d_weight_gradient_gathered_bf16 on (Q, P) with `splits`; (4) prepare_kernels(kern, 1) and bla_conv2d_gathered_bf16 on Q at stride 1, when
 * d_del_x is given.  An addition: the backward entry above is not changed.  May grow the workspace (the capture rule above applies). */
BLA_API bla_status bla_conv2d_backward_gathered_f32_as_bf16(void* stream, const float* d_del_y, const float* d_x, const float* d_kern, float* d_del_kern,
                                                            float* d_del_x, int batch, int h, int w, int k, int c_in, int f_n, int stride, int splits);
/* ---- group norm into a bf16 map (csrc/bla_norm_bf16.hip) ---------------------------------------------------------------------------------
 * Inside a ResNet block a convolution's input is the output of a group norm + ReLU (+ dropout), not of another convolution.  These two entries run the fp32
 * group norm family's arithmetic and write the result where the bf16 product gathers it: a bla_conv_bf16_map, with the store contract of
 * bla_conv2d_gathered_bf16_chained.  An addition: no fp32 norm entry or kernel changes.
 * bla_group_norm_relu_bf16_map: d_in fp32 [batch][channels][h][w]; d_drop optional [batch][channels][h w], non-zero = dropped; d_means / d_stdevs
 * [batch][groups], groups = ceil(channels / group_size) -- the layout bla_group_norm_relu_batched_f32 leaves; the last group of an image may be short and a
 * group never reaches into the next image; d_out_f32 optional [batch][channels][h][w].  Per group of n elements (quirk Q3 kept: `stdevs` holds the variance
 * and the output is divided by it):
 *   m = (float)(sum x / n), fp64 sums;  v = (float) of the variance about that float m, fp64 sums;  y = (x - m) / v, one fp32 subtraction and one IEEE fp32
 *   division;  y = y < 0 ? +0 : y;  y = drop ? +0 : y;  out_f32[b][c][y][x] = y (if given);  dst(b, y, x, c) = rne(y), bla_f32_to_bf16's rounding (if dst.d).
 * The fp64 sums run in a fixed order: the same call gives the same bits every time.
 * In dst, for every pixel ALL dst.cp channels of position (top + y dilate, left + x dilate) are written -- channels `channels` .. dst.cp - 1 as +0 -- in
 * 16-byte stores of whole aligned 8-channel chunks, and nothing else is touched: halo, holes of a dilation and guards keep their bits.  A caller zero-fills
 * a map once; its halo stays valid for every later pass.
 * Two launches: a statistics kernel (one workgroup per image and group), then an apply kernel that reads 16 bytes at a time when w % 4 == 0 and d_in and
 * d_out_f32 are 16-byte aligned and d_drop is 4-byte aligned, 4 bytes at a time otherwise (the same bits either way).
 * BLA_ERR_INVALID, before the device is asked for and with every output untouched: a NULL d_in, d_means, d_stdevs or dst; dst->d and d_out_f32 both NULL; an
 * extent <= 0; batch or h above 65,535; and, with dst->d: dst->cp != channels rounded up to 8, a map base off 16-byte alignment, top or left < 0,
 * dilate < 1, a map the tensor does not fit (top + (h-1) dilate >= hp, left + (w-1) dilate >= wp), a map of 2^31 elements or more.  No workspace. */
BLA_API bla_status bla_group_norm_relu_bf16_map(void* stream, int batch, const float* d_in, int channels, int group_size, int h, int w, const unsigned char* d_drop,
                                                float* d_stdevs, float* d_means, float* d_out_f32, const bla_conv_bf16_map* dst);
/* group_norm_ddx (lib/norm.c:52-93) as the fp32 kernels compute it, with no gate and no addend, into a bf16 map.  Per group, m and v from d_means / d_stdevs:
 *   nv = (data - m) / v;  A = (float)(sum source / n), B = (float)(sum nv source / n), fp64 sums in a fixed order;  r = (source - A - nv B) / v;
 *   dest_f32[b][c][y][x] = r (if given);  dst(b, y, x, c) = rne(r) (if dst.d); at least one of the two.
 * dst is typically the data-gradient layout of the convolution below (bla_conv_bf16_layout(.., data_gradient = 1), dilate = its stride).  The store
 * contract, the apply kernel and the refusals (plus a NULL d_source or d_data) are those of the entry above.  Workspace: 8 bytes per (image, group). */
BLA_API bla_status bla_group_norm_ddx_bf16_map(void* stream, int batch, const float* d_source, const float* d_data, const float* d_means, const float* d_stdevs,
                                               int channels, int group_size, int h, int w, float* d_dest_f32, const bla_conv_bf16_map* dst);
/* What the last bla_conv2d_* call launched (host side only, as bla_gemm_last_kernel): reset on entry to every forward / backward call, one token per product
 * in launch order, separated by spaces.  A token is <role>:<path>[/<attribute>...]:
 *   role   fwd, wgrad, dgrad, dgrad.dil (the data gradient on a zero-dilated del_y); pair (both gradients in one launch of the tiled kernels, weight
 *          gradient + data gradient); wskpair (the same on the 32x32 kernel)
 *   path   m1 / m2/sN      the bounds-checked tiled gather (forward shape / weight gradient), N = K splits
 *          m3hs/sN, m3/s1  the padded copy on the half-slab kernel with its taps cut over N workgroups, or on the older form
 *          m4hs/sN, m4/sN  the weight gradient on the padded copy, half-slab or older form
 *          m7w16, m7w32    the image window, rows of 16 or 32 pixels
 *          wsk/vec/sN, wsk/scalar/sN   the 32x32 wave-split-K kernel with 16-byte or 4-byte loads of its dense operand, N = K splits
 *          parity/one[m3hs/x4]         the stride-2 data gradient by output parity, four classes in one launch
 *          parity/each[m3hs/sN,...]    ... class by class
 *          thin            the direct kernels for at most four channels on one side
 *   attributes   ep=tile|fold|pass|wsk|thin|none  where the epilogue was applied: the tile store, the fold of the K-split slabs, a pass behind the product,
 *                                                 inside the 32x32 (thin) kernel; none = the call had no epilogue
 *                pad=caller|image|copy            the padded operand: the caller's, the image itself, a copy made by the call (pair: padw / padd)
 *                A=prep                           the product read the caller's prepared kernel matrix */
BLA_API const char* bla_conv_last_plan(void);
/* The operand forms the U-Net uses internally, as entry points (no kernel and no decision of their own).
 * bla_conv2d_forward_fused_f32: out = conv + ep_bias[image * ep_bias_stride + channel]; ep_out2 = out + ep_add (ep_add and ep_out2 go together; any may be NULL).
 * x_padded / dy_padded: zero-padded copies of x / del_y in bla_conv_padded_layout(h, w, k, stride) -- per plane `plane` floats, rows of `wh` floats, the
 * image at row pt, column pl, zeros elsewhere (plane = 0: this geometry has none); ignored by the paths that gather from no padded copy.
 * prepared: the kernels in the form bla_conv_prep_mode names for this convolution's forward (data_gradient = 0) or data-gradient product -- 0: none is
 * taken; 1: window order [F][(g, tap, c16)]; 2: flipped and transposed, window order [C][(g, tap, f16)]; 3: flipped and transposed [C][F][k][k] --
 * written by bla_conv_prepare_kernels_f32 (mode 1, 2: 3x3 kernels, the grouped channel count a multiple of 16). */
BLA_API bla_status bla_conv2d_forward_fused_f32(void* stream, const float* d_x, const float* d_kern, float* d_out, int batch, int h, int w, int k, int c_in, int f_n,
                                                int stride, const float* ep_bias, int ep_bias_stride, const float* ep_add, float* ep_out2, const float* x_padded,
                                                const float* prepared);
BLA_API bla_status bla_conv2d_backward_prepared_f32(void* stream, const float* d_del_y, const float* d_x, const float* d_kern, float* d_del_kern, float* d_del_x,
                                                    float* d_scratch, int batch, int h, int w, int k, int c_in, int f_n, int stride, const float* x_padded,
                                                    const float* prepared, const float* dy_padded);
BLA_API bla_status bla_conv_prepare_kernels_f32(void* stream, const float* d_src, float* d_dst, int f_n, int c_n, int k, int mode);
BLA_API int bla_conv_prep_mode(int batch, int h, int w, int k, int c_in, int f_n, int stride, int data_gradient);
BLA_API bla_status bla_conv_padded_layout(int h, int w, int k, int stride, int* w_out, int* wh, int* plane, int* pt, int* pl);
/* group_norm / group_norm_ddx, lib/norm.c:5-93, on [C][H*W]; quirk Q3 kept (epsilon == 0, "stdevs" holds the variance,
 * out = (x - mean) / variance).  Note the reference's argument orders (lib/norm.h:6-7). */
BLA_API bla_status bla_group_norm_f32(void* stream, const float* d_in, float* d_out, float* d_stdevs, float* d_means, int channels, int group_size, int hw);
BLA_API bla_status bla_group_norm_ddx_f32(void* stream, const float* d_source, float* d_dest, const float* d_data, const float* d_means,
                                          const float* d_stdevs, int channels, int group_size, int hw);

/* ---- U-Net glue ops around the conv path, model/cifar_unet.c; channel arrays are [C][H*W] ----
 * _add_time_embedding (:1024-1030) is bla_add_tile_columns_f32(x, C, H*W, t, 1); _concat_skip / _split_concat
 * (:1088-1097,1339-1349) are bla_memcpy_d2d on channel ranges; the time-bias gradient (:1191-1196) is
 * bla_col_sum_f32(..., BLA_COLSUM_INTENDED). */
BLA_API bla_status bla_relu_mask_f32(void* stream, float* d_dest, const float* d_source, const float* d_relu_result, size_t n);   /* multi_channel_relu_ddx, :241-253 */
/* _dropout (:1032-1042): the reference draws `(float) rand() / RAND_MAX < DROPOUT_RATE` per element in order; the host
 * makes those draws (same libc stream) and passes them as d_drop (non-zero = dropped). */
BLA_API bla_status bla_dropout_f32(void* stream, const float* d_x, float* d_y, const unsigned char* d_drop, size_t n);
BLA_API bla_status bla_dropout_mask_f32(void* stream, float* d_x, const float* d_dropout_result, size_t n);                         /* _dropout_mask, :1168-1178 */
BLA_API bla_status bla_nearest_neighbours_f32(void* stream, const float* d_in, float* d_out, int channels, int in_h, int in_w, int out_h, int out_w, int scale);   /* :1074-1086 */
BLA_API bla_status bla_nearest_neighbours_ddx_f32(void* stream, const float* d_source, float* d_dest, int channels, int src_h, int src_w, int dest_h, int dest_w, int scale);   /* :1229-1244 */
BLA_API bla_status bla_softmax_ddx_f32(void* stream, const float* d_softmax_output, const float* d_gradient, float* d_out, int rows, int dim);   /* _softmax_ddx, :1246-1259 */

/* Self-attention block of the U-Net (model/cifar_unet.c:999-1022 forward, :1261-1337 backward), device-resident, with the
 * channel reshapes in the direction their call sites need (as written they are swapped and the block reads stale
 * buffers).  x/out/del_y/del_x: [C][S], S = H*W; wq/wk/wv: [C][d]; w: [d][C]; bias: [C].
 * Workspaces (caller allocated): q,k,v,attention [S][d]; scores_raw (= attention_weights_raw, scaled scores) and
 * weights (= attention_weights, softmax) [S][S].  The backward's gradient workspace reuses the struct:
 * q,k,v,attention = del_Q,del_K,del_V,del_P; scores_raw = del_I; weights = del_S.
 * jacobian_from_raw != 0 reproduces :1307 literally (_softmax_ddx gets the RAW scores where the softmax output is meant). */
typedef struct bla_attention_ws { float *q, *k, *v, *scores_raw, *weights, *attention; } bla_attention_ws;
BLA_API bla_status bla_attention_forward_f32(void* stream, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, const float* d_w,
                                             const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int d);
BLA_API bla_status bla_attention_backward_f32(void* stream, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                              const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad,
                                              float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x, int c, int s, int d,
                                              int jacobian_from_raw);

/* ResNet block of the U-Net (model/cifar_unet.c:1044-1072 forward, :1180-1227 backward), device-resident, intended
 * composition (conv() delivers its result; gradients land in the gradient struct -- as written :1203,1216 hand conv_ddx
 * the parameter kernels as the sink).  x/del_x: [Cin][H*W]; result/del_out: [Cout][H*W]; temb: [T];
 * conv1 [Cout][Cin][k][k]; conv2 [Cout][Cout][k][k]; time_w [T][Cout]; time_b [Cout]; res [Cout][Cin][1][1] or NULL when
 * Cin == Cout; d_drop [Cout*H*W]: the host's rand() draws, non-zero = dropped.  Stride 1. */
typedef struct bla_resnet_params { const float *conv1, *conv2, *time_w, *time_b, *res; } bla_resnet_params;
typedef struct bla_resnet_grads { float *conv1, *conv2, *time_w, *time_b, *res; } bla_resnet_grads;
/* saved by the forward pass for the backward pass: mu/sd per group; relu1 [Cin][HW]; c1 (conv 1 + time embedding), relu2, dp
 * (dropout output), c2, res (residual conv output, may be NULL when Cin == Cout) [Cout][HW]; tdense [Cout] */
typedef struct bla_resnet_ws { float *mu1, *sd1, *relu1, *c1, *tdense, *mu2, *sd2, *relu2, *dp, *c2, *res; } bla_resnet_ws;
/* backward scratch: g_out_a, g_out_b [Cout][HW]; g_in [Cin][HW]; flip [Cout*max(Cin,Cout)*k*k] */
typedef struct bla_resnet_scratch { float *g_out_a, *g_out_b, *g_in, *flip; } bla_resnet_scratch;
BLA_API bla_status bla_group_norm_relu_f32(void* stream, const float* d_in, float* d_out, float* d_stdevs, float* d_means, int channels, int group_size, int hw);   /* group_norm then relu, fused */
BLA_API bla_status bla_sum_f32(void* stream, float* d_out, const float* d_a, const float* d_b, size_t n);   /* out = a + b, :1067-1071 */
BLA_API bla_status bla_resnet_forward_f32(void* stream, const float* d_x, const float* d_temb, const bla_resnet_params* p, const unsigned char* d_drop,
                                          const bla_resnet_ws* ws, float* d_result, int h, int w, int cin, int cout, int k, int tdim, int group_size);
BLA_API bla_status bla_resnet_backward_f32(void* stream, const float* d_del_out, const float* d_x, const float* d_temb, const bla_resnet_params* p,
                                           const bla_resnet_ws* ws, const bla_resnet_grads* g, const bla_resnet_scratch* sc, float* d_del_x, int h, int w,
                                           int cin, int cout, int k, int tdim, int group_size);

/* The same blocks for a batch of images (what a mini-batch of the reference's one-image-at-a-time training loop computes, gradients summed over the
 * images): x / out / del_* [B][C][H*W], temb [B][T] (every image its own time step), d_drop [B][Cout*H*W]; every workspace / scratch buffer is B
 * times its single-image size (tdense [B][Cout], mu / sd [B][groups]).  The convolutions run as batched implicit GEMMs, the norms over B*C
 * channels, each per-image product of the attention block as one launch over the batch.  batch = 1 is the single-image entry point.
 * d_partials: [B][C*d] scratch (per-image weight gradients before their sum); d_dtb: [B][Cout] scratch.  bla_resnet_backward_batched_f32 takes
 * d_del_x = NULL when nothing consumes the gradient of the block's input (a network's first block): only the weight gradients are formed. */
BLA_API bla_status bla_gemm_batched_f32(void* stream, int transa, int transb, int m, int n, int k, const float* A, int lda, long stride_a, const float* B, int ldb,
                                        long stride_b, float* C, int ldc, long stride_c, int batch, const bla_gemm_epilogue* ep, long stride_pre);
BLA_API bla_status bla_group_norm_relu_batched_f32(void* stream, int batch, const float* d_in, float* d_out, float* d_stdevs, float* d_means, int channels,
                                                   int group_size, int hw);
BLA_API bla_status bla_group_norm_ddx_gated_batched_f32(void* stream, int batch, const float* d_source, float* d_dest, const float* d_data, const float* d_means,
                                                        const float* d_stdevs, int channels, int group_size, int hw, const float* d_relu_gate,
                                                        const float* d_addend);
BLA_API bla_status bla_attention_forward_batched_f32(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv,
                                                     const float* d_w, const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int d);
BLA_API bla_status bla_attention_backward_batched_f32(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                      const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad,
                                                      float* d_partials, float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x,
                                                      int c, int s, int d, int jacobian_from_raw);
/* The batched attention block with bf16 products inside: the fp32 entries' tensors, layouts and bla_attention_ws.  One rule: BOTH OPERANDS
 * OF EVERY MATRIX PRODUCT ARE ROUNDED TO bf16 WITH bla_f32_to_bf16's ROUNDING (r) IMMEDIATELY BEFORE THE PRODUCT; accumulation, softmax, its derivative,
 * bias, scaling and every stored tensor are fp32.  Per image, Z = X^T (S x C), inv = (float)(1 / sqrt((double)d)):
 *   forward:  Q = r(Z) r(Wq), K = r(Z) r(Wk), V = r(Z) r(Wv);  T = inv (r(Q) r(K)^T);  P = softmax of T's rows, the row maximum subtracted;
 *             A = r(P) r(V);  out [C][S] = (r(A) r(W) + bias)^T.
 *             Written: ws->q, k, v, weights (= P), attention (= A), all fp32, and d_out; ws->scores_raw is not written and may be NULL.
 *   backward (the intended composition only, no jacobian_from_raw):
 *             del_W = sum_b r(A)^T r(del_Y');  del_P = r(del_Y') r(W)^T;  del_S = r(del_P) r(V)^T;  del_V = r(P)^T r(del_P);
 *             del_I = inv P o (del_S - <P, del_S> per row);  del_Q = r(del_I) r(K);  del_K = r(del_I)^T r(Q);
 *             del_Wq/k/v = sum_b r(Z)^T r(del_Q/K/V);  del_X = r(Wq) r(del_Q)^T + r(Wk) r(del_K)^T + r(Wv) r(del_V)^T.
 *             grad->q, k, v receive del_Q, del_K, del_V; the other grad fields may be NULL and are not written.  d_partials: caller-owned scratch of
 *             [batch][4 c d] floats.  Of the S x S tensors only `weights` is in memory: T, del_S and del_I never leave the chip.
 * Sums over the batch and across waves have a fixed order: no atomics, the same bits on every run, and image b of a batch equals a batch-1 run of it.
 * bla_attention_bf16_applies (host only, no device needed) is 1 exactly when s % 32 == 0, 32 <= s <= 256, d % 8 == 0, 8 <= d <= 64 and c % 8 == 0 (a d
 * that is no multiple of 16 contracts over zero padding); outside that set both entries return BLA_ERR_INVALID before any launch, outputs untouched.  A
 * wave holds a query's whole row of scores in registers, which is what bounds s: longer sequences run on the online-softmax entries below
 * (bla_attention_{forward,backward}_batched_online_bf16, s up to 4096).
 * Any batch in 1 .. 65535; no workspace growth, so the entries can be captured without a warm-up rule. */
BLA_API int bla_attention_bf16_applies(int c, int s, int d);
BLA_API bla_status bla_attention_forward_batched_bf16(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv,
                                                      const float* d_w, const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int d);
BLA_API bla_status bla_attention_backward_batched_bf16(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                       const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad,
                                                       float* d_partials, float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x,
                                                       int c, int s, int d);
/* The bf16 attention block for long sequences: the softmax runs ONLINE over blocks of BLA_ATTENTION_ONLINE_KEYS keys taken in ascending
 * order, and NO S x S TENSOR EXISTS IN MEMORY in either direction.  The forward pass saves one float per query, the row's log-sum-exp; the backward pass
 * recomputes the probabilities from Q, K and that float.  The rule is unchanged: BOTH OPERANDS OF EVERY MATRIX PRODUCT ARE ROUNDED WITH bla_f32_to_bf16's
 * ROUNDING (r) IMMEDIATELY BEFORE THE PRODUCT; everything else is fp32.  Per image, Z = X^T, inv = (float)(1 / sqrt((double)d)), key blocks j ascending:
 *   forward:  Q, K, V as in the bf16 entry (the same kernel: the same bits).
 *             m = -inf, l = 0, Acc = 0;  per key block j:
 *               T_j = inv (r(Q) r(K_j)^T);  m' = max(m, rowmax T_j);  a = exp(m - m');  p = exp(T_j - m')
 *               l = l a + rowsum(p)  (p unrounded);  Acc = Acc a + r(p) r(V_j);  m = m'
 *             A = Acc / l;  lse = m + log(l);  out = (r(A) r(W) + bias)^T
 *             Written: ws->q, k, v, attention (= A) as [B][S][d] fp32 and d_out, like the bf16 entry; ws->scores_raw as [B][S] FLOATS, THE ROW
 *             LOG-SUM-EXP lse.  ws->weights is neither read nor written and may be NULL.
 *   backward: del_W = sum_b r(A)^T r(del_Y');  del_P = r(del_Y') r(W)^T;  dot_i = sum_dd del_P[i][dd] A[i][dd]   (fp32)
 *             per key block j:  T_j as above (the same instructions);  P_j = exp(T_j - lse);  del_S_j = r(del_P) r(V_j)^T
 *               del_I_j = inv P_j o (del_S_j - dot);  del_V_j = r(P_j)^T r(del_P);  del_K_j = r(del_I_j)^T r(Q);  del_Q += r(del_I_j) r(K_j)
 *             del_Wq/k/v, del_X: as in the bf16 entry.
 *             Read: fwd->q, k, v, attention, scores_raw (= lse).  grad->q, k, v receive del_Q, del_K, del_V; grad->attention receives del_P as
 *             [B][S][d]; grad->scores_raw receives the row dots as [B][S]; grad->weights is unused and may be NULL.  d_partials: [batch][4 c d].
 *             dot_i = <del_P_i, A_i> equals <P_i, del_S_i> of the materialised block in exact arithmetic: that is what lets the pass run without P.
 * Every sum over key blocks, query blocks, waves and the batch has a fixed order: no atomics, the same bits on every run, and image b of a batch equals a
 * batch-1 run of it.  The entries are NOT bit-equal to bla_attention_*_batched_bf16 on shapes both accept (the unnormalised p is what is rounded here).
 * bla_attention_online_bf16_applies (host only) is 1 exactly when s % 32 == 0, 32 <= s <= 4096, d % 8 == 0, 8 <= d <= 64, c % 8 == 0 and c > 0; outside
 * that set both entries return BLA_ERR_INVALID before any launch, outputs untouched.  Any batch in 1 .. 65535; no workspace growth, so the entries can
 * be captured without a warm-up rule. */
#define BLA_ATTENTION_ONLINE_KEYS 32   /* keys per step of the online softmax */
BLA_API int bla_attention_online_bf16_applies(int c, int s, int d);
BLA_API bla_status bla_attention_forward_batched_online_bf16(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv,
                                                             const float* d_w, const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int d);
BLA_API bla_status bla_attention_backward_batched_online_bf16(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                              const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad,
                                                              float* d_partials, float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w,
                                                              float* d_del_x, int c, int s, int d);
/* Multi-head attention on the online block: `heads` heads of width d, D = heads d the width of the block.  bla_unet_create_heads routes
 * to these entries.  Layouts: Wq, Wk, Wv [C][D], head h in columns h d .. h d + d - 1;  W [D][C], head h in rows h d .. h d + d - 1;  bias [C];
 * ws->q, k, v, attention and grad->q, k, v, attention [B][S][D], a head's columns as in Wq;  ws->scores_raw [B][heads][S], the row log-sum-exp of each
 * head;  grad->scores_raw [B][heads][S], the row dots of each head;  `weights` unused, may be NULL;  d_partials [batch][4 c D].  Float alignment only.
 * Arithmetic: the rule and the notation of the online entries above.  Q = r(Z) r(Wq), K, V likewise, at width D (the contraction over C in ascending
 * 16-deep steps: a column's bits do not depend on D).  Per head h, with Q_h, K_h, V_h, A_h, del_P_h the head's d columns and
 * inv = (float)(1 / sqrt((double)d)) -- THE HEAD'S WIDTH, NOT D -- the forward recurrence above with the head's own m, l, Acc and lse_h, and the
 * backward pass above with dot_h,i = sum over the head's d columns of del_P[i][dd] A[i][dd], P_j = exp(T_h,j - lse_h), del_Q_h, del_K_h, del_V_h.
 * Across heads:  out = (r(A) r(W) + bias)^T, the contraction over all D columns in ascending 16-deep steps;  del_P = r(del_Y') r(W)^T (head h from W's
 * rows of head h);  del_W, del_Wq/k/v and del_X as in the bf16 entry at width D (del_X sums the three products over all D columns).
 * A head's q, k, v, attention, lse, del_P, dots, del_Q/K/V and its slices of the four weight gradients are bit for bit what the single-head online
 * entries give on that head's slices of the weights; out and del_X are sums over the heads and equal them only at heads == 1, where both entries ARE
 * the single-head entries (every layout above is then theirs).  Every sum has a fixed order: no atomics, the same bits on every run, and image b of a
 * batch equals a batch-1 run of it.  No S x S tensor exists in memory.
 * bla_attention_online_bf16_heads_applies (host only) is 1 exactly when s % 32 == 0, 32 <= s <= 4096, d % 8 == 0, 8 <= d <= 64, heads >= 1,
 * heads d <= 256, c % 8 == 0 and c > 0; outside that set, or with batch outside 1 .. 65535 or a NULL operand or workspace field that is read or written,
 * both entries return BLA_ERR_INVALID before any launch, outputs untouched.  Forward: 3 launches (qkv, core, output product); backward: 5.  No workspace
 * growth, so the entries can be captured without a warm-up rule. */
BLA_API int bla_attention_online_bf16_heads_applies(int c, int s, int heads, int d);
BLA_API bla_status bla_attention_forward_batched_online_bf16_heads(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk,
                                                                   const float* d_wv, const float* d_w, const float* d_bias, const bla_attention_ws* ws,
                                                                   float* d_out, int c, int s, int heads, int d);
BLA_API bla_status bla_attention_backward_batched_online_bf16_heads(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq,
                                                                    const float* d_wk, const float* d_wv, const float* d_w, const bla_attention_ws* fwd,
                                                                    const bla_attention_ws* grad, float* d_partials, float* d_del_wq, float* d_del_wk,
                                                                    float* d_del_wv, float* d_del_w, float* d_del_x, int c, int s, int heads, int d);
/* Multi-head attention in fp32 for short sequences: the fp32 batched block's arithmetic per head, with the materialised softmax -- what a
 * multi-head block runs where the online entries above do not apply (S < 32 or no multiple of 32: the 4 x 4 mid block).  bla_unet_create_heads routes to it.
 * Layouts, as in the online heads entries: Wq, Wk, Wv [C][D], D = heads d, head h in columns h d .. h d + d - 1;  W [D][C], head h in rows h d .. h d + d - 1;
 * bias [C];  ws->q, k, v, attention and grad->q, k, v, attention (= del_P) [B][S][D], a head's columns as in Wq;  ws->weights = P as [B][heads][S][S];
 * scores_raw is neither read nor written and may be NULL in both workspaces;  grad->weights is unused and may be NULL;  d_partials [batch][C D].  Float
 * alignment only; S and d need not be multiples of anything.
 * Per image, Z = X^T, inv = (float)(1 / sqrt((double)d)) -- THE HEAD'S WIDTH, NOT D:
 *   forward:  Q = Z Wq, K = Z Wk, V = Z Wv at width D;  per head h:  T_h = inv (Q_h K_h^T);  P_h = softmax of T_h's rows, the row maximum subtracted;
 *             A_h = P_h V_h;  out [C][S] = (A W + bias)^T, the contraction over all D columns.
 *   backward (the intended composition only, no jacobian_from_raw):  del_W = sum_b A^T del_Y';  del_P = del_Y' W^T (head h from W's rows of head h);  per head:
 *             del_S_h = del_P_h V_h^T;  dot_i = <P_h,i, del_S_h,i> (double, rounded once);  del_I_h = inv P_h o (del_S_h - dot);  del_V_h = P_h^T del_P_h;
 *             del_Q_h = del_I_h K_h;  del_K_h = del_I_h^T Q_h;  then del_Wq/k/v = sum_b Z^T del_Q/K/V and del_X = Wq del_Q^T + Wk del_K^T + Wv del_V^T at width D.
 * The products at width D are the fp32 batched block's own calls (bla_gemm_batched_f32, the sums over the batch in image order) with d := D.  The per-head
 * part is two fused kernels, one workgroup per (image, head): T, del_S and del_I never leave the chip, P is stored once.  Every sum in them is one thread's
 * loop in ascending index order: no atomics, the same bits on every run, and in them image b of a batch equals a batch-1 run of it (the width-D products
 * keep bla_gemm_batched_f32's plan, which is the same for every batch while 32 x 32 tiles x batch stays below 129).  Forward: 5 launches; backward: 11 or 13.
 * heads == 1: the entries ARE bla_attention_{forward,backward}_batched_f32 (jacobian_from_raw = 0) -- the same launches, the same bits, every layout above
 * is then theirs -- and scores_raw (both workspaces) and grad->weights are REQUIRED, as they are there.
 * bla_attention_f32_heads_applies (host only) is 1 exactly when 1 <= s <= 64, 1 <= d <= 64, heads >= 1, heads d <= 256 and c > 0; outside that set, or with
 * batch outside 1 .. 65535 or a NULL operand or workspace field that is read or written, both entries return BLA_ERR_INVALID before any launch, outputs
 * untouched.  No workspace growth beyond what bla_gemm_batched_f32 may ask for. */
BLA_API int bla_attention_f32_heads_applies(int c, int s, int heads, int d);
BLA_API bla_status bla_attention_forward_batched_f32_heads(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv,
                                                           const float* d_w, const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int heads,
                                                           int d);
BLA_API bla_status bla_attention_backward_batched_f32_heads(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                            const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad,
                                                            float* d_partials, float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x,
                                                            int c, int s, int heads, int d);
/* Online-softmax attention in fp32: the recurrence of the online bf16 entries with NOTHING ROUNDED TO bf16, for any S up to 4096, any head width
 * up to 64 and any C -- the fp32 path for the long blocks of a multi-head model, for sequence lengths no other multi-head path takes (S % 32 != 0 past 64), and
 * an fp32 block without S x S tensors.  Layouts are the online heads entries': Wq, Wk, Wv [C][D], D = heads d, head h in columns h d .. h d + d - 1;  W [D][C];
 * bias [C];  ws->q, k, v, attention and grad->q, k, v, attention (= del_P) [B][S][D];  ws->scores_raw [B][heads][S], the row log-sum-exp of each head;
 * grad->scores_raw [B][heads][S], the row dots of each head;  `weights` is neither read nor written and may be NULL in both;  d_partials [batch][C D].  Float
 * alignment only; S, d and C need not be multiples of anything.  heads = 1 is the single-head block.
 * Per image, Z = X^T, inv = (float)(1 / sqrt((double)d)) -- THE HEAD'S WIDTH, NOT D -- key blocks j of BLA_ATTENTION_ONLINE_KEYS keys in ascending order:
 *   forward:  Q = Z Wq, K = Z Wk, V = Z Wv at width D (the fp32 batched block's products).  Per head and query row:  m = -inf, l = 0, Acc = 0;  per key block j:
 *               T_j = (Q K_j^T) inv, the scaling a rounding of its own (__fmul_rn: the backward pass sees the same bits);  m' = max(m, rowmax T_j);
 *               a = exp(m - m');  p = exp(T_j - m');  l = l a + rowsum(p);  Acc = Acc a + p V_j;  m = m'
 *             A = Acc / l;  lse = m + log(l);  out = (A W + bias)^T, the contraction over all D columns.
 *   backward: del_W = sum_b A^T del_Y';  del_P = del_Y' W^T;  dot_i = sum over the head's d columns of del_P[i][dd] A[i][dd] (dd ascending);  per key block j:
 *               P_j = exp(T_j - lse);  del_S_j = del_P V_j^T;  del_I_j = (P_j o (del_S_j - dot)) inv;  del_V_j = P_j^T del_P;  del_K_j = del_I_j^T Q;
 *               del_Q += del_I_j K_j
 *             then del_Wq/k/v = sum_b Z^T del_Q/K/V and del_X = Wq del_Q^T + Wk del_K^T + Wv del_V^T at width D.
 * The last key block may be ragged: a key at or beyond S counts as T = -inf, p = 0, and its K and V rows are read as zeros; every block holds at least one real
 * key, so no row is ever all -inf.  A query row at or beyond S is neither stored nor fed into a sum.  Every product of the per-head core runs on the fp32 MFMA
 * (v_mfma_f32_32x32x2_f32); every sum has a fixed order: no atomics, the same bits on every run, and in the core image b of a batch equals a batch-1 run of it
 * (the width-D products keep bla_gemm_batched_f32's plan, as in the fp32 heads entries).  Forward: 5 launches; backward: 4 beside the shared stages'.
 * bla_attention_online_f32_applies (host only) is 1 exactly when 1 <= s <= 4096, 1 <= d <= 64, heads >= 1, heads d <= 256 and c > 0; outside that set, or with
 * batch outside 1 .. 65535 or a NULL operand or workspace field that is read or written, both entries return BLA_ERR_INVALID before any launch, outputs
 * untouched. */
BLA_API int bla_attention_online_f32_applies(int c, int s, int heads, int d);
BLA_API bla_status bla_attention_forward_batched_online_f32(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv,
                                                            const float* d_w, const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int heads,
                                                            int d);
BLA_API bla_status bla_attention_backward_batched_online_f32(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                             const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad,
                                                             float* d_partials, float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x,
                                                             int c, int s, int heads, int d);
BLA_API bla_status bla_resnet_forward_batched_f32(void* stream, int batch, const float* d_x, const float* d_temb, const bla_resnet_params* p,
                                                  const unsigned char* d_drop, const bla_resnet_ws* ws, float* d_result, int h, int w, int cin, int cout, int k,
                                                  int tdim, int group_size);
BLA_API bla_status bla_resnet_backward_batched_f32(void* stream, int batch, const float* d_del_out, const float* d_x, const float* d_temb,
                                                   const bla_resnet_params* p, const bla_resnet_ws* ws, const bla_resnet_grads* g, const bla_resnet_scratch* sc,
                                                   float* d_dtb, float* d_del_x, int h, int w, int cin, int cout, int k, int tdim, int group_size);
/* The batched ResNet block with bf16 products inside: bla_resnet_{forward,backward}_batched_f32's arguments, every tensor with the same
 * meaning, layout and type (x, temb, parameters, d_drop, result, del_out, gradients, d_dtb, del_x -- which may be NULL), plus the three padded channel-last
 * bf16 maps that take the role of ws->relu1, ws->relu2 and ws->dp (those three are not written and may be NULL; mu1 / sd1, c1, tdense, mu2 / sd2, c2 and
 * res keep their meaning).  With (hp, wp, top, left) = bla_conv_bf16_layout(h, w, k, 1, 0) and (hq, wq, ..) = bla_conv_bf16_layout(h, w, k, 1, 1):
 *   maps->p1 [B][hp][wp][round8(cin)], maps->p2 [B][hp][wp][round8(cout)] in the forward layout, maps->q1 [B][hq][wq][round8(cout)] in the data-gradient
 *   layout; 16-byte aligned; the caller zero-fills each ONCE -- the entries write pixel positions only, so the halos stay valid for every later pass.
 * The kernel matrices and Q2 live in the context workspace: these calls may grow it (the capture rule of the _as_bf16 entries applies).  Any batch >= 1.
 * Forward, exactly this composition of public entries, bit for bit:
 *   (1) bla_group_norm_relu_bf16_map(x -> p1; mu1, sd1);  (2) tdense = temb . W_t + b_t by bla_gemm_f32 (bias_col), as the fp32 block;
 *   (3) bla_conv_bf16_prepare_kernels(conv1, 0); c1 = bla_conv2d_gathered_bf16(A1, p1) with ep_bias = tdense, stride cout;
 *   (4) bla_group_norm_relu_bf16_map(c1, d_drop -> p2; mu2, sd2);  (5) prepare_kernels(conv2, 0); c2 = bla_conv2d_gathered_bf16(A2, p2);
 *   (6) r = x, or for cin != cout  ws->res = bla_conv2d_forward_batched_f32_as_bf16(x, res, k = 1);  (7) result = bla_sum_f32(c2, r).
 * Backward (splits: the weight gradients' K-split, 0 = the automatic rule), exactly this composition, bit for bit:
 *   (1) Q2 = bla_conv_bf16_pad(del_out) in conv2's data-gradient layout;  (2) g->conv2 = bla_conv2d_weight_gradient_gathered_bf16(Q2, p2, splits);
 *   (3) prepare_kernels(conv2, 1); sc->g_out_a = bla_conv2d_gathered_bf16_chained(A2', Q2, stride 1, gate = p2, out_f32) -- the gate on the bf16 map is the
 *       dropout mask and ReLU's derivative at once, as dp <= 0 is in the fp32 block;
 *   (4) bla_group_norm_ddx_bf16_map(g_out_a, c1, mu2, sd2 -> dest_f32 = sc->g_out_b, dst = q1);
 *   (5) d_dtb = bla_col_sum_f32(g_out_b, B cout, h w, INTENDED); g->time_b = the sum of d_dtb's rows in image order; g->time_w = temb^T . d_dtb (bla_gemm_f32);
 *   (6) g->conv1 = bla_conv2d_weight_gradient_gathered_bf16(q1, p1, splits);
 *   (7) with d_del_x: for cin != cout first bla_conv2d_backward_gathered_f32_as_bf16(del_out, x, res, g->res, g_res, k = 1, splits), g_res in the context's
 *       second scratch; prepare_kernels(conv1, 1); sc->g_in = chained(A1', q1, gate = p1, out_f32);
 *       del_x = bla_group_norm_ddx_gated_batched_f32(g_in, x, mu1, sd1, gate NULL, addend = del_out or g_res);
 *   (8) with d_del_x == NULL the two data gradients and the last norm gradient are skipped; the weight gradients, the residual kernel's included, are formed.
 * The gates read the bf16 activation the forward product actually multiplied: the derivative of the mixed-precision forward pass.  It differs from the fp32
 * block's gate only where a positive fp32 activation rounds to bf16 zero.  sc->flip is not used.
 * BLA_ERR_INVALID, before the device is asked for and with every output untouched: a NULL tensor, parameter, gradient, workspace field named above, scratch or
 * map; an extent <= 0; splits < 0; a map off 16-byte alignment; cin != cout without the residual kernels (their gradient, ws->res). */
typedef struct bla_resnet_bf16_maps { uint16_t *p1, *p2, *q1; } bla_resnet_bf16_maps;
BLA_API bla_status bla_resnet_forward_batched_bf16(void* stream, int batch, const float* d_x, const float* d_temb, const bla_resnet_params* p,
                                                   const unsigned char* d_drop, const bla_resnet_ws* ws, float* d_result, int h, int w, int cin, int cout, int k,
                                                   int tdim, int group_size, const bla_resnet_bf16_maps* maps);
BLA_API bla_status bla_resnet_backward_batched_bf16(void* stream, int batch, const float* d_del_out, const float* d_x, const float* d_temb,
                                                    const bla_resnet_params* p, const bla_resnet_ws* ws, const bla_resnet_grads* g, const bla_resnet_scratch* sc,
                                                    float* d_dtb, float* d_del_x, int h, int w, int cin, int cout, int k, int tdim, int group_size,
                                                    const bla_resnet_bf16_maps* maps, int splits);

/* ---- lib/layer.h on the device, batched: feed_forward (lib/layer.c:6-20) and back_propagate_errors with its recursion
 * (:48-107) for `batch` samples (columns) at once, parameters resident in one bucket (W_1, b_1, W_2, b_2, ...; W_l is n_l x n_{l-1}).  The
 * reference's activation callbacks become one of a few device functions; with batch = 1 the arithmetic is layer.c's step by step, with more
 * columns the weight / bias steps are summed over the columns (all gradients taken at the weights as they were before the call). */
enum { BLA_LAYER_ACT_IDENTITY = 0, BLA_LAYER_ACT_SCALE = 1 /* a = p x, a' = p (main.c:7-17 with p = 0.1) */, BLA_LAYER_ACT_RELU = 2,
       BLA_LAYER_ACT_LEAKY = 3 /* a = x < 0 ? p x : x */ };
typedef struct bla_layer_net bla_layer_net;
/* sizes[num_layers] incl. the input layer; acts / act_params [num_layers - 1] for the computing layers */
BLA_API bla_status bla_layer_net_create(bla_layer_net** out, const int* sizes, int num_layers, int batch, const int* acts, const float* act_params);
BLA_API bla_status bla_layer_net_destroy(bla_layer_net* m);
BLA_API size_t bla_layer_net_param_count(const bla_layer_net* m);
BLA_API float* bla_layer_net_params(bla_layer_net* m);
BLA_API float* bla_layer_net_weights(bla_layer_net* m, int layer);     /* device, layer >= 1 */
BLA_API float* bla_layer_net_biases(bla_layer_net* m, int layer);
BLA_API float* bla_layer_net_nodes(bla_layer_net* m, int layer);       /* [n_layer][batch] after a forward pass */
BLA_API float* bla_layer_net_raw_nodes(bla_layer_net* m, int layer);
/* d_x is read again by the backward pass (it is the first computing layer's a_prev, lib/layer.c:67): keep it valid until then */
BLA_API bla_status bla_layer_net_forward_f32(bla_layer_net* m, void* stream, const float* d_x /* [n_0][batch] */);
BLA_API bla_status bla_layer_net_backward_f32(bla_layer_net* m, void* stream, const float* d_expect /* [n_L][batch] */, float learn_rate);

/* ---- the U-Net of model/cifar_unet.c assembled from the blocks above: forward() (:1099-1166) and backward() (:1351-1436) for one image.
 * 18 ResNet blocks, 5 self-attention blocks, 3 stride-2 convolutions, 3 nearest-neighbour up-samplings (+ a convolution where the widths of the
 * two resolutions differ), 4 skip concatenations, output group norm + ReLU + convolution.  Parameters and gradients live in two flat buckets;
 * bla_unet_tensor_info enumerates the tensors (names follow the reference's struct members, e.g. "down_2_resnet_1.conv_1_kernels",
 * "mid_self_attention.Q_proj", "up_3_conv_kernels") in the order forward() first uses them.  The wiring is the INTENDED network: see
 * csrc/bla_unet_model.hip for the four places where the reference's work-in-progress call sites differ.
 * Reference constants (:26-37): image 32 x 32 x 3, dims {128, 256, 256, 256}, time_dim 512, kernel 3, group_size 32, key_dim 16. */
typedef struct bla_unet_config { int image_h, image_w, in_channels, dims[4], time_dim, kernel, group_size, key_dim; } bla_unet_config;
typedef struct bla_unet bla_unet;
BLA_API bla_status bla_unet_create(bla_unet** out, const bla_unet_config* cfg);
/* The same network for `batch` images per pass: d_x / the output / d_noise are [B][C][H][W], d_time_embedding [B][time_dim] (every image its own
 * time step), the gradients are summed over the images (what `batch` passes of the reference's one-image loop accumulate).  d_drop: the blocks
 * in forward order, inside a block image by image.  bla_unet_create = batch 1. */
BLA_API bla_status bla_unet_create_batched(bla_unet** out, const bla_unet_config* cfg, int batch);
/* The same network with its convolutions multiplied in bf16.  products = BLA_UNET_PRODUCTS_F32: exactly bla_unet_create_batched (which, like
 * bla_unet_create, is this call).  BLA_UNET_PRODUCTS_BF16, any batch >= 1: the 18 ResNet blocks run bla_resnet_{forward,backward}_batched_bf16's arithmetic
 * (each block owns its maps p1, p2, q1, laid out as stated there, zero-filled once here and freed with the model), the stride-2, up-sampling and output
 * convolutions run bla_conv2d_forward_batched_f32_as_bf16 / bla_conv2d_backward_gathered_f32_as_bf16 (splits 0); attention, the output norm, resizing,
 * concatenation, the skip additions and the loss seed stay fp32, on one stream.  Parameters, gradients, the tensor table, the dropout layout and the output
 * are fp32 with the same order and layout in both modes, so bla_unet_forward_f32, bla_unet_backward_f32, bla_unet_backward_from_f32,
 * bla_unet_embedding_grad_f32, every sampler, bla_unet_evaluate_f32 and the optimiser entries take either model, and parameters trained in one mode load in
 * the other.  All bf16 kernel matrices of a pass are prepared by ONE bla_conv_bf16_prepare_kernels_table launch at its head, into matrices the model owns
 * (not the context workspace); BLA_UNET_BF16_PREP=0 in the environment, read at every create call, makes a model created afterwards prepare each matrix in
 * front of its product instead (the same bits).  Any other `products` value: BLA_ERR_INVALID before the device is asked for, *out untouched. */
enum { BLA_UNET_PRODUCTS_F32 = 0, BLA_UNET_PRODUCTS_BF16 = 1 };
BLA_API bla_status bla_unet_create_mixed(bla_unet** out, const bla_unet_config* cfg, int batch, int products);
BLA_API int bla_unet_products(const bla_unet* m);               /* the mode the model was created with */
/* Where the model's self-attention blocks multiply; orthogonal to `products`.  BLA_UNET_ATTENTION_F32 (the default after every create entry):
 * bla_attention_{forward,backward}_batched_f32, as always -- a model never switched is bit-equal to before in both `products` modes.
 * BLA_UNET_ATTENTION_BF16: an attention block whose shape bla_attention_bf16_applies accepts runs bla_attention_{forward,backward}_batched_bf16, bit for
 * bit those entries; a block it refuses (at the reference's constants the 4 x 4 mid block, S = 16) keeps the fp32 entries.  Both paths share the block's
 * bla_attention_ws, so the setter is legal between passes (not between a forward pass and its backward pass).
 * BLA_UNET_ATTENTION_BF16_ONLINE: a block that bla_attention_online_bf16_applies accepts (S up to 4096) runs
 * bla_attention_{forward,backward}_batched_online_bf16, bit for bit those entries; every other block keeps the fp32 entries.  The row log-sum-exp lives in
 * the first B S floats of the block's scores_raw, the row dots in the gradient workspace's; nothing more is allocated.
 * The mode is a bit set: bit 0 = bf16 products, bit 1 = the online softmax.  2 (an online softmax on fp32 products) does not exist; it and any other
 * value: BLA_ERR_INVALID, the model unchanged.
 * BLA_UNET_ATTENTION_F32_ONLINE = 4 (outside the bit set): a block with S > 64 runs bla_attention_{forward,backward}_batched_online_f32, bit for bit
 * those entries, for any number of heads; every other block keeps the route it has under BLA_UNET_ATTENTION_F32.  The row log-sum-exp and the row dots live
 * where mode 3 and the online heads route keep them (the first B heads S floats of scores_raw).  A model switched to mode 4 and back behaves as before.
 * On a model that bla_unet_create_attention created in mode 4 the setter returns BLA_ERR_INVALID, mode and routes unchanged, where the new mode would leave a
 * block without a route or give a block a route whose buffers the model does not own. */
enum { BLA_UNET_ATTENTION_F32 = 0, BLA_UNET_ATTENTION_BF16 = 1, BLA_UNET_ATTENTION_BF16_ONLINE = 3, BLA_UNET_ATTENTION_F32_ONLINE = 4 };
BLA_API bla_status bla_unet_set_attention(bla_unet* m, int mode);
BLA_API int bla_unet_attention(const bla_unet* m);
/* The same network with multi-head self-attention: every attention block has `heads` heads of width cfg->key_dim -- bla_unet_config is unchanged,
 * key_dim stays the width of ONE head -- so its Q_proj, K_proj, V_proj tensors are [C][D] and its `weights` tensor [D][C], D = heads key_dim, laid out as the
 * heads entries above state; bla_unet_tensor_info and bla_unet_param_count report those sizes.  heads == 1 is bla_unet_create_mixed in every respect.
 * heads > 1, routing per block, asked at every call:
 *   BLA_UNET_ATTENTION_F32 (the default): bla_attention_{forward,backward}_batched_f32_heads where bla_attention_f32_heads_applies accepts the block (S <= 64),
 *     otherwise bla_attention_{forward,backward}_batched_online_bf16_heads;
 *   BLA_UNET_ATTENTION_BF16_ONLINE: the online heads entries where bla_attention_online_bf16_heads_applies accepts the block, otherwise the fp32 heads entries;
 *   BLA_UNET_ATTENTION_BF16: bla_unet_set_attention returns BLA_ERR_INVALID, the model unchanged (the materialising bf16 block has no heads).
 * SO A heads > 1 MODEL'S LONG BLOCKS (S > 64) MULTIPLY IN bf16 ON THE ONLINE SOFTMAX IN BOTH OF THESE MODES, BLA_UNET_ATTENTION_F32 INCLUDED; the fp32 path
 * for them is BLA_UNET_ATTENTION_F32_ONLINE (above; bla_unet_create_attention below).  At the reference's constants that is the four 16 x 16 blocks (S = 256); the 4 x 4 mid block (S = 16) is fp32 in mode 0.
 * A block that neither predicate accepts (e.g. 36 x 36 images: S = 324 at level 1), heads < 1 or heads key_dim > 256: BLA_ERR_INVALID, nothing allocated
 * is left behind, *out untouched.  A heads > 1 model allocates P ([B][heads][S][S]) only for the blocks the fp32 heads predicate accepts; its other per-block
 * buffers beside q, k, v, attention are B heads S floats (the row log-sum-exp / the row dots): no S x S buffer exists for the long blocks. */
BLA_API bla_status bla_unet_create_heads(bla_unet** out, const bla_unet_config* cfg, int batch, int products, int heads);
BLA_API int bla_unet_heads(const bla_unet* m);                  /* the number of heads the model was created with (1 for every other create entry) */
/* The same network created IN its attention mode.  attention = BLA_UNET_ATTENTION_F32, _BF16 or _BF16_ONLINE: bla_unet_create_heads followed by
 * bla_unet_set_attention -- the same refusals, bits and bytes.  BLA_UNET_ATTENTION_F32_ONLINE: every block has a route (a 36 x 36 or 40 x 40 multi-head model is
 * created), a block routed to the online fp32 entries owns B heads S floats beside q, k, v, attention and NO S x S buffer, and the shared gradient workspace is
 * sized for the largest block that still materialises.  Such a model refuses bla_unet_set_attention to a mode it lacks a route or the buffers for (see there).
 * Any other `attention`: BLA_ERR_INVALID, *out untouched.  bla_unet_device_bytes: the sum of the device allocations the model owns, in bytes. */
BLA_API bla_status bla_unet_create_attention(bla_unet** out, const bla_unet_config* cfg, int batch, int products, int heads, int attention);
BLA_API size_t bla_unet_device_bytes(const bla_unet* m);
BLA_API int bla_unet_batch(const bla_unet* m);
BLA_API bla_status bla_unet_destroy(bla_unet* m);
BLA_API size_t bla_unet_param_count(const bla_unet* m);         /* floats in each bucket (every tensor starts 16-byte aligned) */
BLA_API float* bla_unet_params(bla_unet* m);                    /* device */
BLA_API float* bla_unet_grads(bla_unet* m);                     /* device; written by bla_unet_backward_f32 */
BLA_API float* bla_unet_output(bla_unet* m);                    /* device, [in_channels][H][W]: the predicted noise */
BLA_API int bla_unet_tensor_count(const bla_unet* m);
BLA_API bla_status bla_unet_tensor_info(const bla_unet* m, int index, size_t* offset, size_t* count, char* name, int name_len);
/* _dropout (:1032-1042) draws one decision per element of every ResNet block's second ReLU, in forward order: d_drop holds
 * bla_unet_dropout_count() of them (non-zero = dropped; the host makes the draws from its own rand() stream), NULL = keep everything. */
BLA_API size_t bla_unet_dropout_count(const bla_unet* m);
BLA_API bla_status bla_unet_forward_f32(bla_unet* m, void* stream, const float* d_x /* [C][H][W] */, const float* d_time_embedding /* [time_dim] */,
                                        const unsigned char* d_drop);
/* del_Y = 2 (prediction - noise) (:1353-1364), then every block backwards; uses the activations of the last forward pass */
BLA_API bla_status bla_unet_backward_f32(bla_unet* m, void* stream, const float* d_noise /* [C][H][W] */);
/* The same pass seeded with the caller's gradient of the loss with respect to the output instead of 2 (prediction - noise): d_del_y has the output's
 * layout ([B][C][H][W] on a batched model) and is only read (it must stay as it is until the stream has passed this call).  With d_del_y =
 * 2 (output - noise) in fp32 the gradient bucket is bla_unet_backward_f32's, bit for bit.  Refused like it: a NULL argument, or no forward pass so far.
 * bla_unet_embedding_grad_f32 works behind either. */
BLA_API bla_status bla_unet_backward_from_f32(bla_unet* m, void* stream, const float* d_del_y);

/* ---- training the U-Net as a diffusion model (DDPM, Ho et al. 2020) and drawing images from it ----------------------------------------------
 * Not in the reference: its train() allocates Adam's two moment sets and never uses them (:1887-1888), never noises an image at a timestep, never
 * writes the time embedding (:535), and run() is empty (:1936).  examples/cifar_unet_gpu.c `fit` / `sample` drive these.
 *
 * Counter-based random numbers, Philox4x32-10 (Salmon et al., SC'11): key = (lo32(seed), hi32(seed)); element i of the stream (seed, offset) is word
 * i % 4 of block j = offset + i / 4 (64-bit), counter {lo32(j), hi32(j), tag, 0}, tag 0 = u32, 1 = normal, 2 = Bernoulli (the three streams never
 * share a block).  A round maps (c0, c1, c2, c3) to (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), M0 = 0xD2511F53,
 * M1 = 0xCD9E8D57; the key adds (0x9E3779B9, 0xBB67AE85) between rounds; 10 rounds.  Normal: Box-Muller on the word pairs (w0, w1) and (w2, w3),
 * u = ((w >> 8) + 0.5) * 2^-24 evaluated in fp32 (in (0, 1]), r = sqrt(-2 ln u_first), element 4j + 0 / 1 = r cos / r sin (2 pi u_second), the same
 * for 4j + 2 / 3; out = mean + stddev * z.  Bernoulli: 1 = w < floor(p * 2^32), one byte per decision (the d_drop layout of bla_unet_forward_f32).
 * Any alignment and any n; 16-byte stores in the body. */
BLA_API bla_status bla_rand_u32(void* stream, unsigned int* d_out, size_t n, unsigned long long seed, unsigned long long offset);
BLA_API bla_status bla_rand_normal_f32(void* stream, float* d_out, size_t n, float mean, float stddev, unsigned long long seed, unsigned long long offset);
BLA_API bla_status bla_rand_bernoulli_u8(void* stream, unsigned char* d_out, size_t n, float p, unsigned long long seed, unsigned long long offset);
/* A permutation from the stream, one per epoch for a shuffled training set: d_keys [n] = bla_rand_u32(seed, offset)[0..n); d_out [n] = the stable
 * ascending argsort of d_keys (equal keys: lower index first) -- np.argsort(keys, kind="stable"), bit-reproducible.  A rank kernel, O(n^2) compares
 * (2.5e9 for CIFAR-10's 50,000 records).  1 <= n <= 2^20, else BLA_ERR_INVALID; n = 0 does nothing.  The two buffers must differ. */
BLA_API bla_status bla_rand_permutation_u32(void* stream, unsigned int* d_out, unsigned int* d_keys, size_t n, unsigned long long seed,
                                            unsigned long long offset);
/* Adam / AdamW over n floats in one pass (torch.optim.AdamW(foreach=False), step for step): g = grad_scale * grad; p *= 1 - lr * weight_decay;
 * m = beta1 m + (1 - beta1) g; v = beta2 v + (1 - beta2) g^2; p -= lr / (1 - beta1^step) * m / (sqrt(v) / sqrt(1 - beta2^step) + eps).  The bias
 * corrections are formed in double on the host.  step >= 1 counts the updates so far, this one included; grad_scale = 1 / B for the U-Net's
 * gradients (summed over the images).  m and v start zeroed. */
BLA_API bla_status bla_adam_f32(void* stream, float* d_params, const float* d_grads, float* d_m, float* d_v, size_t n, float lr, float beta1, float beta2, float eps,
                                float weight_decay, float grad_scale, int step);
/* Global-norm gradient clipping without a host round trip (torch.nn.utils.clip_grad_norm_): bla_memset the accumulator, one
 * bla_sumsq_accumulate_f32 per gradient bucket, bla_clip_scale_f32, then bla_adam_scaled_f32 on every bucket.  None of the three allocates or waits,
 * so the sequence can be captured.
 * *d_acc += sum_i a_i^2, double, fixed order: bit-reproducible run to run.  Many workgroups (partials into d_scratch [BLA_SUMSQ_SCRATCH_DOUBLES],
 * combined in index order).  Any alignment and any n (0: nothing); 16-byte loads in the body.  A non-finite sum is passed on as it is. */
#define BLA_SUMSQ_SCRATCH_DOUBLES 1024
BLA_API bla_status bla_sumsq_accumulate_f32(void* stream, const float* d_a, size_t n, double* d_acc, double* d_scratch);
/* norm = |grad_scale| sqrt(*d_sumsq); *d_scale = (float)(grad_scale * min(1, max_norm / (norm + 1e-6))), formed in double on the device;
 * *d_norm (may be NULL) = (float)norm.  max_norm <= 0 or not finite: BLA_ERR_INVALID.  torch.nn.utils.clip_grad_norm_'s coefficient. */
BLA_API bla_status bla_clip_scale_f32(void* stream, const double* d_sumsq, float grad_scale, float max_norm, float* d_scale, float* d_norm);
/* bla_adam_f32 with grad_scale read from device memory: the clipped gradient is (*d_grad_scale) * grad, a single fp32 factor, and the update is bit
 * for bit bla_adam_f32's with that value as grad_scale. */
BLA_API bla_status bla_adam_scaled_f32(void* stream, float* d_params, const float* d_grads, float* d_m, float* d_v, size_t n, float lr, float beta1,
                                       float beta2, float eps, float weight_decay, const float* d_grad_scale, int step);
/* Exponential moving average of a bucket (the weights DDPM samples from, Ho et al. 2020): e <- e + w (p - e), w = 1 - decay formed in double on the
 * host and rounded to fp32 once, every operation rounded on its own -- bit-equal to numpy float32 e + float32(w) * (p - e).  decay in [0, 1] (else
 * BLA_ERR_INVALID; 1 leaves e as it is).  This applies the decay it is given: any warm-up (e.g. min(decay, (1 + step) / (10 + step)), what
 * examples/cifar_unet_gpu.c uses) is the caller's.  Any alignment and any n (0: nothing); 16-byte loads and stores in the body. */
BLA_API bla_status bla_ema_f32(void* stream, float* d_ema, const float* d_params, size_t n, float decay);
/* Linear beta schedule over `steps` timesteps (DDPM: 1e-4 .. 0.02, steps = 1000): beta_t = beta_start + (beta_end - beta_start) t / (steps - 1),
 * alpha_bar_t = prod_{s <= t} (1 - beta_s), in double at create time; the kernels read fp32 tables of the per-step coefficients. */
typedef struct bla_diffusion bla_diffusion;
BLA_API bla_status bla_diffusion_create(bla_diffusion** out, int steps, float beta_start, float beta_end);
BLA_API bla_status bla_diffusion_destroy(bla_diffusion* d);
BLA_API int bla_diffusion_steps(const bla_diffusion* d);
BLA_API bla_status bla_diffusion_schedule(const bla_diffusion* d, int t, double* beta, double* alpha_bar);   /* host values of step t */
/* d_temb [batch][time_dim] for the timesteps d_t [batch]: w_i = exp(-ln(1e4) i / half), element i = relu(sin(t w_i)), half + i = relu(cos(t w_i)),
 * half = time_dim / 2 (an odd time_dim leaves the last element 0) -- the ReLU'd embedding of :168, evaluated in double. */
BLA_API bla_status bla_time_embedding_f32(void* stream, const int* d_t, int batch, int time_dim, float* d_temb);
/* One launch noises a training batch d_x0 [batch][image_floats] for pass `pass` (< 2^32): t_b = bla_rand_u32(seed, pass << 32)[b] % steps,
 * d_eps = bla_rand_normal_f32(batch * image_floats, 0, 1, seed, pass << 32), d_xt = sqrt(alpha_bar_t) x0 + sqrt(1 - alpha_bar_t) eps,
 * d_temb [batch][time_dim] = the embedding of t_b; all four written.  batch <= 4096. */
BLA_API bla_status bla_diffusion_noise_f32(const bla_diffusion* d, void* stream, const float* d_x0, int batch, size_t image_floats, int time_dim,
                                           unsigned long long seed, unsigned long long pass, int* d_t, float* d_eps, float* d_xt, float* d_temb);
/* Batch assembly fused into the noising launch: exactly bla_diffusion_noise_f32's job, in one launch, on the batch whose image b is record
 * d_index[b] of d_data [records][image_floats] (d_index NULL = records 0 .. batch-1).  Images are [C][H][W] with W = width; when flip is non-zero,
 * image b is mirrored along its innermost axis (out[.., i] = in[.., width-1-i]) where bla_rand_bernoulli_u8(0.5, seed, (pass << 32) + 2^31 + 2^30)[b]
 * is 1 (see the offset table below).  t_b, d_eps and d_temb are indexed by OUTPUT position as in bla_diffusion_noise_f32, so they depend on neither
 * d_index nor flip, and d_xt is bit-equal to what bla_diffusion_noise_f32 writes for the same assembled batch and the same alignment of the buffers.
 * d_x0 (may be NULL) receives the clean assembled batch; d_labels_out[b] = d_labels[d_index[b]] when both are given, ready for
 * bla_class_embedding_f32.  An index >= records reads nothing: that image is all zero and its label -1 (which the class embedding skips).
 * image_floats % width != 0: BLA_ERR_INVALID.  16-byte loads and stores when image_floats % 4 == 0, width % 4 == 0 and d_data, d_eps, d_xt, d_x0 are
 * 16-byte aligned (a mirrored float4 is the float4 at the mirrored position with its components reversed), one element per lane otherwise.
 * batch <= 4096. */
BLA_API bla_status bla_diffusion_noise_gather_f32(const bla_diffusion* d, void* stream, const float* d_data /* [records][image_floats] */, size_t records,
                                                  const unsigned int* d_index /* [batch]; NULL = 0 .. batch-1 */, int flip, int width,
                                                  const int* d_labels /* [records], may be NULL */, int* d_labels_out /* [batch], may be NULL */, int batch,
                                                  size_t image_floats, int time_dim, unsigned long long seed, unsigned long long pass, int* d_t, float* d_eps,
                                                  float* d_xt, float* d_temb, float* d_x0 /* [batch][image_floats], may be NULL */);
/* The DDPM ancestral step at t (sigma_t^2 = beta_t), in place: x <- (x - beta_t / sqrt(1 - alpha_bar_t) eps_hat) / sqrt(1 - beta_t) + sigma_t z,
 * z = bla_rand_normal_f32(batch * image_floats, 0, 1, seed, (t + 1) << 32) (offset 0 stays free for x_T), z = 0 at t = 0.  d_temb_next (may be
 * NULL): the same launch writes the embedding of t - 1 for every image ([batch][time_dim]; nothing at t = 0). */
BLA_API bla_status bla_diffusion_step_f32(const bla_diffusion* d, void* stream, float* d_x, const float* d_eps_hat, int batch, size_t image_floats, int t,
                                          unsigned long long seed, int time_dim, float* d_temb_next);
/* The whole reverse process on the model's batch: for t = steps - 1 .. 0, bla_unet_forward_f32 (no dropout) then bla_diffusion_step_f32 with the model's
 * output.  d_x: in x_T, out x_0, [B][C][H][W].  The [B][time_dim] embedding workspace belongs to the diffusion object and is allocated on first use:
 * like the model's own workspaces, run the sampler once eagerly before capturing it into a graph. */
BLA_API bla_status bla_unet_sample_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, unsigned long long seed);
/* Few-step sampling with DDIM (Song, Meng, Ermon 2021): the same trained network, S << steps forward passes.
 * The timesteps of a run of S = sample_steps, "trailing" spacing: out[i] = floor(steps (i + 1) / S) - 1 for i = 0 .. S-1, increasing; the last is
 * always steps - 1, and S = steps gives every step.  1 <= S <= steps, else BLA_ERR_INVALID.  Host only. */
BLA_API bla_status bla_diffusion_ddim_timesteps(const bla_diffusion* d, int sample_steps, int* out);
/* One DDIM step from t to t_prev (-1: to the data) in place, one launch.  With abar_p = alpha_bar[t_prev] (1 at t_prev = -1):
 *   x0^ = (x - sqrt(1 - abar_t) eps_hat) / sqrt(abar_t), clamped to [-1, 1] (the data range of load_example) when clip is non-zero (eps_hat is
 *         used as it is);
 *   sigma = eta sqrt((1 - abar_p) / (1 - abar_t)) sqrt(1 - abar_t / abar_p);
 *   x <- sqrt(abar_p) x0^ + sqrt(max(0, 1 - abar_p - sigma^2)) eps_hat + sigma z,
 * z = bla_rand_normal_f32(batch * image_floats, 0, 1, seed, (t + 1) << 32) -- bla_diffusion_step_f32's stream layout, x_T keeps offset 0 -- drawn
 * only when sigma > 0 (eta = 0 is deterministic).  The five coefficients are formed in double on the host and passed by value: nothing is uploaded
 * per step, so a captured sampler replays correctly.  d_temb_next (may be NULL) [batch][time_dim]: the embedding of t_prev (nothing at t_prev = -1).
 * t outside [0, steps), t_prev outside [-1, t), eta outside [0, 1] or not finite: BLA_ERR_INVALID.
 * eta = 1 at S = steps is DDPM with the posterior variance beta~_t = beta_t (1 - abar_{t-1}) / (1 - abar_t); the ancestral step above uses
 * sigma_t^2 = beta_t, so the two samplers are not bit-equal there. */
BLA_API bla_status bla_diffusion_ddim_step_f32(const bla_diffusion* d, void* stream, float* d_x, const float* d_eps_hat, int batch, size_t image_floats, int t,
                                               int t_prev, float eta, int clip, unsigned long long seed, int time_dim, float* d_temb_next);
/* DDIM sampling on the model's batch: over the bla_diffusion_ddim_timesteps of sample_steps from the last, bla_unet_forward_f32 (no dropout) then
 * bla_diffusion_ddim_step_f32 with the model's output.  d_x: in x_T, out x_0.  The embedding workspace is bla_unet_sample_f32's (allocated on first
 * use: run once eagerly before capturing it into a graph).  Bad sample_steps or eta: BLA_ERR_INVALID. */
BLA_API bla_status bla_unet_sample_ddim_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, int sample_steps, float eta, int clip,
                                            unsigned long long seed);
/* *d_acc += sum_i (a_i - b_i)^2, accumulated in double in a fixed order (one workgroup): the training loss without a host round trip per pass */
BLA_API bla_status bla_mse_accumulate_f32(void* stream, const float* d_a, const float* d_b, size_t n, double* d_acc);

/* ---- class-conditional diffusion with classifier-free guidance (Ho & Salimans 2022) ----------------------------------------------------------
 * Not in the reference.  A learned class embedding, a table [classes + 1][time_dim] whose row `classes` is the null class, is added to the time
 * embedding; during training the label is dropped at random (the image then uses the null row), so the one network learns the conditional and the
 * unconditional noise prediction.  At sampling time the two are mixed: eps~ = eps_u + s (eps_c - eps_u).  examples/cifar_unet_gpu.c drives these
 * (BLA_UNET_CLASSES / BLA_UNET_CLASS).
 *
 * Philox offsets of a conditional training pass `pass` (bla_diffusion_noise_f32's layout above): noise and timesteps at pass << 32 (tags 0 and 1),
 * the dropout decisions at pass << 32 (tag 2, bla_unet_dropout_count() / 4 blocks), the label dropout at (pass << 32) + (1 << 31) (tag 2, batch / 4
 * blocks, at most 1024), the horizontal flips of bla_diffusion_noise_gather_f32 at (pass << 32) + (1 << 31) + (1 << 30) (tag 2, batch / 4 blocks, at most
 * 1024).  The three tag-2 ranges are disjoint as long as bla_unet_dropout_count() < 2^33, and all stay below the next pass's (pass + 1) << 32.
 * A shuffled epoch e draws its permutation with bla_rand_permutation_u32 at (e << 32) + (1 << 31) (tag 0, at most 2^18 blocks), behind the timestep
 * draws of pass e (tag 0 at e << 32, at most 1024 blocks).
 * Held-out evaluation (bla_unet_evaluate_f32 below) noises its batch at timestep t with the normal stream (tag 1) at offset_base + ((t + 1) << 32),
 * batch * image_floats / 4 blocks.  examples/cifar_unet_gpu.c `eval` gives the batch that starts at record r offset_base = r * image_floats / 4, so
 * record r owns the blocks [r F / 4, (r + 1) F / 4) behind (t + 1) << 32 whatever the batch size (below the next timestep's range up to 2^32 / (F / 4)
 * records).  With offset_base 0 these are the blocks of the samplers' z at the same seed: an evaluation and a sampling run are separate uses. */

/* Gradient of the time-embedding input: d_dtemb [B][time_dim] = dL/dtemb for the loss of the last bla_unet_backward_f32 (del_Y = 2 (pred - noise)).
 * The embedding feeds nothing but the 18 ResNet blocks' projections temb . W_k + bias_k, so dtemb[b] = sum_k W_k . dtb_k[b] with dtb_k[b] the per-image
 * channel sums of the gradient each block's backward pass already forms.  One launch, deterministic (a fixed summation order), changes nothing the
 * backward pass computed.  Every configuration bla_unet_create[_batched] accepts.  BLA_ERR_INVALID when no backward pass has run since the last forward. */
BLA_API bla_status bla_unet_embedding_grad_f32(bla_unet* m, void* stream, float* d_dtemb);
/* Class embedding with label dropout, in place: row_b = classes if bla_rand_bernoulli_u8(p_uncond, seed, offset)[b] is 1, else labels[b];
 * d_temb[b] += d_table[row_b] ([batch][time_dim], table [classes + 1][time_dim]); d_rows [batch] receives the rows.  labels[b] == classes is allowed
 * (that image is forced unconditional).  Labels in host memory are checked on the host: one outside [0, classes] is BLA_ERR_INVALID before anything
 * runs (the call then waits for the stream: not capturable).  Labels in device memory cannot be checked without a round trip: an image whose label
 * lies outside [0, classes] gets row -1 and its embedding is left as it was (bla_class_embedding_grad_f32 skips it).  batch <= 4096. */
BLA_API bla_status bla_class_embedding_f32(void* stream, const float* d_table, int classes, const int* labels, int batch, int time_dim, float p_uncond,
                                           unsigned long long seed, unsigned long long offset, int* d_rows, float* d_temb);
/* Gradient of the table: d_gtable[k] = sum over the images b with d_rows[b] == k, in image order, of d_dtemb[b] ([classes + 1][time_dim]; no atomics,
 * bit-reproducible); rows no image used are written as 0.  Adam on the table is bla_adam_f32 with grad_scale = 1 / batch. */
BLA_API bla_status bla_class_embedding_grad_f32(void* stream, const float* d_dtemb, const int* d_rows, int batch, int classes, int time_dim, float* d_gtable);
/* The guided ancestral step: eps~ = eps_u + guidance (eps_c - eps_u), then exactly bla_diffusion_step_f32's update of d_x [batch][image_floats] with the
 * same z stream (seed, (t + 1) << 32).  guidance 0 = the unguided step on eps_u (bit for bit), 1 = the conditional model alone, > 1 = guidance (Ho &
 * Salimans' w is guidance - 1).  d_x_copy (may be NULL) receives the new x as well: the null-class half of a batch-2n model input.  d_temb_next (may be
 * NULL) [2 batch][time_dim]: the embedding of t - 1 (nothing at t = 0) plus, where d_table is given, d_table[d_rows[b]] for its 2 batch rows (a row
 * outside [0, classes] adds nothing).  One launch. */
BLA_API bla_status bla_diffusion_guided_step_f32(const bla_diffusion* d, void* stream, float* d_x, float* d_x_copy, const float* d_eps_cond,
                                                 const float* d_eps_uncond, float guidance, int batch, size_t image_floats, int t, unsigned long long seed,
                                                 int time_dim, float* d_temb_next, const float* d_table, int classes, const int* d_rows);
/* Guided sampling on a model of batch 2n: images 0 .. n-1 carry their class rows, images n .. 2n-1 the null class on copies of the same x, so every step is
 * ONE batch-2n forward pass followed by bla_diffusion_guided_step_f32.  d_x [n][C][H][W]: in x_T, out x_0.  labels [n] as for bla_class_embedding_f32
 * (host labels checked, BLA_ERR_INVALID; a device label outside [0, classes] adds no class row).  An odd model batch is BLA_ERR_INVALID.  The model input,
 * embedding and row workspaces belong to the diffusion object and are allocated on first use: run once eagerly before capturing it into a graph. */
BLA_API bla_status bla_unet_sample_guided_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, const float* d_table, int classes,
                                              const int* labels, float guidance, unsigned long long seed);
/* The guided DDIM step: eps~ = eps_u + guidance (eps_c - eps_u) with bla_diffusion_guided_step_f32's single fmaf, then bla_diffusion_ddim_step_f32's
 * update from t to t_prev (the same kernel: guidance 0 = the unguided DDIM step on eps_u, bit for bit).  d_x_copy and d_temb_next [2 batch][time_dim]
 * (the embedding of t_prev plus the class rows; nothing at t_prev = -1) as for bla_diffusion_guided_step_f32.  One launch. */
BLA_API bla_status bla_diffusion_guided_ddim_step_f32(const bla_diffusion* d, void* stream, float* d_x, float* d_x_copy, const float* d_eps_cond,
                                                      const float* d_eps_uncond, float guidance, int batch, size_t image_floats, int t, int t_prev,
                                                      float eta, int clip, unsigned long long seed, int time_dim, float* d_temb_next,
                                                      const float* d_table, int classes, const int* d_rows);
/* Guided DDIM sampling: bla_unet_sample_guided_f32's loop (model batch 2n, labels, workspaces and their rules) over the DDIM timesteps of
 * sample_steps, one batch-2n forward pass and one bla_diffusion_guided_ddim_step_f32 per step. */
BLA_API bla_status bla_unet_sample_guided_ddim_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, const float* d_table, int classes,
                                                   const int* labels, float guidance, int sample_steps, float eta, int clip, unsigned long long seed);

/* ---- DPM-Solver++(2M) sampling (Lu, Zhou, Bao, Chen, Li, Zhu 2022) ----------------------------------------------------------------------------
 * Not in the reference.  The second-order multistep solver of the probability-flow ODE in the data-prediction form: one forward pass per step like
 * DDIM at eta = 0 (which is its first-order member), plus one buffer with the previous step's x0 prediction.  Deterministic: no noise, no seed.
 * With abar_t the doubles of bla_diffusion_schedule: alpha_t = sqrt(abar_t), sigma_t = sqrt(1 - abar_t), lambda_t = ln(alpha_t / sigma_t) =
 * ln(abar_t / (1 - abar_t)) / 2 (half the log-SNR, strictly decreasing in t); past the last step (t_prev = -1) alpha = 1 and sigma = 0.
 *
 * The timesteps of a run of S = sample_steps, increasing, out[S - 1] = steps - 1.  Host only.
 *   BLA_SPACING_TRAILING: exactly bla_diffusion_ddim_timesteps.
 *   BLA_SPACING_LOGSNR:   uniform in lambda, where the solver's error constants are smallest.  S = 1: {steps - 1}.  S >= 2: the grid
 *                         g_i = lambda_0 + (lambda_{T-1} - lambda_0) i / (S - 1), out[i] = the t whose lambda_t is nearest g_i (a tie takes the lower t),
 *                         then out[i] = max(out[i], out[i-1] + 1) for i = 1 .. S-1 and out[i] = min(out[i], T-1 - (S-1-i)) for i = S-1 .. 0: strictly
 *                         increasing, out[0] = 0, and S = steps gives every step.
 * S outside [1, steps] or any other spacing: BLA_ERR_INVALID. */
enum { BLA_SPACING_TRAILING = 0, BLA_SPACING_LOGSNR = 1 };
BLA_API bla_status bla_diffusion_sample_timesteps(const bla_diffusion* d, int sample_steps, int spacing, int* out);
/* The coefficients of the step from t to t_prev (-1: to the data) whose previous step came from t_last (-1: there was none), in double:
 * out = {inv_sab = 1 / alpha_t, s1m = sigma_t, c_x, c_d, w1, w0}.  With h = lambda_{t_prev} - lambda_t (> 0):
 *   t_prev >= 0:  c_x = sigma_p / sigma_t, c_d = -alpha_p expm1(-h);      t_prev = -1:  c_x = 0, c_d = 1 (the step returns the x0 prediction);
 *   t_last >= 0 and t_prev >= 0 (second order):  r = (lambda_t - lambda_{t_last}) / h, w1 = 1 + 1 / (2 r), w0 = -1 / (2 r);      otherwise w1 = 1, w0 = 0.
 * Differences of lambda are taken as one logarithm of one ratio of the schedule's doubles, not as a difference of two logarithms.
 * t outside [0, steps), t_prev outside [-1, t), t_last neither -1 nor inside (t, steps): BLA_ERR_INVALID.  Host only. */
BLA_API bla_status bla_diffusion_dpmpp_coefficients(const bla_diffusion* d, int t_last, int t, int t_prev, double out[6]);
/* One DPM-Solver++(2M) step in place, one launch.  Per element, with the six coefficients above rounded to fp32 once on the host and passed by value
 * (nothing is uploaded per step, so a captured sampler replays correctly) and every fused operation spelled out:
 *   x0   = fmaf(-s1m, eps_hat, x) * inv_sab, clamped to [-1, 1] when clip is non-zero;
 *   D    = fmaf(w0, hist, w1 * x0) in the second-order case, else x0;
 *   x    = fmaf(c_x, x, c_d * D);      hist = x0 (the clamped one), always written.
 * d_x0_hist [batch][image_floats] (never NULL) is the caller's: it is read only in the second-order case, so its contents before the first step of
 * a run (t_last = -1) do not matter; hand the same buffer to every step of a run.  The last step (t_prev = -1) is first order and leaves x equal to
 * the x0 prediction it stores.  With t_last = -1 and clip 0 the step is the DDIM step at eta = 0 in another arrangement (where the clamp acts the two differ: DDIM keeps eps_hat beside the clamped prediction, this solver's update sees eps only through it).  d_temb_next (may be NULL)
 * [batch][time_dim]: the embedding of t_prev (nothing at t_prev = -1).  16-byte loads and stores when d_x, d_eps_hat and d_x0_hist are 16-byte
 * aligned (a tail of batch * image_floats % 4 elements one by one), one element per lane otherwise.  Arguments refused as by
 * bla_diffusion_ddim_step_f32 and bla_diffusion_dpmpp_coefficients. */
BLA_API bla_status bla_diffusion_dpmpp_step_f32(const bla_diffusion* d, void* stream, float* d_x, const float* d_eps_hat, float* d_x0_hist, int batch,
                                                size_t image_floats, int t_last, int t, int t_prev, int clip, int time_dim, float* d_temb_next);
/* The guided step: eps~ = fmaf(guidance, eps_c - eps_u, eps_u) as in bla_diffusion_guided_ddim_step_f32, then the step above (the same kernel:
 * guidance 0 = the unguided step on eps_u, bit for bit).  d_x_copy (may be NULL) receives the new x, d_temb_next [2 batch][time_dim] the embedding of
 * t_prev plus the class rows (nothing at t_prev = -1), as for bla_diffusion_guided_step_f32.  d_x0_hist is [batch][image_floats].  One launch. */
BLA_API bla_status bla_diffusion_guided_dpmpp_step_f32(const bla_diffusion* d, void* stream, float* d_x, float* d_x_copy, const float* d_eps_cond,
                                                       const float* d_eps_uncond, float guidance, float* d_x0_hist, int batch, size_t image_floats,
                                                       int t_last, int t, int t_prev, int clip, int time_dim, float* d_temb_next, const float* d_table,
                                                       int classes, const int* d_rows);
/* DPM-Solver++(2M) sampling on the model's batch: bla_unet_sample_ddim_f32's loop over bla_diffusion_sample_timesteps(sample_steps, spacing) from
 * the last, bla_unet_forward_f32 (no dropout) then bla_diffusion_dpmpp_step_f32, t_last = -1 at the first step and the previous step's t afterwards.
 * d_x: in x_T, out x_0.  The history buffer [B][C][H][W] joins the diffusion object's workspaces (allocated on first use: run once eagerly before
 * capturing it into a graph); no host round trip inside the loop.  Bad sample_steps or spacing: BLA_ERR_INVALID. */
BLA_API bla_status bla_unet_sample_dpmpp_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, int sample_steps, int spacing, int clip);
/* Guided DPM-Solver++(2M) sampling: bla_unet_sample_guided_ddim_f32's loop (model batch 2n, labels, rows, workspaces and their rules) with the
 * timesteps, the guided step and the t_last bookkeeping above; the history buffer is [n][C][H][W]. */
BLA_API bla_status bla_unet_sample_guided_dpmpp_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, const float* d_table, int classes,
                                                    const int* labels, float guidance, int sample_steps, int spacing, int clip);

/* ---- held-out evaluation: the variational bound of Ho et al. 2020 (eq. 5) in nats per image ------------------------------------------------
 * Not in the reference.  With T = bla_diffusion_steps, beta_t / abar_t the doubles of bla_diffusion_schedule, alpha_t = 1 - beta_t, abar_{-1} = 1,
 * beta~_t = beta_t (1 - abar_{t-1}) / (1 - abar_t), F = image_floats and this project's fixed variance sigma_t^2 = beta_t:
 *   -ln p(x0) <= KL(q(x_{T-1} | x0) || N(0, I)) + sum_{t=1}^{T-1} KL(q(x_{t-1} | x_t, x0) || N(mu_theta, beta_t I)) + (-ln p(x0 | x_1 -> t = 0)),
 * every expectation estimated by ONE draw of x_t per image and timestep.  All arithmetic on image data below is in double on the fp32 inputs as they are,
 * with coefficients formed in double from the schedule (on the host and passed by value, or a double table made at create time): nothing is uploaded per
 * call, so the sequences can be captured into a graph.  examples/cifar_unet_gpu.c `eval` drives these and reports bits/dim = nats / (F ln 2).
 *
 * Noising at given timesteps: d_t [batch] on the device (NULL: every image at t_const), d_eps = bla_rand_normal_f32(batch * image_floats, 0, 1, seed,
 * offset), d_xt = sqrt(abar_t) x0 + sqrt(1 - abar_t) eps from the fp32 tables with bla_diffusion_noise_f32's rounding on either path (16-byte body when
 * image_floats % 4 == 0 and d_x0, d_eps, d_xt are 16-byte aligned), d_temb [batch][time_dim] the embedding of each image's t.  With d_t what
 * bla_diffusion_noise_f32(seed, pass) wrote and offset = pass << 32 all three are that call's, bit for bit.  t_const outside [0, T): BLA_ERR_INVALID; a
 * device entry outside [0, T) cannot be checked without a round trip: that image's d_xt and d_temb rows are written as zeros.  batch <= 4096. */
BLA_API bla_status bla_diffusion_noise_at_f32(const bla_diffusion* d, void* stream, const float* d_x0, int batch, size_t image_floats, int time_dim,
                                              const int* d_t /* [batch], may be NULL */, int t_const, unsigned long long seed, unsigned long long offset,
                                              float* d_eps, float* d_xt, float* d_temb);
/* One term of the bound per image, one launch: d_sqerr[b] (may be NULL) = sum_i (eps_i - eps_hat_i)^2 and
 *   t_b >= 1: d_terms[b] = KL(q(x_{t-1} | x_t, x0) || N(mu_theta, beta_t I)) = F c_t + w_t sqerr_b, c_t = (ln(beta_t / beta~_t) + beta~_t / beta_t - 1) / 2,
 *             w_t = beta_t / (2 alpha_t (1 - abar_t)): mu_theta is bla_diffusion_step_f32's mean and the posterior mean is the same expression with the true
 *             eps, so the means differ by beta_t / sqrt(alpha_t (1 - abar_t)) (eps - eps_hat) and only the squared error enters;
 *   t_b = 0:  d_terms[b] = -sum_i ln p_i, the discretised decoder of 8-bit data on [-1, 1] (Ho et al. 3.3): mu_i = (x_t,i - beta_0 / sqrt(1 - abar_0) eps_hat_i)
 *             / sqrt(alpha_0), sigma = sqrt(beta_0), z+- = (x0_i +- 1/255 - mu_i) / sigma, p_i = Phi(z+) where x0_i < -0.999, 1 - Phi(z-) where x0_i > 0.999,
 *             Phi(z+) - Phi(z-) otherwise, clamped below at 1e-12 (the floor of the published implementations).  Phi through erfc on the side where it is
 *             small; the interior difference between the two upper tails when z- > 0, else between the two lower ones.
 * d_t [batch] on the device (NULL: every image at t_const; t_const outside [0, T): BLA_ERR_INVALID); an image whose device-side t lies outside [0, T) gets
 * d_terms[b] = NaN and d_sqerr[b] = 0.  One workgroup per image, 16-byte loads when image_floats % 4 == 0 and the four inputs are 16-byte aligned, every
 * lane sums its elements in index order in double, the 256 partials go through LDS in a fixed tree: no atomics, bit-reproducible. */
BLA_API bla_status bla_diffusion_vlb_terms_f32(const bla_diffusion* d, void* stream, const float* d_x0, const float* d_xt, const float* d_eps,
                                               const float* d_eps_hat, const int* d_t /* [batch], may be NULL */, int t_const, int batch, size_t image_floats,
                                               double* d_terms /* [batch] */, double* d_sqerr /* [batch], may be NULL */);
/* d_kl[b] = KL(q(x_{T-1} | x0) || N(0, I)) = (abar_{T-1} sum_i x0_i^2 - F abar_{T-1} - F ln(1 - abar_{T-1})) / 2; the same reduction, one launch. */
BLA_API bla_status bla_diffusion_prior_kl_f32(const bla_diffusion* d, void* stream, const float* d_x0, int batch, size_t image_floats, double* d_kl /* [batch] */);
/* c_t and w_t above for 1 <= t < T (either pointer may be NULL); t = 0 or out of range: BLA_ERR_INVALID.  Host only. */
BLA_API bla_status bla_diffusion_vlb_weights(const bla_diffusion* d, int t, double* c_t, double* w_t);
/* The timesteps of an evaluation with K KL terms: out[0] = 0, out[1 + i] = 1 + floor((T - 1)(2 i + 1) / (2 K)) for i < K, the midpoints of K equal strata of
 * 1 .. T-1 (strictly increasing; K = T - 1 gives every step, K = 0 only the decoder's).  out holds K + 1 ints; 0 <= K <= T - 1, else BLA_ERR_INVALID.  Host
 * only.  The estimate of the bound is prior + terms(0) + (T - 1) / K sum_i terms(out[1 + i]).  It is exact (up to the one draw per term) only at K = T - 1:
 * the midpoint rule is biased at small K, because c_t and w_t fall steeply at small t and a stratum's midpoint under-weights its first steps. */
BLA_API bla_status bla_diffusion_eval_timesteps(const bla_diffusion* d, int K, int* out);
/* The evaluation loop on the model's batch B, d_x0 [B][C][H][W]: for each of the `count` timesteps t (a host array, each in [0, T), else BLA_ERR_INVALID
 * before anything runs) bla_diffusion_noise_at_f32 with t_const = t and offset offset_base + ((t + 1) << 32); where d_table is given, the class rows
 * d_table[d_rows[b]] added to the embedding (bla_class_embedding_f32 with p_uncond 0 on the device rows d_rows [B]: a row outside [0, classes] adds
 * nothing); bla_unet_forward_f32 without dropout; bla_diffusion_vlb_terms_f32 into d_terms [count][B] and d_sqerr [count][B] (may be NULL).  The values are
 * those of that composition, bit for bit; no host round trip inside the loop.  The eps, x_t and embedding workspaces belong to the diffusion object and are
 * allocated on first use: run once eagerly before capturing it into a graph. */
BLA_API bla_status bla_unet_evaluate_f32(bla_unet* m, const bla_diffusion* d, void* stream, const float* d_x0, const int* timesteps, int count,
                                         unsigned long long seed, unsigned long long offset_base, const float* d_table, int classes, const int* d_rows,
                                         double* d_terms, double* d_sqerr);

/* ---- training objectives: the schedule, what the network predicts, how a timestep's loss is weighted ---------------------------------------
 * Not in the reference.  Everything above is Ho et al. 2020: linear betas, the output read as eps_hat, every timestep at weight 1.  The entries below add
 * the cosine schedule (Nichol & Dhariwal 2021), v- and x0-prediction (Salimans & Ho 2022) and Min-SNR-gamma weighting (Hang et al. 2023).  A diffusion
 * object that none of them touched behaves exactly as before.
 *
 * The cosine betas, host only (no device needed): f(i) = cos^2(((i / steps) + s) / (1 + s) pi / 2), out[i] = min(1 - f(i + 1) / f(i), max_beta) for
 * i = 0 .. steps-1, in double.  The published values are s = 0.008 and max_beta = 0.999.  steps < 1, s < 0 or not finite, max_beta outside (0, 1):
 * BLA_ERR_INVALID. */
BLA_API bla_status bla_diffusion_cosine_betas(int steps, double s, double max_beta, double* out /* [steps] */);
/* A diffusion object over any betas: alpha_bar_t = prod_{s <= t} (1 - beta_s) in double, then the same fp32 tables and variational-bound weights through the
 * same code as bla_diffusion_create (whose betas, handed to this entry, give the same object bit for bit).  No kernel assumes a linear schedule: all read
 * the tables or the doubles of bla_diffusion_schedule.  A beta outside (0, 1) or NaN, steps outside [1, 2^24]: BLA_ERR_INVALID. */
BLA_API bla_status bla_diffusion_create_from_betas(bla_diffusion** out, int steps, const double* betas /* [steps], host */);
/* The objective the object carries.  `prediction` says what the network's output is, with a = sqrt(abar_t), c = sqrt(1 - abar_t):
 *   BLA_PREDICT_EPS  the noise eps (the default);     BLA_PREDICT_X0  the image x0;     BLA_PREDICT_V  v = a eps - c x0.
 * min_snr_gamma = 0: every timestep weighs 1.  gamma > 0: with SNR_t = abar_t / (1 - abar_t) and m = min(SNR_t, gamma) the weight of timestep t is
 *   EPS: m / SNR_t (1 where abar_t has underflown to 0, the limit);     X0: m;     V: m / (SNR_t + 1)
 * -- one weighting of the x0 error expressed in each parametrisation: the three weighted losses of one prediction are equal.  The table w [steps] is
 * formed in double on the host, rounded to fp32 once and uploaded: this entry may allocate and waits for the device, so it is not for use inside a
 * capture.  Every sampling loop and bla_unet_evaluate_f32 convert the output to eps_hat by bla_diffusion_to_eps_f32 right behind the forward pass when the
 * prediction is not EPS (with EPS nothing is launched: their bits are unchanged).  The step kernels always take eps_hat.  Going through eps_hat
 * amplifies the output's fp32 rounding by sqrt(abar_prev) / sqrt(abar_t) where the SNR is near zero.
 * A prediction other than the three, gamma negative, infinite or NaN: BLA_ERR_INVALID, nothing changed.  A fresh object: EPS, gamma 0. */
enum { BLA_PREDICT_EPS = 0, BLA_PREDICT_X0 = 1, BLA_PREDICT_V = 2 };
BLA_API bla_status bla_diffusion_set_objective(bla_diffusion* d, int prediction, double min_snr_gamma);
BLA_API bla_status bla_diffusion_objective(const bla_diffusion* d, int* prediction, double* min_snr_gamma);   /* either pointer may be NULL */
BLA_API bla_status bla_diffusion_loss_weight(const bla_diffusion* d, int t, double* w);   /* the host double of w_t; t outside [0, steps): BLA_ERR_INVALID */
/* The regression target of d's prediction type, one launch: d_target [batch][image_floats] = eps (EPS), x0 (X0: both bit-equal copies) or
 * fmaf(a, eps, -(c x0)) (V) with a, c the fp32 table values of each image's timestep, and d_weight [batch] (may be NULL) = the fp32 w of that timestep.
 * Timesteps as for bla_diffusion_noise_at_f32: d_t [batch] on the device, NULL = every image at t_const (outside [0, steps): BLA_ERR_INVALID); an image
 * whose device-side t lies outside [0, steps) gets a zero target and weight 0.  Only the inputs the type reads are looked at (d_x0 may be NULL for EPS,
 * d_eps for X0).  16-byte loads and stores when the pointers read and d_target are 16-byte aligned (a tail of batch * image_floats % 4 elements one by
 * one; image_floats need not be a multiple of 4), one element per lane otherwise. */
BLA_API bla_status bla_diffusion_target_f32(const bla_diffusion* d, void* stream, const float* d_x0, const float* d_eps, const int* d_t /* may be NULL */,
                                            int t_const, int batch, size_t image_floats, float* d_target, float* d_weight /* [batch], may be NULL */);
/* The model's output turned into eps_hat in place, given the x_t the model saw (d_x, not written; it must not overlap d_pred):
 *   V:  eps_hat = fmaf(a, v, c x);      X0:  eps_hat = fmaf(-a, x0_hat, x) / c, a correctly rounded division by the table's c (no reciprocal);
 *   EPS: BLA_OK without a launch.
 * Timesteps, alignment rule and arguments refused as for bla_diffusion_target_f32; an image whose device-side t lies outside [0, steps) is left as it is. */
BLA_API bla_status bla_diffusion_to_eps_f32(const bla_diffusion* d, void* stream, float* d_pred, const float* d_x, const int* d_t /* may be NULL */, int t_const,
                                            int batch, size_t image_floats);
/* The weighted squared error and its gradient, one launch, one workgroup per image (batch <= 2^31 - 1 workgroups):
 *   d_g [batch][image_floats] (may be NULL) = (2 w_b) (out - target) in fp32: 2 w_b is exact, the difference is rounded once and the product once.
 *   d_loss [batch] (may be NULL)           = w_b sum_i ((double)out_i - (double)target_i)^2, summed in double in a fixed order: bit-reproducible.
 * d_weight [batch] on the device, NULL = 1: then d_g is 2 (out - target), what bla_unet_backward_f32 seeds its pass with, bit for bit.  Hand d_g to
 * bla_unet_backward_from_f32.  16-byte accesses when image_floats % 4 == 0 and d_out, d_target, d_g are 16-byte aligned.  Both outputs NULL: nothing
 * is launched. */
BLA_API bla_status bla_diffusion_loss_f32(void* stream, const float* d_out, const float* d_target, const float* d_weight /* [batch], may be NULL */, int batch,
                                          size_t image_floats, float* d_g, double* d_loss);

/* ---- device-resident MNIST-NN trainer: the hot loop of model/mnist_nn.c:218-315 with everything in HBM -------
 * sizes = {n0, n1, n2, n3} (784, 256, 128, 10 in the reference, model/mnist_nn.c:25-28); samples are columns.
 * Parameters sit in one flat bucket ordered W1,b1,W2,b2,W3,b3 (each row-major), gradients in a second bucket of
 * the same layout (un-scaled sums over the batch columns).  Data parallelism = SUM-all-reduce the gradient
 * bucket between bla_mnist_nn_forward_backward and bla_mnist_nn_apply.
 * colsum_mode: BLA_COLSUM_AS_WRITTEN reproduces matrix_col_sum literally (needs n_i <= batch, else
 * BLA_ERR_UNDEFINED); BLA_COLSUM_INTENDED uses true row sums (required for sharded batches). */
typedef struct bla_mnist_nn bla_mnist_nn;
BLA_API bla_status bla_mnist_nn_create(bla_mnist_nn** out, const int* sizes /* [4] */, int batch);
BLA_API bla_status bla_mnist_nn_destroy(bla_mnist_nn* nn);
BLA_API size_t bla_mnist_nn_param_count(const bla_mnist_nn* nn);
BLA_API float* bla_mnist_nn_params(bla_mnist_nn* nn);     /* device pointer, param_count floats */
BLA_API float* bla_mnist_nn_grads(bla_mnist_nn* nn);      /* device pointer, param_count floats */
BLA_API float* bla_mnist_nn_input(bla_mnist_nn* nn);      /* resident raw-pixel buffer [n0][batch] (used when d_x_raw == NULL) */
BLA_API float* bla_mnist_nn_labels(bla_mnist_nn* nn);     /* resident one-hot buffer [n3][batch] (used when d_y == NULL) */
/* Adopt caller-owned buckets (e.g. tensors a collective library registered); current parameters are copied over. */
BLA_API bla_status bla_mnist_nn_use_buckets(bla_mnist_nn* nn, float* d_params, float* d_grads);
BLA_API bla_status bla_mnist_nn_set_params(bla_mnist_nn* nn, const float* h_flat);
BLA_API bla_status bla_mnist_nn_get_params(bla_mnist_nn* nn, float* h_flat);
BLA_API bla_status bla_mnist_nn_activation(bla_mnist_nn* nn, int which /* 0..8: z1,a1,z2,a2,z3,a3,dz3,dz2,dz1 */, float** d_ptr, int* rows);
BLA_API bla_status bla_mnist_nn_forward_backward(bla_mnist_nn* nn, void* stream, const float* d_x_raw, const float* d_y, int colsum_mode);
BLA_API bla_status bla_mnist_nn_apply(bla_mnist_nn* nn, void* stream, float lr /* reference: (float)-0.02 */);
BLA_API bla_status bla_mnist_nn_train_step(bla_mnist_nn* nn, void* stream, const float* d_x_raw, const float* d_y, float lr, int colsum_mode);
/* ---- the rest of the reference's training loop, device-resident (examples/mnist_nn_gpu.c drives these from C) ----
 * Batch construction, model/mnist_nn.c:204-217: with the whole dataset resident in HBM in the reference's feature-major layout
 * (lib/mnist_csv2.c: X[pixel * num_examples + example], labels y[example]) the host only sends the example indices its sampler drew;
 * x_raw[p][k] = X[p * num_examples + idx[k]], one-hot[label][k] = 1 land in the trainer's resident input / label buffers. */
BLA_API bla_status bla_mnist_nn_gather_batch(bla_mnist_nn* nn, void* stream, const float* d_X, const float* d_labels, int num_examples,
                                             const int* d_indices);
/* Forward pass only (model/mnist_nn.c:221-234; the whole of run(), :447-463): fills z1..a3 (and dz3, which run() ignores). */
BLA_API bla_status bla_mnist_nn_forward(bla_mnist_nn* nn, void* stream, const float* d_x_raw, const float* d_y);
/* Loss / accuracy bookkeeping (model/mnist_nn.c:237-257, run(): :476-490) inside the output layer's launch: once enabled every forward
 * pass adds its batch's cross-entropy (double) and its number of correct predictions to device-side accumulators -- no extra launch, no
 * host round trip per batch.  read: synchronises, returns the totals since the last reset (summed over the batch columns in order). */
BLA_API bla_status bla_mnist_nn_metrics_enable(bla_mnist_nn* nn, int on);
BLA_API bla_status bla_mnist_nn_metrics_read(bla_mnist_nn* nn, double* loss_sum, long long* num_correct, int reset);

/* One step with the update folded into the weight-gradient products (see graph_step below), issued directly on the stream: six launches
 * from one host call, no gradient bucket.  Falls back to bla_mnist_nn_train_step where the fused form does not apply. */
BLA_API bla_status bla_mnist_nn_fused_step(bla_mnist_nn* nn, void* stream, const float* d_x_raw, const float* d_y, float lr, int colsum_mode);
/* Same step from the resident buffers, captured once into a hipGraph and replayed (launch-bound otherwise).  with_update = 1 and
 * BLA_COLSUM_INTENDED on the reference's layer sizes takes the fused form: the update rides inside the weight-gradient products
 * (W += lr * dZ.A^T, b += lr * rowsum(dZ)), six launches, and the gradient bucket is NOT written; with_update = 0 always fills it. */
BLA_API bla_status bla_mnist_nn_graph_step(bla_mnist_nn* nn, void* stream, float lr, int colsum_mode, int with_update);

/* ---- data-parallel exchange (the one exchange step of the MNIST-NN path) ------------------------
 * The reference has no multi-device code; this is what a data-parallel driver of model/mnist_nn.c needs between
 * backward (:260-293) and the update (:296-315): SUM of the flat gradient bucket over the ranks (the reference's
 * gradient is a sum over batch columns, so no rescale).  One process per GPU; each rank owns two gradient buckets
 * (used alternately) in fine-grained memory that the peers map through IPC and read directly over xGMI; the sum is
 * taken in rank order on every rank (bit-identical results) and the update is fused.  See csrc/bla_dp.hip. */
typedef struct bla_dp bla_dp;
#define BLA_DP_HANDLE_BYTES 256
BLA_API bla_status bla_dp_create(bla_dp** out, int rank, int world, size_t count /* floats per bucket */);
BLA_API bla_status bla_dp_destroy(bla_dp* dp);
/* BLA_DP_HANDLE_BYTES opaque bytes for the other ranks (exchange them with any host-side channel: MPI, torch.distributed, a file,
 * or a plain array when all ranks live in one process) */
BLA_API bla_status bla_dp_export(bla_dp* dp, void* handle);
/* handles: world x BLA_DP_HANDLE_BYTES, slot r = rank r's export (own slot ignored); call once, after every rank has exported.
 * Ranks in other processes are mapped through IPC, ranks of the calling process (other contexts) are addressed directly. */
BLA_API bla_status bla_dp_connect(bla_dp* dp, const void* handles);
BLA_API float* bla_dp_bucket(bla_dp* dp, int parity);   /* device pointer of this rank's bucket 0 / 1 */
BLA_API size_t bla_dp_count(const bla_dp* dp);
/* sum_i = SUM_r bucket_r[parity][i] (r ascending); d_out[i] = sum_i if d_out; d_target[i] += alpha * sum_i if d_target.
 * Collective and asynchronous on `stream`; successive calls alternate the parity; capturable into a hipGraph. */
BLA_API bla_status bla_dp_allreduce_f32(bla_dp* dp, void* stream, int parity, float* d_out, float* d_target, float alpha);
/* *status = 0 healthy, 1 = some earlier exchange gave up waiting for a peer (4 s) and skipped its sums; synchronises */
BLA_API bla_status bla_dp_status(bla_dp* dp, int* status);
/* the same as a return code: BLA_ERR_TIMEOUT when some earlier exchange gave up waiting (BLA_DP_TIMEOUT_MS, default 4000) -- that exchange delivered
 * NOTHING (out / target keep what they held; never zeros in place of sums); the exchange object is then out of step with its peers: destroy it */
BLA_API bla_status bla_dp_check(bla_dp* dp);
/* workgroups of the two-shot exchange kernel this device holds at once (occupancy x CUs, asked of the runtime at create): its grid is capped at a
 * quarter of that (at most 128), so that the phase that waits for workgroups of the same launch is always fully resident */
BLA_API int bla_dp_resident_blocks(const bla_dp* dp);
/* forward + backward + exchange + update of one data-parallel step as one graph launch (BLA_COLSUM_INTENDED only) */
BLA_API bla_status bla_mnist_nn_dp_step(bla_mnist_nn* nn, bla_dp* dp, void* stream, float lr, int colsum_mode);
/* the same step issued directly on the stream (seven launches from one host call); may be mixed with the graph form */
BLA_API bla_status bla_mnist_nn_dp_step_direct(bla_mnist_nn* nn, bla_dp* dp, void* stream, float lr, int colsum_mode);

/* ---- the same exchange through the library collective: RCCL ncclAllReduce(ncclFloat, ncclSum) over xGMI (north_star) ----
 * librccl is opened on first use, not linked: bla_dp_rccl_available() says whether it could be (a single-GPU box needs none).
 * One process (or one host thread) per rank: rank 0 makes the 128-byte unique id, the host program hands it to the other ranks over any
 * channel, every rank calls bla_dp_rccl_init on its current context's device -- ncclCommInitRank is COLLECTIVE and BLOCKS until all ranks
 * have called it, so a single host thread must not call it rank after rank.
 * ONE host thread driving all ranks of a process: bla_dp_rccl_init_all (ncclCommInitAll, distinct devices), then per step every rank's
 * bla_dp_rccl_allreduce_f32 between bla_dp_rccl_group_begin / _end.
 * Not executed with world > 1 anywhere yet: the build pool has one-GPU boxes and RCCL refuses duplicate devices (tests: world 1). */
typedef struct bla_rccl bla_rccl;
#define BLA_RCCL_ID_BYTES 128
BLA_API int bla_dp_rccl_available(void);
BLA_API bla_status bla_dp_rccl_unique_id(void* id128);
BLA_API bla_status bla_dp_rccl_init(bla_rccl** out, const void* id128, int rank, int world);   /* ncclCommInitRank; collective, blocking */
BLA_API bla_status bla_dp_rccl_init_all(bla_rccl** out, const int* devices, int world);        /* ncclCommInitAll: out[world] from one thread */
BLA_API bla_status bla_dp_rccl_group_begin(void);                                               /* ncclGroupStart */
BLA_API bla_status bla_dp_rccl_group_end(void);                                                 /* ncclGroupEnd */
BLA_API bla_status bla_dp_rccl_destroy(bla_rccl* c);
BLA_API bla_status bla_dp_rccl_allreduce_f32(bla_rccl* c, void* stream, float* d_buf, size_t count);   /* in place, SUM, async on stream */
/* forward + backward into the trainer's gradient bucket, ncclAllReduce of the bucket, params += lr * sum (model/mnist_nn.c:218-315 sharded) */
BLA_API bla_status bla_mnist_nn_dp_step_rccl(bla_mnist_nn* nn, bla_rccl* c, void* stream, float lr, int colsum_mode);

#ifdef __cplusplus
}
#endif
#endif /* BLA_H */
