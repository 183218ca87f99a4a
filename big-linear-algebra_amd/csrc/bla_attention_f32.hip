// bla_attention_f32.hip -- the fp32 self-attention block (model/cifar_unet.c:999-1022 / :1261-1337) in its three forms: one image
// (paired GEMM launches; what batch == 1 delegates to), a batch with one head, and a batch with several heads for SHORT sequences (S <= 64, d <= 64,
// heads d <= 256).  The two batched forms share every stage that does not depend on the heads, stated once at a row width D = heads d: project_qkv, project_out,
// grad_out_weight_and_del_p, grad_qkv_weights_and_del_x.  Between them the one-head form runs batched GEMMs and the row softmax at S x S; the multi-head form
// runs the same arithmetic per head, with the materialised softmax, in two fused kernels, one workgroup per (image, head):
//   forward core:   the head's Q, K, V slices into LDS;  T = inv Q K^T;  row softmax, the maximum subtracted;  P stored once;  A = P V.
//   backward core:  the head's Q, K, V, P, del_P into LDS;  del_S = del_P V^T;  dot = <P, del_S> per row;  del_I = inv P o (del_S - dot);
//                   del_V = P^T del_P;  del_Q = del_I K;  del_K = del_I^T Q.  del_S and del_I live in LDS only.
// Every sum is one thread's loop over its index in ascending order (plain fp32 FMAs; the row dot in double, rounded once, as the fp32 block's Jacobian kernel
// has it): no atomics, no cross-lane reduction, the same bits on every run, and a workgroup reads nothing of another image.  S and d are run-time values: all
// loads and stores are single floats inside the head's own rows and columns, so no address outside an operand is ever formed (DESIGN 3.27's rule).
// LDS rows are padded to an odd number of floats: a wave's lanes read a row-major tile either along a row (consecutive banks) or down a column (stride odd:
// 64 different banks), never 2-way.  At S = d = 64 the forward core takes 65 KB and the backward core 98 KB of the CU's 160 KB: one workgroup a CU, which is what
// these launch-bound shapes (a few thousand to a few million FLOPs) can use anyway; a launch above 64 KB raises the kernel's dynamic LDS limit first.
#include "bla_internal.h"
#include <cmath>

namespace bla {
namespace {

constexpr int kThreads = 256;
__host__ __device__ constexpr int odd(int n) { return n | 1; }   // an LDS row stride with no power of two in it

// floats of dynamic LDS
size_t fwd_lds_floats(int s, int d) { return (size_t)3 * s * odd(d) + (size_t)s * odd(s) + 2 * (size_t)s; }
size_t bwd_lds_floats(int s, int d) { return (size_t)4 * s * odd(d) + (size_t)2 * s * odd(s) + (size_t)s; }

// the head's d columns of a [B][S][D] tensor, image b, as a [S][dp] tile
__device__ __forceinline__ void load_slice(float* __restrict__ dst, const float* __restrict__ src, int s, int d, int dp, int ld) {
	for (int e = threadIdx.x; e < s * d; e += kThreads) {
		const int r = e / d, cc = e - r * d;
		dst[r * dp + cc] = src[(size_t)r * ld + cc];
	}
}
// out[i][j] = sum_cc a[i][cc] b[j][cc], cc ascending: a, b [S][dp] tiles, out [S][sp]
__device__ __forceinline__ void rows_times_rows(float* __restrict__ out, const float* __restrict__ a, const float* __restrict__ b, int s, int d, int dp, int sp, float alpha) {
	for (int e = threadIdx.x; e < s * s; e += kThreads) {
		const int i = e / s, j = e - i * s;
		const float *ai = a + i * dp, *bj = b + j * dp;
		float acc = 0.f;
		for (int cc = 0; cc < d; ++cc) acc = fmaf(ai[cc], bj[cc], acc);
		out[i * sp + j] = acc * alpha;
	}
}
// dst[i][cc] (global, the head's columns) = sum_j p[i][j] m[j][cc], j ascending: p [S][sp], m [S][dp]
__device__ __forceinline__ void square_times_tile(float* __restrict__ dst, const float* __restrict__ p, const float* __restrict__ m, int s, int d, int dp, int sp, int ld) {
	for (int e = threadIdx.x; e < s * d; e += kThreads) {
		const int i = e / d, cc = e - i * d;
		float acc = 0.f;
		for (int j = 0; j < s; ++j) acc = fmaf(p[i * sp + j], m[j * dp + cc], acc);
		dst[(size_t)i * ld + cc] = acc;
	}
}
// dst[j][cc] (global, the head's columns) = sum_i p[i][j] m[i][cc], i ascending
__device__ __forceinline__ void square_t_times_tile(float* __restrict__ dst, const float* __restrict__ p, const float* __restrict__ m, int s, int d, int dp, int sp, int ld) {
	for (int e = threadIdx.x; e < s * d; e += kThreads) {
		const int j = e / d, cc = e - j * d;
		float acc = 0.f;
		for (int i = 0; i < s; ++i) acc = fmaf(p[i * sp + j], m[i * dp + cc], acc);
		dst[(size_t)j * ld + cc] = acc;
	}
}

// grid (heads, batch).  q, k, v, attention [B][S][D]; weights [B][heads][S][S]
__global__ void __launch_bounds__(kThreads) att_f32_heads_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                     float* __restrict__ weights, float* __restrict__ attention, int s, int d, int ld, float inv) {
	extern __shared__ float lds[];
	const int dp = odd(d), sp = odd(s), h = blockIdx.x, b = blockIdx.y;
	float *Q = lds, *K = Q + s * dp, *V = K + s * dp, *P = V + s * dp, *rmax = P + s * sp, *rsum = rmax + s;
	const size_t img = (size_t)b * s * ld + (size_t)h * d;
	load_slice(Q, q + img, s, d, dp, ld);
	load_slice(K, k + img, s, d, dp, ld);
	load_slice(V, v + img, s, d, dp, ld);
	__syncthreads();
	rows_times_rows(P, Q, K, s, d, dp, sp, inv);   // T = inv (Q K^T)
	__syncthreads();
	for (int i = threadIdx.x; i < s; i += kThreads) {
		float m = P[i * sp];
		for (int j = 1; j < s; ++j) m = fmaxf(m, P[i * sp + j]);
		rmax[i] = m;
	}
	__syncthreads();
	for (int e = threadIdx.x; e < s * s; e += kThreads) {
		const int i = e / s, j = e - i * s;
		P[i * sp + j] = expf(P[i * sp + j] - rmax[i]);
	}
	__syncthreads();
	for (int i = threadIdx.x; i < s; i += kThreads) {
		float sum = 0.f;
		for (int j = 0; j < s; ++j) sum += P[i * sp + j];
		rsum[i] = sum;
	}
	__syncthreads();
	float* wout = weights + ((size_t)b * gridDim.x + h) * s * s;
	for (int e = threadIdx.x; e < s * s; e += kThreads) {
		const int i = e / s, j = e - i * s;
		const float p = P[i * sp + j] / rsum[i];
		P[i * sp + j] = p;
		wout[e] = p;
	}
	__syncthreads();
	square_times_tile(attention + img, P, V, s, d, dp, sp, ld);   // A = P V
}

// grid (heads, batch).  q, k, v, dp_ (= del_P), gq, gk, gv [B][S][D]; weights [B][heads][S][S]
__global__ void __launch_bounds__(kThreads) att_f32_heads_bwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                     const float* __restrict__ weights, const float* __restrict__ dp_, float* __restrict__ gq,
                                                                     float* __restrict__ gk, float* __restrict__ gv, int s, int d, int ld, float inv) {
	extern __shared__ float lds[];
	const int dp = odd(d), sp = odd(s), h = blockIdx.x, b = blockIdx.y;
	float *Q = lds, *K = Q + s * dp, *V = K + s * dp, *G = V + s * dp, *P = G + s * dp, *I = P + s * sp, *dots = I + s * sp;
	const size_t img = (size_t)b * s * ld + (size_t)h * d;
	load_slice(Q, q + img, s, d, dp, ld);
	load_slice(K, k + img, s, d, dp, ld);
	load_slice(V, v + img, s, d, dp, ld);
	load_slice(G, dp_ + img, s, d, dp, ld);
	const float* win = weights + ((size_t)b * gridDim.x + h) * s * s;
	for (int e = threadIdx.x; e < s * s; e += kThreads) {
		const int i = e / s, j = e - i * s;
		P[i * sp + j] = win[e];
	}
	__syncthreads();
	rows_times_rows(I, G, V, s, d, dp, sp, 1.f);   // del_S = del_P V^T
	__syncthreads();
	for (int i = threadIdx.x; i < s; i += kThreads) {
		double dot = 0;
		for (int j = 0; j < s; ++j) dot += (double)P[i * sp + j] * I[i * sp + j];
		dots[i] = (float)dot;
	}
	__syncthreads();
	for (int e = threadIdx.x; e < s * s; e += kThreads) {
		const int i = e / s, j = e - i * s;
		I[i * sp + j] = (P[i * sp + j] * (I[i * sp + j] - dots[i])) * inv;   // del_I
	}
	__syncthreads();
	square_t_times_tile(gv + img, P, G, s, d, dp, sp, ld);   // del_V = P^T del_P
	square_times_tile(gq + img, I, K, s, d, dp, sp, ld);     // del_Q = del_I K
	square_t_times_tile(gk + img, I, Q, s, d, dp, sp, ld);   // del_K = del_I^T Q
}

// a launch that asks for more than 64 KB of dynamic LDS has to be allowed it first (per device: asked whenever such a launch is about to be made)
bla_status allow_lds(const void* kern, size_t bytes) {
	if (bytes > 64 * 1024) BLA_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
	return BLA_OK;
}

bla_status ep_gemm(void* s, int ta, int tb, int m, int n, int k, const float* A, int lda, const float* B, int ldb, float* C, int ldc, float alpha, float beta,
                   const float* bias_row) {
	bla_gemm_epilogue ep = {};
	ep.alpha = alpha; ep.beta = beta; ep.bias_row = bias_row;
	return bla_gemm_f32(s, ta, tb, m, n, k, A, lda, B, ldb, C, ldc, &ep);
}

// two independent products in one launch where both are latency-bound shapes (bla_gemm_pair_f32); plain alpha/beta epilogues
bla_status pair_gemm(void* s, int ta1, int tb1, int m1, int n1, int k1, const float* A1, int lda1, const float* B1, int ldb1, float* C1, int ldc1,
                     int ta2, int tb2, int m2, int n2, int k2, const float* A2, int lda2, const float* B2, int ldb2, float* C2, int ldc2, float alpha2 = 1.f) {
	bla_gemm_epilogue e1 = {}, e2 = {};
	e1.alpha = 1.f; e2.alpha = alpha2;
	bla_gemm_desc p = {ta1, tb1, m1, n1, k1, A1, lda1, B1, ldb1, C1, ldc1, &e1};
	bla_gemm_desc q = {ta2, tb2, m2, n2, k2, A2, lda2, B2, ldb2, C2, ldc2, &e2};
	return bla_gemm_pair_f32(s, &p, &q);
}

// one per-image product as one launch over the batch (strides in floats per image, 0: shared by the images)
bla_status bgemm(void* s, int ta, int tb, int m, int n, int k, const float* A, int lda, long sa, const float* B, int ldb, long sb, float* C, int ldc, long sc, int batch,
                 float alpha = 1.f, float beta = 0.f, const float* bias_row = nullptr, float* pre = nullptr, int ld_pre = 0, long spre = 0) {
	bla_gemm_epilogue ep = {};
	ep.alpha = alpha; ep.beta = beta; ep.bias_row = bias_row; ep.pre_act = pre; ep.ld_pre = ld_pre;
	return bla_gemm_batched_f32(s, ta, tb, m, n, k, A, lda, sa, B, ldb, sb, C, ldc, sc, batch, &ep, spre);
}

}  // namespace

// ---- the stages the batched forms share (declared in bla_internal.h: bla_attention_online_f32.hip runs them too), at a row width D (one head: d; several: heads d, the heads side by side) -----------------------------------------
// x / out / del_y / del_x [B][C][S]; q, k, v, attention, their gradients [B][S][D]; wq / wk / wv [C][D]; w [D][C]; partials: [B][C*D] scratch, summed in image order
bla_status project_qkv(void* stream, int batch, const float* x, const float* wq, const float* wk, const float* wv, const bla_attention_ws* ws, int c, int s, int D) {
	const long xs = (long)c * s, qs = (long)s * D;
	bla_status st;
	if ((st = bgemm(stream, 1, 0, s, D, c, x, s, xs, wq, D, 0, ws->q, D, qs, batch))) return st;   // Q = Z Wq, Z = X^T   :1003-1004
	if ((st = bgemm(stream, 1, 0, s, D, c, x, s, xs, wk, D, 0, ws->k, D, qs, batch))) return st;
	return bgemm(stream, 1, 0, s, D, c, x, s, xs, wv, D, 0, ws->v, D, qs, batch);
}
bla_status project_out(void* stream, int batch, const float* w, const float* bias, const float* attention, float* out, int c, int s, int D) {
	return bgemm(stream, 1, 1, c, s, D, w, c, 0, attention, D, (long)s * D, out, s, (long)c * s, batch, 1.f, 0.f, bias);   // out = (A W + bias)^T   :1019-1021
}
bla_status grad_out_weight_and_del_p(void* stream, int batch, const float* del_y, const float* w, const float* attention, float* partials, float* del_w, float* del_p,
                                     int c, int s, int D) {
	const long xs = (long)c * s, qs = (long)s * D, ws_ = (long)c * D;
	bla_status st;
	if ((st = bgemm(stream, 1, 1, D, c, s, attention, D, qs, del_y, s, xs, partials, c, ws_, batch))) return st;   // del_W = sum_b A^T del_Y'   :1291-1293
	if ((st = batch_sum(stream, partials, del_w, batch, (size_t)ws_))) return st;
	return bgemm(stream, 1, 1, s, D, c, del_y, s, xs, w, c, 0, del_p, D, qs, batch);   // del_P = del_Y' W^T: head h from W's rows of head h   :1295-1297
}
bla_status grad_qkv_weights_and_del_x(void* stream, int batch, const float* x, const float* wq, const float* wk, const float* wv, const float* del_q, const float* del_k,
                                      const float* del_v, float* partials, float* del_wq, float* del_wk, float* del_wv, float* del_x, int c, int s, int D) {
	const long xs = (long)c * s, qs = (long)s * D, ws_ = (long)c * D;
	bla_status st;
	auto weight_grad = [&](const float* del, float* del_wt) -> bla_status {   // sum_b Z_b^T del_b, Z^T = X   :1316-1319
		bla_status s2 = bgemm(stream, 0, 0, c, D, s, x, s, xs, del, D, qs, partials, D, ws_, batch);
		return s2 ? s2 : batch_sum(stream, partials, del_wt, batch, (size_t)ws_);
	};
	if ((st = weight_grad(del_k, del_wk)) || (st = weight_grad(del_q, del_wq)) || (st = weight_grad(del_v, del_wv))) return st;
	if (gemm_thin_applies(c, s, D, batch)) {   // the three D-deep terms of del_Z^T accumulate in registers (q, then k, then v) and are stored once   :1322-1334
		const ThinPart parts[3] = {{wq, del_q, 0, qs, D, D}, {wk, del_k, 0, qs, D, D}, {wv, del_v, 0, qs, D, D}};
		if ((st = gemm_thin_parts(stream, 0, 1, c, s, D, parts, 3, del_x, s, xs, batch, 1.f, 0.f, nullptr, nullptr, 0, 0))) return st;
		char name[64];   // (gemm_thin_parts is below bla_gemm_batched_f32, which names its own launches: without this bla_gemm_last_kernel() still showed del_Wv's product)
		snprintf(name, sizeof(name), "gemm_f32_thin_nt_x%d_parts3", batch);
		gemm_note_last_kernel(name);
		return BLA_OK;
	}
	if ((st = bgemm(stream, 0, 1, c, s, D, wq, D, 0, del_q, D, qs, del_x, s, xs, batch))) return st;   // del_Z^T, same add order   :1322-1334
	if ((st = bgemm(stream, 0, 1, c, s, D, wk, D, 0, del_k, D, qs, del_x, s, xs, batch, 1.f, 1.f))) return st;
	return bgemm(stream, 0, 1, c, s, D, wv, D, 0, del_v, D, qs, del_x, s, xs, batch, 1.f, 1.f);
}

}  // namespace bla

using namespace bla;

extern "C" {

/* ---- single image, intended composition ---------------------------------------------------------------------------------
 * x, out, del_y, del_x: [C][S] (S = H*W); wq/wk/wv: [C][d]; w: [d][C]; bias: [C].  Every matrix_transpose the reference
 * materialises (9 of them) and both channel reshapes disappear into the GEMM's transa/transb: the [S][C] "input" matrix
 * is X^T, so Z.Wq is a TN product on X itself, and output = dense^T comes straight out of a TT product. */
bla_status bla_attention_forward_f32(void* stream, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, const float* d_w,
                                     const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int d) {
	BLA_ENTER();
	BLA_REQUIRE(c > 0 && s > 0 && d > 0, BLA_ERR_INVALID, "bad attention shape C=%d S=%d d=%d", c, s, d);
	BLA_REQUIRE(d_x && d_wq && d_wk && d_wv && d_w && d_bias && d_out && ws && ws->q && ws->k && ws->v && ws->scores_raw && ws->weights && ws->attention,
	            BLA_ERR_INVALID, "null operand");
	const float inv = (float)(1.0 / sqrt((double)d));                                                  // :1010
	st = pair_gemm(stream, 1, 0, s, d, c, d_x, s, d_wq, d, ws->q, d,                                       // Q = Z Wq, Z = X^T   :1003-1004
	               1, 0, s, d, c, d_x, s, d_wk, d, ws->k, d); if (st) return st;                          // beside K = Z Wk (one launch)
	st = ep_gemm(stream, 1, 0, s, d, c, d_x, s, d_wv, d, ws->v, d, 1.f, 0.f, nullptr); if (st) return st;
	{   // (Q K^T) / sqrt(d) :1007-1014, stored twice by the product itself: scores_raw (kept) and weights (softmaxed in place, :1015)
		bla_gemm_epilogue ep = {};
		ep.alpha = inv; ep.pre_act = ws->scores_raw; ep.ld_pre = s;
		st = bla_gemm_f32(stream, 0, 1, s, s, d, ws->q, d, ws->k, d, ws->weights, s, &ep); if (st) return st;
	}
	st = bla_softmax_rows_f32(stream, ws->weights, s, s); if (st) return st;                               // :1015
	st = ep_gemm(stream, 0, 0, s, d, s, ws->weights, s, ws->v, d, ws->attention, d, 1.f, 0.f, nullptr); if (st) return st;   // :1018
	return ep_gemm(stream, 1, 1, c, s, d, d_w, c, ws->attention, d, d_out, s, 1.f, 0.f, d_bias);              // (P W + b)^T   :1019-1021
}

bla_status bla_attention_backward_f32(void* stream, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv,
                                      const float* d_w, const bla_attention_ws* fw, const bla_attention_ws* g, float* d_del_wq, float* d_del_wk,
                                      float* d_del_wv, float* d_del_w, float* d_del_x, int c, int s, int d, int jacobian_from_raw) {
	BLA_ENTER();
	BLA_REQUIRE(c > 0 && s > 0 && d > 0, BLA_ERR_INVALID, "bad attention shape C=%d S=%d d=%d", c, s, d);
	BLA_REQUIRE(d_del_y && d_x && d_wq && d_wk && d_wv && d_w && fw && g && d_del_wq && d_del_wk && d_del_wv && d_del_w && d_del_x, BLA_ERR_INVALID, "null operand");
	BLA_REQUIRE(g->q && g->k && g->v && g->scores_raw && g->weights && g->attention, BLA_ERR_INVALID, "null gradient workspace");
	const float inv = (float)(1.0 / sqrt((double)d));
	float *del_q = g->q, *del_k = g->k, *del_v = g->v, *del_i = g->scores_raw, *del_s = g->weights, *del_p = g->attention;
	// independent products share a launch (the reference runs all fourteen one after the other)
	st = pair_gemm(stream, 1, 1, d, c, s, fw->attention, d, d_del_y, s, d_del_w, c,                                          // del_W = P^T del_Y'     :1291-1293
	               1, 1, s, d, c, d_del_y, s, d_w, c, del_p, d); if (st) return st;                                         // del_P = del_Y' W^T     :1295-1297
	st = pair_gemm(stream, 0, 1, s, s, d, del_p, d, fw->v, d, del_s, s,                                                     // del_S = del_P V^T      :1303-1305
	               1, 0, s, d, s, fw->weights, s, del_p, d, del_v, d); if (st) return st;                                   // del_V = S^T del_P      :1299-1301
	st = bla_softmax_ddx_f32(stream, jacobian_from_raw ? fw->scores_raw : fw->weights, del_s, del_i, s, s); if (st) return st;   // :1307
	st = bla_scale_f32(stream, del_i, (size_t)s * s, inv); if (st) return st;                                                // :1308
	st = pair_gemm(stream, 0, 0, s, d, s, del_i, s, fw->k, d, del_q, d,                                                     // :1310
	               1, 0, s, d, s, del_i, s, fw->q, d, del_k, d); if (st) return st;                                         // :1312-1314
	st = pair_gemm(stream, 0, 0, c, d, s, d_x, s, del_k, d, d_del_wk, d,                                                    // Z^T = X              :1316-1319
	               0, 0, c, d, s, d_x, s, del_q, d, d_del_wq, d); if (st) return st;
	st = pair_gemm(stream, 0, 0, c, d, s, d_x, s, del_v, d, d_del_wv, d,
	               0, 1, c, s, d, d_wq, d, del_q, d, d_del_x, s); if (st) return st;                                        // del_Z^T, same add order :1322-1334
	st = ep_gemm(stream, 0, 1, c, s, d, d_wk, d, del_k, d, d_del_x, s, 1.f, 1.f, nullptr); if (st) return st;
	return ep_gemm(stream, 0, 1, c, s, d, d_wv, d, del_v, d, d_del_x, s, 1.f, 1.f, nullptr);
}

/* ---- a batch of images, one head: x / out [B][C][S], every workspace buffer B times the single-image size.  Each per-image product becomes one launch
 * over the batch (bla_gemm_batched_f32); the shared stages above around the scores, the row softmax and its Jacobian at S x S. */
bla_status bla_attention_forward_batched_f32(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, const float* d_w,
                                             const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int d) {
	if (batch == 1) return bla_attention_forward_f32(stream, d_x, d_wq, d_wk, d_wv, d_w, d_bias, ws, d_out, c, s, d);
	BLA_ENTER();
	BLA_REQUIRE(batch > 0 && c > 0 && s > 0 && d > 0, BLA_ERR_INVALID, "bad attention shape B=%d C=%d S=%d d=%d", batch, c, s, d);
	BLA_REQUIRE(d_x && d_wq && d_wk && d_wv && d_w && d_bias && d_out && ws && ws->q && ws->k && ws->v && ws->scores_raw && ws->weights && ws->attention,
	            BLA_ERR_INVALID, "null operand");
	const float inv = (float)(1.0 / sqrt((double)d));
	const long qs = (long)s * d, ss = (long)s * s;
	if ((st = project_qkv(stream, batch, d_x, d_wq, d_wk, d_wv, ws, c, s, d))) return st;
	if ((st = bgemm(stream, 0, 1, s, s, d, ws->q, d, qs, ws->k, d, qs, ws->weights, s, ss, batch, inv, 0.f, nullptr, ws->scores_raw, s, ss))) return st;   // :1007-1014
	if ((st = bla_softmax_rows_f32(stream, ws->weights, batch * s, s))) return st;                                          // :1015
	if ((st = bgemm(stream, 0, 0, s, d, s, ws->weights, s, ss, ws->v, d, qs, ws->attention, d, qs, batch))) return st;        // :1018
	return project_out(stream, batch, d_w, d_bias, ws->attention, d_out, c, s, d);
}

bla_status bla_attention_backward_batched_f32(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                              const float* d_wv, const float* d_w, const bla_attention_ws* fw, const bla_attention_ws* g, float* d_partials,
                                              float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x, int c, int s, int d,
                                              int jacobian_from_raw) {
	if (batch == 1)
		return bla_attention_backward_f32(stream, d_del_y, d_x, d_wq, d_wk, d_wv, d_w, fw, g, d_del_wq, d_del_wk, d_del_wv, d_del_w, d_del_x, c, s, d, jacobian_from_raw);
	BLA_ENTER();
	BLA_REQUIRE(batch > 0 && c > 0 && s > 0 && d > 0, BLA_ERR_INVALID, "bad attention shape B=%d C=%d S=%d d=%d", batch, c, s, d);
	BLA_REQUIRE(d_del_y && d_x && d_wq && d_wk && d_wv && d_w && fw && g && d_partials && d_del_wq && d_del_wk && d_del_wv && d_del_w && d_del_x, BLA_ERR_INVALID, "null operand");
	BLA_REQUIRE(g->q && g->k && g->v && g->scores_raw && g->weights && g->attention, BLA_ERR_INVALID, "null gradient workspace");
	const float inv = (float)(1.0 / sqrt((double)d));
	const long qs = (long)s * d, ss = (long)s * s;
	float *del_q = g->q, *del_k = g->k, *del_v = g->v, *del_i = g->scores_raw, *del_s = g->weights, *del_p = g->attention;
	if ((st = grad_out_weight_and_del_p(stream, batch, d_del_y, d_w, fw->attention, d_partials, d_del_w, del_p, c, s, d))) return st;
	if ((st = bgemm(stream, 0, 1, s, s, d, del_p, d, qs, fw->v, d, qs, del_s, s, ss, batch))) return st;                      // del_S = del_P V^T        :1303-1305
	if ((st = bgemm(stream, 1, 0, s, d, s, fw->weights, s, ss, del_p, d, qs, del_v, d, qs, batch))) return st;                // del_V = S^T del_P        :1299-1301
	if ((st = softmax_ddx_launch(stream, jacobian_from_raw ? fw->scores_raw : fw->weights, del_s, del_i, batch * s, s, inv))) return st;   // :1307-1308 in one pass
	if ((st = bgemm(stream, 0, 0, s, d, s, del_i, s, ss, fw->k, d, qs, del_q, d, qs, batch))) return st;                      // :1310
	if ((st = bgemm(stream, 1, 0, s, d, s, del_i, s, ss, fw->q, d, qs, del_k, d, qs, batch))) return st;                      // :1312-1314
	return grad_qkv_weights_and_del_x(stream, batch, d_x, d_wq, d_wk, d_wv, del_q, del_k, del_v, d_partials, d_del_wq, d_del_wk, d_del_wv, d_del_x, c, s, d);
}

/* ---- a batch of images, several heads of width d side by side: the shared stages at D = heads d around the two fused kernels */
int bla_attention_f32_heads_applies(int c, int s, int heads, int d) {
	return s >= 1 && s <= 64 && d >= 1 && d <= 64 && heads >= 1 && heads <= 256 / d && c > 0;   // heads d <= 256
}

bla_status bla_attention_forward_batched_f32_heads(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, const float* d_w,
                                                   const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int heads, int d) {
	BLA_ENTER();
	BLA_REQUIRE(batch > 0 && batch <= 65535 && bla_attention_f32_heads_applies(c, s, heads, d), BLA_ERR_INVALID,
	            "fp32 multi-head attention: B=%d C=%d S=%d heads=%d d=%d (S in 1..64, d in 1..64, heads d <= 256)", batch, c, s, heads, d);
	BLA_REQUIRE(d_x && d_wq && d_wk && d_wv && d_w && d_bias && d_out && ws && ws->q && ws->k && ws->v && ws->weights && ws->attention && (heads > 1 || ws->scores_raw),
	            BLA_ERR_INVALID, "null operand");
	if (heads == 1) return bla_attention_forward_batched_f32(stream, batch, d_x, d_wq, d_wk, d_wv, d_w, d_bias, ws, d_out, c, s, d);
	const int D = heads * d;
	const size_t lds = fwd_lds_floats(s, d) * sizeof(float);
	if ((st = allow_lds((const void*)att_f32_heads_fwd_kernel, lds))) return st;
	if ((st = project_qkv(stream, batch, d_x, d_wq, d_wk, d_wv, ws, c, s, D))) return st;
	hipLaunchKernelGGL(att_f32_heads_fwd_kernel, dim3(heads, batch), dim3(kThreads), lds, pick_stream(stream), ws->q, ws->k, ws->v,
	                   ws->weights, ws->attention, s, d, D, (float)(1.0 / sqrt((double)d)));
	BLA_HIP(hipGetLastError());
	return project_out(stream, batch, d_w, d_bias, ws->attention, d_out, c, s, D);
}

bla_status bla_attention_backward_batched_f32_heads(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                    const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad, float* d_partials,
                                                    float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x, int c, int s, int heads, int d) {
	BLA_ENTER();
	BLA_REQUIRE(batch > 0 && batch <= 65535 && bla_attention_f32_heads_applies(c, s, heads, d), BLA_ERR_INVALID,
	            "fp32 multi-head attention: B=%d C=%d S=%d heads=%d d=%d (S in 1..64, d in 1..64, heads d <= 256)", batch, c, s, heads, d);
	BLA_REQUIRE(d_del_y && d_x && d_wq && d_wk && d_wv && d_w && fwd && grad && d_partials && d_del_wq && d_del_wk && d_del_wv && d_del_w && d_del_x, BLA_ERR_INVALID,
	            "null operand");
	BLA_REQUIRE(fwd->q && fwd->k && fwd->v && fwd->weights && fwd->attention && grad->q && grad->k && grad->v && grad->attention &&
	            (heads > 1 || (fwd->scores_raw && grad->scores_raw && grad->weights)), BLA_ERR_INVALID, "null workspace");
	if (heads == 1)
		return bla_attention_backward_batched_f32(stream, batch, d_del_y, d_x, d_wq, d_wk, d_wv, d_w, fwd, grad, d_partials, d_del_wq, d_del_wk, d_del_wv, d_del_w, d_del_x, c,
		                                          s, d, 0);
	const int D = heads * d;
	float *del_q = grad->q, *del_k = grad->k, *del_v = grad->v, *del_p = grad->attention;
	const size_t lds = bwd_lds_floats(s, d) * sizeof(float);
	if ((st = allow_lds((const void*)att_f32_heads_bwd_kernel, lds))) return st;
	if ((st = grad_out_weight_and_del_p(stream, batch, d_del_y, d_w, fwd->attention, d_partials, d_del_w, del_p, c, s, D))) return st;
	hipLaunchKernelGGL(att_f32_heads_bwd_kernel, dim3(heads, batch), dim3(kThreads), lds, pick_stream(stream), fwd->q, fwd->k, fwd->v,
	                   fwd->weights, del_p, del_q, del_k, del_v, s, d, D, (float)(1.0 / sqrt((double)d)));
	BLA_HIP(hipGetLastError());
	return grad_qkv_weights_and_del_x(stream, batch, d_x, d_wq, d_wk, d_wv, del_q, del_k, del_v, d_partials, d_del_wq, d_del_wk, d_del_wv, d_del_x, c, s, D);
}

}  // extern "C"
