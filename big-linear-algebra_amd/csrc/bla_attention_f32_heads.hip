// bla_attention_f32_heads.hip -- fp32 multi-head self-attention for SHORT sequences (S <= 64, d <= 64, heads d <= 256): the fp32 batched
// block's arithmetic per head, with the materialised softmax.  What does not depend on the heads -- Q / K / V = Z W* at width D = heads d, out, del_W, del_P,
// del_Wq/k/v and del_X -- goes through the calls the fp32 block makes (bla_gemm_batched_f32, batch_sum, the three-part thin launch) with d := D.  What does
// runs in two fused kernels, one workgroup per (image, head):
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

bla_status bgemm(void* s, int ta, int tb, int m, int n, int k, const float* A, int lda, long sa, const float* B, int ldb, long sb, float* C, int ldc, long sc, int batch,
                 float beta = 0.f, const float* bias_row = nullptr) {
	bla_gemm_epilogue ep = {};
	ep.alpha = 1.f; ep.beta = beta; ep.bias_row = bias_row;
	return bla_gemm_batched_f32(s, ta, tb, m, n, k, A, lda, sa, B, ldb, sb, C, ldc, sc, batch, &ep, 0);
}

}  // namespace
}  // namespace bla

using namespace bla;

extern "C" {

int bla_attention_f32_heads_applies(int c, int s, int heads, int d) {
	return s >= 1 && s <= 64 && d >= 1 && d <= 64 && heads >= 1 && heads <= 256 / d && c > 0;   // heads d <= 256
}

bla_status bla_attention_forward_batched_f32_heads(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, const float* d_w,
                                                   const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int heads, int d) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(batch > 0 && batch <= 65535 && bla_attention_f32_heads_applies(c, s, heads, d), BLA_ERR_INVALID,
	            "fp32 multi-head attention: B=%d C=%d S=%d heads=%d d=%d (S in 1..64, d in 1..64, heads d <= 256)", batch, c, s, heads, d);
	BLA_REQUIRE(d_x && d_wq && d_wk && d_wv && d_w && d_bias && d_out && ws && ws->q && ws->k && ws->v && ws->weights && ws->attention && (heads > 1 || ws->scores_raw),
	            BLA_ERR_INVALID, "null operand");
	if (heads == 1) return bla_attention_forward_batched_f32(stream, batch, d_x, d_wq, d_wk, d_wv, d_w, d_bias, ws, d_out, c, s, d);
	const int D = heads * d;
	const long xs = (long)c * s, qs = (long)s * D;
	const size_t lds = fwd_lds_floats(s, d) * sizeof(float);
	if ((st = allow_lds((const void*)att_f32_heads_fwd_kernel, lds))) return st;
	if ((st = bgemm(stream, 1, 0, s, D, c, d_x, s, xs, d_wq, D, 0, ws->q, D, qs, batch))) return st;   // Q = Z Wq, Z = X^T, all heads side by side
	if ((st = bgemm(stream, 1, 0, s, D, c, d_x, s, xs, d_wk, D, 0, ws->k, D, qs, batch))) return st;
	if ((st = bgemm(stream, 1, 0, s, D, c, d_x, s, xs, d_wv, D, 0, ws->v, D, qs, batch))) return st;
	hipLaunchKernelGGL(att_f32_heads_fwd_kernel, dim3(heads, batch), dim3(kThreads), lds, pick_stream(stream), ws->q, ws->k, ws->v,
	                   ws->weights, ws->attention, s, d, D, (float)(1.0 / sqrt((double)d)));
	BLA_HIP(hipGetLastError());
	return bgemm(stream, 1, 1, c, s, D, d_w, c, 0, ws->attention, D, qs, d_out, s, xs, batch, 0.f, d_bias);   // out = (A W + bias)^T over all D columns
}

bla_status bla_attention_backward_batched_f32_heads(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                    const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad, float* d_partials,
                                                    float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x, int c, int s, int heads, int d) {
	bla_status st = require_ready();
	if (st) return st;
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
	const long xs = (long)c * s, qs = (long)s * D, ws_ = (long)c * D;
	float *del_q = grad->q, *del_k = grad->k, *del_v = grad->v, *del_p = grad->attention;
	const size_t lds = bwd_lds_floats(s, d) * sizeof(float);
	if ((st = allow_lds((const void*)att_f32_heads_bwd_kernel, lds))) return st;
	if ((st = bgemm(stream, 1, 1, D, c, s, fwd->attention, D, qs, d_del_y, s, xs, d_partials, c, ws_, batch))) return st;   // del_W = sum_b A^T del_Y'
	if ((st = batch_sum(stream, d_partials, d_del_w, batch, (size_t)ws_))) return st;
	if ((st = bgemm(stream, 1, 1, s, D, c, d_del_y, s, xs, d_w, c, 0, del_p, D, qs, batch))) return st;                    // del_P = del_Y' W^T: head h from W's rows of head h
	hipLaunchKernelGGL(att_f32_heads_bwd_kernel, dim3(heads, batch), dim3(kThreads), lds, pick_stream(stream), fwd->q, fwd->k, fwd->v,
	                   fwd->weights, del_p, del_q, del_k, del_v, s, d, D, (float)(1.0 / sqrt((double)d)));
	BLA_HIP(hipGetLastError());
	if ((st = bgemm(stream, 0, 0, c, D, s, d_x, s, xs, del_k, D, qs, d_partials, D, ws_, batch))) return st;               // Z^T = X
	if ((st = batch_sum(stream, d_partials, d_del_wk, batch, (size_t)ws_))) return st;
	if ((st = bgemm(stream, 0, 0, c, D, s, d_x, s, xs, del_q, D, qs, d_partials, D, ws_, batch))) return st;
	if ((st = batch_sum(stream, d_partials, d_del_wq, batch, (size_t)ws_))) return st;
	if ((st = bgemm(stream, 0, 0, c, D, s, d_x, s, xs, del_v, D, qs, d_partials, D, ws_, batch))) return st;
	if ((st = batch_sum(stream, d_partials, d_del_wv, batch, (size_t)ws_))) return st;
	if (gemm_thin_applies(c, s, D, batch)) {   // the three D-deep terms of del_Z^T in one launch (q, then k, then v), as in the fp32 block
		const ThinPart parts[3] = {{d_wq, del_q, 0, qs, D, D}, {d_wk, del_k, 0, qs, D, D}, {d_wv, del_v, 0, qs, D, D}};
		st = gemm_thin_parts(stream, 0, 1, c, s, D, parts, 3, d_del_x, s, xs, batch, 1.f, 0.f, nullptr, nullptr, 0, 0);
		if (st == BLA_OK) {
			char name[64];
			snprintf(name, sizeof(name), "gemm_f32_thin_nt_x%d_parts3", batch);
			gemm_note_last_kernel(name);
		}
		return st;
	}
	if ((st = bgemm(stream, 0, 1, c, s, D, d_wq, D, 0, del_q, D, qs, d_del_x, s, xs, batch))) return st;
	if ((st = bgemm(stream, 0, 1, c, s, D, d_wk, D, 0, del_k, D, qs, d_del_x, s, xs, batch, 1.f))) return st;
	return bgemm(stream, 0, 1, c, s, D, d_wv, D, 0, del_v, D, qs, d_del_x, s, xs, batch, 1.f);
}

}  // extern "C"
