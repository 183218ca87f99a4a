// bla_attention_online_f32.hip -- the fp32 self-attention block with the softmax ONLINE over blocks of 32 keys: bla_attention_online_bf16.hip's
// recurrence (3.29) and head layout (3.30) with NOTHING rounded to bf16 -- every product of the per-head core runs on v_mfma_f32_32x32x2_f32 -- for any S up to
// 4096, any head width d up to 64 and any C: no S x S tensor exists in memory in either direction, and nothing beyond float alignment is asked of a tensor.
// The stages that do not depend on the softmax are bla_attention_f32.hip's at the row width D = heads d (project_qkv, project_out, grad_out_weight_and_del_p,
// grad_qkv_weights_and_del_x); the four kernels here are the per-head core, gridDim.z the head, a row stride ld = D beside the head width d:
//   forward core: a wave owns 32 queries and walks the key blocks in ascending order with the running maximum m, the running sum l and ceil(d / 32) tiles of
//                 Acc^T.  The score tile is formed transposed (K . Q^T), so a lane holds ONE query: m, l and the rescale are per-lane scalars.
//   preamble:     dot = <del_P, A> over the head's d columns, one thread a row, dd ascending (a dot product a row: there is no matrix product in it).
//   dq:           a wave per 32 queries walks the key blocks, del_Q^T tiles in registers, the forward's score tile instruction for instruction.
//   dkv:          a wave per 32 keys walks the query blocks, del_K^T and del_V^T tiles in registers; a lane holds one KEY.
// The fp32 MFMA takes ONE float per lane per operand: lane 32 h + f gives A[row f][k = h] and B[k = h][col f], accumulator register r of that lane is
// D[row (r & 3) + 8 (r >> 2) + 4 h][col f].  Two consequences carry the whole file:
//   * a contraction over d is 8 ND steps (ND = ceil(d / 16), the template parameter), step i multiplying dd = 8 ND h + i: a lane reads 8 ND CONSECUTIVE floats
//     of its row, from any float offset;
//   * register r of a score tile IS the B operand of a step whose k = h stands for tile row (r & 3) + 8 (r >> 2) + 4 h (bla_attention_tile.h's trick, one float
//     wide): the other operand is read at that same row, 16 steps a tile, and no accumulator is ever transposed.
// Edges without branches (DESIGN 3.27's rule): a row at or beyond S is read from a block of zeros (the address is chosen, the load unconditional); a column at
// or beyond d is read at the row's LAST column and replaced by zero; a key at or beyond S counts as p = 0.  Only stores are guarded.  No LDS, no barrier, no
// atomics, no scratch; every sum has one order, so a run and its repeat give the same bits and a workgroup reads nothing of another image.
#include "bla_attention_tile.h"
#include <cmath>

namespace bla {
namespace {

constexpr int kWaves = 4;   // independent waves a workgroup: one 32-row block each
#define BLA_MFMA_F32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

static __device__ float f32_zeros[64];   // (zero-initialised, never written: what a row outside its operand is read from; 64 = the widest fragment's last offset + 1)

// the lane's 8 ND floats of a head's row for a contraction over d: v[i] = row[8 ND h + i], zero at and beyond d and for a row outside the operand
template <int ND>
struct RowFrag {
	float v[8 * ND];
	__device__ __forceinline__ void load(const float* row, bool row_ok, int d, int fh) {
		const float* p = row_ok ? row : f32_zeros;
		const int last = row_ok ? d - 1 : 63;
#pragma unroll
		for (int i = 0; i < 8 * ND; ++i) {
			const int dd = 8 * ND * fh + i;
			const float x = p[dd < last ? dd : last];
			v[i] = dd < d ? x : 0.f;
		}
	}
};
// one float of a column fragment: tensor[row][dd] of the head, zero outside
__device__ __forceinline__ float ld_or_zero(const float* p, bool ok) { return *(ok ? p : f32_zeros); }

// the 32 x 32 tile sum over dd of a[row f][dd] b[col f][dd]
template <int ND>
__device__ __forceinline__ f32x16 rows_dot_rows(const RowFrag<ND>& a, const RowFrag<ND>& b) {
	f32x16 t = zero16();
#pragma unroll
	for (int i = 0; i < 8 * ND; ++i) t = BLA_MFMA_F32(a.v[i], b.v[i], t);
	return t;
}
// a score tile: the products scaled by inv with a rounding of its own (never contracted into what follows), so that all three walking kernels see the same bits
template <int ND>
__device__ __forceinline__ f32x16 score_tile(const RowFrag<ND>& a, const RowFrag<ND>& b, float inv) {
	f32x16 t = rows_dot_rows<ND>(a, b);
#pragma unroll
	for (int r = 0; r < 16; ++r) t[r] = __fmul_rn(t[r], inv);
	return t;
}
// acc[dt] (rows dd = 32 dt + tile row, column = the lane's row) += sum over the 32 rows of a block of m[block row][32 dt + f] t[block row][lane's column]:
// register r of t as the B operand, m read at the same permuted block row
template <int DT>
__device__ __forceinline__ void tile_t_times_cols(f32x16 (&acc)[DT], const float* m, const f32x16& t, int row0, int s, int d, int ld, int fr, int fh) {
#pragma unroll
	for (int r = 0; r < 16; ++r) {
		const int row = row0 + acc_row(r, fh);
#pragma unroll
		for (int dt = 0; dt < DT; ++dt) acc[dt] = BLA_MFMA_F32(ld_or_zero(m + (size_t)row * ld + 32 * dt + fr, row < s && 32 * dt + fr < d), t[r], acc[dt]);
	}
}
// the same for two products that share the block rows (dkv)
template <int DT>
__device__ __forceinline__ void tile_t_times_cols2(f32x16 (&acc1)[DT], const float* m1, const f32x16& t1, f32x16 (&acc2)[DT], const float* m2, const f32x16& t2, int row0,
                                                   int s, int d, int ld, int fr, int fh) {
#pragma unroll
	for (int r = 0; r < 16; ++r) {
		const int row = row0 + acc_row(r, fh);
#pragma unroll
		for (int dt = 0; dt < DT; ++dt) {
			const bool ok = row < s && 32 * dt + fr < d;
			const size_t at = (size_t)row * ld + 32 * dt + fr;
			acc1[dt] = BLA_MFMA_F32(ld_or_zero(m1 + at, ok), t1[r], acc1[dt]);
			acc2[dt] = BLA_MFMA_F32(ld_or_zero(m2 + at, ok), t2[r], acc2[dt]);
		}
	}
}
// rows dd (registers), column = the lane's row of a [S][ld] tensor; single floats: the head's slice starts at any float
template <int DT>
__device__ __forceinline__ void store_tiles_t(float* row, bool row_ok, const f32x16 (&a)[DT], int d, int fh) {
#pragma unroll
	for (int dt = 0; dt < DT; ++dt)
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			const int dd = 32 * dt + acc_row(r, fh);
			if (row_ok && dd < d) row[dd] = a[dt][r];
		}
}

// ---- forward core: grid (ceil(ceil(S / 32) / kWaves), batch, heads) -------------------------------------------------------------------------------------------
template <int ND>
__global__ void __launch_bounds__(64 * kWaves) att_online_f32_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                          float* __restrict__ lse, float* __restrict__ attention, int s, int d, int ld, float inv) {
	constexpr int DT = (ND + 1) / 2;
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int rb = blockIdx.x * kWaves + wave, b = blockIdx.y, nk = (s + 31) >> 5;
	if (rb >= nk) return;
	const size_t img = (size_t)b * s * ld + (size_t)blockIdx.z * d, vec = ((size_t)b * gridDim.z + blockIdx.z) * s;
	const float *qb = q + img, *kb = k + img, *vb = v + img;
	const int query = rb * 32 + fr;
	const bool qok = query < s;   // (a query row at or beyond S: zeros in, nothing stored)

	RowFrag<ND> qf, kf;
	qf.load(qb + (size_t)query * ld, qok, d, fh);
	float m = -INFINITY, l = 0.f;
	f32x16 at[DT];   // Acc^T[dd][query]
#pragma unroll
	for (int dt = 0; dt < DT; ++dt) at[dt] = zero16();
	for (int t = 0; t < nk; ++t) {
		const int key = t * 32 + fr;
		kf.load(kb + (size_t)key * ld, key < s, d, fh);
		f32x16 sc = score_tile<ND>(kf, qf, inv);   // T^T[key][query]
		float mx = m;
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			sc[r] = t * 32 + acc_row(r, fh) < s ? sc[r] : -INFINITY;   // (every block holds a real key: mx is finite)
			mx = fmaxf(mx, sc[r]);
		}
		mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
		const float a = expf(m - mx);   // the first block: exp(-inf) = 0 against l = 0 and Acc = 0
		float sum = 0.f;
#pragma unroll
		for (int r = 0; r < 16; ++r) { sc[r] = expf(sc[r] - mx); sum += sc[r]; }
		sum += __shfl_xor(sum, 32, 64);
		l = l * a + sum;
		m = mx;
#pragma unroll
		for (int dt = 0; dt < DT; ++dt)
#pragma unroll
			for (int r = 0; r < 16; ++r) at[dt][r] *= a;
		tile_t_times_cols<DT>(at, vb, sc, t * 32, s, d, ld, fr, fh);   // Acc^T[dd][query] += sum over the block's keys of V[key][dd] p[query][key]
	}
	if (fh == 0 && qok) lse[vec + query] = m + logf(l);
#pragma unroll
	for (int dt = 0; dt < DT; ++dt)
#pragma unroll
		for (int r = 0; r < 16; ++r) at[dt][r] /= l;
	store_tiles_t<DT>(attention + img + (size_t)query * ld, qok, at, d, fh);
}

// ---- backward preamble: dot = <del_P, A> over the head's columns.  grid (ceil(S / 256), batch, heads) ---------------------------------------------------------
__global__ void __launch_bounds__(256) att_online_f32_dots_kernel(const float* __restrict__ dp, const float* __restrict__ attention, float* __restrict__ dots, int s, int d,
                                                                   int ld) {
	const int query = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
	if (query >= s) return;
	const size_t row = ((size_t)b * s + query) * ld + (size_t)blockIdx.z * d;
	float dot = 0.f;
	for (int dd = 0; dd < d; ++dd) dot = fmaf(dp[row + dd], attention[row + dd], dot);
	dots[((size_t)b * gridDim.z + blockIdx.z) * s + query] = dot;
}

// ---- backward dq: del_Q of 32 queries over all key blocks -----------------------------------------------------------------------------------------------------
// Everything transposed, as in the forward core: T^T, del_S^T = V . del_P^T and del_I^T tiles with the query on the lane; del_I^T's registers are the B operands
// of del_Q^T = K^T . del_I^T.
template <int ND>
__global__ void __launch_bounds__(64 * kWaves) att_online_f32_dq_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                         const float* __restrict__ dp, const float* __restrict__ lse, const float* __restrict__ dots,
                                                                         float* __restrict__ gq, int s, int d, int ld, float inv) {
	constexpr int DT = (ND + 1) / 2;
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int rb = blockIdx.x * kWaves + wave, b = blockIdx.y, nk = (s + 31) >> 5;
	if (rb >= nk) return;
	const size_t img = (size_t)b * s * ld + (size_t)blockIdx.z * d, vec = ((size_t)b * gridDim.z + blockIdx.z) * s;
	const float *qb = q + img, *kb = k + img, *vb = v + img, *dpb = dp + img;
	const int query = rb * 32 + fr;
	const bool qok = query < s;
	RowFrag<ND> qf, pf, kf, vf;
	qf.load(qb + (size_t)query * ld, qok, d, fh);
	pf.load(dpb + (size_t)query * ld, qok, d, fh);
	const float L = ld_or_zero(lse + vec + query, qok), dot = ld_or_zero(dots + vec + query, qok);
	f32x16 dQ[DT];
#pragma unroll
	for (int dt = 0; dt < DT; ++dt) dQ[dt] = zero16();
	for (int t = 0; t < nk; ++t) {
		const int key = t * 32 + fr;
		kf.load(kb + (size_t)key * ld, key < s, d, fh);
		vf.load(vb + (size_t)key * ld, key < s, d, fh);
		const f32x16 sc = score_tile<ND>(kf, qf, inv);
		f32x16 dI = rows_dot_rows<ND>(vf, pf);   // del_S^T[key][query] first
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			const float p = t * 32 + acc_row(r, fh) < s ? expf(sc[r] - L) : 0.f;
			dI[r] = (p * (dI[r] - dot)) * inv;
		}
		tile_t_times_cols<DT>(dQ, kb, dI, t * 32, s, d, ld, fr, fh);   // del_Q^T[dd][query] += sum over the block's keys of K[key][dd] del_I[query][key]
	}
	store_tiles_t<DT>(gq + img + (size_t)query * ld, qok, dQ, d, fh);
}

// ---- backward dkv: del_K and del_V of 32 keys over all query blocks -------------------------------------------------------------------------------------------
// A lane holds one KEY (column f), the registers the queries: T = Q . K^T is the forward's tile with the operands' roles exchanged (the same products in the
// same order of dd), del_S = del_P . V^T.  P's and del_I's registers are the B operands of del_V^T = del_P^T . P and del_K^T = Q^T . del_I.  A query row at or
// beyond S has P = 0 and del_I = 0: it enters no sum.
template <int ND>
__global__ void __launch_bounds__(64 * kWaves) att_online_f32_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                          const float* __restrict__ dp, const float* __restrict__ lse, const float* __restrict__ dots,
                                                                          float* __restrict__ gk, float* __restrict__ gv, int s, int d, int ld, float inv) {
	constexpr int DT = (ND + 1) / 2;
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int kt = blockIdx.x * kWaves + wave, b = blockIdx.y, nk = (s + 31) >> 5;
	if (kt >= nk) return;
	const size_t img = (size_t)b * s * ld + (size_t)blockIdx.z * d, vec = ((size_t)b * gridDim.z + blockIdx.z) * s;
	const float *qb = q + img, *kb = k + img, *vb = v + img, *dpb = dp + img, *lb = lse + vec, *db = dots + vec;
	const int key = kt * 32 + fr;
	const bool kok = key < s;
	RowFrag<ND> kf, vf, rows;
	kf.load(kb + (size_t)key * ld, kok, d, fh);
	vf.load(vb + (size_t)key * ld, kok, d, fh);
	f32x16 dK[DT], dV[DT];
#pragma unroll
	for (int dt = 0; dt < DT; ++dt) { dK[dt] = zero16(); dV[dt] = zero16(); }
	for (int t = 0; t < nk; ++t) {
		const int query = t * 32 + fr;
		rows.load(qb + (size_t)query * ld, query < s, d, fh);
		f32x16 P = score_tile<ND>(rows, kf, inv);   // T[query][key]
		rows.load(dpb + (size_t)query * ld, query < s, d, fh);
		f32x16 dI = rows_dot_rows<ND>(rows, vf);    // del_S[query][key]
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			const int row = t * 32 + acc_row(r, fh);
			const bool ok = row < s;
			const float Lr = ld_or_zero(lb + row, ok), Dr = ld_or_zero(db + row, ok);
			P[r] = ok ? expf(P[r] - Lr) : 0.f;
			dI[r] = (P[r] * (dI[r] - Dr)) * inv;
		}
		tile_t_times_cols2<DT>(dV, dpb, P, dK, qb, dI, t * 32, s, d, ld, fr, fh);
	}
	store_tiles_t<DT>(gv + img + (size_t)key * ld, kok, dV, d, fh);
	store_tiles_t<DT>(gk + img + (size_t)key * ld, kok, dK, d, fh);
}

}  // namespace
}  // namespace bla

using namespace bla;

// ND = ceil(d / 16)
#define BLA_ATT_ONLINE_F32_BY_ND(KERNEL, ...)                                                   \
	switch ((d + 15) / 16) {                                                                    \
	case 1: hipLaunchKernelGGL((KERNEL<1>), grid, block, 0, hs, __VA_ARGS__); break;              \
	case 2: hipLaunchKernelGGL((KERNEL<2>), grid, block, 0, hs, __VA_ARGS__); break;              \
	case 3: hipLaunchKernelGGL((KERNEL<3>), grid, block, 0, hs, __VA_ARGS__); break;              \
	default: hipLaunchKernelGGL((KERNEL<4>), grid, block, 0, hs, __VA_ARGS__); break;             \
	}
#define BLA_ATT_ONLINE_F32_SHAPE(batch, c, s, heads, d)                                                                                            \
	BLA_REQUIRE(batch > 0 && batch <= 65535 && bla_attention_online_f32_applies(c, s, heads, d), BLA_ERR_INVALID,                                  \
	            "online fp32 attention: B=%d C=%d S=%d heads=%d d=%d (S in 1..4096, d in 1..64, heads d <= 256)", batch, c, s, heads, d)

extern "C" {

int bla_attention_online_f32_applies(int c, int s, int heads, int d) {
	return s >= 1 && s <= 4096 && d >= 1 && d <= 64 && heads >= 1 && heads <= 256 / d && c > 0;   // heads d <= 256
}

bla_status bla_attention_forward_batched_online_f32(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, const float* d_w,
                                                    const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int heads, int d) {
	BLA_ENTER();
	BLA_ATT_ONLINE_F32_SHAPE(batch, c, s, heads, d);
	BLA_REQUIRE(d_x && d_wq && d_wk && d_wv && d_w && d_bias && d_out && ws && ws->q && ws->k && ws->v && ws->scores_raw && ws->attention, BLA_ERR_INVALID, "null operand");
	const int D = heads * d;
	hipStream_t hs = pick_stream(stream);
	if ((st = project_qkv(stream, batch, d_x, d_wq, d_wk, d_wv, ws, c, s, D))) return st;
	const dim3 grid(((s + 31) / 32 + kWaves - 1) / kWaves, batch, heads), block(64 * kWaves);
	BLA_ATT_ONLINE_F32_BY_ND(att_online_f32_fwd_kernel, ws->q, ws->k, ws->v, ws->scores_raw, ws->attention, s, d, D, (float)(1.0 / sqrt((double)d)))
	BLA_HIP(hipGetLastError());
	return project_out(stream, batch, d_w, d_bias, ws->attention, d_out, c, s, D);
}

bla_status bla_attention_backward_batched_online_f32(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                     const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad, float* d_partials,
                                                     float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x, int c, int s, int heads, int d) {
	BLA_ENTER();
	BLA_ATT_ONLINE_F32_SHAPE(batch, c, s, heads, d);
	BLA_REQUIRE(d_del_y && d_x && d_wq && d_wk && d_wv && d_w && fwd && grad && d_partials && d_del_wq && d_del_wk && d_del_wv && d_del_w && d_del_x, BLA_ERR_INVALID,
	            "null operand");
	BLA_REQUIRE(fwd->q && fwd->k && fwd->v && fwd->scores_raw && fwd->attention && grad->q && grad->k && grad->v && grad->attention && grad->scores_raw, BLA_ERR_INVALID,
	            "null workspace");
	const int D = heads * d;
	const float inv = (float)(1.0 / sqrt((double)d));
	hipStream_t hs = pick_stream(stream);
	float *del_q = grad->q, *del_k = grad->k, *del_v = grad->v, *del_p = grad->attention, *dots = grad->scores_raw;
	if ((st = grad_out_weight_and_del_p(stream, batch, d_del_y, d_w, fwd->attention, d_partials, d_del_w, del_p, c, s, D))) return st;
	hipLaunchKernelGGL(att_online_f32_dots_kernel, dim3((s + 255) / 256, batch, heads), dim3(256), 0, hs, del_p, fwd->attention, dots, s, d, D);
	BLA_HIP(hipGetLastError());
	const dim3 grid(((s + 31) / 32 + kWaves - 1) / kWaves, batch, heads), block(64 * kWaves);
	BLA_ATT_ONLINE_F32_BY_ND(att_online_f32_dkv_kernel, fwd->q, fwd->k, fwd->v, del_p, fwd->scores_raw, dots, del_k, del_v, s, d, D, inv)
	BLA_HIP(hipGetLastError());
	BLA_ATT_ONLINE_F32_BY_ND(att_online_f32_dq_kernel, fwd->q, fwd->k, fwd->v, del_p, fwd->scores_raw, dots, del_q, s, d, D, inv)
	BLA_HIP(hipGetLastError());
	return grad_qkv_weights_and_del_x(stream, batch, d_x, d_wq, d_wk, d_wv, del_q, del_k, del_v, d_partials, d_del_wq, d_del_wk, d_del_wv, d_del_x, c, s, D);
}

}  // extern "C"
