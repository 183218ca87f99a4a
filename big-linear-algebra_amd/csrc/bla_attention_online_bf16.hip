// bla_attention_online_bf16.hip -- the bf16 self-attention block for long sequences: the softmax runs ONLINE over blocks of 32 keys, no S x S tensor
// exists in memory in either direction.  The rule is bla_attention_bf16.hip's (include/bla.h): both operands of every matrix product are
// rounded to bf16 immediately before the product; everything else is fp32.
//
// Forward: a wave owns 32 queries and walks the key blocks in ascending order with the running maximum m, the running sum l and ceil(d / 32)
// accumulator tiles of Acc^T.  The score tile is formed transposed (K . Q^T), so a lane holds ONE query: m, l and the rescale factor are per-lane
// scalars, the tile maximum and sum are a pass over 16 registers and one exchange with lane + 32.  Saved per query: lse = m + log(l).
// Backward: P is recomputed as exp(T - lse).  A preamble writes del_P and the row dots <del_P, A> (= <P, del_S> in exact arithmetic, which is what lets
// the pass run without P).  Then two kernels, so that every accumulator stays in one wave's registers and no sum crosses waves:
//   dkv: a wave per 32-key block walks the query blocks; del_K^T and del_V^T tiles stay in registers; a lane holds one KEY.
//   dq:  a wave per 32-query block walks the key blocks;  del_Q^T tiles stay in registers; a lane holds one QUERY (the forward's tile, the same instructions).
// All four kernels are straight-line code per wave: no LDS, no barrier, no atomics; four independent waves a workgroup share their K / V (Q / del_P)
// reads through the caches.  The three walking kernels are templated on ND = ceil(d / 16), the 16-deep steps of a contraction over d (and with it on
// DT = ceil(d / 32), the 32-row tiles across d): the model's d = 16 then keeps one accumulator tile where d = 64 keeps two, and several waves fit a SIMD.
// dkv at d <= 16 loads the fp32 words of the NEXT block's fragments before it works on the current block (the last step loads its own block again: no
// address past the tensors is formed): measured 7 % off that kernel; the same in the forward core and dq measured nothing and is not done.
// qkv, grads and fold are bla_attention_bf16.hip's (bla_attention_tile.h).
//
// Several heads (bla_attention_*_batched_online_bf16_heads): the heads lie side by side in rows of ld = heads x d floats, head h in columns
// h d .. h d + d - 1, and gridDim.z is the head.  The four kernels take the row stride ld beside the head width d: every edge test and every tile store
// is bounded by d, every row step is ld, lse and the row dots sit at (b heads + h) S.  One body serves both pairs of entries (the single-head entries
// pass ld = d and one grid plane), so a head's arithmetic is the single-head block's instruction for instruction.  With several heads the forward core
// stops after A (template flag): out contracts over all heads and is a launch of its own (att_bf16_launch_project), as are qkv, grads and fold at
// width ld.
#include "bla_attention_tile.h"
#include <cmath>

namespace bla {
namespace {

constexpr int kWaves = 4;   // independent waves a workgroup: one 32-row block each

// the fp32 words of a fragment, and their rounding: frag_row8 / frag_colperm in two halves, so that the load can be issued a block ahead
struct Row8 { F4 a, b; };
struct Col8 { float v[8]; };
__device__ __forceinline__ Row8 ld_row8(const float* p, bool ok) { return {ld4(p, ok), ld4(p + 4, ok)}; }
__device__ __forceinline__ bf16x8 pack(const Row8& r) { return frag_pack(r.a, r.b); }
__device__ __forceinline__ Col8 ld_colperm(const float* p, size_t stride, bool ok) {   // rows 0 .. 3 and 8 .. 11 of a column
	Col8 c;
	const float *lo = ok ? p : att_zeros, *hi = ok ? p + 8 * stride : att_zeros;
	const size_t st = ok ? stride : 0;
#pragma unroll
	for (int j = 0; j < 4; ++j) { c.v[j] = lo[j * st]; c.v[4 + j] = hi[j * st]; }
	return c;
}
__device__ __forceinline__ bf16x8 pack(const Col8& c) {
	const u32x4 u = {pack2(c.v[0], c.v[1]), pack2(c.v[2], c.v[3]), pack2(c.v[4], c.v[5]), pack2(c.v[6], c.v[7])};
	return __builtin_bit_cast(bf16x8, u);
}

// the fragments of block t that the forward core and dq read: rows of one tensor (key f of the block, 8 consecutive dd per step i) and columns of another
// (dd = 32 dt + f, the block's keys in permuted order per half u)
template <int ND>
struct BlockWords {
	static constexpr int DT = (ND + 1) / 2;
	Row8 row[ND];
	Col8 col[2][DT];
	__device__ __forceinline__ void load(const float* rows, const float* cols, int t, int d, int ld, int fr, int fh) {
#pragma unroll
		for (int i = 0; i < ND; ++i) row[i] = ld_row8(rows + (size_t)(t * 32 + fr) * ld + 16 * i + 8 * fh, 16 * i + 8 * fh < d);
#pragma unroll
		for (int u = 0; u < 2; ++u)
#pragma unroll
			for (int dt = 0; dt < DT; ++dt) col[u][dt] = ld_colperm(cols + (size_t)(t * 32 + 16 * u + 4 * fh) * ld + dt * 32 + fr, (size_t)ld, dt * 32 + fr < d);
	}
};

// T^T's tile: rows = the 32 keys of a block, column = the lane's query; scaled by inv with a rounding of its own (never contracted into what follows), so
// that the forward pass and the backward pass see the same bits.
template <int ND>
__device__ __forceinline__ f32x16 score_tile_t(const Row8 (&krow)[ND], const bf16x8 (&qf)[ND], float inv) {
	f32x16 sc = zero16();
#pragma unroll
	for (int i = 0; i < ND; ++i) sc = BLA_MFMA(pack(krow[i]), qf[i], sc);
#pragma unroll
	for (int r = 0; r < 16; ++r) sc[r] = __fmul_rn(sc[r], inv);
	return sc;
}
// rows dd (registers), column = the lane's row of a [S][d] tensor: stored as runs of four consecutive dd
__device__ __forceinline__ void store_tile_t(float* row, const f32x16& a, int dt, int d, int fh) {
#pragma unroll
	for (int g = 0; g < 4; ++g) {
		const int dd = dt * 32 + 8 * g + 4 * fh;
		if (dd < d) *(F4*)(row + dd) = F4{a[4 * g], a[4 * g + 1], a[4 * g + 2], a[4 * g + 3]};
	}
}

// ---- forward core ----------------------------------------------------------------------------------------------------------------------------------
template <int ND, bool PROJ>
__global__ void __launch_bounds__(64 * kWaves) att_online_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                      const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ lse,
                                                                      float* __restrict__ attention, float* __restrict__ out, int c, int s, int d, int ld, float inv) {
	constexpr int DT = (ND + 1) / 2;
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int rb = blockIdx.x * kWaves + wave, b = blockIdx.y, nk = s >> 5;
	if (rb >= nk) return;
	const size_t img = (size_t)b * s * ld + (size_t)blockIdx.z * d, vec = ((size_t)b * gridDim.z + blockIdx.z) * s;
	const float *qb = q + img, *kb = k + img, *vb = v + img;
	const int query = rb * 32 + fr;

	bf16x8 qf[ND];
#pragma unroll
	for (int i = 0; i < ND; ++i) qf[i] = frag_row8(qb + (size_t)query * ld + 16 * i + 8 * fh, 16 * i + 8 * fh < d);
	float m = -INFINITY, l = 0.f;
	f32x16 at[DT];   // Acc^T[dd][query]
#pragma unroll
	for (int dt = 0; dt < DT; ++dt) at[dt] = zero16();
	BlockWords<ND> cur;   // rows of K, columns of V
	for (int t = 0; t < nk; ++t) {
		cur.load(kb, vb, t, d, ld, fr, fh);
		f32x16 sc = score_tile_t<ND>(cur.row, qf, inv);
		float mx = m;
#pragma unroll
		for (int r = 0; r < 16; ++r) mx = fmaxf(mx, sc[r]);
		mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
		const float a = __expf(m - mx);   // the first block: exp(-inf) = 0 against l = 0 and Acc = 0
		float sum = 0.f;
#pragma unroll
		for (int r = 0; r < 16; ++r) { sc[r] = __expf(sc[r] - mx); sum += sc[r]; }
		sum += __shfl_xor(sum, 32, 64);
		l = l * a + sum;
		m = mx;
#pragma unroll
		for (int dt = 0; dt < DT; ++dt)
#pragma unroll
			for (int r = 0; r < 16; ++r) at[dt][r] *= a;
		// Acc^T[dd][query] += sum over the block's keys of V[key][dd] p[query][key]
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const bf16x8 pf = frag_acc(sc, u);
#pragma unroll
			for (int dt = 0; dt < DT; ++dt) at[dt] = BLA_MFMA(pack(cur.col[u][dt]), pf, at[dt]);
		}
	}
	if (fh == 0) lse[vec + query] = m + logf(l);
	bf16x8 af[DT][2];
#pragma unroll
	for (int dt = 0; dt < DT; ++dt) {
#pragma unroll
		for (int r = 0; r < 16; ++r) at[dt][r] /= l;
		store_tile_t(attention + img + (size_t)query * ld, at[dt], dt, d, fh);
		af[dt][0] = frag_acc(at[dt], 0);
		af[dt][1] = frag_acc(at[dt], 1);
	}
	if (!PROJ) return;   // several heads: the contraction of out runs over all of them (att_bf16_launch_project)
	// out^T[cc][query] = sum over dd of W[dd][cc] A[query][dd] + bias[cc]
	for (int c0 = 0; c0 < c; c0 += 32) {
		f32x16 o = zero16();
		const int cc = c0 + fr;
#pragma unroll
		for (int dt = 0; dt < DT; ++dt)
#pragma unroll
			for (int u = 0; u < 2; ++u) {
				const int base = dt * 32 + 16 * u;
				if (base >= 16 * ND) continue;
				o = BLA_MFMA(frag_colperm(w + (size_t)(base + 4 * fh) * c + cc, (size_t)c, cc < c && base + 4 * fh < d, cc < c && base + 4 * fh + 8 < d), af[dt][u], o);
			}
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			const int ch = c0 + acc_row(r, fh);
			if (ch < c) out[((size_t)b * c + ch) * s + query] = o[r] + bias[ch];
		}
	}
}

// ---- backward preamble: del_P = r(del_Y') r(W)^T and dot = <del_P, A> per query -----------------------------------------------------------------------
// del_P^T's tiles (rows dd, column = the lane's query), so the dot is a pass over the lane's registers and one exchange with lane + 32.
__global__ void __launch_bounds__(64 * kWaves) att_online_bwd_pre_kernel(const float* __restrict__ dy, const float* __restrict__ w, const float* __restrict__ attention,
                                                                          float* __restrict__ dp, float* __restrict__ dots, int c, int s, int d, int ld) {
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int rb = blockIdx.x * kWaves + wave, b = blockIdx.y, ndt = (d + 31) >> 5;
	if (rb * 32 >= s) return;
	const int query = rb * 32 + fr;
	const float* dyb = dy + (size_t)b * c * s;
	w += (size_t)blockIdx.z * d * c;   // the head's rows of W
	f32x16 dPT[2];
	dPT[0] = zero16(); dPT[1] = zero16();
	for (int c0 = 0; c0 < c; c0 += 16) {
		const int cc = c0 + 8 * fh;
		const bool okc = cc < c;
		const bf16x8 yf = frag_col8(dyb + (size_t)cc * s + query, (size_t)s, okc);   // del_Y'[query f][cc + j]
#pragma unroll
		for (int dt = 0; dt < 2; ++dt) {
			if (dt >= ndt) continue;
			const int dd = dt * 32 + fr;
			dPT[dt] = BLA_MFMA(frag_row8(w + (size_t)dd * c + cc, okc && dd < d), yf, dPT[dt]);   // rows dd, column query
		}
	}
	const size_t row = ((size_t)b * s + query) * ld + (size_t)blockIdx.z * d;
	float dot = 0.f;
#pragma unroll
	for (int dt = 0; dt < 2; ++dt) {
		if (dt >= ndt) continue;
		store_tile_t(dp + row, dPT[dt], dt, d, fh);
#pragma unroll
		for (int g = 0; g < 4; ++g) {
			const int dd = dt * 32 + 8 * g + 4 * fh;
			const F4 a = ld4(attention + row + dd, dd < d);   // (past d the tile holds exact zeros)
			dot += dPT[dt][4 * g] * a.x + dPT[dt][4 * g + 1] * a.y + dPT[dt][4 * g + 2] * a.z + dPT[dt][4 * g + 3] * a.w;
		}
	}
	dot += __shfl_xor(dot, 32, 64);
	if (fh == 0) dots[((size_t)b * gridDim.z + blockIdx.z) * s + query] = dot;
}

// ---- backward dq: del_Q of 32 queries over all key blocks ------------------------------------------------------------------------------------------------
// Everything transposed, as in the forward core: T^T, del_S^T = V . del_P^T and del_I^T tiles with the query on the lane; del_I^T's registers are the B
// fragments of del_Q^T = K^T . del_I^T (keys permuted; K is read in the same order).
template <int ND>
__global__ void __launch_bounds__(64 * kWaves) att_online_bwd_dq_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                         const float* __restrict__ dp, const float* __restrict__ lse, const float* __restrict__ dots,
                                                                         float* __restrict__ gq, int s, int d, int ld, float inv) {
	constexpr int DT = (ND + 1) / 2;
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int rb = blockIdx.x * kWaves + wave, b = blockIdx.y, nk = s >> 5;
	if (rb >= nk) return;
	const size_t img = (size_t)b * s * ld + (size_t)blockIdx.z * d, vec = ((size_t)b * gridDim.z + blockIdx.z) * s;
	const float *qb = q + img, *kb = k + img, *vb = v + img, *dpb = dp + img;
	const int query = rb * 32 + fr;
	bf16x8 qf[ND], pf[ND];
#pragma unroll
	for (int i = 0; i < ND; ++i) {
		const bool ok = 16 * i + 8 * fh < d;
		qf[i] = frag_row8(qb + (size_t)query * ld + 16 * i + 8 * fh, ok);
		pf[i] = frag_row8(dpb + (size_t)query * ld + 16 * i + 8 * fh, ok);
	}
	const float L = lse[vec + query], dot = dots[vec + query];
	f32x16 dQ[DT];
#pragma unroll
	for (int dt = 0; dt < DT; ++dt) dQ[dt] = zero16();
	BlockWords<ND> cur;   // rows and columns of K
	Row8 vrow[ND];        // rows of V
	for (int t = 0; t < nk; ++t) {
		cur.load(kb, kb, t, d, ld, fr, fh);
#pragma unroll
		for (int i = 0; i < ND; ++i) vrow[i] = ld_row8(vb + (size_t)(t * 32 + fr) * ld + 16 * i + 8 * fh, 16 * i + 8 * fh < d);
		const f32x16 sc = score_tile_t<ND>(cur.row, qf, inv);
		f32x16 dI = zero16();   // del_S^T[key][query] first
#pragma unroll
		for (int i = 0; i < ND; ++i) dI = BLA_MFMA(pack(vrow[i]), pf[i], dI);
#pragma unroll
		for (int r = 0; r < 16; ++r) dI[r] = (__expf(sc[r] - L) * (dI[r] - dot)) * inv;
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const bf16x8 f = frag_acc(dI, u);
#pragma unroll
			for (int dt = 0; dt < DT; ++dt) dQ[dt] = BLA_MFMA(pack(cur.col[u][dt]), f, dQ[dt]);
		}
	}
#pragma unroll
	for (int dt = 0; dt < DT; ++dt) store_tile_t(gq + img + (size_t)query * ld, dQ[dt], dt, d, fh);
}

// ---- backward dkv: del_K and del_V of 32 keys over all query blocks ---------------------------------------------------------------------------------------
// A lane holds one KEY (column f), the registers the queries: T = Q . K^T is the forward's tile with the operands' roles exchanged (the same products
// in the same order of k), del_S = del_P . V^T.  P's and del_I's registers are the B fragments of del_V^T = del_P^T . P and del_K^T = Q^T . del_I
// (queries permuted; del_P and Q are read down their columns in the same order).
template <int ND>
__global__ void __launch_bounds__(64 * kWaves) att_online_bwd_dkv_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                          const float* __restrict__ dp, const float* __restrict__ lse, const float* __restrict__ dots,
                                                                          float* __restrict__ gk, float* __restrict__ gv, int s, int d, int ld, float inv) {
	constexpr int DT = (ND + 1) / 2;
	constexpr bool PF = ND == 1;   // a block ahead where it was measured to pay
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int kt = blockIdx.x * kWaves + wave, b = blockIdx.y, nk = s >> 5;
	if (kt >= nk) return;
	const size_t img = (size_t)b * s * ld + (size_t)blockIdx.z * d, vec = ((size_t)b * gridDim.z + blockIdx.z) * s;
	const float *qb = q + img, *kb = k + img, *vb = v + img, *dpb = dp + img, *lb = lse + vec, *db = dots + vec;
	const int key = kt * 32 + fr;
	bf16x8 kf[ND], vf[ND];
#pragma unroll
	for (int i = 0; i < ND; ++i) {
		const bool ok = 16 * i + 8 * fh < d;
		kf[i] = frag_row8(kb + (size_t)key * ld + 16 * i + 8 * fh, ok);
		vf[i] = frag_row8(vb + (size_t)key * ld + 16 * i + 8 * fh, ok);
	}
	f32x16 dK[DT], dV[DT];
#pragma unroll
	for (int dt = 0; dt < DT; ++dt) { dK[dt] = zero16(); dV[dt] = zero16(); }
	BlockWords<ND> qc, qn, pc, pn;   // rows and columns of Q and of del_P for a block of queries
	if (PF) { qn.load(qb, qb, 0, d, ld, fr, fh); pn.load(dpb, dpb, 0, d, ld, fr, fh); }
	for (int t = 0; t < nk; ++t) {
		if (PF) {
			qc = qn; pc = pn;
			const int tn = t + 1 < nk ? t + 1 : t;
			qn.load(qb, qb, tn, d, ld, fr, fh); pn.load(dpb, dpb, tn, d, ld, fr, fh);
		} else { qc.load(qb, qb, t, d, ld, fr, fh); pc.load(dpb, dpb, t, d, ld, fr, fh); }
		f32x16 P = zero16(), dI = zero16();
#pragma unroll
		for (int i = 0; i < ND; ++i) {
			P = BLA_MFMA(pack(qc.row[i]), kf[i], P);
			dI = BLA_MFMA(pack(pc.row[i]), vf[i], dI);
		}
#pragma unroll
		for (int g = 0; g < 4; ++g) {   // rows 8 g + 4 h .. + 3 of the tile are registers 4 g .. 4 g + 3
			const F4 L = *(const F4*)(lb + t * 32 + 8 * g + 4 * fh), D = *(const F4*)(db + t * 32 + 8 * g + 4 * fh);
			const float Lr[4] = {L.x, L.y, L.z, L.w}, Dr[4] = {D.x, D.y, D.z, D.w};
#pragma unroll
			for (int e = 0; e < 4; ++e) {
				const int r = 4 * g + e;
				P[r] = __expf(__fmul_rn(P[r], inv) - Lr[e]);
				dI[r] = (P[r] * (dI[r] - Dr[e])) * inv;
			}
		}
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const bf16x8 pfr = frag_acc(P, u), ifr = frag_acc(dI, u);
#pragma unroll
			for (int dt = 0; dt < DT; ++dt) {
				dV[dt] = BLA_MFMA(pack(pc.col[u][dt]), pfr, dV[dt]);
				dK[dt] = BLA_MFMA(pack(qc.col[u][dt]), ifr, dK[dt]);
			}
		}
	}
#pragma unroll
	for (int dt = 0; dt < DT; ++dt) {
		store_tile_t(gk + img + (size_t)key * ld, dK[dt], dt, d, fh);
		store_tile_t(gv + img + (size_t)key * ld, dV[dt], dt, d, fh);
	}
}

}  // namespace
}  // namespace bla

using namespace bla;

extern "C" {

int bla_attention_online_bf16_applies(int c, int s, int d) {
	return s % 32 == 0 && s >= 32 && s <= 4096 && d % 8 == 0 && d >= 8 && d <= 64 && c % 8 == 0 && c > 0;
}
int bla_attention_online_bf16_heads_applies(int c, int s, int heads, int d) {
	return bla_attention_online_bf16_applies(c, s, d) && heads >= 1 && heads <= 256 / d;   // heads d <= 256
}

}  // extern "C"

#define BLA_ATT_ONLINE_SHAPE(batch, c, s, d)                                                                                     \
	BLA_REQUIRE(batch > 0 && batch <= 65535 && bla_attention_online_bf16_applies(c, s, d), BLA_ERR_INVALID,                       \
	            "online bf16 attention: B=%d C=%d S=%d d=%d (S %% 32 == 0 in 32..4096, d %% 8 == 0 in 8..64, C %% 8 == 0)", batch, c, s, d)
#define BLA_ATT_HEADS_SHAPE(batch, c, s, heads, d)                                                                                               \
	BLA_REQUIRE(batch > 0 && batch <= 65535 && bla_attention_online_bf16_heads_applies(c, s, heads, d), BLA_ERR_INVALID,                          \
	            "online bf16 attention: B=%d C=%d S=%d heads=%d d=%d (S %% 32 == 0 in 32..4096, d %% 8 == 0 in 8..64, heads d <= 256, C %% 8 == 0)", \
	            batch, c, s, heads, d)
#define BLA_ATT_FWD_NULLS(ws) \
	BLA_REQUIRE(d_x && d_wq && d_wk && d_wv && d_w && d_bias && d_out && ws && ws->q && ws->k && ws->v && ws->scores_raw && ws->attention, BLA_ERR_INVALID, "null operand")
#define BLA_ATT_BWD_NULLS(fwd, grad)                                                                                                                            \
	BLA_REQUIRE(d_del_y && d_x && d_wq && d_wk && d_wv && d_w && fwd && grad && d_partials && d_del_wq && d_del_wk && d_del_wv && d_del_w && d_del_x,           \
	            BLA_ERR_INVALID, "null operand");                                                                                                               \
	BLA_REQUIRE(fwd->q && fwd->k && fwd->v && fwd->scores_raw && fwd->attention && grad->q && grad->k && grad->v && grad->attention && grad->scores_raw,        \
	            BLA_ERR_INVALID, "null workspace")
// ND = ceil(d / 16)
#define BLA_ATT_ONLINE_BY_ND(KERNEL, ...)                                                         \
	switch ((d + 15) / 16) {                                                                      \
	case 1: hipLaunchKernelGGL(KERNEL(1), grid, block, 0, hs, __VA_ARGS__); break;                \
	case 2: hipLaunchKernelGGL(KERNEL(2), grid, block, 0, hs, __VA_ARGS__); break;                \
	case 3: hipLaunchKernelGGL(KERNEL(3), grid, block, 0, hs, __VA_ARGS__); break;                \
	default: hipLaunchKernelGGL(KERNEL(4), grid, block, 0, hs, __VA_ARGS__); break;               \
	}
#define BLA_ATT_FWD_FUSED(ND) (att_online_fwd_kernel<ND, true>)
#define BLA_ATT_FWD_HEADS(ND) (att_online_fwd_kernel<ND, false>)
#define BLA_ATT_DKV(ND) (att_online_bwd_dkv_kernel<ND>)
#define BLA_ATT_DQ(ND) (att_online_bwd_dq_kernel<ND>)

namespace {
// both pairs of entries: `heads` heads of width d side by side in rows of heads * d floats, a head per grid plane; one head is the single-head block, whose
// forward core also multiplies by W (with several the contraction of `out` runs over all of them: a launch of its own)
bla_status online_forward(hipStream_t hs, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, const float* d_w, const float* d_bias,
                          const bla_attention_ws* ws, float* d_out, int c, int s, int heads, int d) {
	const int ld = heads * d;
	bla_status st = att_bf16_launch_qkv(hs, batch, d_x, d_wq, d_wk, d_wv, ws->q, ws->k, ws->v, c, s, ld);
	if (st) return st;
	const float inv = (float)(1.0 / sqrt((double)d));
	const dim3 grid((s / 32 + kWaves - 1) / kWaves, batch, heads), block(64 * kWaves);
	if (heads == 1) {
		BLA_ATT_ONLINE_BY_ND(BLA_ATT_FWD_FUSED, ws->q, ws->k, ws->v, d_w, d_bias, ws->scores_raw, ws->attention, d_out, c, s, d, ld, inv)
		BLA_HIP(hipGetLastError());
		return BLA_OK;
	}
	BLA_ATT_ONLINE_BY_ND(BLA_ATT_FWD_HEADS, ws->q, ws->k, ws->v, d_w, d_bias, ws->scores_raw, ws->attention, d_out, c, s, d, ld, inv)
	BLA_HIP(hipGetLastError());
	return att_bf16_launch_project(hs, batch, ws->attention, d_w, d_bias, d_out, c, s, ld);
}

bla_status online_backward(hipStream_t hs, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, const float* d_w,
                           const bla_attention_ws* fwd, const bla_attention_ws* grad, float* d_partials, float* d_del_wq, float* d_del_wk, float* d_del_wv,
                           float* d_del_w, float* d_del_x, int c, int s, int heads, int d) {
	const int ld = heads * d;
	const float inv = (float)(1.0 / sqrt((double)d));
	const dim3 grid((s / 32 + kWaves - 1) / kWaves, batch, heads), block(64 * kWaves);
	hipLaunchKernelGGL(att_online_bwd_pre_kernel, grid, block, 0, hs, d_del_y, d_w, fwd->attention, grad->attention, grad->scores_raw, c, s, d, ld);
	BLA_HIP(hipGetLastError());
	BLA_ATT_ONLINE_BY_ND(BLA_ATT_DKV, fwd->q, fwd->k, fwd->v, grad->attention, fwd->scores_raw, grad->scores_raw, grad->k, grad->v, s, d, ld, inv)
	BLA_HIP(hipGetLastError());
	BLA_ATT_ONLINE_BY_ND(BLA_ATT_DQ, fwd->q, fwd->k, fwd->v, grad->attention, fwd->scores_raw, grad->scores_raw, grad->q, s, d, ld, inv)
	BLA_HIP(hipGetLastError());
	// (nothing in grads or fold bounds the width: at heads * d they are the multi-head weight gradients and del_X)
	return att_bf16_launch_grads_fold(hs, batch, d_del_y, d_x, d_wq, d_wk, d_wv, fwd->attention, grad->q, grad->k, grad->v, d_partials, d_del_wq, d_del_wk, d_del_wv,
	                                  d_del_w, d_del_x, c, s, ld);
}
}  // namespace

extern "C" {

bla_status bla_attention_forward_batched_online_bf16(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv,
                                                     const float* d_w, const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int d) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_ATT_ONLINE_SHAPE(batch, c, s, d);
	BLA_ATT_FWD_NULLS(ws);
	return online_forward(pick_stream(stream), batch, d_x, d_wq, d_wk, d_wv, d_w, d_bias, ws, d_out, c, s, 1, d);
}

bla_status bla_attention_backward_batched_online_bf16(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                      const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad,
                                                      float* d_partials, float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x, int c,
                                                      int s, int d) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_ATT_ONLINE_SHAPE(batch, c, s, d);
	BLA_ATT_BWD_NULLS(fwd, grad);
	return online_backward(pick_stream(stream), batch, d_del_y, d_x, d_wq, d_wk, d_wv, d_w, fwd, grad, d_partials, d_del_wq, d_del_wk, d_del_wv, d_del_w, d_del_x, c, s, 1,
	                       d);
}

bla_status bla_attention_forward_batched_online_bf16_heads(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv,
                                                           const float* d_w, const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int heads,
                                                           int d) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_ATT_HEADS_SHAPE(batch, c, s, heads, d);
	BLA_ATT_FWD_NULLS(ws);
	return online_forward(pick_stream(stream), batch, d_x, d_wq, d_wk, d_wv, d_w, d_bias, ws, d_out, c, s, heads, d);
}

bla_status bla_attention_backward_batched_online_bf16_heads(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                                            const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad,
                                                            float* d_partials, float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x,
                                                            int c, int s, int heads, int d) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_ATT_HEADS_SHAPE(batch, c, s, heads, d);
	BLA_ATT_BWD_NULLS(fwd, grad);
	return online_backward(pick_stream(stream), batch, d_del_y, d_x, d_wq, d_wk, d_wv, d_w, fwd, grad, d_partials, d_del_wq, d_del_wk, d_del_wv, d_del_w, d_del_x, c, s,
	                       heads, d);
}

}  // extern "C"
