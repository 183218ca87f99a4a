// bla_attention_bf16.hip -- the U-Net's self-attention block with bf16 operands on v_mfma_f32_32x32x16_bf16.
//
// The rule (include/bla.h): both operands of every matrix product are rounded to bf16 (bla_f32_to_bf16's rounding) immediately before the product;
// accumulation, softmax, its derivative, bias, scaling and every stored tensor are fp32.  Of the S x S tensors only `weights` reaches memory: the forward
// writes it once, the backward reads it once; T, del_S and del_I live in accumulator registers (del_I crosses a 32 x 32 bf16 LDS tile to change hands).
//
// The shapes (S <= 256, d <= 64) make the block a kernel family of its own: a wave owns 32 query rows and ALL keys, so a row of scores is 8 accumulator
// tiles at most and the softmax runs in registers.  No operand is staged: the fp32 tensors are read from memory (L2-resident between the launches) in
// exactly the fragment order and rounded in registers.
//
// Fragment and accumulator maps (bla_bf16_tile.h): lane l = 32 h + f holds A[row f][k = 8 h + j] and B[k = 8 h + j][col f], j < 8; accumulator register r
// of lane l is D[row (r & 3) + 8 (r >> 2) + 4 h][col f].  The recurring trick: registers 8 u .. 8 u + 7 of an accumulator tile, rounded and packed, ARE an
// operand fragment whose k index j stands for row perm(h, j, u) = (j & 3) + 8 (j >> 2) + 16 u + 4 h of the tile.  A contraction does not care in which
// order k runs as long as both operands agree, so the other operand is simply read in the same permuted order (two runs of four consecutive elements)
// and no accumulator ever has to be transposed to be multiplied again.
//
// Launches: forward 2 (qkv, core); backward 3 (core: one workgroup per image; grads: del_X and the image's four weight-gradient partials, one wave per
// 32 x 32 output tile; fold: the partials summed in image order).  Every sum has a fixed order: no atomics, the same bits on every run.
#include "bla_attention_tile.h"
#include <cmath>

namespace bla {
namespace {

// (the fragment readers -- ld4, frag_row8, frag_perm, frag_col8, frag_colperm, frag_acc -- are bla_attention_tile.h's, shared with the online block)

// ---- qkv: Q | K | V = r(Z) . r([Wq | Wk | Wv]), Z = X^T ------------------------------------------------------------------------------------------
// One wave per 32 rows of Z (four to a workgroup, independent).  A fragment: X[k][s0 + f] down the channels (a half-wave reads 128 contiguous bytes per
// k); B fragment: column n of the C x 3d concatenation, i.e. column n % d of matrix n / d.  A wave holds six accumulator tiles, 192 columns: all of them
// at d <= 64; the multi-head block's d (its heads side by side, up to 256) takes groups of six tiles on gridDim.z.  An element's contraction over C is the
// same ascending 16-deep steps whatever group its column falls in.
__global__ void __launch_bounds__(256) att_bf16_qkv_kernel(const float* __restrict__ x, const float* __restrict__ wq, const float* __restrict__ wk,
                                                           const float* __restrict__ wv, float* __restrict__ q, float* __restrict__ k, float* __restrict__ v,
                                                           int c, int s, int d) {
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int rb = blockIdx.x * 4 + wave, b = blockIdx.y;
	if (rb * 32 >= s) return;
	const float* xb = x + (size_t)b * c * s + rb * 32 + fr;
	const int nt = (3 * d + 31) / 32, j0 = blockIdx.z * 6;
	f32x16 acc[6];
	const float* wp[6];
	bool wok[6];
#pragma unroll
	for (int j = 0; j < 6; ++j) {
		acc[j] = zero16();
		const int n = 32 * (j0 + j) + fr, mi = n / d;
		wok[j] = j0 + j < nt && n < 3 * d;
		wp[j] = wok[j] ? (mi == 0 ? wq : mi == 1 ? wk : wv) + n % d : wq;
	}
	for (int k0 = 0; k0 < c; k0 += 16) {
		const int kk = k0 + 8 * fh;
		const bool okk = kk < c;
		const bf16x8 a = frag_col8(xb + (size_t)kk * s, (size_t)s, okk);
#pragma unroll
		for (int j = 0; j < 6; ++j)
			if (j0 + j < nt) acc[j] = BLA_MFMA(a, frag_col8(wp[j] + (size_t)kk * d, (size_t)d, okk && wok[j]), acc[j]);
	}
#pragma unroll
	for (int j = 0; j < 6; ++j) {
		if (!wok[j]) continue;
		const int n = 32 * (j0 + j) + fr, mi = n / d;
		float* dst = (mi == 0 ? q : mi == 1 ? k : v) + (size_t)b * s * d + n % d;
#pragma unroll
		for (int r = 0; r < 16; ++r) dst[(size_t)(rb * 32 + acc_row(r, fh)) * d] = acc[j][r];
	}
}

// ---- project: out^T = r(W)^T r(A)^T + bias, the multi-head block's output product ----------------------------------------------------
// One wave per 32 channels x 32 queries (four query blocks to a workgroup, independent), the contraction over all d = heads x head width columns of A in
// ascending 16-deep steps.  A fragment: W[dd + j][cc] down a column of W; B fragment: A[query f][dd + j], a row of A.  `out` is stored in runs of 32
// consecutive pixels of a channel, like the forward cores' fused product.  Channel tiles run fastest over the grid, so the tiles that read the same rows
// of A are neighbours.
__global__ void __launch_bounds__(256) att_bf16_project_kernel(const float* __restrict__ attention, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ out, int c, int s, int d) {
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int ct = blockIdx.x, rb = blockIdx.y * 4 + wave, b = blockIdx.z;
	if (rb * 32 >= s) return;
	const int cc = ct * 32 + fr, query = rb * 32 + fr;
	const float* arow = attention + ((size_t)b * s + query) * d;
	f32x16 o = zero16();
	for (int d0 = 0; d0 < d; d0 += 16) {
		const int dd = d0 + 8 * fh;
		o = BLA_MFMA(frag_col8(w + (size_t)dd * c + cc, (size_t)c, cc < c && dd < d), frag_row8(arow + dd, dd < d), o);
	}
#pragma unroll
	for (int r = 0; r < 16; ++r) {
		const int ch = ct * 32 + acc_row(r, fh);
		if (ch < c) out[((size_t)b * c + ch) * s + query] = o[r] + bias[ch];
	}
}

// ---- forward core --------------------------------------------------------------------------------------------------------------------------------
// One wave per 32 queries of an image.  The score tiles are formed TRANSPOSED, K . Q^T: a lane holds one query (column f) and, over the S / 32 tiles,
// half of its keys; the other half sits in lane f + 32.  Row maximum and row sum are a pass over the lane's registers and one exchange with that lane.
// The same registers are the B fragments of A^T = V^T . P^T (keys permuted; V is read in the same order), and A^T's registers the B fragments of
// out^T = W^T . A^T (d permuted; W's rows are read in the same order), so `out` is stored in runs of 32 consecutive pixels of one channel.
__global__ void __launch_bounds__(64) att_bf16_fwd_kernel(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                          const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ weights,
                                                          float* __restrict__ attention, float* __restrict__ out, int c, int s, int d, float inv) {
	const int lane = threadIdx.x & 63, fr = lane & 31, fh = lane >> 5;
	const int rb = blockIdx.x, b = blockIdx.y, nk = s >> 5, nd = (d + 15) >> 4, ndt = (d + 31) >> 5;
	const size_t img = (size_t)b * s * d;
	const float *qb = q + img, *kb = k + img, *vb = v + img;
	const int query = rb * 32 + fr;

	bf16x8 qf[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) qf[i] = frag_row8(qb + (size_t)query * d + 16 * i + 8 * fh, i < nd && 16 * i + 8 * fh < d);
	f32x16 sc[8];
#pragma unroll
	for (int t = 0; t < 8; ++t) {
		if (t >= nk) continue;
		sc[t] = zero16();
#pragma unroll
		for (int i = 0; i < 4; ++i)
			if (i < nd) sc[t] = BLA_MFMA(frag_row8(kb + (size_t)(t * 32 + fr) * d + 16 * i + 8 * fh, 16 * i + 8 * fh < d), qf[i], sc[t]);
	}
	// softmax of the query's row, the row maximum subtracted
	float mx = -INFINITY;
#pragma unroll
	for (int t = 0; t < 8; ++t) {
		if (t >= nk) continue;
#pragma unroll
		for (int r = 0; r < 16; ++r) { sc[t][r] *= inv; mx = fmaxf(mx, sc[t][r]); }
	}
	mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
	float sum = 0.f;
#pragma unroll
	for (int t = 0; t < 8; ++t) {
		if (t >= nk) continue;
#pragma unroll
		for (int r = 0; r < 16; ++r) { sc[t][r] = __expf(sc[t][r] - mx); sum += sc[t][r]; }
	}
	sum += __shfl_xor(sum, 32, 64);
	const float rs = 1.f / sum;
	float* wrow = weights + ((size_t)b * s + query) * s;
#pragma unroll
	for (int t = 0; t < 8; ++t) {
		if (t >= nk) continue;
#pragma unroll
		for (int r = 0; r < 16; ++r) sc[t][r] *= rs;
#pragma unroll
		for (int g = 0; g < 4; ++g) *(F4*)(wrow + t * 32 + 8 * g + 4 * fh) = F4{sc[t][4 * g], sc[t][4 * g + 1], sc[t][4 * g + 2], sc[t][4 * g + 3]};
	}
	// A^T[dd][query] = sum over keys of V[key][dd] P[query][key]
	f32x16 at[2];
	at[0] = zero16(); at[1] = zero16();
#pragma unroll
	for (int t = 0; t < 8; ++t) {
		if (t >= nk) continue;
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const bf16x8 pf = frag_acc(sc[t], u);
#pragma unroll
			for (int dt = 0; dt < 2; ++dt) {
				if (dt >= ndt) continue;
				const int dd = dt * 32 + fr;
				at[dt] = BLA_MFMA(frag_colperm(vb + (size_t)(t * 32 + 16 * u + 4 * fh) * d + dd, (size_t)d, dd < d, dd < d), pf, at[dt]);
			}
		}
	}
	bf16x8 af[2][2];
#pragma unroll
	for (int dt = 0; dt < 2; ++dt) {
		if (dt >= ndt) continue;
		float* arow = attention + ((size_t)b * s + query) * d;
#pragma unroll
		for (int g = 0; g < 4; ++g) {
			const int dd = dt * 32 + 8 * g + 4 * fh;
			if (dd < d) *(F4*)(arow + dd) = F4{at[dt][4 * g], at[dt][4 * g + 1], at[dt][4 * g + 2], at[dt][4 * g + 3]};
		}
		af[dt][0] = frag_acc(at[dt], 0);
		af[dt][1] = frag_acc(at[dt], 1);
	}
	// out^T[cc][query] = sum over dd of W[dd][cc] A[query][dd] + bias[cc]
	for (int c0 = 0; c0 < c; c0 += 32) {
		f32x16 o = zero16();
		const int cc = c0 + fr;
#pragma unroll
		for (int dt = 0; dt < 2; ++dt)
#pragma unroll
			for (int u = 0; u < 2; ++u) {
				const int base = dt * 32 + 16 * u;
				if (base >= d) continue;
				o = BLA_MFMA(frag_colperm(w + (size_t)(base + 4 * fh) * c + cc, (size_t)c, cc < c && base + 4 * fh < d, cc < c && base + 4 * fh + 8 < d), af[dt][u], o);
			}
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			const int ch = c0 + acc_row(r, fh);
			if (ch < c) out[((size_t)b * c + ch) * s + query] = o[r] + bias[ch];
		}
	}
}

// ---- backward core: del_Q, del_K, del_V of one image ---------------------------------------------------------------------------------------------
// One workgroup of four waves per image; a wave takes the 32-query row blocks wave, wave + 4, ...  Per row block:
//   del_P (32 x d) in both orientations from the same fragments (del_Y' W^T and its transpose);
//   pass 1 over the key tiles: P's tile is read (its only read) into registers, del_S's tile = r(del_P) r(V)^T, the row dots <P, del_S> accumulate,
//     and del_V^T += r(del_P)^T r(P) goes to the image's LDS accumulator;
//   pass 2: del_S's tile again (the same instructions, the same bits), del_I = inv P (del_S - <P, del_S>), del_K^T += r(Q)^T r(del_I) to LDS, and
//     del_Q += r(del_I) r(K) after del_I, rounded, has crossed a 32 x 32 LDS tile of the wave's own (the contraction runs over the lane index).
// Here a lane holds one KEY (column f) and the registers the queries.  In step i the wave with row block rb works on key tile (rb + i) % nk, so no two
// waves add into the same LDS tile between two barriers and every tile receives its row blocks in a fixed order.
// del_S[query rows][key t * 32 + f] = r(del_P) r(V)^T: the A fragments are del_P^T's accumulators (dd permuted), V's row is read in the same order
__device__ __forceinline__ f32x16 del_s_tile(const bf16x8 (&dPd)[2][2], const float* vb, int t, int d, int fr, int fh) {
	f32x16 dS = zero16();
#pragma unroll
	for (int dt = 0; dt < 2; ++dt)
#pragma unroll
		for (int u = 0; u < 2; ++u) {
			const int base = dt * 32 + 16 * u;
			if (base >= d) continue;
			dS = BLA_MFMA(dPd[dt][u], frag_perm(vb + (size_t)(t * 32 + fr) * d + base + 4 * fh, base + 4 * fh < d, base + 4 * fh + 8 < d), dS);
		}
	return dS;
}
// One step of the backward core's second pass (see the kernel): key tile t of a row block whose P tile, row dots and fragments the caller holds.
__device__ __forceinline__ void pass2_step(const f32x16& Pi, const float (&rowdot)[16], const bf16x8 (&dPd)[2][2], const bf16x8 (&qf)[2][2], f32x16 (&dQ)[2],
                                           float* accK, unsigned char* xt, const float* vb, const float* kb, int t, int s, int d,
                                           int ndt, int fr, int fh, float inv, bool active) {
	f32x16 dI = del_s_tile(dPd, vb, t, d, fr, fh);
#pragma unroll
	for (int r = 0; r < 16; ++r) dI[r] = (Pi[r] * (dI[r] - rowdot[r])) * inv;
	const bf16x8 i0 = frag_acc(dI, 0), i1 = frag_acc(dI, 1);
#pragma unroll
	for (int dt = 0; dt < 2; ++dt) {
		if (dt >= ndt) continue;
		f32x16 D = BLA_MFMA(qf[dt][0], i0, zero16());
		D = BLA_MFMA(qf[dt][1], i1, D);
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			const int dd = dt * 32 + acc_row(r, fh);
			if (active) accK[(size_t)dd * s + t * 32 + fr] += D[r];
		}
	}
	// r(del_I) changes hands: written [query][key], read back as the A fragment [query f][key 16 u + 8 h + j]
#pragma unroll
	for (int r = 0; r < 16; ++r) *(uint16_t*)(xt + acc_row(r, fh) * 80 + fr * 2) = f32_to_bf16_rne(dI[r]);
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
	__builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
	for (int u = 0; u < 2; ++u) {
		const bf16x8 a = *(const bf16x8*)(xt + fr * 80 + (16 * u + 8 * fh) * 2);
#pragma unroll
		for (int dt = 0; dt < 2; ++dt) {
			if (dt >= ndt) continue;
			const int dd = dt * 32 + fr;
			dQ[dt] = BLA_MFMA(a, frag_col8(kb + (size_t)(t * 32 + 16 * u + 8 * fh) * d + dd, (size_t)d, dd < d), dQ[dt]);
		}
	}
	__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	__builtin_amdgcn_wave_barrier();
}
constexpr int kCoreWaves = 4, kXTileBytes = 32 * 80;   // the wave's transposition tile: 32 rows of 32 bf16, rows 80 bytes apart (16-byte aligned reads)
template <int NK, int DT>   // DT = tiles of 32 across d; S / 32: the steps of a pass are spelled out, so that a P tile is sixteen registers and never an indexed array
__global__ void __launch_bounds__(64 * kCoreWaves) att_bf16_bwd_core_kernel(const float* dy, const float* w, const float* q,
                                                                             const float* k, const float* v,
                                                                             const float* weights, float* gq, float* gk,
                                                                             float* gv, int c, int s, int d, float inv) {
	extern __shared__ __attribute__((aligned(16))) unsigned char att_lds[];
	const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), fr = lane & 31, fh = lane >> 5;
	const int b = blockIdx.x;
	constexpr int nk = NK, ndt = DT;
	float* accV = (float*)att_lds;       // [32 ndt][s]: del_V^T (rows d .. 32 ndt - 1 receive exact zeros: no edge test on the accumulation)
	float* accK = accV + (size_t)32 * ndt * s;  // the same for del_K^T
	unsigned char* xt = (unsigned char*)(accK + (size_t)32 * ndt * s) + wave * kXTileBytes;
	const size_t img = (size_t)b * s * d;
	const float *qb = q + img, *kb = k + img, *vb = v + img, *dyb = dy + (size_t)b * c * s, *pb = weights + (size_t)b * s * s;
	for (int e = threadIdx.x; e < 2 * 32 * ndt * s; e += 64 * kCoreWaves) accV[e] = 0.f;
	__syncthreads();

	for (int o = 0; o * kCoreWaves < nk; ++o) {
		// a wave without a row block in this round works on block 0 again and keeps the result to itself: every wave meets every barrier, and no
		// accumulator array lives across a branch
		const bool active = o * kCoreWaves + wave < nk;
		const int rb = active ? o * kCoreWaves + wave : 0;
		f32x16 P[NK];
		bf16x8 dPq[2][2];   // [dd tile][query half]: A fragment [dd f][query perm] of del_V^T = del_P^T P
		bf16x8 dPd[2][2];   // [dd tile][dd half]:    A fragment [query f][dd perm] of del_S = del_P V^T
		bf16x8 qf[2][2];    // [dd tile][query half]: A fragment [dd f][query perm] of del_K^T = Q^T del_I
		float rowdot[16];
		f32x16 dQ[2];
		{
			f32x16 dP[2], dPT[2];
			dP[0] = dP[1] = dPT[0] = dPT[1] = zero16();
			for (int c0 = 0; c0 < c; c0 += 16) {
				const int cc = c0 + 8 * fh;
				const bool okc = cc < c;
				const bf16x8 yf = frag_col8(dyb + (size_t)cc * s + rb * 32 + fr, (size_t)s, okc);   // del_Y'[query f][cc + j]
#pragma unroll
				for (int dt = 0; dt < 2; ++dt) {
					if (dt >= ndt) continue;
					const int dd = dt * 32 + fr;
					const bf16x8 wf = frag_row8(w + (size_t)dd * c + cc, okc && dd < d);   // W[dd f][cc + j]
					dPT[dt] = BLA_MFMA(wf, yf, dPT[dt]);   // rows dd, column query
					dP[dt] = BLA_MFMA(yf, wf, dP[dt]);     // rows query, column dd
				}
			}
#pragma unroll
			for (int dt = 0; dt < 2; ++dt) {
				if (dt >= ndt) continue;
				const int dd = dt * 32 + fr;
#pragma unroll
				for (int u = 0; u < 2; ++u) {
					dPq[dt][u] = frag_acc(dP[dt], u);
					dPd[dt][u] = frag_acc(dPT[dt], u);
					qf[dt][u] = frag_colperm(qb + (size_t)(rb * 32 + 16 * u + 4 * fh) * d + dd, (size_t)d, dd < d, dd < d);
				}
				dQ[dt] = zero16();
			}
#pragma unroll
			for (int r = 0; r < 16; ++r) rowdot[r] = 0.f;
		}
		// pass 1
#pragma unroll
		for (int i = 0; i < NK; ++i) {
			{
				const int t = (rb + i) % nk;
#pragma unroll
				for (int r = 0; r < 16; ++r) P[i][r] = pb[(size_t)(rb * 32 + acc_row(r, fh)) * s + t * 32 + fr];
				const f32x16 dS = del_s_tile(dPd, vb, t, d, fr, fh);
#pragma unroll
				for (int r = 0; r < 16; ++r) rowdot[r] += P[i][r] * dS[r];
				const bf16x8 p0 = frag_acc(P[i], 0), p1 = frag_acc(P[i], 1);
#pragma unroll
				for (int dt = 0; dt < 2; ++dt) {
					if (dt >= ndt) continue;
					f32x16 D = BLA_MFMA(dPq[dt][0], p0, zero16());
					D = BLA_MFMA(dPq[dt][1], p1, D);
#pragma unroll
					for (int r = 0; r < 16; ++r) {
						const int dd = dt * 32 + acc_row(r, fh);
						if (active) accV[(size_t)dd * s + t * 32 + fr] += D[r];
					}
				}
			}
			__syncthreads();
		}
		{   // <P, del_S> of a query: over the keys, i.e. over the 32 lanes of the half-wave
#pragma unroll
			for (int r = 0; r < 16; ++r)
#pragma unroll
				for (int m = 1; m < 32; m <<= 1) rowdot[r] += __shfl_xor(rowdot[r], m, 64);
		}
		// pass 2
		// (eight spelled-out steps: as one loop the body is past the size the compiler unrolls, and P[i] has to be a register, not an indexed array)
#define BLA_ATT_PASS2(i)                                                                                                            \
		if constexpr (NK > i) {                                                                                                     \
			pass2_step(P[i], rowdot, dPd, qf, dQ, accK, xt, vb, kb, (rb + i) % nk, s, d, ndt, fr, fh, inv, active);                 \
			__syncthreads();                                                                                                        \
		}
		BLA_ATT_PASS2(0) BLA_ATT_PASS2(1) BLA_ATT_PASS2(2) BLA_ATT_PASS2(3) BLA_ATT_PASS2(4) BLA_ATT_PASS2(5) BLA_ATT_PASS2(6) BLA_ATT_PASS2(7)
#undef BLA_ATT_PASS2
		{
#pragma unroll
			for (int dt = 0; dt < 2; ++dt) {
				if (dt >= ndt) continue;
				const int dd = dt * 32 + fr;
				if (dd < d && active)
#pragma unroll
					for (int r = 0; r < 16; ++r) gq[img + (size_t)(rb * 32 + acc_row(r, fh)) * d + dd] = dQ[dt][r];
			}
		}
	}
	__syncthreads();
	for (int e = threadIdx.x; e < s * d; e += 64 * kCoreWaves) {
		const int key = e / d, dd = e % d;
		gv[img + e] = accV[(size_t)dd * s + key];
		gk[img + e] = accK[(size_t)dd * s + key];
	}
}

// ---- backward grads: del_X and the image's four weight-gradient partials ------------------------------------------------------------------------
// One wave per 32 x 32 output tile, grid (tiles, batch).  Tiles in order: del_X [C][S]; del_Wq, del_Wk, del_Wv partials [C][d] (contraction over S);
// del_W partial [d][C] (contraction over S).  partials: [batch][Wq | Wk | Wv | W], 4 C d floats an image.
__global__ void __launch_bounds__(64) att_bf16_bwd_grads_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ wq,
                                                                const float* __restrict__ wk, const float* __restrict__ wv, const float* __restrict__ attention,
                                                                const float* __restrict__ gq, const float* __restrict__ gk, const float* __restrict__ gv,
                                                                float* __restrict__ partials, float* __restrict__ dx, int c, int s, int d) {
	const int lane = threadIdx.x & 63, fr = lane & 31, fh = lane >> 5;
	const int b = blockIdx.y, nct = (c + 31) >> 5, nst = s >> 5, ndt = (d + 31) >> 5, nd = (d + 15) >> 4;
	const size_t img = (size_t)b * s * d, cd = (size_t)c * d;
	int job = blockIdx.x;
	f32x16 acc = zero16();
	if (job < nct * nst) {   // del_X = r(Wq) r(del_Q)^T + r(Wk) r(del_K)^T + r(Wv) r(del_V)^T, accumulated in that order
		const int ct = job / nst, st = job % nst, cc = ct * 32 + fr;
#pragma unroll
		for (int m = 0; m < 3; ++m) {
			const float* wm = m == 0 ? wq : m == 1 ? wk : wv;
			const float* gm = (m == 0 ? gq : m == 1 ? gk : gv) + img;
			for (int i = 0; i < nd; ++i) {
				const int dd = 16 * i + 8 * fh;
				acc = BLA_MFMA(frag_row8(wm + (size_t)cc * d + dd, cc < c && dd < d), frag_row8(gm + (size_t)(st * 32 + fr) * d + dd, dd < d), acc);
			}
		}
#pragma unroll
		for (int r = 0; r < 16; ++r) {
			const int ch = ct * 32 + acc_row(r, fh);
			if (ch < c) dx[((size_t)b * c + ch) * s + st * 32 + fr] = acc[r];
		}
		return;
	}
	job -= nct * nst;
	float* part = partials + (size_t)b * 4 * cd;
	if (job < 3 * nct * ndt) {   // del_Wm partial = r(Z)^T r(del_M): [cc][dd] = sum over s of X[cc][s] del_M[s][dd]
		const int m = job / (nct * ndt), ct = (job % (nct * ndt)) / ndt, dt = job % ndt, cc = ct * 32 + fr, dd = dt * 32 + fr;
		const float* gm = (m == 0 ? gq : m == 1 ? gk : gv) + img;
		const float* xb = x + (size_t)b * c * s;
		for (int s0 = 0; s0 < s; s0 += 16) {
			const int ss = s0 + 8 * fh;
			acc = BLA_MFMA(frag_row8(xb + (size_t)cc * s + ss, cc < c), frag_col8(gm + (size_t)ss * d + dd, (size_t)d, dd < d), acc);
		}
		if (dd < d)
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int ch = ct * 32 + acc_row(r, fh);
				if (ch < c) part[m * cd + (size_t)ch * d + dd] = acc[r];
			}
		return;
	}
	job -= 3 * nct * ndt;
	{   // del_W partial = r(A)^T r(del_Y'): [dd][cc] = sum over s of A[s][dd] del_Y[cc][s]
		const int dt = job / nct, ct = job % nct, cc = ct * 32 + fr, dd = dt * 32 + fr;
		const float* ab = attention + img;
		const float* dyb = dy + (size_t)b * c * s;
		for (int s0 = 0; s0 < s; s0 += 16) {
			const int ss = s0 + 8 * fh;
			acc = BLA_MFMA(frag_col8(ab + (size_t)ss * d + dd, (size_t)d, dd < d), frag_row8(dyb + (size_t)cc * s + ss, cc < c), acc);
		}
		if (cc < c)
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int dr = dt * 32 + acc_row(r, fh);
				if (dr < d) part[3 * cd + (size_t)dr * c + cc] = acc[r];
			}
	}
}

// ---- fold: the four gradients = the partials summed in image order (batch_sum's arithmetic) -----------------------------------------------------
__global__ void __launch_bounds__(256) att_bf16_fold_kernel(const float* __restrict__ src, float* __restrict__ g0, float* __restrict__ g1, float* __restrict__ g2,
                                                            float* __restrict__ g3, int batch, size_t cd) {
	const size_t n = 4 * cd;
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
		float acc = 0.f;
		int b = 0;
		for (; b + 8 <= batch; b += 8) {
			float v[8];
#pragma unroll
			for (int u = 0; u < 8; u++) v[u] = src[(size_t)(b + u) * n + i];
#pragma unroll
			for (int u = 0; u < 8; u++) acc += v[u];
		}
		for (; b < batch; b++) acc += src[(size_t)b * n + i];
		const size_t which = i / cd;
		(which == 0 ? g0 : which == 1 ? g1 : which == 2 ? g2 : g3)[i - which * cd] = acc;
	}
}

}  // namespace

bla_status att_bf16_launch_qkv(hipStream_t hs, int batch, const float* x, const float* wq, const float* wk, const float* wv, float* q, float* k, float* v, int c, int s,
                               int d) {
	const int nt = (3 * d + 31) / 32;
	hipLaunchKernelGGL(att_bf16_qkv_kernel, dim3((s / 32 + 3) / 4, batch, (nt + 5) / 6), dim3(256), 0, hs, x, wq, wk, wv, q, k, v, c, s, d);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status att_bf16_launch_project(hipStream_t hs, int batch, const float* attention, const float* w, const float* bias, float* out, int c, int s, int d) {
	hipLaunchKernelGGL(att_bf16_project_kernel, dim3((c + 31) / 32, (s / 32 + 3) / 4, batch), dim3(256), 0, hs, attention, w, bias, out, c, s, d);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status att_bf16_launch_grads_fold(hipStream_t hs, int batch, const float* dy, const float* x, const float* wq, const float* wk, const float* wv,
                                      const float* attention, const float* gq, const float* gk, const float* gv, float* partials, float* del_wq, float* del_wk,
                                      float* del_wv, float* del_w, float* dx, int c, int s, int d) {
	const int nct = (c + 31) / 32, nst = s / 32, ndt = (d + 31) / 32;
	hipLaunchKernelGGL(att_bf16_bwd_grads_kernel, dim3(nct * nst + 4 * nct * ndt, batch), dim3(64), 0, hs, dy, x, wq, wk, wv, attention, gq, gk, gv, partials, dx, c, s, d);
	BLA_HIP(hipGetLastError());
	const size_t cd = (size_t)c * d;
	hipLaunchKernelGGL(att_bf16_fold_kernel, dim3((unsigned)((4 * cd + 255) / 256)), dim3(256), 0, hs, partials, del_wq, del_wk, del_wv, del_w, batch, cd);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

}  // namespace bla

using namespace bla;

extern "C" {

int bla_attention_bf16_applies(int c, int s, int d) {
	return s % 32 == 0 && s >= 32 && s <= 256 && d % 8 == 0 && d >= 8 && d <= 64 && c % 8 == 0 && c > 0;
}

bla_status bla_attention_forward_batched_bf16(void* stream, int batch, const float* d_x, const float* d_wq, const float* d_wk, const float* d_wv, const float* d_w,
                                              const float* d_bias, const bla_attention_ws* ws, float* d_out, int c, int s, int d) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(batch > 0 && batch <= 65535 && bla_attention_bf16_applies(c, s, d), BLA_ERR_INVALID,
	            "bf16 attention: B=%d C=%d S=%d d=%d (S %% 32 == 0 in 32..256, d %% 8 == 0 in 8..64, C %% 8 == 0)", batch, c, s, d);
	BLA_REQUIRE(d_x && d_wq && d_wk && d_wv && d_w && d_bias && d_out && ws && ws->q && ws->k && ws->v && ws->weights && ws->attention, BLA_ERR_INVALID, "null operand");
	hipStream_t hs = pick_stream(stream);
	const int nk = s / 32;
	if ((st = att_bf16_launch_qkv(hs, batch, d_x, d_wq, d_wk, d_wv, ws->q, ws->k, ws->v, c, s, d))) return st;
	const float inv = (float)(1.0 / sqrt((double)d));
	hipLaunchKernelGGL(att_bf16_fwd_kernel, dim3(nk, batch), dim3(64), 0, hs, ws->q, ws->k, ws->v, d_w, d_bias, ws->weights, ws->attention, d_out, c, s, d, inv);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_attention_backward_batched_bf16(void* stream, int batch, const float* d_del_y, const float* d_x, const float* d_wq, const float* d_wk,
                                               const float* d_wv, const float* d_w, const bla_attention_ws* fwd, const bla_attention_ws* grad, float* d_partials,
                                               float* d_del_wq, float* d_del_wk, float* d_del_wv, float* d_del_w, float* d_del_x, int c, int s, int d) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(batch > 0 && batch <= 65535 && bla_attention_bf16_applies(c, s, d), BLA_ERR_INVALID,
	            "bf16 attention: B=%d C=%d S=%d d=%d (S %% 32 == 0 in 32..256, d %% 8 == 0 in 8..64, C %% 8 == 0)", batch, c, s, d);
	BLA_REQUIRE(d_del_y && d_x && d_wq && d_wk && d_wv && d_w && fwd && grad && d_partials && d_del_wq && d_del_wk && d_del_wv && d_del_w && d_del_x, BLA_ERR_INVALID,
	            "null operand");
	BLA_REQUIRE(fwd->q && fwd->k && fwd->v && fwd->weights && fwd->attention && grad->q && grad->k && grad->v, BLA_ERR_INVALID, "null workspace");
	hipStream_t hs = pick_stream(stream);
	const float inv = (float)(1.0 / sqrt((double)d));
	const size_t lds = (size_t)2 * 32 * ((d + 31) / 32) * s * sizeof(float) + kCoreWaves * kXTileBytes;
#define BLA_ATT_CORE(NK)                                                                                                                              \
	case NK: {                                                                                                                                        \
		auto kern = d > 32 ? att_bf16_bwd_core_kernel<NK, 2> : att_bf16_bwd_core_kernel<NK, 1>;                                                                                                   \
		if (lds > 48 * 1024) BLA_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));                   \
		hipLaunchKernelGGL(kern, dim3(batch), dim3(64 * kCoreWaves), lds, hs, d_del_y, d_w, fwd->q, fwd->k, fwd->v, fwd->weights, grad->q, grad->k,   \
		                   grad->v, c, s, d, inv);                                                                                                    \
	} break;
	switch (s / 32) { BLA_ATT_CORE(1) BLA_ATT_CORE(2) BLA_ATT_CORE(3) BLA_ATT_CORE(4) BLA_ATT_CORE(5) BLA_ATT_CORE(6) BLA_ATT_CORE(7) BLA_ATT_CORE(8) }
#undef BLA_ATT_CORE
	BLA_HIP(hipGetLastError());
	return att_bf16_launch_grads_fold(hs, batch, d_del_y, d_x, d_wq, d_wk, d_wv, fwd->attention, grad->q, grad->k, grad->v, d_partials, d_del_wq, d_del_wk, d_del_wv,
	                                  d_del_w, d_del_x, c, s, d);
}

}  // extern "C"
