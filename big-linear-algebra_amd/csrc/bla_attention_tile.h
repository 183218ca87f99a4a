// bla_attention_tile.h -- what the bf16 attention kernels share (bla_attention_bf16.hip; bla_attention_online_bf16.hip): the
// fragment readers that take fp32 tensors from memory in v_mfma_f32_32x32x16_bf16's operand order and round them in registers, and the launchers of the
// three kernels that do not depend on how the softmax is done (qkv, grads, fold; defined in bla_attention_bf16.hip).
//
// Fragment and accumulator maps (bla_bf16_tile.h): lane l = 32 h + f holds A[row f][k = 8 h + j] and B[k = 8 h + j][col f], j < 8; accumulator register r
// of lane l is D[row (r & 3) + 8 (r >> 2) + 4 h][col f].  The recurring trick: registers 8 u .. 8 u + 7 of an accumulator tile, rounded and packed, ARE an
// operand fragment whose k index j stands for row perm(h, j, u) = (j & 3) + 8 (j >> 2) + 16 u + 4 h of the tile.  A contraction does not care in which
// order k runs as long as both operands agree, so the other operand is simply read in the same permuted order (two runs of four consecutive elements)
// and no accumulator ever has to be transposed to be multiplied again.
#pragma once
#include "bla_internal.h"
#include "bla_bf16_tile.h"

namespace bla {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
struct F4 { float x, y, z, w; };   // four floats at 4-byte alignment (the tensors are float-aligned, nothing more is asked of the caller)

// Edges without branches: a fragment piece outside its operand is read from these zeros instead (the address is chosen, the load is unconditional), so
// no address outside an operand is ever formed into a load and the kernels stay straight-line code between their barriers.
static __device__ float att_zeros[12];   // (zero-initialised, never written; not const, so that it lives in the same address space as the operands and the loads stay global; one per translation unit)
__device__ __forceinline__ F4 ld4(const float* p, bool ok) { return *(const F4*)(ok ? p : att_zeros); }
__device__ __forceinline__ bf16x8 frag_pack(const F4& a, const F4& b) {
	const u32x4 v = {pack2(a.x, a.y), pack2(a.z, a.w), pack2(b.x, b.y), pack2(b.z, b.w)};
	return __builtin_bit_cast(bf16x8, v);
}
// k = j: p[0 .. 7]
__device__ __forceinline__ bf16x8 frag_row8(const float* p, bool ok) { return frag_pack(ld4(p, ok), ld4(p + 4, ok)); }
// k = j in permuted order: p[0 .. 3], p[8 .. 11]
__device__ __forceinline__ bf16x8 frag_perm(const float* p, bool ok_lo, bool ok_hi) { return frag_pack(ld4(p, ok_lo), ld4(p + 8, ok_hi)); }
// k = j down a column: p[j * stride]
__device__ __forceinline__ bf16x8 frag_col8(const float* p, size_t stride, bool ok) {
	float v[8];
	p = ok ? p : att_zeros;
	stride = ok ? stride : 0;
#pragma unroll
	for (int j = 0; j < 8; ++j) v[j] = p[j * stride];
	const u32x4 u = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
	return __builtin_bit_cast(bf16x8, u);
}
// k = j down a column in permuted order: rows 0 .. 3 and 8 .. 11
__device__ __forceinline__ bf16x8 frag_colperm(const float* p, size_t stride, bool ok_lo, bool ok_hi) {
	float v[8];
	const float *lo = ok_lo ? p : att_zeros, *hi = ok_hi ? p + 8 * stride : att_zeros;
	const size_t sl = ok_lo ? stride : 0, sh = ok_hi ? stride : 0;
#pragma unroll
	for (int j = 0; j < 4; ++j) { v[j] = lo[j * sl]; v[4 + j] = hi[j * sh]; }
	const u32x4 u = {pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7])};
	return __builtin_bit_cast(bf16x8, u);
}
// registers 8 u .. 8 u + 7 of an accumulator tile: k = j stands for tile row perm(h, j, u)
__device__ __forceinline__ bf16x8 frag_acc(const f32x16& a, int u) {
	const u32x4 v = u == 0 ? u32x4{pack2(a[0], a[1]), pack2(a[2], a[3]), pack2(a[4], a[5]), pack2(a[6], a[7])}
	                       : u32x4{pack2(a[8], a[9]), pack2(a[10], a[11]), pack2(a[12], a[13]), pack2(a[14], a[15])};
	return __builtin_bit_cast(bf16x8, v);
}
__device__ __forceinline__ f32x16 zero16() {
	f32x16 z;
#pragma unroll
	for (int r = 0; r < 16; ++r) z[r] = 0.f;
	return z;
}
__device__ __forceinline__ int acc_row(int r, int fh) { return (r & 3) + 8 * (r >> 2) + 4 * fh; }
#define BLA_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16((a), (b), (c), 0, 0, 0)

// ---- the launches both attention blocks share (kernels in bla_attention_bf16.hip; none of them is bounded by S: their grids are S / 32 row blocks or
// 32 x 32 output tiles by the batch) ------------------------------------------------------------------------------------------------------------------
// Q | K | V = r(Z) r([Wq | Wk | Wv]) -> q, k, v [batch][S][d]; any d % 8 == 0 (the multi-head block passes heads x head width)
bla_status att_bf16_launch_qkv(hipStream_t hs, int batch, const float* x, const float* wq, const float* wk, const float* wv, float* q, float* k, float* v, int c, int s,
                               int d);
// out [batch][C][S] = (r(A) r(W) + bias)^T over all d columns of A [batch][S][d]: the multi-head block's output product
bla_status att_bf16_launch_project(hipStream_t hs, int batch, const float* attention, const float* w, const float* bias, float* out, int c, int s, int d);
// del_X, the per-image weight-gradient partials, and their fold in image order
bla_status att_bf16_launch_grads_fold(hipStream_t hs, int batch, const float* dy, const float* x, const float* wq, const float* wk, const float* wv,
                                      const float* attention, const float* gq, const float* gk, const float* gv, float* partials, float* del_wq, float* del_wk,
                                      float* del_wv, float* del_w, float* dx, int c, int s, int d);

}  // namespace bla
