// bla_gemm_mxfp8.hip -- OCP MXFP8 operands (e4m3 elements, one E8M0 scale byte per 32 elements of the contraction), fp32 accumulation (include/bla.h,
// "MXFP8"): the quantiser, the dequantiser, the product and its composition from fp32 operands.
//
// The fast kernel (gemm_mxfp8_nt_kernel) is the tile of bla_mx_tile.h with a dense B [n][k] and bla_gemm_bf16's epilogue; the general kernel decodes in
// software.  The fp32 -> e4m3 rounding is written out in integer arithmetic (mx_round_e4m3), so the contract does not hang on a conversion instruction.
#include "bla_internal.h"
#include "bla_mx_tile.h"

namespace bla {
namespace {

// ---- the format, device side -------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float mx_decode_e4m3(uint32_t b) {   // finite bytes only
	const uint32_t e = (b >> 3) & 15u, m = b & 7u, sign = (b & 0x80u) << 24;
	const float mag = e ? __uint_as_float(((e + 120u) << 23) | (m << 20)) : (float)m * 0.001953125f;   // subnormals: m 2^-9
	return __uint_as_float(__float_as_uint(mag) | sign);
}
__device__ __forceinline__ float mx_decode_scale(uint32_t s) { return __uint_as_float(s ? s << 23 : 0x00400000u); }   // 2^(s - 127); s = 0 is the subnormal 2^-127
// decode(elem) 2^(s - 127) in fp32; NaN (0x7FC00000) when either byte is NaN
__device__ __forceinline__ float mx_dequant(uint32_t b, uint32_t s) {
	if ((b & 0x7fu) == 0x7fu || s == 0xffu) return __uint_as_float(0x7fc00000u);
	return mx_decode_e4m3(b) * mx_decode_scale(s);
}
// |x| < 512 as fp32 bits (sign removed) -> the e4m3 magnitude byte, round to nearest even, saturating at 448 (0x7E)
__device__ __forceinline__ uint32_t mx_round_e4m3(uint32_t a) {
	const uint32_t e = a >> 23;
	if (e >= 121u) {   // |x| >= 2^-6: a normal e4m3; a carry out of the mantissa moves into the exponent by itself
		const uint32_t r = ((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (120u << 3);
		return r > 0x7eu ? 0x7eu : r;
	}
	const uint32_t sh = 141u - e;   // a multiple of 2^-9: mantissa >> sh, >= 21
	if (sh >= 25u) return 0u;       // below half of 2^-9 (fp32 subnormals and zero included)
	const uint32_t mant = (a & 0x7fffffu) | 0x800000u, q = mant >> sh, rem = mant & ((1u << sh) - 1u), half = 1u << (sh - 1u);
	return q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u);   // 8 is the smallest normal, 0x08
}
// the scale byte of a block whose largest |v| has the fp32 bits amax (sign removed); 0xFF for a block with a NaN or an infinity
__device__ __forceinline__ uint32_t mx_scale_byte(uint32_t amax) {
	if (amax >= 0x7f800000u) return 0xffu;
	if (amax == 0u) return 127u;
	const uint32_t e = amax >> 23;   // floor(log2) + 127 (0 for fp32 subnormals); the byte is clamp(floor(log2) - 8, -127, 127) + 127
	return e > 8u ? e - 8u : 0u;
}
__device__ __forceinline__ uint32_t mx_quant(float v, uint32_t sbyte) {   // one element of a block with a finite scale byte
	const float x = v * __uint_as_float((254u - sbyte) << 23);            // v 2^-e, exact barring underflow
	const uint32_t u = __float_as_uint(x);
	return mx_round_e4m3(u & 0x7fffffffu) | ((u >> 24) & 0x80u);
}

// ---- the quantiser, trans = 0: one thread per 4 consecutive elements of a row, 8 lanes per block of 32 ------------------------------------------------
__global__ __launch_bounds__(256) void f32_to_mxfp8_kernel(const float* src, long ld_src, uint8_t* el, long ld, uint8_t* sc, long ld_s, int rows, int cols, int vec_src, int vec_dst) {
	const int quads = ((cols + 31) >> 5) * 8;
	const long id = (long)blockIdx.x * 256 + threadIdx.x;
	const bool live = id < (long)rows * quads;   // every lane stays for the shuffles
	const int r = live ? (int)(id / quads) : 0, c0 = live ? (int)(id % quads) * 4 : 0;
	float v[4] = {0.f, 0.f, 0.f, 0.f};
	if (live) {
		const float* s = src + r * ld_src + c0;
		if (vec_src && c0 + 4 <= cols) {
			const float4 x = *(const float4*)s;
			v[0] = x.x; v[1] = x.y; v[2] = x.z; v[3] = x.w;
		} else {
			for (int j = 0; j < 4; ++j)
				if (c0 + j < cols) v[j] = s[j];
		}
	}
	uint32_t amax = 0;
#pragma unroll
	for (int j = 0; j < 4; ++j) amax = max(amax, __float_as_uint(v[j]) & 0x7fffffffu);
#pragma unroll
	for (int d = 1; d < 8; d <<= 1) amax = max(amax, (uint32_t)__shfl_xor((int)amax, d));
	if (!live) return;
	const uint32_t sb = mx_scale_byte(amax);
	uint32_t o = 0x7f7f7f7fu;
	if (sb != 0xffu) o = mx_quant(v[0], sb) | (mx_quant(v[1], sb) << 8) | (mx_quant(v[2], sb) << 16) | (mx_quant(v[3], sb) << 24);
	uint8_t* d = el + r * ld + c0;
	if (vec_dst) *(uint32_t*)d = o;
	else for (int j = 0; j < 4; ++j) d[j] = (uint8_t)(o >> (8 * j));
	if ((c0 & 31) == 0) sc[r * ld_s + (c0 >> 5)] = (uint8_t)sb;
}

// ---- the quantiser, trans = 1: the source is [cols][rows] (the contraction index is the slow one).  A workgroup takes 128 contraction rows x 32 output
// rows through an LDS tile: the loads run along the source rows, the stores along the output rows (8 lanes write 128 consecutive bytes). -----------------
constexpr int QT_K = 128, QT_R = 32;
__global__ __launch_bounds__(256) void f32_to_mxfp8_trans_kernel(const float* src, long ld_src, uint8_t* el, long ld, uint8_t* sc, long ld_s, int rows, int cols, int vec_dst) {
	__shared__ float tile[QT_K][QT_R + 1];
	const int k0 = blockIdx.x * QT_K, r0 = blockIdx.y * QT_R;
#pragma unroll
	for (int q = 0; q < QT_K / 8; ++q) {
		const int kk = q * 8 + (threadIdx.x >> 5), rr = threadIdx.x & 31;
		tile[kk][rr] = (k0 + kk < cols && r0 + rr < rows) ? src[(k0 + kk) * ld_src + r0 + rr] : 0.f;
	}
	__syncthreads();
	const int rr = threadIdx.x >> 3, kq = threadIdx.x & 7, r = r0 + rr, kbase = k0 + kq * 16;   // 16 consecutive k of one output row; 2 lanes per block
	float v[16];
	uint32_t amax = 0;
#pragma unroll
	for (int j = 0; j < 16; ++j) {
		v[j] = tile[kq * 16 + j][rr];
		amax = max(amax, __float_as_uint(v[j]) & 0x7fffffffu);
	}
	amax = max(amax, (uint32_t)__shfl_xor((int)amax, 1));
	if (r >= rows || (kbase & ~31) >= cols) return;   // the window ends at cols rounded up to 32
	const uint32_t sb = mx_scale_byte(amax);
	uint32_t o[4];
#pragma unroll
	for (int w = 0; w < 4; ++w) {
		o[w] = 0x7f7f7f7fu;
		if (sb != 0xffu) o[w] = mx_quant(v[4 * w], sb) | (mx_quant(v[4 * w + 1], sb) << 8) | (mx_quant(v[4 * w + 2], sb) << 16) | (mx_quant(v[4 * w + 3], sb) << 24);
	}
	uint8_t* d = el + r * ld + kbase;
	if (vec_dst) *(uint4*)d = make_uint4(o[0], o[1], o[2], o[3]);
	else for (int j = 0; j < 16; ++j) d[j] = (uint8_t)(o[j >> 2] >> (8 * (j & 3)));
	if ((kq & 1) == 0) sc[r * ld_s + (kbase >> 5)] = (uint8_t)sb;
}

// ---- the dequantiser: one thread per 4 consecutive elements --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mxfp8_to_f32_kernel(const uint8_t* el, long ld, const uint8_t* sc, long ld_s, float* dst, long ld_dst, int rows, int cols, int vec_src, int vec_dst) {
	const int quads = (cols + 3) >> 2;
	const long id = (long)blockIdx.x * 256 + threadIdx.x;
	if (id >= (long)rows * quads) return;
	const int r = (int)(id / quads), c0 = (int)(id % quads) * 4;
	const uint8_t* s = el + r * ld + c0;
	const uint32_t scale = sc[r * ld_s + (c0 >> 5)];
	float* d = dst + r * ld_dst + c0;
	if (c0 + 4 <= cols) {
		uint32_t x;
		if (vec_src) x = *(const uint32_t*)s;
		else x = s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16) | ((uint32_t)s[3] << 24);
		const float4 o = make_float4(mx_dequant(x & 0xffu, scale), mx_dequant((x >> 8) & 0xffu, scale), mx_dequant((x >> 16) & 0xffu, scale), mx_dequant(x >> 24, scale));
		if (vec_dst) *(float4*)d = o;
		else { d[0] = o.x; d[1] = o.y; d[2] = o.z; d[3] = o.w; }
	} else {
		for (int j = 0; c0 + j < cols; ++j) d[j] = mx_dequant(s[j], scale);
	}
}

// ---- the product -------------------------------------------------------------------------------------------------------------------------------------
struct MxArgs {
	const uint8_t* A; const uint8_t* SA; const uint8_t* B; const uint8_t* SB; void* C; const void* zero;
	int m, n, k, lda, ldsa, ldb, ldsb, ldc, tiles_m, tiles_n;
	float alpha, beta;
	const float* bias_row; const float* bias_col;
	int relu;
};

template <bool C_BF16>
__device__ __forceinline__ void mx_epilogue_store(const MxArgs& p, int r, int c, float acc) {   // bla_gemm_bf16's epilogue, in its order
	float v = p.alpha * acc;
	if (p.bias_row) v += p.bias_row[r];
	if (p.bias_col) v += p.bias_col[c];
	if (p.relu) v = v < 0.f ? 0.f : v;
	const size_t at = (size_t)r * p.ldc + c;
	if (C_BF16) {
		uint16_t* C = (uint16_t*)p.C;
		if (p.beta != 0.f) v += p.beta * bf16_to_f32(C[at]);
		C[at] = f32_to_bf16_rne(v);
	} else {
		float* C = (float*)p.C;
		if (p.beta != 0.f) v += p.beta * C[at];
		C[at] = v;
	}
}

template <bool C_BF16>
__global__ __launch_bounds__(256) void gemm_mxfp8_nt_kernel(MxArgs p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const Bf16Tile t = bf16_tile_of(blockIdx.x, p.tiles_m, p.tiles_n);
	const int row0 = t.tm * BM, col0 = t.tn * BN;

	const uint8_t* pb[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int row = col0 + bf16_piece_row(wave, lane, i);
		pb[i] = p.B + (size_t)(row < p.n ? row : 0) * p.ldb + bf16_piece_chunk(lane, i) * 16;
	}
	const uint32_t* psb[2];
#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const int row = col0 + (wave & 1) * 64 + j * 32 + (lane & 31);
		psb[j] = (const uint32_t*)(p.SB + (size_t)(row < p.n ? row : 0) * p.ldsb);
	}
	f32x16 acc[2][2];
	mx_tile_product(lds, {p.A, p.SA, p.lda, p.ldsa, p.m, p.n, p.k, row0, col0, p.zero}, 0, p.k,
	                [&](int i, int kb) { return pb[i] + kb; }, [&](int j, int kb) { return psb[j] + (kb >> 7); }, acc);
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j) {
			const int c = col0 + bf16_acc_col(j);
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int row = row0 + bf16_acc_row(i, r);
				if (row < p.m && c < p.n) mx_epilogue_store<C_BF16>(p, row, c, acc[i][j][r]);
			}
		}
}

// Any alignment and pitch: one output element per thread, software decode, a k-ascending fp32 fma chain of dequantised values.
template <bool C_BF16>
__global__ __launch_bounds__(256) void gemm_mxfp8_general_kernel(MxArgs p) {
	const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
	if (r >= p.m || c >= p.n) return;
	const uint8_t* a = p.A + (size_t)r * p.lda;
	const uint8_t* b = p.B + (size_t)c * p.ldb;
	const uint8_t* sa = p.SA + (size_t)r * p.ldsa;
	const uint8_t* sb = p.SB + (size_t)c * p.ldsb;
	float acc = 0.f;
	for (int g = 0; g < p.k / MX_BLOCK; ++g) {
		const uint32_t ea = sa[g], eb = sb[g];
		for (int kk = g * MX_BLOCK; kk < (g + 1) * MX_BLOCK; ++kk) acc = fmaf(mx_dequant(a[kk], ea), mx_dequant(b[kk], eb), acc);
	}
	mx_epilogue_store<C_BF16>(p, r, c, acc);
}

// ---- argument checks (pure: they run before the device is asked for) -----------------------------------------------------------------------------------
bla_status mx_check_epilogue(const bla_gemm_epilogue* ep) {
	if (!ep) return BLA_OK;
	BLA_REQUIRE(!ep->pre_act && ep->ld_pre == 0 && !ep->relu_mask && ep->ld_mask == 0 && !ep->row_sum_a && !ep->softmax_y && ep->softmax_scale == 0.f &&
	            !ep->softmax_grad && ep->row_sum_alpha == 0.f && ep->row_sum_beta == 0.f && !ep->softmax_loss_acc && !ep->softmax_correct_acc,
	            BLA_ERR_INVALID, "bla_gemm_mxfp8: the epilogue sets a field other than alpha, beta, bias_row, bias_col, act");
	BLA_REQUIRE(ep->act == BLA_ACT_NONE || ep->act == BLA_ACT_RELU, BLA_ERR_INVALID, "bla_gemm_mxfp8: act %d", ep->act);
	return BLA_OK;
}

// pure: before the device is asked for
bla_status mx_check_extents(int m, int n, int k, bool whole_blocks) {
	BLA_REQUIRE(m >= 0 && n >= 0 && k >= 0, BLA_ERR_INVALID, "bla_gemm_mxfp8: negative extent m %d n %d k %d", m, n, k);
	BLA_REQUIRE(!whole_blocks || k % MX_BLOCK == 0, BLA_ERR_INVALID, "bla_gemm_mxfp8: k %d is not a multiple of 32", k);
	return BLA_OK;
}

bla_status mx_check_product(int m, int n, int k, const void* A, int lda, const void* SA, int ldsa, const void* B, int ldb, const void* SB, int ldsb, const void* C, int ldc) {
	if (m == 0 || n == 0) return BLA_OK;
	BLA_REQUIRE(C && (k == 0 || (A && B && SA && SB)), BLA_ERR_INVALID, "bla_gemm_mxfp8: NULL operand or scales");
	BLA_REQUIRE(lda >= k && ldb >= k && ldsa >= k / MX_BLOCK && ldsb >= k / MX_BLOCK && ldc >= n, BLA_ERR_INVALID,
	            "bla_gemm_mxfp8: pitch too small (lda %d ldsa %d ldb %d ldsb %d ldc %d)", lda, ldsa, ldb, ldsb, ldc);
	return BLA_OK;
}

inline bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }
bool mx_fast_path(int k, const void* A, int lda, const void* SA, int ldsa, const void* B, int ldb, const void* SB, int ldsb) {
	return k > 0 && aligned16(A) && aligned16(B) && lda % 16 == 0 && ldb % 16 == 0 && aligned4(SA) && aligned4(SB) && ldsa % 4 == 0 && ldsb % 4 == 0;
}

bla_status launch_gemm_mxfp8(hipStream_t s, int m, int n, int k, const uint8_t* A, int lda, const uint8_t* SA, int ldsa, const uint8_t* B, int ldb, const uint8_t* SB,
                             int ldsb, void* C, int ldc, int c_type, const bla_gemm_epilogue* ep) {
	if (m == 0 || n == 0) return BLA_OK;
	MxArgs a{};
	a.A = A; a.SA = SA; a.B = B; a.SB = SB; a.C = C; a.m = m; a.n = n; a.k = k; a.lda = lda; a.ldsa = ldsa; a.ldb = ldb; a.ldsb = ldsb; a.ldc = ldc;
	a.alpha = ep ? ep->alpha : 1.f; a.beta = ep ? ep->beta : 0.f;
	a.bias_row = ep ? ep->bias_row : nullptr; a.bias_col = ep ? ep->bias_col : nullptr;
	a.relu = ep && ep->act == BLA_ACT_RELU;
	char name[64];
	const char* ct = c_type == BLA_C_BF16 ? "bf16" : "f32";
	if (mx_fast_path(k, A, lda, SA, ldsa, B, ldb, SB, ldsb)) {
		a.zero = zero_word();
		a.tiles_m = (m + BM - 1) / BM; a.tiles_n = (n + BN - 1) / BN;
		const long tiles = (long)a.tiles_m * a.tiles_n;
		BLA_REQUIRE(tiles < (1L << 31), BLA_ERR_INVALID, "bla_gemm_mxfp8: %ld tiles exceed the grid", tiles);
		if (c_type == BLA_C_BF16) hipLaunchKernelGGL(gemm_mxfp8_nt_kernel<true>, dim3((unsigned)tiles), dim3(256), 2 * SLAB_BYTES, s, a);
		else hipLaunchKernelGGL(gemm_mxfp8_nt_kernel<false>, dim3((unsigned)tiles), dim3(256), 2 * SLAB_BYTES, s, a);
		BLA_HIP(hipGetLastError());
		snprintf(name, sizeof name, "gemm_mxfp8_mfma128x128x128_%s", ct);
	} else {
		BLA_REQUIRE((m + 15) / 16 <= 65535, BLA_ERR_INVALID, "bla_gemm_mxfp8: m %d exceeds the general kernel's grid", m);
		const dim3 grid((n + 15) / 16, (m + 15) / 16);
		if (c_type == BLA_C_BF16) hipLaunchKernelGGL(gemm_mxfp8_general_kernel<true>, grid, dim3(256), 0, s, a);
		else hipLaunchKernelGGL(gemm_mxfp8_general_kernel<false>, grid, dim3(256), 0, s, a);
		BLA_HIP(hipGetLastError());
		snprintf(name, sizeof name, "gemm_mxfp8_general_%s", ct);
	}
	gemm_note_last_kernel(name);
	return BLA_OK;
}

bla_status mx_check_quant(const void* src, int ld_src, int trans, int rows, int cols, const void* el, int ld, const void* sc, int ld_s) {
	if (rows == 0 || cols == 0) return BLA_OK;
	BLA_REQUIRE(src && el && sc, BLA_ERR_INVALID, "bla_f32_to_mxfp8: NULL pointer");
	BLA_REQUIRE(ld_src >= (trans ? rows : cols), BLA_ERR_INVALID, "bla_f32_to_mxfp8: ld_src %d too small", ld_src);
	BLA_REQUIRE(ld >= (cols + 31) / 32 * 32 && ld_s >= (cols + 31) / 32, BLA_ERR_INVALID, "bla_f32_to_mxfp8: ld %d or ld_s %d below the window of %d columns", ld, ld_s, cols);
	return BLA_OK;
}

bla_status launch_f32_to_mxfp8(hipStream_t s, const float* src, int ld_src, int trans, int rows, int cols, uint8_t* el, int ld, uint8_t* sc, int ld_s) {
	if (rows == 0 || cols == 0) return BLA_OK;
	if (!trans) {
		const long n = (long)rows * ((cols + 31) / 32) * 8;
		const int vs = aligned16(src) && ld_src % 4 == 0, vd = aligned4(el) && ld % 4 == 0;
		hipLaunchKernelGGL(f32_to_mxfp8_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, (long)ld_src, el, (long)ld, sc, (long)ld_s, rows, cols, vs, vd);
	} else {
		BLA_REQUIRE((rows + QT_R - 1) / QT_R <= 65535, BLA_ERR_INVALID, "bla_f32_to_mxfp8: %d rows exceed the grid", rows);
		const int vd = aligned16(el) && ld % 16 == 0;
		hipLaunchKernelGGL(f32_to_mxfp8_trans_kernel, dim3((cols + QT_K - 1) / QT_K, (rows + QT_R - 1) / QT_R), dim3(256), 0, s, src, (long)ld_src, el, (long)ld, sc, (long)ld_s,
		                   rows, cols, vd);
	}
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

}  // namespace
}  // namespace bla

using namespace bla;

extern "C" {

bla_status bla_f32_to_mxfp8(void* stream, const float* d_src, int ld_src, int trans, int rows, int cols, uint8_t* d_elems, int ld, uint8_t* d_scales, int ld_s) {
	BLA_REQUIRE(rows >= 0 && cols >= 0, BLA_ERR_INVALID, "bla_f32_to_mxfp8: negative extent %d x %d", rows, cols);
	bla_status st = require_ready();
	if (st != BLA_OK) return st;
	st = mx_check_quant(d_src, ld_src, trans != 0, rows, cols, d_elems, ld, d_scales, ld_s);
	if (st != BLA_OK) return st;
	return launch_f32_to_mxfp8(pick_stream(stream), d_src, ld_src, trans != 0, rows, cols, d_elems, ld, d_scales, ld_s);
}

bla_status bla_mxfp8_to_f32(void* stream, const uint8_t* d_elems, int ld, const uint8_t* d_scales, int ld_s, float* d_dst, int ld_dst, int rows, int cols) {
	BLA_REQUIRE(rows >= 0 && cols >= 0, BLA_ERR_INVALID, "bla_mxfp8_to_f32: negative extent %d x %d", rows, cols);
	bla_status st = require_ready();
	if (st != BLA_OK) return st;
	BLA_REQUIRE(rows == 0 || cols == 0 || (d_elems && d_scales && d_dst), BLA_ERR_INVALID, "bla_mxfp8_to_f32: NULL pointer");
	BLA_REQUIRE(rows == 0 || cols == 0 || (ld >= cols && ld_s >= (cols + 31) / 32 && ld_dst >= cols), BLA_ERR_INVALID, "bla_mxfp8_to_f32: pitch too small (ld %d ld_s %d ld_dst %d)",
	            ld, ld_s, ld_dst);
	const long n = (long)rows * ((cols + 3) / 4);
	if (n == 0) return BLA_OK;
	const int vs = aligned4(d_elems) && ld % 4 == 0, vd = aligned16(d_dst) && ld_dst % 4 == 0;
	hipLaunchKernelGGL(mxfp8_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, pick_stream(stream), d_elems, (long)ld, d_scales, (long)ld_s, d_dst, (long)ld_dst,
	                   rows, cols, vs, vd);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_gemm_mxfp8(void* stream, int m, int n, int k, const uint8_t* d_a, int lda, const uint8_t* d_sa, int ldsa, const uint8_t* d_b, int ldb, const uint8_t* d_sb,
                          int ldsb, void* d_c, int ldc, int c_type, const bla_gemm_epilogue* ep) {
	bla_status st = mx_check_epilogue(ep);
	if (st != BLA_OK) return st;
	BLA_REQUIRE(c_type == BLA_C_F32 || c_type == BLA_C_BF16, BLA_ERR_INVALID, "bla_gemm_mxfp8: c_type %d", c_type);
	st = mx_check_extents(m, n, k, true);
	if (st != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	st = mx_check_product(m, n, k, d_a, lda, d_sa, ldsa, d_b, ldb, d_sb, ldsb, d_c, ldc);
	if (st != BLA_OK) return st;
	return launch_gemm_mxfp8(pick_stream(stream), m, n, k, d_a, lda, d_sa, ldsa, d_b, ldb, d_sb, ldsb, d_c, ldc, c_type, ep);
}

bla_status bla_gemm_f32_as_mxfp8(void* stream, int transa, int transb, int m, int n, int k, const float* d_a, int lda, const float* d_b, int ldb, float* d_c, int ldc,
                                 const bla_gemm_epilogue* ep) {
	bla_status st = mx_check_epilogue(ep);
	if (st != BLA_OK) return st;
	st = mx_check_extents(m, n, k, false);
	if (st != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	if (m == 0 || n == 0) return BLA_OK;
	transa = transa != 0; transb = transb != 0;
	BLA_REQUIRE(d_c && (k == 0 || (d_a && d_b)), BLA_ERR_INVALID, "bla_gemm_f32_as_mxfp8: NULL operand");
	BLA_REQUIRE(lda >= (transa ? m : k) && ldb >= (transb ? k : n) && ldc >= n, BLA_ERR_INVALID, "bla_gemm_f32_as_mxfp8: pitch too small (lda %d ldb %d ldc %d)", lda, ldb, ldc);
	// both operands contraction-contiguous at k rounded up to 32 (a multiple of 16, so it is the element pitch), scale pitches rounded up to 4: with the
	// 256-byte aligned workspace every base and pitch meets the fast path's conditions
	const int kp = (int)round_up((size_t)k, MX_BLOCK), lds = (int)round_up((size_t)kp / MX_BLOCK, 4);
	const size_t a_bytes = round_up((size_t)m * kp, 256), b_bytes = round_up((size_t)n * kp, 256), sa_bytes = round_up((size_t)m * lds, 256), sb_bytes = round_up((size_t)n * lds, 256);
	void* ws = nullptr;
	st = ensure_workspace(a_bytes + b_bytes + sa_bytes + sb_bytes + 256, &ws);
	if (st != BLA_OK) return st;
	uint8_t* a8 = (uint8_t*)ws;
	uint8_t* b8 = a8 + a_bytes;
	uint8_t* sa = b8 + b_bytes;
	uint8_t* sb = sa + sa_bytes;
	hipStream_t s = pick_stream(stream);
	if (k > 0) {
		st = launch_f32_to_mxfp8(s, d_a, lda, transa, m, k, a8, kp, sa, lds);    // A stored k x m (transa): the contraction is the slow index
		if (st != BLA_OK) return st;
		st = launch_f32_to_mxfp8(s, d_b, ldb, !transb, n, k, b8, kp, sb, lds);   // B stored k x n (!transb): likewise
		if (st != BLA_OK) return st;
	}
	return launch_gemm_mxfp8(s, m, n, kp, a8, kp, sa, lds, b8, kp, sb, lds, d_c, ldc, BLA_C_F32, ep);
}

}  // extern "C"
