// bla_gemm_bf16.hip -- bf16 operands, fp32 accumulation (include/bla.h, "mixed precision"): the conversions, the 16-bit transpose, the product.
//
// The fast kernel (gemm_bf16_nt_kernel) is the tile of bla_bf16_tile.h with a dense B [n][k]; its epilogue honours alpha, beta, both biases and ReLU.
//   * K-split (SPLIT = true): a grid of tiles x S workgroups; workgroup (tile, s) runs the same slab loop over the slabs [s sps, (s + 1) sps)
//     and stores its fp32 accumulator tile whole to partial [s][tile][128][128]; gemm_bf16_fold_kernel adds the S partials of an element in ascending s
//     and runs the epilogue.  No atomics, no arrival counters: the result does not depend on the order in which workgroups run.
#include "bla_internal.h"
#include "bla_bf16_tile.h"

namespace bla {
namespace {

struct Bf16Args {
	const uint16_t* A; const uint16_t* B; void* C; const void* zero;
	int m, n, k, lda, ldb, ldc, tiles_m, tiles_n;
	float alpha, beta;
	const float* bias_row; const float* bias_col;
	int relu;
	long sa_r, sa_k, sb_k, sb_c;   // general kernel: element strides of op(A)[r][kk] and op(B)[kk][c]
	float* partial; int sps;       // K-split: the partial tiles [split][tile][128][128], slabs per split
};

template <bool C_BF16>
__device__ __forceinline__ void epilogue_store(const Bf16Args& p, int r, int c, float acc) {
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

template <bool C_BF16, bool SPLIT>
__global__ __launch_bounds__(256) void gemm_bf16_nt_kernel(Bf16Args p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int tiles = p.tiles_m * p.tiles_n;
	const int split = SPLIT ? blockIdx.x / tiles : 0;        // split-major: the tiles of one split are consecutive workgroups, in the unsplit order
	const Bf16Tile t = bf16_tile_of(SPLIT ? blockIdx.x - split * tiles : blockIdx.x, p.tiles_m, p.tiles_n);
	const int row0 = t.tm * BM, col0 = t.tn * BN;

	const uint16_t* pb[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int row = col0 + bf16_piece_row(wave, lane, i);
		pb[i] = p.B + (size_t)(row < p.n ? row : 0) * p.ldb + bf16_piece_chunk(lane, i) * 8;
	}
	f32x16 acc[2][2];
	const int k_begin = SPLIT ? split * p.sps * BK : 0, k_end = SPLIT ? min(p.k, k_begin + p.sps * BK) : p.k;
	bf16_tile_product(lds, {p.A, p.lda, p.m, p.n, p.k, row0, col0, p.zero}, k_begin, k_end, [&](int i, int kb) { return pb[i] + kb; }, acc);

	if (SPLIT) {   // the whole tile, unconditioned: rows past m and columns past n hold the zeros their lanes fetched
		float* P = p.partial + ((size_t)split * tiles + (size_t)t.tm * p.tiles_n + t.tn) * (BM * BN);
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int j = 0; j < 2; ++j)
#pragma unroll
				for (int r = 0; r < 16; ++r) P[bf16_acc_row(i, r) * BN + bf16_acc_col(j)] = acc[i][j][r];
		return;
	}
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j) {
			const int c = col0 + bf16_acc_col(j);
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int row = row0 + bf16_acc_row(i, r);
				if (row < p.m && c < p.n) epilogue_store<C_BF16>(p, row, c, acc[i][j][r]);
			}
		}
}

// The fold of a K-split product: one thread per 4 consecutive columns of one row of C (they lie in one tile: 128 % 4 == 0).  acc starts as partial 0 and
// takes partials 1 .. S-1 in ascending order, one fp32 add each; then the unsplit kernel's epilogue, on elements inside m x n only.
template <bool C_BF16>
__global__ __launch_bounds__(256) void gemm_bf16_fold_kernel(Bf16Args p, int splits) {
	const int quads = (p.n + 3) >> 2;
	const long id = (long)blockIdx.x * 256 + threadIdx.x;
	if (id >= (long)p.m * quads) return;
	const int r = (int)(id / quads), c = (int)(id % quads) * 4;
	const size_t per_split = (size_t)p.tiles_m * p.tiles_n * (BM * BN);
	const float* P = p.partial + ((size_t)(r >> 7) * p.tiles_n + (c >> 7)) * (BM * BN) + (r & 127) * BN + (c & 127);
	float4 acc = *(const float4*)P;
#pragma unroll 4
	for (int s = 1; s < splits; ++s) {
		const float4 v = *(const float4*)(P + (size_t)s * per_split);
		acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
	}
	const float a4[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
	for (int j = 0; j < 4; ++j)
		if (c + j < p.n) epilogue_store<C_BF16>(p, r, c + j, a4[j]);
}

// Any shape, pitch, alignment and layout: one output element per thread, 2-byte loads, a k-ascending fp32 fma chain (products of bf16 values are exact).
template <bool C_BF16>
__global__ __launch_bounds__(256) void gemm_bf16_general_kernel(Bf16Args p) {
	const int c = blockIdx.x * 16 + (threadIdx.x & 15), r = blockIdx.y * 16 + (threadIdx.x >> 4);
	if (r >= p.m || c >= p.n) return;
	const uint16_t* a = p.A + (size_t)r * p.sa_r;
	const uint16_t* b = p.B + (size_t)c * p.sb_c;
	float acc = 0.f;
	for (int kk = 0; kk < p.k; ++kk) acc = fmaf(bf16_to_f32(a[(size_t)kk * p.sa_k]), bf16_to_f32(b[(size_t)kk * p.sb_k]), acc);
	epilogue_store<C_BF16>(p, r, c, acc);
}

// ---- conversions: one thread per 8 consecutive elements of a row -----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void f32_to_bf16_kernel(const float* src, long ld_src, uint16_t* dst, long ld_dst, int rows, int cols, int vec) {
	const int chunks = (cols + 7) >> 3;
	const long id = (long)blockIdx.x * 256 + threadIdx.x;
	if (id >= (long)rows * chunks) return;
	const int r = (int)(id / chunks), c0 = (int)(id % chunks) * 8;
	const float* s = src + r * ld_src + c0;
	uint16_t* d = dst + r * ld_dst + c0;
	if (vec && c0 + 8 <= cols) {
		const float4 x = *(const float4*)s, y = *(const float4*)(s + 4);
		uint4 o;
		o.x = f32_to_bf16_rne(x.x) | ((uint32_t)f32_to_bf16_rne(x.y) << 16);
		o.y = f32_to_bf16_rne(x.z) | ((uint32_t)f32_to_bf16_rne(x.w) << 16);
		o.z = f32_to_bf16_rne(y.x) | ((uint32_t)f32_to_bf16_rne(y.y) << 16);
		o.w = f32_to_bf16_rne(y.z) | ((uint32_t)f32_to_bf16_rne(y.w) << 16);
		*(uint4*)d = o;
	} else {
		for (int j = 0; j < 8 && c0 + j < cols; ++j) d[j] = f32_to_bf16_rne(s[j]);
	}
}

__global__ __launch_bounds__(256) void bf16_to_f32_kernel(const uint16_t* src, long ld_src, float* dst, long ld_dst, int rows, int cols, int vec) {
	const int chunks = (cols + 7) >> 3;
	const long id = (long)blockIdx.x * 256 + threadIdx.x;
	if (id >= (long)rows * chunks) return;
	const int r = (int)(id / chunks), c0 = (int)(id % chunks) * 8;
	const uint16_t* s = src + r * ld_src + c0;
	float* d = dst + r * ld_dst + c0;
	if (vec && c0 + 8 <= cols) {
		const uint4 x = *(const uint4*)s;
		*(float4*)d = make_float4(__uint_as_float(x.x << 16), __uint_as_float(x.x & 0xffff0000u), __uint_as_float(x.y << 16), __uint_as_float(x.y & 0xffff0000u));
		*(float4*)(d + 4) = make_float4(__uint_as_float(x.z << 16), __uint_as_float(x.z & 0xffff0000u), __uint_as_float(x.w << 16), __uint_as_float(x.w & 0xffff0000u));
	} else {
		for (int j = 0; j < 8 && c0 + j < cols; ++j) d[j] = bf16_to_f32(s[j]);
	}
}

// ---- 16-bit transpose: 64 x 64 tiles through LDS; a thread moves two 8-element chunks in, two out -------------------------------------------------
constexpr int TT = 64, TP = TT + 8;   // rows of 144 bytes: 16-byte aligned chunks, and a column walk that moves 36 banks per row
__global__ __launch_bounds__(256) void transpose_b16_kernel(const uint16_t* src, long ld_src, uint16_t* dst, long ld_dst, int rows, int cols, int vec_src, int vec_dst) {
	__shared__ __attribute__((aligned(16))) uint16_t tile[TT][TP];
	const int r0 = blockIdx.y * TT, c0 = blockIdx.x * TT;
#pragma unroll
	for (int q = 0; q < 2; ++q) {
		const int id = threadIdx.x + q * 256, tr = id >> 3, tc = (id & 7) * 8;
		const int r = r0 + tr, c = c0 + tc;
		if (r < rows && c < cols) {
			const uint16_t* s = src + r * ld_src + c;
			if (vec_src && c + 8 <= cols) *(uint4*)&tile[tr][tc] = *(const uint4*)s;
			else for (int j = 0; j < 8 && c + j < cols; ++j) tile[tr][tc + j] = s[j];
		}
	}
	__syncthreads();
#pragma unroll
	for (int q = 0; q < 2; ++q) {
		const int id = threadIdx.x + q * 256, tc = id >> 3, tr = (id & 7) * 8;   // output row = source column c0 + tc, output columns = source rows r0 + tr ...
		const int c = c0 + tc, r = r0 + tr;
		if (c < cols && r < rows) {
			uint16_t* d = dst + c * ld_dst + r;
			if (vec_dst && r + 8 <= rows) {
				uint4 o;
				o.x = tile[tr + 0][tc] | ((uint32_t)tile[tr + 1][tc] << 16);
				o.y = tile[tr + 2][tc] | ((uint32_t)tile[tr + 3][tc] << 16);
				o.z = tile[tr + 4][tc] | ((uint32_t)tile[tr + 5][tc] << 16);
				o.w = tile[tr + 6][tc] | ((uint32_t)tile[tr + 7][tc] << 16);
				*(uint4*)d = o;
			} else for (int j = 0; j < 8 && r + j < rows; ++j) d[j] = tile[tr + j][tc];
		}
	}
}

bla_status window_args(const void* src, long ld_src, const void* dst, long ld_dst, int rows, int cols, const char* who) {
	BLA_REQUIRE(rows >= 0 && cols >= 0, BLA_ERR_INVALID, "%s: negative extent %d x %d", who, rows, cols);
	if (rows == 0 || cols == 0) return BLA_OK;
	BLA_REQUIRE(src && dst, BLA_ERR_INVALID, "%s: NULL pointer", who);
	BLA_REQUIRE(ld_src >= cols, BLA_ERR_INVALID, "%s: ld_src %ld < cols %d", who, ld_src, cols);
	return BLA_OK;
}

bla_status launch_f32_to_bf16(hipStream_t s, const float* src, int ld_src, uint16_t* dst, int ld_dst, int rows, int cols) {
	const long n = (long)rows * ((cols + 7) / 8);
	if (n == 0) return BLA_OK;
	const int vec = aligned16(src) && ld_src % 4 == 0 && aligned16(dst) && ld_dst % 8 == 0;
	hipLaunchKernelGGL(f32_to_bf16_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, (long)ld_src, dst, (long)ld_dst, rows, cols, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status launch_transpose(hipStream_t s, const uint16_t* src, int ld_src, uint16_t* dst, int ld_dst, int rows, int cols) {
	if (rows == 0 || cols == 0) return BLA_OK;
	const int vs = aligned16(src) && ld_src % 8 == 0, vd = aligned16(dst) && ld_dst % 8 == 0;
	BLA_REQUIRE((rows + TT - 1) / TT <= 65535, BLA_ERR_INVALID, "bla_transpose_b16: %d rows exceed the grid", rows);
	hipLaunchKernelGGL(transpose_b16_kernel, dim3((cols + TT - 1) / TT, (rows + TT - 1) / TT), dim3(256), 0, s, src, (long)ld_src, dst, (long)ld_dst, rows, cols, vs, vd);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

// the fields of the epilogue a bf16 product honours; everything else must be off.  A pure argument check: it runs before the device is asked for.
bla_status check_epilogue(const bla_gemm_epilogue* ep) {
	if (!ep) return BLA_OK;
	BLA_REQUIRE(!ep->pre_act && ep->ld_pre == 0 && !ep->relu_mask && ep->ld_mask == 0 && !ep->row_sum_a && !ep->softmax_y && ep->softmax_scale == 0.f &&
	            !ep->softmax_grad && ep->row_sum_alpha == 0.f && ep->row_sum_beta == 0.f && !ep->softmax_loss_acc && !ep->softmax_correct_acc,
	            BLA_ERR_INVALID, "bla_gemm_bf16: the epilogue sets a field other than alpha, beta, bias_row, bias_col, act");
	BLA_REQUIRE(ep->act == BLA_ACT_NONE || ep->act == BLA_ACT_RELU, BLA_ERR_INVALID, "bla_gemm_bf16: act %d", ep->act);
	return BLA_OK;
}

bla_status check_product(int m, int n, int k, const void* A, int lda, int transa, const void* B, int ldb, int transb, const void* C, int ldc) {
	BLA_REQUIRE(m >= 0 && n >= 0 && k >= 0, BLA_ERR_INVALID, "bla_gemm_bf16: negative extent m %d n %d k %d", m, n, k);
	if (m == 0 || n == 0) return BLA_OK;
	BLA_REQUIRE(C && (k == 0 || (A && B)), BLA_ERR_INVALID, "bla_gemm_bf16: NULL operand");
	BLA_REQUIRE(lda >= (transa ? m : k) && ldb >= (transb ? k : n) && ldc >= n, BLA_ERR_INVALID, "bla_gemm_bf16: pitch too small (lda %d ldb %d ldc %d)", lda, ldb, ldc);
	return BLA_OK;
}

bool fast_path(int k, const void* A, int lda, const void* B, int ldb) {
	return k > 0 && k % 8 == 0 && aligned16(A) && aligned16(B) && lda % 8 == 0 && ldb % 8 == 0;
}
// bytes of the transposed copies a fast-path product puts into the workspace
size_t tcopy_bytes(bool fast, int transa, int transb, int m, int n, int k) {
	if (m == 0 || n == 0 || !fast) return 0;
	return (transa ? round_up((size_t)m * k * 2, 256) : 0) + (!transb ? round_up((size_t)n * k * 2, 256) : 0);
}

// ---- the K-split's plan: pure functions of the shape (include/bla.h states both rules) -----------------------------------------------------------
struct SplitPlan { int eff, sps; size_t partial_bytes; };

// the automatic rule: the number of splits to ask the partition rule for
int auto_splits(long tiles, int slabs, int cus) {
	const long slots = 3L * (cus > 0 ? cus : 256);   // three workgroups share a CU at the kernel's registers and LDS
	if (tiles >= slots || slabs < 2 * BLA_GEMM_BF16_SPLITK_MIN_SLABS) return 1;
	const long by_slots = slots / tiles, by_slabs = slabs / BLA_GEMM_BF16_SPLITK_MIN_SLABS;
	return (int)(by_slots < by_slabs ? by_slots : by_slabs);
}

SplitPlan split_plan(int m, int n, int k, int splits, int cus) {
	const long tiles = (long)((m + BM - 1) / BM) * ((n + BN - 1) / BN);
	const int slabs = (k + BK - 1) / BK;
	SplitPlan p{1, slabs, 0};
	if (tiles == 0 || slabs == 0) return p;
	int S = splits == 0 ? auto_splits(tiles, slabs, cus) : splits;
	S = S < 1 ? 1 : (S > slabs ? slabs : S);
	p.sps = (slabs + S - 1) / S;
	p.eff = (slabs + p.sps - 1) / p.sps;   // no split is empty
	if (p.eff > 1) p.partial_bytes = (size_t)p.eff * (size_t)tiles * (BM * BN * sizeof(float));
	return p;
}

}  // namespace

// the product itself; ws holds tcopy_bytes() bytes (16-byte aligned)
bla_status gemm_bf16_launch(hipStream_t s, int transa, int transb, int m, int n, int k, const uint16_t* A, int lda, const uint16_t* B, int ldb, void* C, int ldc,
                            int c_type, const bla_gemm_epilogue* ep, unsigned char* ws) {
	return gemm_bf16_launch_splitk(s, transa, transb, m, n, k, A, lda, B, ldb, C, ldc, c_type, ep, ws, 1);
}

size_t gemm_bf16_splitk_partial_bytes(int m, int n, int k, int splits) { return split_plan(m, n, k, splits, ctx().num_cus).partial_bytes; }

// the same with the contraction cut into `splits` ranges (0: the automatic rule for the context's CUs; 1: exactly the launch above); ws holds
// tcopy_bytes() bytes and, behind them at the next multiple of 256, the plan's partial_bytes
bla_status gemm_bf16_launch_splitk(hipStream_t s, int transa, int transb, int m, int n, int k, const uint16_t* A, int lda, const uint16_t* B, int ldb, void* C, int ldc,
                                   int c_type, const bla_gemm_epilogue* ep, unsigned char* ws, int splits) {
	if (m == 0 || n == 0) return BLA_OK;
	Bf16Args a{};
	a.C = C; a.m = m; a.n = n; a.k = k; a.ldc = ldc;
	a.alpha = ep ? ep->alpha : 1.f; a.beta = ep ? ep->beta : 0.f;
	a.bias_row = ep ? ep->bias_row : nullptr; a.bias_col = ep ? ep->bias_col : nullptr;
	a.relu = ep && ep->act == BLA_ACT_RELU;
	char name[96];
	const char* lay = transa ? (transb ? "tt" : "tn") : (transb ? "nt" : "nn");
	const char* ct = c_type == BLA_C_BF16 ? "bf16" : "f32";
	if (fast_path(k, A, lda, B, ldb)) {
		if (transa) {   // A stored k x m -> m x k
			BLA_REQUIRE(ws, BLA_ERR_INVALID, "bla_gemm_bf16: no workspace");
			bla_status st = launch_transpose(s, A, lda, (uint16_t*)ws, k, k, m);
			if (st != BLA_OK) return st;
			A = (const uint16_t*)ws; lda = k; ws += round_up((size_t)m * k * 2, 256);
		}
		if (!transb) {  // B stored k x n -> n x k
			BLA_REQUIRE(ws, BLA_ERR_INVALID, "bla_gemm_bf16: no workspace");
			bla_status st = launch_transpose(s, B, ldb, (uint16_t*)ws, k, k, n);
			if (st != BLA_OK) return st;
			B = (const uint16_t*)ws; ldb = k; ws += round_up((size_t)n * k * 2, 256);
		}
		a.A = A; a.B = B; a.lda = lda; a.ldb = ldb; a.zero = zero_word();
		a.tiles_m = (m + BM - 1) / BM; a.tiles_n = (n + BN - 1) / BN;
		const long tiles = (long)a.tiles_m * a.tiles_n;
		const SplitPlan plan = split_plan(m, n, k, splits, ctx().num_cus);
		if (plan.eff == 1) {
			const dim3 grid((unsigned)tiles);
			if (c_type == BLA_C_BF16) hipLaunchKernelGGL((gemm_bf16_nt_kernel<true, false>), grid, dim3(256), 2 * SLAB_BYTES, s, a);
			else hipLaunchKernelGGL((gemm_bf16_nt_kernel<false, false>), grid, dim3(256), 2 * SLAB_BYTES, s, a);
			BLA_HIP(hipGetLastError());
			snprintf(name, sizeof name, "gemm_bf16_mfma128x128x64_%s_%s%s%s", lay, ct, transa ? "_tcopyA" : "", !transb ? "_tcopyB" : "");
		} else {
			BLA_REQUIRE(ws, BLA_ERR_INVALID, "bla_gemm_bf16_splitk: no workspace");
			const long quads = (long)m * ((n + 3) / 4);
			BLA_REQUIRE(tiles * plan.eff < (1L << 31) && (quads + 255) / 256 < (1L << 31), BLA_ERR_INVALID, "bla_gemm_bf16_splitk: %ld tiles x %d splits exceed the grid", tiles, plan.eff);
			a.partial = (float*)ws; a.sps = plan.sps;
			hipLaunchKernelGGL((gemm_bf16_nt_kernel<false, true>), dim3((unsigned)(tiles * plan.eff)), dim3(256), 2 * SLAB_BYTES, s, a);
			BLA_HIP(hipGetLastError());
			const dim3 fold((unsigned)((quads + 255) / 256));
			if (c_type == BLA_C_BF16) hipLaunchKernelGGL(gemm_bf16_fold_kernel<true>, fold, dim3(256), 0, s, a, plan.eff);
			else hipLaunchKernelGGL(gemm_bf16_fold_kernel<false>, fold, dim3(256), 0, s, a, plan.eff);
			BLA_HIP(hipGetLastError());
			snprintf(name, sizeof name, "gemm_bf16_mfma128x128x64_%s_%s%s%s_splitk%d", lay, ct, transa ? "_tcopyA" : "", !transb ? "_tcopyB" : "", plan.eff);
		}
	} else {
		a.A = A; a.B = B;
		a.sa_r = transa ? 1 : lda; a.sa_k = transa ? lda : 1;
		a.sb_k = transb ? 1 : ldb; a.sb_c = transb ? ldb : 1;
		BLA_REQUIRE((m + 15) / 16 <= 65535, BLA_ERR_INVALID, "bla_gemm_bf16: m %d exceeds the general kernel's grid", m);
		const dim3 grid((n + 15) / 16, (m + 15) / 16);
		if (c_type == BLA_C_BF16) hipLaunchKernelGGL(gemm_bf16_general_kernel<true>, grid, dim3(256), 0, s, a);
		else hipLaunchKernelGGL(gemm_bf16_general_kernel<false>, grid, dim3(256), 0, s, a);
		BLA_HIP(hipGetLastError());
		snprintf(name, sizeof name, "gemm_bf16_general_%s_%s", lay, ct);
	}
	gemm_note_last_kernel(name);
	return BLA_OK;
}

}  // namespace bla

using namespace bla;

extern "C" {

bla_status bla_f32_to_bf16(void* stream, const float* d_src, int ld_src, uint16_t* d_dst, int ld_dst, int rows, int cols) {
	bla_status st = require_ready();
	if (st != BLA_OK) return st;
	st = window_args(d_src, ld_src, d_dst, ld_dst, rows, cols, "bla_f32_to_bf16");
	if (st != BLA_OK) return st;
	BLA_REQUIRE(ld_dst >= cols, BLA_ERR_INVALID, "bla_f32_to_bf16: ld_dst %d < cols %d", ld_dst, cols);
	return launch_f32_to_bf16(pick_stream(stream), d_src, ld_src, d_dst, ld_dst, rows, cols);
}

bla_status bla_bf16_to_f32(void* stream, const uint16_t* d_src, int ld_src, float* d_dst, int ld_dst, int rows, int cols) {
	bla_status st = require_ready();
	if (st != BLA_OK) return st;
	st = window_args(d_src, ld_src, d_dst, ld_dst, rows, cols, "bla_bf16_to_f32");
	if (st != BLA_OK) return st;
	BLA_REQUIRE(ld_dst >= cols, BLA_ERR_INVALID, "bla_bf16_to_f32: ld_dst %d < cols %d", ld_dst, cols);
	const long n = (long)rows * ((cols + 7) / 8);
	if (n == 0) return BLA_OK;
	const int vec = aligned16(d_src) && ld_src % 8 == 0 && aligned16(d_dst) && ld_dst % 4 == 0;
	hipLaunchKernelGGL(bf16_to_f32_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, pick_stream(stream), d_src, (long)ld_src, d_dst, (long)ld_dst, rows, cols, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_transpose_b16(void* stream, const uint16_t* d_src, int ld_src, uint16_t* d_dst, int ld_dst, int rows, int cols) {
	bla_status st = require_ready();
	if (st != BLA_OK) return st;
	st = window_args(d_src, ld_src, d_dst, ld_dst, rows, cols, "bla_transpose_b16");
	if (st != BLA_OK) return st;
	BLA_REQUIRE(ld_dst >= rows, BLA_ERR_INVALID, "bla_transpose_b16: ld_dst %d < rows %d", ld_dst, rows);
	return launch_transpose(pick_stream(stream), d_src, ld_src, d_dst, ld_dst, rows, cols);
}

bla_status bla_gemm_bf16(void* stream, int transa, int transb, int m, int n, int k, const uint16_t* d_a, int lda, const uint16_t* d_b, int ldb,
                         void* d_c, int ldc, int c_type, const bla_gemm_epilogue* ep) {
	bla_status st = check_epilogue(ep);
	if (st != BLA_OK) return st;
	BLA_REQUIRE(c_type == BLA_C_F32 || c_type == BLA_C_BF16, BLA_ERR_INVALID, "bla_gemm_bf16: c_type %d", c_type);
	st = require_ready();
	if (st != BLA_OK) return st;
	transa = transa != 0; transb = transb != 0;
	st = check_product(m, n, k, d_a, lda, transa, d_b, ldb, transb, d_c, ldc);
	if (st != BLA_OK) return st;
	void* ws = nullptr;
	const size_t need = tcopy_bytes(fast_path(k, d_a, lda, d_b, ldb), transa, transb, m, n, k);
	if (need) {
		st = ensure_workspace(need, &ws);
		if (st != BLA_OK) return st;
	}
	return gemm_bf16_launch(pick_stream(stream), transa, transb, m, n, k, d_a, lda, d_b, ldb, d_c, ldc, c_type, ep, (unsigned char*)ws);
}

bla_status bla_gemm_bf16_splitk_plan(int m, int n, int k, int splits, int cus, int* eff_splits, int* slabs_per_split, size_t* partial_bytes) {
	BLA_REQUIRE(m >= 0 && n >= 0 && k >= 0 && splits >= 0, BLA_ERR_INVALID, "bla_gemm_bf16_splitk_plan: negative argument (m %d n %d k %d splits %d)", m, n, k, splits);
	const SplitPlan p = split_plan(m, n, k, splits, cus);
	if (eff_splits) *eff_splits = p.eff;
	if (slabs_per_split) *slabs_per_split = p.sps;
	if (partial_bytes) *partial_bytes = p.partial_bytes;
	return BLA_OK;
}

bla_status bla_gemm_bf16_splitk(void* stream, int transa, int transb, int m, int n, int k, const uint16_t* d_a, int lda, const uint16_t* d_b, int ldb,
                                void* d_c, int ldc, int c_type, const bla_gemm_epilogue* ep, int splits) {
	BLA_REQUIRE(splits >= 0, BLA_ERR_INVALID, "bla_gemm_bf16_splitk: splits %d", splits);
	bla_status st = check_epilogue(ep);
	if (st != BLA_OK) return st;
	BLA_REQUIRE(c_type == BLA_C_F32 || c_type == BLA_C_BF16, BLA_ERR_INVALID, "bla_gemm_bf16_splitk: c_type %d", c_type);
	st = require_ready();
	if (st != BLA_OK) return st;
	transa = transa != 0; transb = transb != 0;
	st = check_product(m, n, k, d_a, lda, transa, d_b, ldb, transb, d_c, ldc);
	if (st != BLA_OK) return st;
	void* ws = nullptr;
	const bool fast = fast_path(k, d_a, lda, d_b, ldb);
	const size_t need = tcopy_bytes(fast, transa, transb, m, n, k) + (fast ? gemm_bf16_splitk_partial_bytes(m, n, k, splits) : 0);   // off the fast path nothing is split
	if (need) {
		st = ensure_workspace(need, &ws);
		if (st != BLA_OK) return st;
	}
	return gemm_bf16_launch_splitk(pick_stream(stream), transa, transb, m, n, k, d_a, lda, d_b, ldb, d_c, ldc, c_type, ep, (unsigned char*)ws, splits);
}

bla_status bla_gemm_f32_as_bf16(void* stream, int transa, int transb, int m, int n, int k, const float* d_a, int lda, const float* d_b, int ldb,
                                float* d_c, int ldc, const bla_gemm_epilogue* ep) {
	bla_status st = check_epilogue(ep);
	if (st != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	transa = transa != 0; transb = transb != 0;
	st = check_product(m, n, k, d_a, lda, transa, d_b, ldb, transb, d_c, ldc);
	if (st != BLA_OK) return st;
	if (m == 0 || n == 0) return BLA_OK;
	// the bf16 operands keep their layout, at a pitch rounded up to 8 elements, in front of the transposed copies the product may add
	const int ar = transa ? k : m, ac = transa ? m : k, br = transb ? n : k, bc = transb ? k : n;
	const int la = (int)round_up((size_t)ac, 8), lb = (int)round_up((size_t)bc, 8);
	const size_t a_bytes = round_up((size_t)ar * la * 2, 256), b_bytes = round_up((size_t)br * lb * 2, 256);
	// the workspace is 256-byte aligned and both pitches are multiples of 8: the product takes the fast path whenever k allows it
	void* ws = nullptr;
	st = ensure_workspace(a_bytes + b_bytes + tcopy_bytes(k > 0 && k % 8 == 0, transa, transb, m, n, k), &ws);
	if (st != BLA_OK) return st;
	unsigned char* base = (unsigned char*)ws;
	uint16_t* a16 = (uint16_t*)base;
	uint16_t* b16 = (uint16_t*)(base + a_bytes);
	hipStream_t s = pick_stream(stream);
	if (k > 0) {
		st = launch_f32_to_bf16(s, d_a, lda, a16, la, ar, ac);
		if (st != BLA_OK) return st;
		st = launch_f32_to_bf16(s, d_b, ldb, b16, lb, br, bc);
		if (st != BLA_OK) return st;
	}
	return gemm_bf16_launch(s, transa, transb, m, n, k, a16, la, b16, lb, d_c, ldc, BLA_C_F32, ep, base + a_bytes + b_bytes);
}

}  // extern "C"
