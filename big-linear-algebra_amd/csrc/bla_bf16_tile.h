// bla_bf16_tile.h -- the 128 x 128 x 64 bf16 tile (fp32 accumulation on v_mfma_f32_32x32x16_bf16), device side, once: bla_gemm_bf16.hip's product and
// bla_conv_bf16.hip's gathered product are both this tile around a B source, a K range and a visitor of the accumulators.  A second slab loop,
// bf16_tile_product_kmajor, takes both operands K-MAJOR (the implicit weight gradient): the same tile, pieces, barriers and accumulator map around
// transposed LDS reads.
//
// The plain LDS-DMA structure: a 128 x 128 output tile per 256-thread workgroup, 64-deep K slabs, one 32 KiB LDS image, two barriers per slab (stage,
// wait, barrier, multiply, barrier); several workgroups per CU overlap one another's staging.
//   * Both operands K-contiguous (A [m][k], B [n][k]).  A slab of an operand is 128 rows x 128 bytes; wave w's i-th global_load_lds_dwordx4 fills the 1 KiB
//     piece (4w + i) = 8 rows, lane l -> row l >> 3, 16-byte chunk l & 7.  The LDS image stays lane-linear (the DMA writes base + 16 * lane); the swizzle is
//     on the SOURCE address: LDS chunk c of row r holds global chunk c ^ ((r >> 1) & 7), and the fragment reads apply the same XOR.  With 128-byte rows two
//     rows share a 256-byte bank row, so the 16 rows a ds_read_b128 lane group reads land on 16 different 16-byte slots.
//   * Edges: a lane whose row is past m (n) or whose chunk is past k fetches from 256 bytes of zeros the context keeps (zero_word()); no address outside
//     the operands is ever formed into a load.  k % 8 == 0 makes every chunk wholly inside or wholly outside.  Stores are bounds-checked by the visitor.
//   * v_mfma_f32_32x32x16_bf16: lane l holds A[row l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][col l & 31], j < 8 -- one 16-byte chunk each;
//     C/D: col = l & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).  Each wave owns 64 x 64 = 2 x 2 such tiles.
//   * Workgroup -> tile: XCD-aware (the 8 XCDs take contiguous chunks of the tile order), then groups of 8 tile rows walked column by column.
//
// What a kernel supplies:
//   * the B source: b_at(piece i, kb) = the address of this lane's 16-byte chunk of B for piece i of the slab at kb, valid whenever the lane's B row is
//     inside n and its chunk inside k (bf16_tile_product asks for it regardless and discards it otherwise, so it must not load).  A dense B [n][k] answers
//     pb[i] + kb; the convolution derives a tap offset.  The A operand is dense in every kernel and staged here.
//   * the K range [k_begin, k_end), a multiple of BK from a multiple of BK (the K-split hands every workgroup its slabs);
//   * what happens to an accumulator element: loops of its own over acc[i][j][r], placed by bf16_acc_row(i, r) and bf16_acc_col(j).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace bla {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

__device__ __forceinline__ uint16_t f32_to_bf16_rne(float f) {   // bla_f32_to_bf16's rounding
	uint32_t u = __float_as_uint(f);
	if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);   // NaN stays NaN
	return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}
__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ __forceinline__ uint32_t pack2(float a, float b) { return f32_to_bf16_rne(a) | ((uint32_t)f32_to_bf16_rne(b) << 16); }

constexpr int BM = 128, BN = 128, BK = 64, SLAB_BYTES = BM * BK * 2;   // a launch asks for 2 * SLAB_BYTES of dynamic LDS: [A slab 16 KiB][B slab 16 KiB]

// ---- workgroup -> tile ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int xcd_tile(int bid, int nwg) {   // bijective for any count
	int q = nwg >> 3, r = nwg & 7, x = bid & 7, i = bid >> 3;
	return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

struct Bf16Tile { int tm, tn; };
__device__ __forceinline__ Bf16Tile bf16_tile_of(int bid, int tiles_m, int tiles_n) {
	const int pid = xcd_tile(bid, tiles_m * tiles_n);
	const int gsz = 8 * tiles_n, first = pid / gsz * 8, gm = min(tiles_m - first, 8);   // the last group may hold fewer than 8 tile rows
	return {first + (pid % gsz) % gm, (pid % gsz) / gm};
}

// ---- piece -> row and chunk -------------------------------------------------------------------------------------------------------------------------
// piece i (< 4) of a wave: this lane's row within the slab, and the global 16-byte chunk of that row it fetches (first k of the chunk = 8 * chunk).
// The swizzle term (row >> 1) & 7 is 4 (i & 1) + (lane >> 4): pieces i and i + 2 share the chunk, so a lane has only two distinct k offsets per slab.
__device__ __forceinline__ int bf16_piece_row(int wave, int lane, int i) { return (wave * 4 + i) * 8 + (lane >> 3); }
__device__ __forceinline__ int bf16_piece_chunk(int lane, int i) { return (lane & 7) ^ (4 * (i & 1) + (lane >> 4)); }

__device__ __forceinline__ void bf16_stage16(const void* src, unsigned char* lds_piece) {   // 64 lanes x 16 bytes -> lds_piece + 16 * lane
	__builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)lds_piece, 16, 0, 0);
}

// ---- the slab loop ----------------------------------------------------------------------------------------------------------------------------------
// acc = A[row0 .. row0 + 128)[k_begin .. k_end) . B[col0 .. col0 + 128)[k_begin .. k_end)^T; rows past m, columns past n and k past k contribute zeros.
struct Bf16TileOperands { const uint16_t* A; int lda, m, n, k, row0, col0; const void* zero; };

template <class BSource>
__device__ __forceinline__ void bf16_tile_product(unsigned char* lds, const Bf16TileOperands& t, int k_begin, int k_end, BSource&& b_at, f32x16 (&acc)[2][2]) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint16_t* pa[4];
	bool oka[4], okb[4];
	int kc[2];   // first k of the chunk this lane fetches: piece i takes kc[i & 1]
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int row = bf16_piece_row(wave, lane, i);
		if (i < 2) kc[i] = bf16_piece_chunk(lane, i) * 8;
		oka[i] = t.row0 + row < t.m;
		okb[i] = t.col0 + row < t.n;
		pa[i] = t.A + (size_t)(oka[i] ? t.row0 + row : 0) * t.lda + kc[i & 1];
	}
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

	const int wm = wave >> 1, wn = wave & 1, fr = lane & 31, fh = lane >> 5;
	for (int kb = k_begin; kb < k_end; kb += BK) {
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const bool in = kb + kc[i & 1] < t.k;
			const void* a = pa[i] + kb;
			const void* b = b_at(i, kb);   // formed in front of the choice, not inside it: a select per address, no branch among the DMAs
			bf16_stage16((oka[i] && in) ? a : t.zero, lds + (wave * 4 + i) * 1024);
			bf16_stage16((okb[i] && in) ? b : t.zero, lds + SLAB_BYTES + (wave * 4 + i) * 1024);
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
#pragma unroll
		for (int s = 0; s < BK / 16; ++s) {
			bf16x8 fa[2], fb[2];
			const int g = 2 * s + fh;
#pragma unroll
			for (int i = 0; i < 2; ++i) {
				const int ra = wm * 64 + i * 32 + fr, rb = wn * 64 + i * 32 + fr;
				fa[i] = *(const bf16x8*)(lds + ra * 128 + ((g ^ ((ra >> 1) & 7)) << 4));
				fb[i] = *(const bf16x8*)(lds + SLAB_BYTES + rb * 128 + ((g ^ ((rb >> 1) & 7)) << 4));
			}
#pragma unroll
			for (int i = 0; i < 2; ++i)
#pragma unroll
				for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
		}
		__syncthreads();
	}
}

// ---- the slab loop, both operands K-MAJOR -----------------------------------------------------------------------------------------------
// acc = A[k_begin .. k_end)[row0 .. row0 + 128)^T . B[k_begin .. k_end)[col0 .. col0 + 128): both operands are stored [k][column] with the columns
// contiguous (the implicit weight gradient contracts over pixels and both its operands are channel-last), and the MFMA fragments -- 8 consecutive k of
// one column -- come out of LDS through the transposed read ds_read_b64_tr_b16.
//   * A slab of an operand is [64 k-rows][128 columns] = 256-byte rows, 16 KiB, 16 pieces of 1 KiB = 4 k-rows; wave w issues pieces 4w + i.  The DMA is
//     lane-linear: lane l of piece pc fills row r = 4 pc + (l >> 4), 16-byte slot l & 15.  The swizzle is again on the SOURCE address: slot c of row r
//     holds global chunk c ^ x(r), x(r) = ((r & 3) << 2) | ((r >> 2) & 3) = ((l >> 4) << 2) | i, so a lane's column chunk per piece is a loop constant
//     and what moves from slab to slab is its k-row.  off(row, ch) = 256 row + 16 (ch ^ x(row)).
//   * Fragment of k-step s (< 4) for the 32-column block at chunk cb: lane L needs column L & 31 at k = 16 s + 8 (L >> 5) + j, j < 8: two transposed
//     reads t = 0, 1 of the 4-row x 16-column block at row r0 = 16 s + 8 (L >> 5) + 4 t, chunk c0 = cb + 2 ((L >> 4) & 1); with L & 15 = 4 q + p the lane
//     supplies off(r0 + q, c0 + (p >> 1)) + 8 (p & 1) and receives column L & 15 of the block, row q in element q: read t is fragment elements 4t .. 4t+3.
//     x(r0 + q) = (q << 2) | (2 (L >> 5) + t) does not depend on s: a lane has one address per (block, t) and adds 4096 s.  A and B are read the same
//     way, so their k order agrees by construction.  Every lane of every wave reads (no lane-dependent branch: the instruction needs EXEC all ones).
//   * Edges as above: a chunk whose first column is at or past m (n), or whose k-row is at or past k, comes from the zero word.  m % 8 == 0 and n % 8 == 0
//     make every chunk wholly inside or wholly outside.
// What a kernel supplies: a_at(piece i, kb) and b_at(piece i, kb) = the address of this lane's 16-byte chunk of A (B) for piece i of the slab at kb,
// i.e. k-row kb + bf16_kmajor_row(wave, lane, i), first column row0 (col0) + 8 bf16_kmajor_chunk(lane, i); asked for regardless, so they must not load.
// next_slab() runs once per slab, behind its eight DMAs and in front of the wait for them: a kernel whose sources keep per-slab state (the convolution's
// pixel offsets) moves it on there, under the loads' latency; kb rises by BK from k_begin.
__device__ __forceinline__ int bf16_kmajor_row(int wave, int lane, int i) { return (wave * 4 + i) * 4 + (lane >> 4); }
__device__ __forceinline__ int bf16_kmajor_chunk(int lane, int i) { return (lane & 15) ^ (((lane >> 4) << 2) | i); }

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16x8 bf16_kmajor_fragment(unsigned char* lds, int off0, int off1) {   // the two transposed reads of one fragment
	const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + off0));
	const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(lds + off1));
	const s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
	return __builtin_bit_cast(bf16x8, v);
}

struct Bf16KmajorOperands { int m, n, k, row0, col0; const void* zero; };   // m, n: the operands' column extents, multiples of 8; k: their k-rows

template <class ASource, class BSource, class NextSlab>
__device__ __forceinline__ void bf16_tile_product_kmajor(unsigned char* lds, const Bf16KmajorOperands& t, int k_begin, int k_end, ASource&& a_at, BSource&& b_at,
                                                         NextSlab&& next_slab, f32x16 (&acc)[2][2]) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	bool oka[4], okb[4];
	int kr[4];   // this lane's k-row within the slab, per piece
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		kr[i] = bf16_kmajor_row(wave, lane, i);
		oka[i] = t.row0 + bf16_kmajor_chunk(lane, i) * 8 < t.m;
		okb[i] = t.col0 + bf16_kmajor_chunk(lane, i) * 8 < t.n;
	}
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

	// the fragment addresses at k-step 0: [operand block i][read t]
	const int wm = wave >> 1, wn = wave & 1, fh = lane >> 5, g16 = (lane >> 4) & 1, q = (lane & 15) >> 2, p = lane & 3;
	int ra[2][2], rb[2][2];
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int tt = 0; tt < 2; ++tt) {
			const int row = 8 * fh + 4 * tt + q, x = (q << 2) | (2 * fh + tt);
			ra[i][tt] = 256 * row + 16 * ((wm * 8 + i * 4 + 2 * g16 + (p >> 1)) ^ x) + 8 * (p & 1);
			rb[i][tt] = SLAB_BYTES + 256 * row + 16 * ((wn * 8 + i * 4 + 2 * g16 + (p >> 1)) ^ x) + 8 * (p & 1);
		}

	for (int kb = k_begin; kb < k_end; kb += BK) {
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const bool in = kb + kr[i] < t.k;
			const void* a = a_at(i, kb);   // formed in front of the choice, not inside it: a select per address, no branch among the DMAs
			const void* b = b_at(i, kb);
			bf16_stage16((oka[i] && in) ? a : t.zero, lds + (wave * 4 + i) * 1024);
			bf16_stage16((okb[i] && in) ? b : t.zero, lds + SLAB_BYTES + (wave * 4 + i) * 1024);
		}
		next_slab();
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
#pragma unroll
		for (int s = 0; s < BK / 16; ++s) {
			bf16x8 fa[2], fb[2];
#pragma unroll
			for (int i = 0; i < 2; ++i) {
				fa[i] = bf16_kmajor_fragment(lds, ra[i][0] + 4096 * s, ra[i][1] + 4096 * s);
				fb[i] = bf16_kmajor_fragment(lds, rb[i][0] + 4096 * s, rb[i][1] + 4096 * s);
			}
#pragma unroll
			for (int i = 0; i < 2; ++i)
#pragma unroll
				for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
		}
		__syncthreads();
	}
}

// ---- accumulator register -> (row, column) in the tile ----------------------------------------------------------------------------------------------
// acc[i][j][r] is element (bf16_acc_row(i, r), bf16_acc_col(j)) of the tile: block (i, j) of the wave's 64 x 64 quadrant, of which a lane holds one
// column and 16 rows.  Lanes run along the columns, so a wave's store instruction writes runs of 32 consecutive columns of one row.  The loops over
// i, j, r are the kernel's own, because their order is measurable: the convolution goes column by column (j outside: image, pixel and bias pointer
// once per column), the dense product block row by block row (i outside) -- column by column its epilogue is 1 to 1.7 us slower per launch, and a
// visitor function called with the element cost it 16 more VGPRs.
__device__ __forceinline__ int bf16_acc_row(int i, int r) { return (threadIdx.x >> 7) * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * ((threadIdx.x & 63) >> 5); }
__device__ __forceinline__ int bf16_acc_col(int j) { return ((threadIdx.x >> 6) & 1) * 64 + j * 32 + (threadIdx.x & 31); }

}  // namespace bla
