// bla_mx_tile.h -- the 128 x 128 x 128 MXFP8 tile (e4m3 elements, E8M0 block scales, fp32 accumulation on v_mfma_scale_f32_32x32x64_f8f6f4), device
// side, once: bla_gemm_mxfp8.hip's product is this tile around a dense B source.  A sibling of bla_bf16_tile.h: the same workgroup, LDS
// image, pieces, DMA, source-side swizzle, edge handling, tile order and accumulator map; what differs is the depth of a slab in elements, the
// fragment a lane reads, and the scales.
//
//   * A 128 x 128 output tile per 256-thread workgroup, 128-deep K slabs: a slab of an operand is 128 rows x 128 BYTES = 16 KiB, the bf16 tile's bytes.
//     Wave w's i-th global_load_lds_dwordx4 fills the 1 KiB piece (4w + i) = 8 rows, lane l -> row l >> 3, 16-byte chunk l & 7 (bf16_piece_row /
//     bf16_piece_chunk, shared); LDS chunk c of row r holds global chunk c ^ ((r >> 1) & 7).  Two barriers per slab, one 32 KiB LDS image.
//   * Edges: a lane whose row is past m (n) or whose chunk is past k fetches from the zero word.  k % 32 == 0 makes every 16-byte chunk wholly inside
//     or wholly outside.  A zero element contributes +0 whatever its (finite) scale.
//   * v_mfma_scale_f32_32x32x64_f8f6f4 with e4m3 operands, VERIFIED with a one-wave probe on exact data (one-hot A against asymmetric integer B,
//     distinct power-of-two scales per row and block): lane l (r = l & 31, h = l >> 5) holds, in its 8 operand registers,
//         registers 0..3:  A[row r][k = 16 h + j],        j < 16
//         registers 4..7:  A[row r][k = 32 + 16 h + j],   j < 16
//     and B likewise by column: NOT 32 consecutive k.  A lane's 32 elements are two 16-byte chunks two chunks apart: chunk h and chunk 2 + h of the
//     64-deep step.  The scale byte the lane supplies (byte opsel of its scale register) scales k-block h of its row, i.e. k = 32 h .. 32 h + 31 --
//     which is NOT the 32 elements the lane itself holds: the block's elements sit half in this lane and half in lane l ^ 32.  C/D is the
//     dtype-independent 32 x 32 map (bf16_acc_row / bf16_acc_col).
//   * A slab is two such k-steps: step s reads chunks 4 s + h and 4 s + 2 + h of the lane's row (two swizzled ds_read_b128) and uses scale blocks
//     2 s + h.
//   * Scales: per slab a row has 4 scale bytes, one aligned dword, which each lane loads for its own 2 + 2 rows straight from global memory (both lane
//     halves read the same dword; the loads are issued with the slab's DMAs and used behind the barrier).  The lane shifts its dword right by 8 h, after
//     which byte 0 is block h and byte 2 is block 2 + h: opsel = 2 s is the same for all lanes.  Bytes at or beyond k / 32 (pitch padding) and the
//     dwords of rows past m (n) are replaced by 127 (scale 1) before use; the aligned dword that holds a valid byte never leaves the byte's page.
//
// What a kernel supplies: b_at(piece i, kb) = the address of this lane's 16-byte chunk of B for piece i of the slab at kb (asked for regardless, so it
// must not load), and sb_at(block j, kb) = the address of the scale dword of B row (wave's column block j, lane & 31) for the slab at kb, valid whenever
// that row is inside n.  A dense B answers pointer + kb and pointer + kb / 32; a gathered B would derive both from its tables.
#pragma once
#include "bla_bf16_tile.h"

namespace bla {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int MX_BK = 128, MX_BLOCK = 32;   // a slab's depth and the elements one scale byte covers; the slab's bytes are SLAB_BYTES

struct MxTileOperands { const uint8_t* A; const uint8_t* SA; int lda, ldsa, m, n, k, row0, col0; const void* zero; };

// the 4 scale bytes of one row for the slab at kb, as the MFMA reads them in lane half h: bytes past k / 32 -> 127, then >> 8 h
__device__ __forceinline__ int mx_scale_arrange(uint32_t d, bool row_ok, int blocks_left, int h) {
	const uint32_t keep = blocks_left >= 4 ? 0xffffffffu : (1u << (8 * blocks_left)) - 1u;
	d = row_ok ? (d & keep) | (0x7f7f7f7fu & ~keep) : 0x7f7f7f7fu;
	return (int)(d >> (8 * h));
}

template <class BSource, class BScale>
__device__ __forceinline__ void mx_tile_product(unsigned char* lds, const MxTileOperands& t, int k_begin, int k_end, BSource&& b_at, BScale&& sb_at, f32x16 (&acc)[2][2]) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint8_t* pa[4];
	bool oka[4], okb[4];
	int kc[2];   // first k of the chunk this lane fetches: piece i takes kc[i & 1]
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int row = bf16_piece_row(wave, lane, i);
		if (i < 2) kc[i] = bf16_piece_chunk(lane, i) * 16;
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
	const uint32_t* psa[2];
	bool oksa[2], oksb[2];
#pragma unroll
	for (int i = 0; i < 2; ++i) {
		const int ra = t.row0 + wm * 64 + i * 32 + fr;
		oksa[i] = ra < t.m;
		oksb[i] = t.col0 + wn * 64 + i * 32 + fr < t.n;
		psa[i] = (const uint32_t*)(t.SA + (size_t)(oksa[i] ? ra : 0) * t.ldsa);
	}
	for (int kb = k_begin; kb < k_end; kb += MX_BK) {
#pragma unroll
		for (int i = 0; i < 4; ++i) {
			const bool in = kb + kc[i & 1] < t.k;
			const void* a = pa[i] + kb;
			const void* b = b_at(i, kb);   // formed in front of the choice, not inside it: a select per address, no branch among the DMAs
			bf16_stage16((oka[i] && in) ? a : t.zero, lds + (wave * 4 + i) * 1024);
			bf16_stage16((okb[i] && in) ? b : t.zero, lds + SLAB_BYTES + (wave * 4 + i) * 1024);
		}
		uint32_t da[2], db[2];
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			da[i] = psa[i][kb >> 7];   // row 0's dword stands in for a row past m: in bounds, replaced below
			db[i] = *(oksb[i] ? sb_at(i, kb) : psa[0] + (kb >> 7));
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
		const int left = (t.k - kb) >> 5;
		int sa[2], sb[2];
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			sa[i] = mx_scale_arrange(da[i], oksa[i], left, fh);
			sb[i] = mx_scale_arrange(db[i], oksb[i], left, fh);
		}
#pragma unroll
		for (int s = 0; s < 2; ++s) {
			i32x8 fa[2], fb[2];
			const int g0 = 4 * s + fh, g1 = g0 + 2;
#pragma unroll
			for (int i = 0; i < 2; ++i) {
				const int ra = wm * 64 + i * 32 + fr, rb = wn * 64 + i * 32 + fr;
				const int xa = (ra >> 1) & 7, xb = (rb >> 1) & 7;
				const i32x4 a0 = *(const i32x4*)(lds + ra * 128 + ((g0 ^ xa) << 4)), a1 = *(const i32x4*)(lds + ra * 128 + ((g1 ^ xa) << 4));
				const i32x4 b0 = *(const i32x4*)(lds + SLAB_BYTES + rb * 128 + ((g0 ^ xb) << 4)), b1 = *(const i32x4*)(lds + SLAB_BYTES + rb * 128 + ((g1 ^ xb) << 4));
				fa[i] = __builtin_shufflevector(a0, a1, 0, 1, 2, 3, 4, 5, 6, 7);
				fb[i] = __builtin_shufflevector(b0, b1, 0, 1, 2, 3, 4, 5, 6, 7);
			}
#pragma unroll
			for (int i = 0; i < 2; ++i)
#pragma unroll
				for (int j = 0; j < 2; ++j) {
					if (s == 0) acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[j], acc[i][j], 0, 0, 0, sa[i], 0, sb[j]);
					else acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fa[i], fb[j], acc[i][j], 0, 0, 2, sa[i], 2, sb[j]);
				}
		}
		__syncthreads();
	}
}

}  // namespace bla
