// bla_gather_kernel.h -- the implicit-GEMM convolution kernels on the direct-to-LDS fp32 MFMA pipeline: one operand of the product is never stored but
// gathered from the image batch while a slab is fetched.  One 128 x 128 x 16 tile; the template is over what varies -- gather mode, older or half-slab
// form, window width.  From bla_gemm_kernel.h: the argument block's dense part, the tile walk, the LDS image of the stored operand.  Here: the gather
// fields, the pipeline loops as templates over the callables that fetch and read a slab, each mode's cursors, the image-shaped tile stores.
// Included by bla_gather.hip alone.
#pragma once
#include "bla_gemm_kernel.h"

namespace bla {

// register r of a 32x32 accumulator block in lane (l31, h): row (r & 3) + 8 (r >> 2) + 4 h of the block, column l31; block_row0: the block's first row
__device__ __forceinline__ int acc_row(int block_row0, int r, int h) { return block_row0 + (r & 3) + 8 * (r >> 2) + 4 * h; }

template <bool BKC>
struct HalfSlabFrags {   // 128 x 128 x 16 tile, 2 x 2 blocks per wave, A K-contiguous; B K-contiguous (mode 4) or row-contiguous (mode 3; mode 7 reads its own)
	static constexpr int BM = 128, BN = 128, BK = 16, TM = 2, TN = 2;
	typedef float v4f __attribute__((ext_vector_type(4)));
	typedef float vrb __attribute__((ext_vector_type(TN)));
	static constexpr int KK = BK / 8, UA = TM, UB = BKC ? TN : 4;   // fragment-read units per k-part and operand
	struct Frag {
		v4f ka[TM], kb[TN];   // K-contiguous: [block], elements = k-offset j
		vrb rb[4];            // row-contiguous: [k-offset j], elements = block -- a lane's two blocks are the columns w0 + 2 l31, + 1 (one 8-byte read)
		float sb[4][TN];      // mode 7: [k-offset j][block], one dword of the image window each
	};
	unsigned a_ad[KK], b_ad[KK];   // byte address in LDS buffer 0 of this lane's reads of k-part kk
	__device__ __forceinline__ HalfSlabFrags(unsigned lds0, int wm0, int wn0, int l31, int h) {
#pragma unroll
		for (int kk = 0; kk < KK; kk++) {
			a_ad[kk] = lds0 + KcImage<BM, BK>::off(wm0 + l31, kk * 2 + h) * 4;
			b_ad[kk] = lds0 + (BM * BK + (BKC ? KcImage<BN, BK>::off(wn0 + l31, kk * 2 + h) : (kk * 8 + 4 * h) * BN + wn0 + TN * l31)) * 4;
		}
	}
	__device__ static __forceinline__ float opa(const Frag& f, int im, int j) { return f.ka[im][j]; }
	__device__ static __forceinline__ float opb(const Frag& f, int in, int j) { return BKC ? f.kb[in][j] : f.rb[j][in]; }
	// read unit x of an operand's k-part kk in the buffer at byte offset buf
	__device__ __forceinline__ void read_a(unsigned buf, int kk, int x, Frag& f) const {
		const unsigned ad = buf + a_ad[kk];
		asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f.ka[x]) : "v"(ad), "n"(x * 32 * BK * 4));
	}
	__device__ __forceinline__ void read_b(unsigned buf, int kk, int x, Frag& f) const {
		const unsigned ad = buf + b_ad[kk];
		if constexpr (BKC) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(f.kb[x]) : "v"(ad), "n"(x * 32 * BK * 4));
		else asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(f.rb[x]) : "v"(ad), "n"(x * BN * 4));
	}
	// behind the s_waitcnt lgkmcnt(0) that every read into f has returned by: the empty statements make each register's later uses depend on the wait
	__device__ static __forceinline__ void land_a(Frag& f) {
#pragma unroll
		for (int x = 0; x < UA; x++) asm volatile("" : "+v"(f.ka[x]));
	}
	__device__ static __forceinline__ void land_b(Frag& f) {
#pragma unroll
		for (int x = 0; x < UB; x++) {
			if constexpr (BKC) asm volatile("" : "+v"(f.kb[x]));
			else asm volatile("" : "+v"(f.rb[x]));
		}
	}
};
// the idx-th MFMA of a k-part: j-major, then im, in; HF::opa / opb pick an operand out of a fragment set
template <class HF, int TM, int TN>
__device__ __forceinline__ void half_slab_mfma(f32x16 (&acc)[TM][TN], const typename HF::Frag& f, int idx) {
	const int j = idx / (TM * TN), im = (idx % (TM * TN)) / TN, in = idx % TN;
	acc[im][in] = __builtin_amdgcn_mfma_f32_32x32x2f32(HF::opa(f, im, j), HF::opb(f, in, j), acc[im][in], 0, 0, 0);
}
typedef __attribute__((address_space(3))) void* lds_ptr_t;
typedef const __attribute__((address_space(1))) void* gbl_ptr_t;

// Implicit-GEMM convolution over a batch of images: the B operand is never stored, element (k, n) is img[g_off(k) + g_off(n)] when
// (y(k) + y(n), x(k) + x(n)) lies inside the H x W image, else 0.
//   mode 1 (forward / data gradient): n = (image, output pixel), k = tap (c, p, q);  C is written as [image][M][HWo]
//   mode 2 (weight gradient):         n = tap,                   k = (image, output pixel);  A = del_y [image][M][HWo]
//   mode 3 (forward, stride 1, zero-PADDED image copy): as mode 1 without bounds checks, and four consecutive output pixels of a
//           row are four consecutive floats of the padded image: 16-byte DMA exactly like a dense row-contiguous operand
//   mode 4 (weight gradient, stride 1, padded copy), transposed: C'[tap][f] = sum_(image,pixel) P[tap][(image,pixel)] . del_y[f][(image,pixel)]:
//           both operands K-contiguous (the gathered one in 16-byte chunks of four pixels), B = del_y [image][N][HWo], the tile is
//           stored transposed (dkern [f][tap], or slab [split][f][tap])
//   mode 7 (forward / data gradient, 3x3, stride 1, image rows of 16 or 32 pixels, straight from the image): "im2col into LDS".  A tile is 128
//           consecutive pixels = 128 / W whole rows of ONE image.  The contraction runs k = (g * 9 + t) * 16 + c: channel group g (16 channels),
//           tap t, channel c of the group -- so the 9 slabs of a group all read the SAME 16 channel planes, and what sits in LDS is not the
//           im2col slab [16][128] but the image window itself: per channel the 128 / W + 2 rows the tile's taps touch (rows outside the image
//           from a zero word), 16 planes per group, two groups (double buffer).  The window of group g + 1 is fetched by 16-byte DMAs (ALIGNED:
//           whole image rows) during the first slabs of group g -- nine slabs ahead of its use, one ninth of the im2col's bytes plus the halo
//           rows -- and an MFMA's B fragment is read at plane c, row r + p, column x + q - 1; a lane at a row's end gets its out-of-row tap as a
//           zero by a select.  No padded copy, no gather table, nothing per slab but one address add.  A [M][(g, t, c)] is re-ordered by the host.
struct GatherArgs : GemmArgs {
	const float* g_img; const float* g_zero;
	const int2* g_ktab; const int2* g_ntab;   // {element offset, y | x << 16} per tap / per output pixel
	int g_H, g_W, g_HWo, g_img_stride;
	int g_wo;                                 // mode 4 on the half-slab pipeline: width of the output map (g_W is the padded copy's row pitch there)
	// mode 3 on the half-slab pipeline, one pass over K: the adds the U-Net puts behind a convolution, applied where the tile is stored
	// (out = product + g_bias[image * g_bias_stride + row]; g_out2 = out + g_add, same layout as out; each optional)
	const float* g_bias; int g_bias_stride; const float* g_add; float* g_out2;
	// mode 3, several products over the SAME gathered image in one launch (the parity classes of a stride-2 data gradient, bla_conv.hip): blockIdx.y =
	// product; each brings its own kernels, contraction length, tap table and output plane; M, N, the image and the pixel table are shared
	// (the table lives in DEVICE memory: arrays inside this by-value block, indexed by blockIdx.y, made hipcc copy the whole block to scratch)
	int g_ncls;
	const GatherClass* g_cls;
};

// mode 7: the image window in LDS behind the two A slab buffers -- [2 groups][16 planes][RH rows][4 zeros + GW] floats (a group rounded up to whole
// 1-KiB DMA instructions, the tail zeros too), 16 bytes of slack before and after.  The one definition behind the kernel's addresses and the launch's LDS size.
template <int GW>
struct Window {
	static constexpr int RH = 128 / GW + 2, PITCH = GW + 4, PL = RH * PITCH, GRP = (16 * PL + 255) / 256 * 256, NI = GRP / 256, PW = (NI + 3) / 4;
	static constexpr size_t LDS_BYTES = (2 * 128 * 16 + 2 * GRP + 8) * sizeof(float);
	static_assert(GRP > 16 * PL && PW <= 9, "the float behind a group's last row is a zero of its own tail; the next group's window arrives within the nine slabs of a group");
	// 16-byte chunk q of a channel group's window -> element offset in the image batch (channel group 0), -1 when it is a row's leading zero chunk, when
	// its image row does not exist, or when it lies in the tail that rounds a group up to whole DMA instructions (the chunk is then fetched from the zero
	// words).  The zero chunk in front of every row is both the column left of that row and the column right of the row before it: the taps dx = -1 / +1
	// of a row's first / last pixel read a zero from LDS, and the fragments need no masking (one v_cndmask per MFMA before).
	__device__ static __forceinline__ int chunk_offset(int q, int i0, int img_h, int img_hw, int img_base) {
		constexpr int CPR = GW / 4 + 1;
		const int plane = q / (PL / 4), r = q - plane * (PL / 4), wrow = r / CPR, c4 = r - wrow * CPR;
		const int row = i0 - 1 + wrow;
		return (plane < 16 && c4 > 0 && (unsigned)row < (unsigned)img_h) ? img_base + plane * img_hw + row * GW + (c4 - 1) * 4 : -1;
	}
};

// One 128 x 128 x 16 tile pipeline, 2 x 2 waves, the stored operand K-contiguous.  MODE: see GatherArgs.  HS: the half-slab form (modes 3, 4, 7) -- the
// gather is one more address per DMA instruction, dealt out between MFMAs like the rest -- else the older two-buffer form (modes 1 - 4).  GW: mode 7's
// image row width.  (blk_* / grid_*: this workgroup's place in ITS product's grid -- blockIdx / gridDim for a launch of one product, a slice of the
// linear grid when two products share a launch, gather_pair_kernel below)
template <int MODE, bool HS, int GW>
__device__ __forceinline__ void gather_body(GatherArgs p, const int blk_x, const int blk_y, const int blk_z, const int grid_x, const int grid_z) {
	static_assert(MODE == 1 || MODE == 2 || MODE == 3 || MODE == 4 || MODE == 7, "gather mode");
	static_assert(HS ? MODE >= 3 : MODE != 7, "half-slab form: the padded-copy modes and the image window (which has no other)");
	static_assert(MODE == 7 ? (GW == 16 || GW == 32) : GW == 0, "mode 7: image rows of 16 or 32 pixels");
	// (mode 3 on a [16][256] image, a 128 x 256 tile, was allowed for and never instantiated: the allowance is gone)
	constexpr int BM = 128, BN = 128, BK = 16, WN = 2, NW = 4, TM = 2, TN = 2, KK = 2;
	constexpr bool G7 = MODE == 7, BKC = MODE == 4;   // modes 1-3 gather B as a [16][128] image, mode 4 gathers A and takes a K-contiguous B
	constexpr int A_SZ = BM * BK, B_SZ = G7 ? 0 : BN * BK;
	typedef KcImage<128, BK> KI;
	typedef Window<GW ? GW : 32> W7;   // (a valid width in the instantiations that have no window)
	constexpr int GWS = GW ? GW : 32;
	extern __shared__ __attribute__((aligned(16))) float lds[];  // [2][A_SZ + B_SZ], mode 7: the window behind them

	const int tid = threadIdx.x, lane = tid & 63;
	const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
	const int l31 = lane & 31, h = lane >> 5;
	const int wm0 = (wave / WN) * 64, wn0 = (wave % WN) * 64;

	if (MODE == 3 && HS && p.g_ncls > 1) {
		const GatherClass c = p.g_cls[blk_y];
		p.A = c.A; p.C = c.C; p.g_ktab = c.ktab; p.K = c.K; p.lda = c.K;
	}
	int m0, n0;
	// Weight gradient (mode 4: few tiles, K cut over many workgroups): every tile of one K-split reads the same del_y columns, and the hardware
	// deals consecutive workgroup ids round-robin to the 8 XCDs -- with (tile, split) = (blockIdx.x, blockIdx.z) the tiles of a split land on
	// different XCDs and each L2 fetches that split's del_y for itself (349 MB of fills for 68 MB of operands at 128->128 @32x32 x64).  So XCD x takes
	// the splits s = x (mod 8) and walks them tile by tile: the tiles of a split are neighbours in ONE XCD's dispatch order and share its L2.
	int vblock = blk_x, zsplit = blk_z;
	if (MODE == 4 && (grid_z & 7) == 0) {
		const int lin = blk_z * grid_x + blk_x, i = lin >> 3;
		zsplit = (i / grid_x) * 8 + (lin & 7); vblock = i % grid_x;
	}
	tile_origin<BM, BN>(p, vblock, m0, n0);
	const int k_begin = zsplit * p.k_per_split;
	const int k_end = min(p.K, k_begin + p.k_per_split);
	const int nkt = (k_end - k_begin) / BK;

	// The stored operand (K-contiguous: A, mode 4: B = del_y): per-lane source of this wave's two DMA instructions for slab 0 (advance by BK per slab)
	constexpr int D_NI = KI::NINST / NW;                                         // its wave-instructions per wave per slab, the gathered operand's:
	constexpr int G_NI = (MODE == 1 || MODE == 2) ? BK * BN / 64 / NW : 2;      // checked gather: dword DMA, 64 columns of one k-row per instruction
	constexpr int D_OFF = MODE == 4 ? A_SZ : 0;                                  // where its image sits in a slab buffer
	constexpr bool D_BUF = MODE >= 3;   // fetched by buffer_load ... lds (the padded-copy and window modes), else global_load_lds
	const float* const dn = MODE == 4 ? p.B : p.A;
	const float* gd[D_NI];
#pragma unroll
	for (int i = 0; i < D_NI; i++) gd[i] = KI::dma_src(dn, MODE == 4 ? p.ldb : p.lda, MODE == 4 ? n0 : m0, MODE == 4 ? p.N : p.M, k_begin, wave * D_NI + i, lane);
	// gather state: this lane's two columns (n0 + lane, n0 + 64 + lane) -> {element offset, y | x << 16}, and the scalar cursor
	int g_loff[2] = {0, 0}, g_lyx[2] = {0, 0};
	bool g_lval[2] = {false, false};
	int g_k = k_begin;            // k of the next slab to fetch
	int g_img = 0, g_r = 0;       // modes 2, 4: image and pixel of g_k
	int g4_tap[D_NI], g4_chunk[D_NI];   // mode 4: padded offset of this lane's tap row, and its (swizzled) pixel chunk, per A instruction
	if (MODE == 4) {
#pragma unroll
		for (int i = 0; i < D_NI; i++) {
			g4_tap[i] = p.g_ntab[min(m0 + KI::dma_row(wave * D_NI + i, lane), p.M - 1)].x;
			g4_chunk[i] = KI::dma_col(wave * D_NI + i, lane);
		}
		g_img = k_begin / p.g_HWo; g_r = k_begin - g_img * p.g_HWo;
#pragma unroll
		for (int i = 0; i < D_NI; i++) gd[i] += (ptrdiff_t)g_img * p.N * p.g_HWo + (g_r - k_begin);   // B = del_y [image][N][HWo], ldb = HWo
	}
	// mode 4, half-slab pipeline: a slab is 16 consecutive output pixels starting at a multiple of 16, and the map is 4, 8 or a multiple of 16 pixels wide
	// (the host checks), so where a lane's chunk of four pixels sits RELATIVE to the slab's first pixel in the padded copy never changes: the lane's byte
	// offset (tap row + that place) is fixed for the whole K loop and goes into the buffer load's VGPR offset, the slab's first pixel (image, row, column:
	// wave-uniform) into its SGPR offset -- no table load, no select and no 64-bit address per DMA instruction (before: four scalar loads per slab, three
	// v_cndmask and a 64-bit add per instruction; the counters showed 0.7 VALU instructions per MFMA beside the MFMAs themselves).
	int g4_voff[D_NI], g4_pix0 = 0, g4_col = 0, g4_soff = 0, g4_step = 0, g4_step_end = 0;
	if (MODE == 4 && HS) {
		const int wo = p.g_wo, wh = p.g_W;
#pragma unroll
		for (int i = 0; i < D_NI; i++) g4_voff[i] = (g4_tap[i] + (g4_chunk[i] / wo) * wh + g4_chunk[i] % wo) * 4;
		g4_col = g_r % wo; g4_pix0 = (g_r / wo) * wh + g4_col;
		g4_step = wo >= 16 ? 16 : (16 / wo) * wh;                  // to the next slab inside a row / over whole rows
		g4_step_end = wo >= 16 ? wh - wo + 16 : g4_step;            // from a row's last slab to the next row's first
		g4_soff = (g_img * p.g_img_stride + g4_pix0) * 4;
	}
	// mode 3: one wave-instruction of the B image (1 KiB = 256 floats) covers two k-rows of 32 sixteen-byte chunks each
	int g3_base = 0;              // padded-image offset of this lane's four columns
	if (MODE == 3) {
		int n = min(n0 + (lane % 32) * 4, p.N - 4);
		int b = n / p.g_HWo, r = n - b * p.g_HWo;
		g3_base = p.g_ntab[r].x + b * p.g_img_stride;
	}
	// mode 7: this wave's window DMA instructions jw = wave + 4 i of a group -- chunk q = 64 jw + lane of the group's 16 planes: plane q / (PL/4), window
	// row, 16-byte column -- as an element offset into the image batch (group 0; a group adds 16 planes) and whether that image row exists; the
	// fragment reads' lane offset; whether the lane's pixel column is a row's first / last
	// (the chunk's offset is worked out when its instruction is issued -- three times per nine slabs: kept in three registers and picked by the run-time
	// tap, hipcc turns the pick into a scratch array, and with it the whole argument block: 720 bytes of scratch per lane, seen in the ISA)
	int w7_i0 = 0, w7_base = 0;
	unsigned w7_lane = 0;
	if (G7) {
		const int b = n0 / p.g_HWo, i0 = (n0 - b * p.g_HWo) / GWS;    // the tile: rows i0 .. i0 + 128 / GW - 1 of image b
		w7_i0 = i0; w7_base = b * p.g_img_stride;
		w7_lane = (unsigned)((4 * h * W7::PL + ((wn0 + l31) / GWS) * W7::PITCH + 4 + (wn0 + l31) % GWS) * 4);
	}
	if (MODE == 1 || MODE == 2) {
#pragma unroll
		for (int hf = 0; hf < 2; hf++) {
			int n = n0 + hf * 64 + lane;
			g_lval[hf] = n < p.N;
			n = min(n, p.N - 1);
			if (MODE == 1) {
				int b = n / p.g_HWo, r = n - b * p.g_HWo;
				int2 t = p.g_ntab[r];
				g_loff[hf] = t.x + b * p.g_img_stride; g_lyx[hf] = t.y;
			} else {
				int2 t = p.g_ntab[n];
				g_loff[hf] = t.x; g_lyx[hf] = t.y;
			}
		}
		if (MODE == 2) {
			g_img = k_begin / p.g_HWo; g_r = k_begin - g_img * p.g_HWo;
#pragma unroll
			for (int i = 0; i < D_NI; i++) gd[i] += (ptrdiff_t)g_img * p.M * p.g_HWo + (g_r - k_begin);   // A = del_y [image][M][HWo]: row stride lda = HWo
		}
	}

#if defined(__HIP_DEVICE_COMPILE__)
	// raw descriptors, no bounds (rows / columns past the matrix are fetched from clamped offsets); lane offsets in bytes
	__amdgpu_buffer_rsrc_t rsrc_dn = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(dn), 0, 0x7fffffff, 0x00020000);
	__amdgpu_buffer_rsrc_t rsrc_img = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(MODE == 4 ? p.g_img : p.A), 0, 0x7fffffff, 0x00020000);
	int voff_dn[D_NI], soff_dn = 0;
#pragma unroll
	for (int i = 0; i < D_NI; i++) voff_dn[i] = D_BUF ? (int)((gd[i] - dn) * 4) : 0;
#endif
	// the older form's fetch: the next slab -> LDS buffer buf, the cursors move on
	auto dma = [&](int buf) {
#if defined(__HIP_DEVICE_COMPILE__)
		float* base = lds + buf * (A_SZ + B_SZ);
		auto dma_stored = [&]() {
#pragma unroll
			for (int i = 0; i < D_NI; i++) {
				if (D_BUF) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_dn, (lds_ptr_t)(base + D_OFF + (wave * D_NI + i) * 256), 16, voff_dn[i], soff_dn, 0, 0);
				else { __builtin_amdgcn_global_load_lds((gbl_ptr_t)gd[i], (lds_ptr_t)(base + D_OFF + (wave * D_NI + i) * 256), 16, 0, 0); gd[i] += BK; }
			}
			if (D_BUF) soff_dn += BK * 4;
		};
		if (MODE == 4) {
			const float* ib = p.g_img + g_img * p.g_img_stride;   // gathered operand: global_load_lds (its 16-byte chunks are mostly unaligned;
#pragma unroll                                          // the buffer form measured slower for them: 254 vs 230 us forward at 128->128 @32x32 x64)
			for (int i = 0; i < D_NI; i++) {
				const float* src = ib + (g4_tap[i] + p.g_ktab[g_r + g4_chunk[i]].x);
				__builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(base + (wave * D_NI + i) * 256), 16, 0, 0);
			}
			dma_stored();
			g_r += BK;
			if (g_r >= p.g_HWo) {   // next image: del_y [image][N][HWo]
				g_r = 0; g_img++;
				soff_dn += (p.N - 1) * p.g_HWo * 4;
			}
			return;
		}
		dma_stored();
		if (MODE == 3) {
#pragma unroll
			for (int i = 0; i < G_NI; i++) {
				const int idx = wave * G_NI + i, kr = idx * 2 + (lane >> 5);
				const float* src = p.g_img + (g3_base + p.g_ktab[g_k + kr].x);
				__builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(base + A_SZ + idx * 256), 16, 0, 0);
			}
			g_k += BK;
		} else {
			const int simg = MODE == 2 ? g_img * p.g_img_stride : 0;
#pragma unroll
			for (int i = 0; i < G_NI; i++) {
				const int idx = wave * G_NI + i, krow = idx >> 1, hf = idx & 1;            // wave-uniform
				const int2 ts = p.g_ktab[MODE == 1 ? g_k + krow : g_r + krow];            // scalar load
				const int yy = (short)(g_lyx[hf] & 0xffff) + (short)(ts.y & 0xffff), xx = (g_lyx[hf] >> 16) + (ts.y >> 16);
				const bool ok = g_lval[hf] && (unsigned)yy < (unsigned)p.g_H && (unsigned)xx < (unsigned)p.g_W;
				const float* src = ok ? p.g_img + (g_loff[hf] + ts.x + simg) : p.g_zero;
				__builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(base + A_SZ + krow * BN + hf * 64), 4, 0, 0);
			}
			g_k += BK;
			if (MODE == 2) {
				g_r += BK;
				if (g_r >= p.g_HWo) {   // next image (HWo % 16 == 0: a slab never straddles two)
					g_r = 0; g_img++;
#pragma unroll
					for (int i = 0; i < D_NI; i++) gd[i] += (size_t)(p.M - 1) * p.g_HWo;
				}
			}
		}
#endif
	};

	f32x16 acc[TM][TN];
#pragma unroll
	for (int i = 0; i < TM; i++)
#pragma unroll
		for (int j = 0; j < TN; j++)
#pragma unroll
			for (int r = 0; r < 16; r++) acc[i][j][r] = 0.f;

	auto store_tile = [&]() {
		if constexpr (MODE == 4) {   // transposed: tile element (row = tap, col = f) -> out[f][tap]; a lane's registers q&3 are 4 consecutive taps
			float* dst = p.splits > 1 ? p.slab + (size_t)zsplit * p.M * p.N : p.C;
			const int ld = p.splits > 1 ? p.M : p.ldc;
#pragma unroll
			for (int in = 0; in < TN; in++) {
				int col = n0 + wn0 + in * 32 + l31;
				if (col >= p.N) continue;
#pragma unroll
				for (int im = 0; im < TM; im++)
#pragma unroll
					for (int qq = 0; qq < 4; qq++) {
						int row = m0 + wm0 + im * 32 + 8 * qq + 4 * h;
						if (row + 3 < p.M)
							*reinterpret_cast<float4*>(dst + (size_t)col * ld + row) =
								make_float4(acc[im][in][4 * qq], acc[im][in][4 * qq + 1], acc[im][in][4 * qq + 2], acc[im][in][4 * qq + 3]);
					}
			}
		} else if constexpr (G7) {   // whole tiles inside one image; block `in` owns the 32 consecutive pixels wn0 + 32 in + l31
			const int b = n0 / p.g_HWo;
			const size_t img_off = (size_t)b * p.M * p.g_HWo + (n0 - b * p.g_HWo) + wn0 + l31;
			const float* bias = p.g_bias ? p.g_bias + (size_t)b * p.g_bias_stride : nullptr;
#pragma unroll
			for (int im = 0; im < TM; im++)
#pragma unroll
				for (int r = 0; r < 16; r++) {
					const int row = acc_row(m0 + wm0 + im * 32, r, h);
					const size_t o = img_off + (size_t)row * p.g_HWo;
					const float bv = bias ? bias[row] : 0.f;
#pragma unroll
					for (int in = 0; in < TN; in++) {
						const float v = acc[im][in][r] + bv;
						p.C[o + in * 32] = v;
						if (p.g_out2) p.g_out2[o + in * 32] = v + p.g_add[o + in * 32];
					}
				}
		} else if constexpr (MODE == 3 && HS) {   // whole tiles; a lane owns two consecutive columns (the row-contiguous operand's interleaved blocks)
			const int col = n0 + wn0 + TN * l31;              // two consecutive pixels of one image (HWo % 4 == 0)
			const int b = col / p.g_HWo, rr = col - b * p.g_HWo;
			const size_t img_off = (size_t)b * p.M * p.g_HWo + rr;
			float* cbase = (p.splits > 1 ? p.slab + (size_t)zsplit * p.M * p.N : p.C) + img_off;   // slabs are C-shaped
			const float* bias = p.g_bias ? p.g_bias + (size_t)b * p.g_bias_stride : nullptr;
#pragma unroll
			for (int im = 0; im < TM; im++)
#pragma unroll
				for (int r = 0; r < 16; r++) {
					const int row = acc_row(m0 + wm0 + im * 32, r, h);
					const size_t o = (size_t)row * p.g_HWo;
					const float bv = bias ? bias[row] : 0.f;
					const float2 v = make_float2(acc[im][0][r] + bv, acc[im][1][r] + bv);
					*reinterpret_cast<float2*>(cbase + o) = v;
					if (p.g_out2) {
						const float2 a2 = *reinterpret_cast<const float2*>(p.g_add + img_off + o);
						*reinterpret_cast<float2*>(p.g_out2 + img_off + o) = make_float2(v.x + a2.x, v.y + a2.y);
					}
				}
		} else if constexpr (MODE == 1 || MODE == 3) {   // C is [image][M][HWo]: column n = (image, pixel)
#pragma unroll
			for (int in = 0; in < TN; in++) {
				int col = n0 + wn0 + in * 32 + l31;
				if (col >= p.N) continue;
				int b = col / p.g_HWo, r = col - b * p.g_HWo;
				float* cbase = p.C + (size_t)b * p.M * p.g_HWo + r;
#pragma unroll
				for (int im = 0; im < TM; im++)
#pragma unroll
					for (int q = 0; q < 16; q++) {
						int row = acc_row(m0 + wm0 + im * 32, q, h);
						if (row < p.M) cbase[(size_t)row * p.g_HWo] = acc[im][in][q];
					}
			}
		} else {   // mode 2: a dense C (alpha = 1, no epilogue: gather_args), or the K-split's slab
			float* dst = p.splits > 1 ? p.slab + (size_t)zsplit * p.M * p.N : p.C;
			const int ld = p.splits > 1 ? p.N : p.ldc;
#pragma unroll
			for (int im = 0; im < TM; im++)
#pragma unroll
				for (int in = 0; in < TN; in++) {
					const int col = n0 + wn0 + in * 32 + l31;
#pragma unroll
					for (int r = 0; r < 16; r++) {
						const int row = acc_row(m0 + wm0 + im * 32, r, h);
						if (row < p.M && col < p.N) dst[(size_t)row * ld + col] = acc[im][in][r];
					}
				}
		}
	};

	if constexpr (!HS) {
		// Two LDS buffers, two fragment register sets (the dense kernel's two-buffer pipeline, bla_gemm_kernel.h): per step the first MFMA group of slab kt,
		// s_waitcnt vmcnt(0) + s_barrier, the reads of slab kt + 1 into the other set, the DMA of slab kt + 2 into slab kt's buffer (AFTER the reads: hipcc
		// waits for vmcnt(0) in front of a ds_read that follows an LDS-DMA), the remaining MFMAs.  sched_barrier(0) pins that order.
		auto frags = [&](int buf, float (&a)[KK][TM][4], float (&b)[KK][TN][4]) {   // the slab in buffer buf -> this lane's MFMA operands
			const float* As = lds + buf * (A_SZ + B_SZ); const float* Bs = As + A_SZ;
#pragma unroll
			for (int kk = 0; kk < KK; kk++)
#pragma unroll
				for (int i = 0; i < 2; i++) {
					const float4 x = *reinterpret_cast<const float4*>(As + KI::off(wm0 + i * 32 + l31, kk * 2 + h));
					a[kk][i][0] = x.x; a[kk][i][1] = x.y; a[kk][i][2] = x.z; a[kk][i][3] = x.w;
					if (BKC) {
						const float4 y = *reinterpret_cast<const float4*>(Bs + KI::off(wn0 + i * 32 + l31, kk * 2 + h));
						b[kk][i][0] = y.x; b[kk][i][1] = y.y; b[kk][i][2] = y.z; b[kk][i][3] = y.w;
					} else {
#pragma unroll
						for (int j = 0; j < 4; j++) b[kk][i][j] = Bs[(kk * 8 + 4 * h + j) * BN + wn0 + i * 32 + l31];
					}
				}
		};
		auto mfmas = [&](float (&a)[KK][TM][4], float (&b)[KK][TN][4], int first, int last) {   // MFMA groups (kk, j) = first .. last - 1 of a slab's eight
#pragma unroll
			for (int g = first; g < last; g++)
#pragma unroll
				for (int im = 0; im < TM; im++)
#pragma unroll
					for (int in = 0; in < TN; in++) acc[im][in] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[g / 4][im][g % 4], b[g / 4][in][g % 4], acc[im][in], 0, 0, 0);
		};
		auto step = [&](int kt, bool do_dma, float (&pa)[KK][TM][4], float (&pb)[KK][TN][4], float (&qa)[KK][TM][4], float (&qb)[KK][TN][4]) {
			mfmas(pa, pb, 0, 1);
			__builtin_amdgcn_sched_barrier(0);
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__builtin_amdgcn_s_barrier();
			frags((kt + 1) & 1, qa, qb);
			if (do_dma) dma(kt & 1);
			__builtin_amdgcn_sched_barrier(0);
			mfmas(pa, pb, 1, 4 * KK);
			__builtin_amdgcn_sched_barrier(0);
		};
		float fa0[KK][TM][4], fb0[KK][TN][4], fa1[KK][TM][4], fb1[KK][TN][4];
		if (nkt > 0) {
			dma(0);
			asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
			__builtin_amdgcn_s_barrier();
			frags(0, fa0, fb0);
			if (nkt > 1) dma(1);
			int kt = 0;
			for (; kt + 2 < nkt; kt += 2) {
				step(kt, true, fa0, fb0, fa1, fb1);               // slab kt+2 exists
				step(kt + 1, kt + 3 < nkt, fa1, fb1, fa0, fb0);
			}
			if (nkt - kt == 2) {
				step(kt, false, fa0, fb0, fa1, fb1);
				mfmas(fa1, fb1, 0, 4 * KK);
			} else mfmas(fa0, fb0, 0, 4 * KK);
		}
		store_tile();
		return;
	} else {
		// the fragment reads of the dense kernel's half-slab pipeline; mode 7 reads its B side from the window instead (element [j][block] of sb is one dword of it)
		struct HF : HalfSlabFrags<BKC> {
			typedef HalfSlabFrags<BKC> Base;
			using Base::Base;
			__device__ static __forceinline__ float opb(const typename Base::Frag& f, int in, int j) { return G7 ? f.sb[j][in] : Base::opb(f, in, j); }
		};
		typedef typename HF::Frag Frag;
		typedef __attribute__((address_space(3))) float* lds_f;
		const unsigned lds0 = (unsigned)(size_t)(lds_f)lds;
		const HF hf(lds0, wm0, wn0, l31, h);
		constexpr unsigned BUF_BYTES = (A_SZ + B_SZ) * 4;
		constexpr int UA = HF::UA, UB = G7 ? 4 * TN : HF::UB, NU = UA + UB, NM = 4 * TM * TN;   // fragment-read units and MFMAs per k-part
		constexpr int NDMA = G7 ? D_NI + 1 : D_NI + G_NI;   // DMA instructions per wave per slab (mode 7: A and at most one window instruction)
		int w7_tap = 0, w7_g = 0;                                    // mode 7: tap and channel group of the slab being computed
		const int w7_groups = G7 ? (p.g_img_stride / p.g_HWo) / 16 : 0, w7_gstep = 16 * p.g_HWo;
		// (plain values, not members of p: a select between p.g_img + x and p.g_zero hipcc rewrites as a load through a selected ADDRESS of the member,
		// which puts the whole argument block into scratch -- 720 bytes per lane, seen in the ISA)
		const float* const w7_img = p.g_img;
		const float* const w7_zero = p.g_zero;
		// mode 7: byte address of (plane 0 of the group, tap) of the slab whose fragments are being read, plus this lane's part; [0] = slab t, [1] = slab t + 1
		unsigned w7_ad[2] = {0, 0}, w7_cur = 0;   // w7_cur: the A buffer offset of slab t (read_unit is told a slab by its A buffer)
		auto w7_addr = [&](int g, int tap) -> unsigned {   // tap (p, q): window row r + p, column x + q - 1
			const int pq = tap / 3;
			return lds0 + (unsigned)((2 * A_SZ + 4 + (g & 1) * W7::GRP + pq * W7::PITCH + (tap - 3 * pq) - 1) * 4) + w7_lane;
		};
		auto w7_slab = [&](unsigned cur) {   // where slab t and slab t + 1 read the window
			const int tap1 = w7_tap == 8 ? 0 : w7_tap + 1, g1 = w7_tap == 8 ? w7_g + 1 : w7_g;
			w7_cur = cur; w7_ad[0] = w7_addr(w7_g, w7_tap); w7_ad[1] = w7_addr(g1, tap1);
		};
#if defined(__HIP_DEVICE_COMPILE__)
		// Mode 3's tap table: the entries a slab's DMA instructions need are wave-uniform (the two tap rows of an instruction), so they are SCALAR loads,
		// issued when the cursor moves -- a whole slab before the DMA that uses them.  (A per-lane
		// table load in front of each DMA waits on vmcnt, i.e. for every LDS-DMA issued before it: 256->256 @16x16 ran 11 % slower that way.)
		int hs_tap[G_NI][2];
		auto hs_prefetch = [&]() {
#pragma unroll
			for (int i = 0; i < G_NI; i++) {
				const int row = __builtin_amdgcn_readfirstlane(g_k + (wave * G_NI + i) * 2);
				hs_tap[i][0] = p.g_ktab[row].x; hs_tap[i][1] = p.g_ktab[row + 1].x;
			}
		};
		if (MODE == 3) hs_prefetch();
#endif
		auto dma_one = [&](int buf, int d) {   // d-th DMA instruction of a slab; the offsets / gather cursors advance in dma_advance()
#if defined(__HIP_DEVICE_COMPILE__)
			float* base = lds + buf * (A_SZ + B_SZ);
			if (d < D_NI) {
				const int i = d;
				if (MODE == 4) {   // gathered operand: 16-byte chunk of four pixels of this lane's tap row (padded image copy): fixed lane offset + the slab's scalar offset
					__builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_img, (lds_ptr_t)(base + (wave * D_NI + i) * 256), 16, g4_voff[i], g4_soff, 0, 0);
				} else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_dn, (lds_ptr_t)(base + (wave * D_NI + i) * 256), 16, voff_dn[i], soff_dn, 0, 0);
			} else if (G7) {
				// the one window slot of a slab: instruction `w7_tap` of the NEXT group's window, in the first W7::PW slabs of a group (its buffer held the
				// group before this one, which nobody reads any more) -- nine slabs ahead of its first use
				if (w7_tap < W7::PW && wave + 4 * w7_tap < W7::NI && w7_g + 1 < w7_groups) {
					const int i = w7_tap;
					const int off = W7::chunk_offset((wave + 4 * i) * 64 + lane, w7_i0, p.g_H, p.g_HWo, w7_base);
					const float* src = off >= 0 ? w7_img + (off + (w7_g + 1) * w7_gstep) : w7_zero;
					float* dst = lds + 2 * A_SZ + 4 + ((w7_g + 1) & 1) * W7::GRP + (wave + 4 * i) * 256;
					__builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)dst, 16, 0, 0);
				}
			} else {
				const int i = d - D_NI;
				if (MODE == 3) {   // gathered operand: four consecutive output pixels = four consecutive floats of the padded copy, tap from the scalar table
					const int idx = wave * G_NI + i;   // the instruction covers k-rows 2 idx (lanes 0-31) and 2 idx + 1: their tap offsets were loaded a slab ahead (hs_tap)
					const float* src = p.g_img + (g3_base + ((lane >> 5) ? hs_tap[i][1] : hs_tap[i][0]));
					__builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(base + A_SZ + idx * 256), 16, 0, 0);
				} else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_dn, (lds_ptr_t)(base + A_SZ + (wave * D_NI + i) * 256), 16, voff_dn[i], soff_dn, 0, 0);
			}
#endif
		};
		auto dma_advance = [&](bool really) {
#if defined(__HIP_DEVICE_COMPILE__)
			if (MODE == 3) { soff_dn += really ? BK * 4 : 0; g_k += really ? BK : 0; hs_prefetch(); return; }
			if (G7) { soff_dn += really ? BK * 4 : 0; return; }
			// mode 4 -- B = del_y [image][N][HWo]: the pixel cursor wraps into the next image (HWo % 16 == 0: a slab never straddles two)
			const int r1 = g_r + (really ? BK : 0);
			const bool wrap = r1 >= p.g_HWo;
			soff_dn += (really ? BK * 4 : 0) + (wrap ? (p.N - 1) * p.g_HWo * 4 : 0);
			g_r = wrap ? 0 : r1; g_img += wrap ? 1 : 0;
			const int c1 = g4_col + 16;
			const bool row_end = c1 >= p.g_wo;
			g4_pix0 = wrap ? 0 : g4_pix0 + (really ? (row_end ? g4_step_end : g4_step) : 0);
			g4_col = (wrap || row_end) ? 0 : (really ? c1 : g4_col);
			g4_soff = __builtin_amdgcn_readfirstlane((g_img * p.g_img_stride + g4_pix0) * 4);
#endif
		};
		auto read_unit = [&](unsigned buf, int kk, int u, Frag& f) {   // units 0..UA-1: A side, then B side
			if (u < UA) hf.read_a(buf, kk, u, f);
			else if constexpr (G7) {
				// unit x = (j, block): channel kk * 8 + 4 h + j of the group (the 4 h planes are in the lane's address), pixels block * 32 + l31 of the wave's 64;
				// `buf` is not a slab buffer here but which of the two slabs in flight (0: t, BUF_BYTES: t + 1)
				const int x = u - UA, j = x / TN, b = x % TN;
				const unsigned ad = buf == w7_cur ? w7_ad[0] : w7_ad[1];
				asm volatile("ds_read_b32 %0, %1 offset:%2" : "=v"(f.sb[j][b]) : "v"(ad), "n"(((kk * 8 + j) * W7::PL + b * (32 / GWS) * W7::PITCH) * 4));
			} else hf.read_b(buf, kk, u - UA, f);
		};
		auto land_regs = [&](Frag& f) {
			HF::land_a(f);
			if constexpr (G7) {
#pragma unroll
				for (int x = 0; x < UB; x++) asm volatile("" : "+v"(f.sb[x / TN][x % TN]));
			} else HF::land_b(f);
		};
		auto mf1 = [&](const Frag& f, int idx) { half_slab_mfma<HF>(acc, f, idx); };
		// The fetch cursor: dma_one(b, d) issues the d-th DMA instruction of the cursor's slab into buffer b; advance() moves the cursor on by one slab -- a
		// uniform select, no branch: past the last slab it stays there (a harmless re-fetch into a buffer nobody reads again)
		int fetched = 0;
		auto advance = [&]() { const bool adv = fetched + 1 < nkt; dma_advance(adv); fetched += adv ? 1 : 0; };
		auto fetch_slab = [&](int buf) {   // prologue form (clumped)
#pragma unroll
			for (int d = 0; d < D_NI + (G7 ? 0 : G_NI); d++) dma_one(buf, d);
			advance();
		};

		if constexpr (MODE == 4) {
			// The dense kernel's half-slab pipeline (bla_gemm_kernel.h) on this tile: fragments per k-HALF of a slab, P = k-half 0, Q = k-half 1; Q of slab t
			// is read under the MFMAs of P, P of slab t + 1 under the MFMAs of Q, so the wait + barrier for slab t + 1 sits in the MIDDLE of slab t; one
			// uniform body for every slab, no tail.  With 16 MFMAs per phase: one read unit per MFMA from the start of the phase and the rest of the MFMAs
			// behind them -- spread evenly, the last unit is issued some 100 cycles before its land, less than an LDS round trip.
			Frag P, Q;
			auto land = [&](Frag& f) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); land_regs(f); };
			auto slab = [&](int t) {
				const unsigned cur = (t & 1) * BUF_BYTES, nxt = ((t + 1) & 1) * BUF_BYTES;
				land(P);
#pragma unroll
				for (int u = 0; u < NU; u++) {    // k-part 1 of slab t -> Q
					read_unit(cur, 1, u, Q);
					__builtin_amdgcn_sched_barrier(0);
#pragma unroll
					for (int m = u; m < (u + 1 < NU ? u + 1 : NM); m++) mf1(P, m);
					__builtin_amdgcn_sched_barrier(0);
				}
				// last phase (k-part 1 from Q): slab t+1 has landed for everyone, and everyone is done reading slab t
				land(Q);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				__builtin_amdgcn_s_barrier();
				static_assert(NU + NDMA <= NM, "too many memory instructions for the MFMAs of one k-part");
#pragma unroll
				for (int u = 0; u < NU; u++) {    // k-part 0 of slab t+1 -> P (all LDS reads before the first DMA)
					read_unit(nxt, 0, u, P);
					__builtin_amdgcn_sched_barrier(0);
					mf1(Q, 2 * u); mf1(Q, 2 * u + 1);
					__builtin_amdgcn_sched_barrier(0);
				}
#pragma unroll
				for (int d = 0; d < NDMA; d++) {  // slab t+2 -> this slab's buffer
					dma_one(t & 1, d);
					__builtin_amdgcn_sched_barrier(0);
					mf1(Q, 2 * (NU + d)); mf1(Q, 2 * (NU + d) + 1);
					__builtin_amdgcn_sched_barrier(0);
				}
				advance();
				__builtin_amdgcn_sched_barrier(0);
			};
			if (nkt > 0) {
				fetch_slab(0);
				fetch_slab(1);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				__builtin_amdgcn_s_barrier();
#pragma unroll
				for (int u = 0; u < NU; u++) read_unit(0, 0, u, P);
				for (int t = 0; t < nkt; t++) slab(t);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the re-fetches of the last slab
			}
			store_tile();
		} else {
			// Whole-slab form for the forward / data-gradient kernels (64 x 64 per wave: 16 MFMAs per k-part): a wave that stops at every
			// k-part boundary for its fragments (land) AND at every slab for the barrier pays that fixed cost per 16 MFMAs -- a quarter of what the 256 x 256
			// kernel's 64-MFMA phases pay it for.  With 64 accumulator registers there is room for TWO whole-slab fragment sets: slab t + 1's fragments are
			// all read under slab t's 32 MFMAs, and a slab has ONE stop (land + vmcnt(0) + barrier, together) instead of three.
			Frag F0[KK], F1[KK];
			auto mf_fs = [&](Frag (&f)[KK], int idx) {   // idx-th MFMA of a slab: k-part major
				mf1(f[idx / NM], idx % NM);
			};
			auto slab_fs = [&](int t, Frag (&use)[KK], Frag (&fill)[KK]) {
				const unsigned nxt = ((t + 1) & 1) * BUF_BYTES;
				if constexpr (G7) w7_slab((t & 1) * BUF_BYTES);
				// the one stop of the slab: this slab's fragments are in registers, slab t + 1 has landed for every wave, nobody needs slab t's LDS any more
				asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
				for (int kk = 0; kk < KK; kk++) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); land_regs(use[kk]); }
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				__builtin_amdgcn_s_barrier();
				// The gather-table entries for the DMAs below were loaded a slab ago and have landed with everything else (vmcnt(0) above) -- but hipcc does not
				// know that wait, and puts its own s_waitcnt vmcnt(0) in front of their first use: BETWEEN this slab's DMA instructions, i.e. the wave would stop
				// until the DMAs it has just issued are back (the ISA showed it after the two A instructions of every slab).  Using the entries HERE makes hipcc put
				// that wait here, where it is free.
#if defined(__HIP_DEVICE_COMPILE__)
				if constexpr (MODE == 3) {
#pragma unroll
					for (int i = 0; i < G_NI; i++) { asm volatile("" : "+v"(hs_tap[i][0])); asm volatile("" : "+v"(hs_tap[i][1])); }
				}
#endif
				static_assert(KK * NU + NDMA <= KK * NM, "one memory instruction per MFMA");
				int idx = 0;
#pragma unroll
				for (int kk = 0; kk < KK; kk++)
#pragma unroll
					for (int u = 0; u < NU; u++) {   // slab t + 1 -> the other set (every LDS read before the first DMA)
						read_unit(nxt, kk, u, fill[kk]);
						__builtin_amdgcn_sched_barrier(0);
						mf_fs(use, idx++);
						__builtin_amdgcn_sched_barrier(0);
					}
#pragma unroll
				for (int d = 0; d < NDMA; d++) {     // slab t + 2 -> this slab's buffer
					dma_one(t & 1, d);
					__builtin_amdgcn_sched_barrier(0);
					mf_fs(use, idx++);
					__builtin_amdgcn_sched_barrier(0);
				}
				advance();
#pragma unroll
				for (int m = KK * NU + NDMA; m < KK * NM; m++) mf_fs(use, m);
				__builtin_amdgcn_sched_barrier(0);
				if constexpr (G7) { const bool wrap = w7_tap == 8; w7_g += wrap ? 1 : 0; w7_tap = wrap ? 0 : w7_tap + 1; }   // on to slab t + 1
			};
			if (nkt > 0) {
				if constexpr (G7) {   // the window of channel group 0, whole; group 1 follows during the first slabs
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
					for (int i = 0; i < W7::PW; i++)
						if (wave + 4 * i < W7::NI) {
							const int off = W7::chunk_offset((wave + 4 * i) * 64 + lane, w7_i0, p.g_H, p.g_HWo, w7_base);
							const float* src = off >= 0 ? w7_img + off : w7_zero;
							__builtin_amdgcn_global_load_lds((gbl_ptr_t)src, (lds_ptr_t)(lds + 2 * A_SZ + 4 + (wave + 4 * i) * 256), 16, 0, 0);
						}
#endif
					w7_cur = 0; w7_ad[0] = w7_addr(0, 0);
				}
				fetch_slab(0);
				fetch_slab(1);
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
				__builtin_amdgcn_s_barrier();
#pragma unroll
				for (int kk = 0; kk < KK; kk++)
#pragma unroll
					for (int u = 0; u < NU; u++) read_unit(0, kk, u, F0[kk]);
				int t = 0;
				for (; t + 1 < nkt; t += 2) { slab_fs(t, F0, F1); slab_fs(t + 1, F1, F0); }
				if (t < nkt) slab_fs(t, F0, F1);      // an odd number of slabs
				asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the re-fetches of the last slab
			}
			store_tile();
		}
	}
}

template <int MODE, bool HS, int GW = 0>
__global__ void __launch_bounds__(256, 1) gather_kernel(GatherArgs p) {
	gather_body<MODE, HS, GW>(p, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, (int)gridDim.x, (int)gridDim.z);
}

// Both gradients of one batched convolution in ONE launch: workgroups [0, blocks_w) run the weight gradient (gather mode 4; (tile, split) = (i % wx, i / wx)),
// the rest the data gradient (DG = gather mode 7 with rows of GW pixels, or mode 3; (tile, split) = (j % dx, j / dx)).  Neither reads what the other
// writes; dealt out in this order the data gradient's workgroups move in as the weight gradient's finish, so one product's prologue, drain and tail are
// covered by the other's body instead of standing alone on an idle chip (two contexts running them side by side measured 375 -> 331 us at 128 -> 128
// @32x32 x64; forking to a second stream per convolution cost as much in cross-stream waits as it gained).  Registers / LDS: the larger of the two.
template <int DG, int GW>
__global__ void __launch_bounds__(256, 1) gather_pair_kernel(GatherArgs w, GatherArgs d, int blocks_w, int wx, int wz, int dx, int dz) {
	const int b = (int)blockIdx.x;
	if (b < blocks_w) gather_body<4, true, 0>(w, b % wx, 0, b / wx, wx, wz);
	else gather_body<DG, true, GW>(d, (b - blocks_w) % dx, 0, (b - blocks_w) / dx, dx, dz);
}

}  // namespace bla
