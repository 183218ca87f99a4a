// bla_conv_bf16.hip -- batched convolution with bf16 operands and fp32 accumulation (include/bla.h, "mixed-precision convolution").
//
// The product (conv_bf16_gather_kernel) is the tile of bla_bf16_tile.h with a gathered B operand and a store of its own:
//   * B row n is the output pixel (image b, i, j) of the padded channel-last copy P [B][Hp][Wp][Cp]; its k-th element is
//         P[pixel_base(n) + (p Wp + q) Cp + c],   pixel_base(n) = ((b Hp + i s) Wp + j s) Cp,   k = (p kk + q) Cp + c   (tap-major, channel-minor).
//     Cp % 8 == 0 makes every 8-element chunk of k one tap's 8 consecutive channels = 16 aligned bytes of P, whatever the stride, kernel and map size; the
//     halo is part of P, so the gather has no bounds checks.  A 64-deep slab may cross tap boundaries (Cp = 24) and the last one may end short (K = 72).
//   * pixel_base is a per-lane loop constant (four 64-bit pointers, one per piece).  A lane's chunk has only TWO distinct k offsets (pieces i and i + 2
//     share the swizzle), so per slab a lane derives two tap offsets from kb + kc by two multiply-high divisions (by Cp, by kk; the magic constants come
//     from the host) -- registers and VALU only, no table load in front of a DMA (a vector load there drains every DMA in flight).
//   * the store maps (row, n) to out [b][row][pix]: lanes run along n, so a wave's store instruction writes runs of consecutive floats, also in a tile that
//     straddles two images.
// conv_bf16_gather_cl_kernel is the same K loop with a channel-last bf16 store: it writes the padded map the next product gathers from.
// Around them: the pad copy (fp32 [B][C][H][W] -> P, a convert-and-transpose through an LDS tile that writes EVERY element of P), the tap-major kernel
// matrices, the materialised weight gradient (a bf16 im2col and a bf16 copy of del_y in front of the existing fast nt product), and the implicit weight
// gradient (conv_bf16_wgrad_kernel): the k-major tile on the two padded copies a backward pass has anyway, K-split with a fixed-order fold.
// At the end: the batched ResNet block composed of these entries and the norms of bla_norm_bf16.hip; it adds no kernel.
#include "bla_internal.h"
#include "bla_bf16_tile.h"

namespace bla {
namespace {

struct GatherArgs {
	const uint16_t* A; const uint16_t* P; float* out; const void* zero;
	int rows, n, K, tiles_m, tiles_n;     // n = batch * ho * wo, K = kk * kk * cp
	int hp, wp, cp, kk, stride, wo, howo;
	uint32_t magic_cp, magic_kk;          // ceil(2^32 / cp); ceil(2^32 / kk), 0 for kk = 1 (every valid chunk is tap 0)
	const float* bias; int bias_stride;
};

// the K loop of both gather kernels: acc = the tile at (row0, col0)
__device__ __forceinline__ void gather_tile_product(const GatherArgs& p, unsigned char* lds, int row0, int col0, f32x16 (&acc)[2][2]) {
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const uint16_t* pb[4];   // pixel_base of the piece's B row
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int row = col0 + bf16_piece_row(wave, lane, i), n = row < p.n ? row : 0;
		const int b = n / p.howo, pix = n - b * p.howo, oi = pix / p.wo, oj = pix - oi * p.wo;
		pb[i] = p.P + (((size_t)b * p.hp + (size_t)oi * p.stride) * p.wp + (size_t)oj * p.stride) * p.cp;
	}
	bf16_tile_product(lds, {p.A, p.K, p.rows, p.n, p.K, row0, col0, p.zero}, 0, p.K, [&](int i, int kb) {
		const uint32_t k0 = (uint32_t)(kb + bf16_piece_chunk(lane, i) * 8);   // the same for pieces i and i + 2: two tap offsets per slab
		const uint32_t tap = __umulhi(k0, p.magic_cp), c = k0 - tap * p.cp;
		const uint32_t tp = __umulhi(tap, p.magic_kk), tq = tap - tp * p.kk;
		return pb[i] + (int)((tp * p.wp + tq) * p.cp + c);   // a lane past K has a meaningless offset and never uses it
	}, acc);
}

__global__ __launch_bounds__(256) void conv_bf16_gather_kernel(GatherArgs p) {
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	const Bf16Tile t = bf16_tile_of(blockIdx.x, p.tiles_m, p.tiles_n);
	const int row0 = t.tm * BM, col0 = t.tn * BN;
	f32x16 acc[2][2];
	gather_tile_product(p, lds, row0, col0, acc);

#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const int n = col0 + bf16_acc_col(j);
		if (n >= p.n) continue;
		const int b = n / p.howo, pix = n - b * p.howo;
		float* o = p.out + (size_t)b * p.rows * p.howo + pix;
		const float* bias = p.bias ? p.bias + (size_t)b * p.bias_stride : nullptr;
#pragma unroll
		for (int i = 0; i < 2; ++i)
#pragma unroll
			for (int r = 0; r < 16; ++r) {
				const int row = row0 + bf16_acc_row(i, r);
				if (row < p.rows) o[(size_t)row * p.howo] = bias ? acc[i][j][r] + bias[row] : acc[i][j][r];
			}
	}
}

// ---- the same product with a channel-last bf16 output: the store writes the padded map the next product gathers from -------------------------
// After the K loop lane l holds ONE pixel (bf16_acc_col) and, per 32-row block, four groups g of four consecutive channels 8 g + 4 (l >> 5) + e: lanes l
// and l + 32 hold the two halves of every 8-channel chunk of the same pixel.  The epilogue runs on the fp32 values in the order of include/bla.h (bias,
// relu, gate, the fp32 store), packs a group to 8 bytes, and v_permlane32_swap exchanges the halves of a pair of groups (2 m, 2 m + 1): afterwards lanes
// 0-31 hold chunk 2 m whole, lanes 32-63 chunk 2 m + 1, and each lane stores 16 bytes -- 8 stores a lane for the tile, every one a whole aligned chunk of
// dst.  The swap runs on every lane, whatever it holds (only loads and stores are predicated): a pixel at or past n stores nothing, a channel at or past
// rows is the literal +0 (never its accumulator, which a NaN in P could have reached), a chunk at or past dst.cp is not stored.  The gate is read by the
// lane that holds the four channels, one 8-byte load per group in front of the swap, because the fp32 output wants the gated value too.  relu, gate, out
// and dst are workgroup-uniform branches around the same 64 accumulators.
struct ChainArgs { GatherArgs g; int relu; bla_conv_bf16_map gate, dst; };

__device__ __forceinline__ size_t map_pixel(const bla_conv_bf16_map& m, int b, int i, int j) {   // element offset of channel 0 of output pixel (b, i, j)
	return (((size_t)b * m.hp + m.top + i * m.dilate) * m.wp + m.left + j * m.dilate) * m.cp;
}

__global__ __launch_bounds__(256, 3) void conv_bf16_gather_cl_kernel(ChainArgs a) {
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	const GatherArgs& p = a.g;
	const Bf16Tile t = bf16_tile_of(blockIdx.x, p.tiles_m, p.tiles_n);
	const int row0 = t.tm * BM, col0 = t.tn * BN;
	f32x16 acc[2][2];
	gather_tile_product(p, lds, row0, col0, acc);

#pragma unroll
	for (int j = 0; j < 2; ++j) {
		const int n = col0 + bf16_acc_col(j);
		const bool live = n < p.n;
		const int nn = live ? n : 0;   // a lane past n computes on pixel 0 and stores nothing
		const int b = nn / p.howo, pix = nn - b * p.howo, oi = pix / p.wo, oj = pix - oi * p.wo;
		float* o = p.out ? p.out + (size_t)b * p.rows * p.howo + pix : nullptr;
		const float* bias = p.bias ? p.bias + (size_t)b * p.bias_stride : nullptr;
		const uint16_t* gate = a.gate.d ? a.gate.d + map_pixel(a.gate, b, oi, oj) : nullptr;
		uint16_t* dst = a.dst.d ? a.dst.d + map_pixel(a.dst, b, oi, oj) : nullptr;
#pragma unroll
		for (int i = 0; i < 2; ++i) {
			uint2 packed[4];
#pragma unroll
			for (int g = 0; g < 4; ++g) {
				const int row = row0 + bf16_acc_row(i, 4 * g);   // the group's first channel, a multiple of 4: row < rows puts row + 3 inside gate.cp
				uint2 gb = make_uint2(0u, 0u);
				if (a.gate.d && row < p.rows) gb = *(const uint2*)(gate + row);
				float v[4];
#pragma unroll
				for (int e = 0; e < 4; ++e) {
					const bool in = row + e < p.rows;
					float x = acc[i][j][4 * g + e];
					if (p.bias) x += bias[in ? row + e : 0];
					if (a.relu) x = x > 0.f ? x : 0.f;
					if (a.gate.d) x = bf16_to_f32((uint16_t)((e < 2 ? gb.x : gb.y) >> (16 * (e & 1)))) > 0.f ? x : 0.f;
					v[e] = in ? x : 0.f;
					if (p.out && live && in) o[(size_t)(row + e) * p.howo] = x;
				}
				packed[g] = make_uint2(pack2(v[0], v[1]), pack2(v[2], v[3]));
			}
			if (a.dst.d) {
#pragma unroll
				for (int m = 0; m < 2; ++m) {
					const uint2 lo = packed[2 * m], hi = packed[2 * m + 1];
					const auto sx = __builtin_amdgcn_permlane32_swap(lo.x, hi.x, false, false);
					const auto sy = __builtin_amdgcn_permlane32_swap(lo.y, hi.y, false, false);
					const int ch = row0 + (threadIdx.x >> 7) * 64 + i * 32 + 16 * m + 8 * ((threadIdx.x & 63) >> 5);   // lanes 0-31: chunk 2 m, 32-63: chunk 2 m + 1
					if (live && ch < a.dst.cp) *(uint4*)(dst + ch) = make_uint4(sx[0], sy[0], sx[1], sy[1]);
				}
			}
		}
	}
}

// ---- the pad copy: fp32 [B][C][H][W] -> bf16 [B][Hp][Wp][Cp], every element of the destination written -----------------------------------------------
// One workgroup: one destination row of one image, 64 channels, 64 source pixels of that row.  A row that holds source pixels ((r - top) % d == 0, inside
// the map) is read [c][x] into an fp32 LDS tile (pitch 65: the 8-channel column walk of the write phase and the 4-pixel row writes of the read phase both
// touch 64 different banks) and written [x][c] as 16-byte chunks of 8 channels; every other destination position of the tile's span -- halo, holes of a
// dilation, channels from C up -- gets +0 from the same store.  The x tiles share the row's destination span between them: tile 0 starts at column 0, the
// last tile ends at Wp.
struct PadArgs16 { const float* src; uint16_t* dst; int c, h, w, hp, wp, cp, top, left, d, xtiles, vec; };

__global__ __launch_bounds__(256) void conv_bf16_pad_kernel(PadArgs16 a) {
	__shared__ float tile[64][65];
	const int xt = blockIdx.x % a.xtiles, ct = blockIdx.x / a.xtiles, r = blockIdx.y, b = blockIdx.z;
	const int c0 = ct * 64, x0 = xt * 64, xn = min(64, a.w - x0);
	const int ry = r - a.top, y = ry / a.d;
	const bool source_row = ry >= 0 && ry % a.d == 0 && y < a.h;   // uniform over the workgroup
	if (source_row) {
		const float* s = a.src + (((size_t)b * a.c + c0) * a.h + y) * a.w + x0;
		for (int id = threadIdx.x; id < 64 * 16; id += 256) {
			const int c = id >> 4, x = (id & 15) * 4;
			if (x >= xn) continue;
			float v[4] = {0.f, 0.f, 0.f, 0.f};
			if (c0 + c < a.c) {
				const float* sp = s + (size_t)c * a.h * a.w + x;
				if (a.vec && x + 4 <= xn) { const float4 q = *(const float4*)sp; v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
				else for (int j = 0; j < 4 && x + j < xn; ++j) v[j] = sp[j];
			}
#pragma unroll
			for (int j = 0; j < 4; ++j) tile[c][x + j] = v[j];   // x + j <= 63; columns from xn up are never read
		}
		__syncthreads();
	}
	const int lo = xt == 0 ? 0 : a.left + x0 * a.d, hi = xt == a.xtiles - 1 ? a.wp : a.left + (x0 + 64) * a.d;
	const int cq = threadIdx.x & 7, c = c0 + cq * 8;
	if (c >= a.cp) return;
	uint16_t* drow = a.dst + ((size_t)b * a.hp + r) * a.wp * a.cp + c;
	for (int t = lo + (threadIdx.x >> 3); t < hi; t += 32) {
		uint4 o = make_uint4(0u, 0u, 0u, 0u);
		const int sx = t - a.left, x = sx / a.d - x0;
		if (source_row && sx >= 0 && sx % a.d == 0 && x >= 0 && x < xn) {
			o.x = pack2(tile[cq * 8 + 0][x], tile[cq * 8 + 1][x]);
			o.y = pack2(tile[cq * 8 + 2][x], tile[cq * 8 + 3][x]);
			o.z = pack2(tile[cq * 8 + 4][x], tile[cq * 8 + 5][x]);
			o.w = pack2(tile[cq * 8 + 6][x], tile[cq * 8 + 7][x]);
		}
		*(uint4*)(drow + (size_t)t * a.cp) = o;
	}
}

// ---- kernel matrices, tap-major: one thread per 8-element chunk of a destination row ------------------------------------------------------------------
//   forward:        dst [f][(p k + q) Cp + c]                 = kern[f][c][p][q]          rows = F, inner = C
//   data gradient:  dst [c][((k-1-p) k + (k-1-q)) Fp + f]     = kern[f][c][p][q]          rows = C, inner = F
// (one chunk; both launches below run this body, so a table launch and a single launch cannot diverge)
__device__ __forceinline__ void conv_bf16_kernels_chunk(const float* __restrict__ kern, uint16_t* __restrict__ dst, int f_n, int c_n, int k, int dgrad, long id) {
	const int inner = dgrad ? f_n : c_n, rows = dgrad ? c_n : f_n, ip = (inner + 7) & ~7, chunks = k * k * (ip >> 3);
	if (id >= (long)rows * chunks) return;
	const int row = (int)(id / chunks), ch = (int)(id % chunks), tap = ch / (ip >> 3), i0 = (ch % (ip >> 3)) * 8;
	const int tp = dgrad ? k - 1 - tap / k : tap / k, tq = dgrad ? k - 1 - tap % k : tap % k;
	float v[8];
#pragma unroll
	for (int j = 0; j < 8; ++j) {
		const int in = i0 + j, f = dgrad ? in : row, c = dgrad ? row : in;
		v[j] = in < inner ? kern[(((size_t)f * c_n + c) * k + tp) * k + tq] : 0.f;
	}
	*(uint4*)(dst + (size_t)row * k * k * ip + (size_t)ch * 8) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
}

__global__ __launch_bounds__(256) void conv_bf16_kernels_kernel(const float* __restrict__ kern, uint16_t* __restrict__ dst, int f_n, int c_n, int k, int dgrad) {
	conv_bf16_kernels_chunk(kern, dst, f_n, c_n, k, dgrad, (long)blockIdx.x * 256 + threadIdx.x);
}

// Many matrices in one launch: grid (chunks of the largest job / 256, jobs).  A workgroup reads its job -- blockIdx.y is uniform, so the 32
// bytes come through scalar loads -- and the threads past that job's extent return inside the chunk body.
__global__ __launch_bounds__(256) void conv_bf16_kernels_table_kernel(const bla_conv_bf16_prep_job* __restrict__ jobs) {
	const bla_conv_bf16_prep_job j = jobs[blockIdx.y];
	conv_bf16_kernels_chunk(j.kern, j.dst, j.f_n, j.c_n, j.k, j.data_gradient != 0, (long)blockIdx.x * 256 + threadIdx.x);
}

// ---- the weight gradient's operands, both [row][n] with n = (image, i, j) at a pitch np = B Ho Wo rounded up to 8, the tail zero ----------------------
//   G [(c, p, q)][n] = x[b][c][i s + p - pt][j s + q - pl] (0 outside the map);   dY16 [f][n] = del_y[b][f][i][j]
struct WgradArgs { const float* src; uint16_t* dst; int rows, n, np, c, h, w, k, s, wo, howo, pt, pl; };

template <bool IM2COL>
__global__ __launch_bounds__(256) void conv_bf16_wgrad_operand_kernel(WgradArgs a) {
	const int chunks = a.np >> 3;
	const long id = (long)blockIdx.x * 256 + threadIdx.x;
	if (id >= (long)a.rows * chunks) return;
	const int row = (int)(id / chunks), n0 = (int)(id % chunks) * 8;
	int c = row, tp = 0, tq = 0;
	if (IM2COL) { const int kk = a.k * a.k, t = row % kk; c = row / kk; tp = t / a.k; tq = t % a.k; }
	float v[8];
#pragma unroll
	for (int j = 0; j < 8; ++j) {
		const int n = n0 + j;
		v[j] = 0.f;
		if (n < a.n) {
			const int b = n / a.howo, pix = n - b * a.howo;
			if (IM2COL) {
				const int oi = pix / a.wo, oj = pix - oi * a.wo, y = oi * a.s + tp - a.pt, x = oj * a.s + tq - a.pl;
				if (y >= 0 && y < a.h && x >= 0 && x < a.w) v[j] = a.src[(((size_t)b * a.c + c) * a.h + y) * a.w + x];
			} else {
				v[j] = a.src[((size_t)b * a.rows + row) * a.howo + pix];
			}
		}
	}
	*(uint4*)(a.dst + (size_t)row * a.np + n0) = make_uint4(pack2(v[0], v[1]), pack2(v[2], v[3]), pack2(v[4], v[5]), pack2(v[6], v[7]));
}

// ---- the implicit weight gradient: no operand pass of its own ------------------------------------------------------------------------------
//   D[f][(p k + q) Cp + c] = sum_n Q[b][top + i d][left + j d][f] . P[b][i s + p][j s + q][c],   n = (b, i, j) over the N = B Ho Wo output pixels
// Q is the data gradient's padded, dilated channel-last copy of del_y, P the forward pass's padded channel-last copy of x: the contraction runs over
// pixels, so both operands are k-major with contiguous columns -- bf16_tile_product_kmajor.  k-row n of A is the Fp channels of Q's pixel n, k-row n of B
// the k x k window of P's pixel n, one tap's Cp channels after the other.  A lane's column chunk is a loop constant (for B: a tap offset and a channel,
// derived once); its four k-rows per slab are four pixels.  Their (i, j) and their element offsets in Q and P are derived once, by division, for the
// split's first slab, and then move INCREMENTALLY: the next slab is 64 pixels on, 64 = db Ho Wo + di Wo + dj, so j += dj and i += di with at most one
// carry each, and the offsets take a constant step plus one correction per carry (host-made constants; adds, compares and selects only -- registers
// and VALU, no table load in front of a DMA and no multiplication in the loop).  The step runs behind the slab's DMAs, before the wait for them.
// Every workgroup stores its accumulator tile whole to partial [split][tile][128][128] (also with one split); the fold permutes (tap, c) -> [c][p][q].
struct WgradImplicitArgs {
	const uint16_t* Q; const uint16_t* P; float* partial; const void* zero;
	int fp, ncols, n, tiles_m, tiles_n, sps;      // ncols = kk * kk * cp, n = batch * ho * wo
	int hq, wq, top, left, dilate;
	int hp, wp, cp, kk, stride;
	int ho, wo;
	int dj, di;                                   // 64 pixels on: j += dj, i += di (+ carries), the image += db (only inside the steps below)
	int q_step, q_carry_j, q_carry_i;             // Q's element offset: the step without carries, the correction when j wraps, when i wraps
	int p_step, p_carry_j, p_carry_i;             // P's
};

__global__ __launch_bounds__(256) void conv_bf16_wgrad_kernel(WgradImplicitArgs a) {
	extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	const int tiles = a.tiles_m * a.tiles_n, split = blockIdx.x / tiles;   // split-major
	const Bf16Tile t = bf16_tile_of(blockIdx.x - split * tiles, a.tiles_m, a.tiles_n);
	const int row0 = t.tm * BM, col0 = t.tn * BN;
	const int k_begin = split * a.sps * BK, k_end = min(a.n, k_begin + a.sps * BK);

	// per piece: the pixel's (i, j) and the element offsets of this lane's chunk in Q and P, for the slab that is staged next.  A k-row at or past n has
	// meaningless offsets (uint32 arithmetic, wrapping) and the tile never uses them.
	int oi[4], oj[4];
	uint32_t oq[4], op[4];
#pragma unroll
	for (int i = 0; i < 4; ++i) {
		const int f0 = row0 + bf16_kmajor_chunk(lane, i) * 8, col = col0 + bf16_kmajor_chunk(lane, i) * 8;
		const int cc = col < a.ncols ? col : 0, tap = cc / a.cp, c0 = cc - tap * a.cp, tp = tap / a.kk, tq = tap - tp * a.kk;   // cp % 8 == 0: a chunk stays inside one tap
		const int n = k_begin + bf16_kmajor_row(wave, lane, i), howo = a.ho * a.wo, b = n / howo, pix = n - b * howo;
		oi[i] = pix / a.wo; oj[i] = pix - oi[i] * a.wo;
		oq[i] = (((uint32_t)b * a.hq + a.top + oi[i] * a.dilate) * a.wq + a.left + oj[i] * a.dilate) * a.fp + (f0 < a.fp ? f0 : 0);
		op[i] = (((uint32_t)b * a.hp + oi[i] * a.stride + tp) * a.wp + oj[i] * a.stride + tq) * a.cp + c0;
	}
	f32x16 acc[2][2];
	bf16_tile_product_kmajor(lds, {a.fp, a.ncols, a.n, row0, col0, a.zero}, k_begin, k_end,
		[&](int i, int) { return a.Q + oq[i]; },
		[&](int i, int) { return a.P + op[i]; },
		[&]() {
#pragma unroll
			for (int i = 0; i < 4; ++i) {
				int j = oj[i] + a.dj;
				const bool cj = j >= a.wo;
				j -= cj ? a.wo : 0;
				int r = oi[i] + a.di + (cj ? 1 : 0);
				const bool ci = r >= a.ho;
				r -= ci ? a.ho : 0;
				oj[i] = j; oi[i] = r;
				oq[i] += (uint32_t)a.q_step + (cj ? (uint32_t)a.q_carry_j : 0u) + (ci ? (uint32_t)a.q_carry_i : 0u);
				op[i] += (uint32_t)a.p_step + (cj ? (uint32_t)a.p_carry_j : 0u) + (ci ? (uint32_t)a.p_carry_i : 0u);
			}
		}, acc);

	// the whole tile, unconditioned: rows from Fp up and columns from k k Cp up hold the zeros their lanes fetched
	float* T = a.partial + ((size_t)split * tiles + (size_t)t.tm * a.tiles_n + t.tn) * (BM * BN);
#pragma unroll
	for (int i = 0; i < 2; ++i)
#pragma unroll
		for (int j = 0; j < 2; ++j)
#pragma unroll
			for (int r = 0; r < 16; ++r) T[bf16_acc_row(i, r) * BN + bf16_acc_col(j)] = acc[i][j][r];
}

// The fold: one thread per element of del_kern [F][C][k][k]: acc = partial[0]; acc += partial[1]; ... ascending, at row f, column (p k + q) Cp + c.
// Rows from F up and channels from C up are never read.  With one split it is a permuting copy.
__global__ __launch_bounds__(256) void conv_bf16_wgrad_fold_kernel(const float* __restrict__ partial, float* __restrict__ del_kern, int f_n, int c_n, int kk, int cp,
                                                                   int tiles_m, int tiles_n, int splits) {
	const int ckk = c_n * kk * kk;
	const long id = (long)blockIdx.x * 256 + threadIdx.x;
	if (id >= (long)f_n * ckk) return;
	const int f = (int)(id / ckk), rest = (int)(id % ckk), c = rest / (kk * kk), tap = rest % (kk * kk);   // tap = p k + q
	const int col = tap * cp + c;
	const size_t per_split = (size_t)tiles_m * tiles_n * (BM * BN);
	const float* T = partial + ((size_t)(f >> 7) * tiles_n + (col >> 7)) * (BM * BN) + (f & 127) * BN + (col & 127);
	float acc = T[0];
#pragma unroll 4
	for (int s = 1; s < splits; ++s) acc += T[(size_t)s * per_split];
	del_kern[id] = acc;
}

struct Layout16 { int hp, wp, top, left, dilate; };
Layout16 layout16(int h, int w, int k, int stride, bool dgrad) {
	const Geometry g = same_geometry(h, w, k, stride);
	if (dgrad) return {h + k - 1, w + k - 1, k - 1 - g.pt, k - 1 - g.pl, stride};
	return {h + g.vpad, w + g.hpad, g.pt, g.pl, 1};
}

// ---- pure argument checks (no device is asked for) ---------------------------------------------------------------------------------------------------
// (the shape checks stand apart from the pointer checks: the _as_bf16 entries run them before they have a workspace)
bla_status check_pad_shape(int batch, int c, int h, int w, int hp, int wp, int top, int left, int dilate) {
	BLA_REQUIRE(batch > 0 && c > 0 && h > 0 && w > 0 && hp > 0 && wp > 0, BLA_ERR_INVALID, "bla_conv_bf16_pad: extent <= 0 (batch %d c %d h %d w %d hp %d wp %d)", batch, c, h, w, hp, wp);
	BLA_REQUIRE(top >= 0 && left >= 0 && dilate >= 1, BLA_ERR_INVALID, "bla_conv_bf16_pad: top %d left %d dilate %d", top, left, dilate);
	BLA_REQUIRE((long)top + (long)(h - 1) * dilate < hp && (long)left + (long)(w - 1) * dilate < wp, BLA_ERR_INVALID,
	            "bla_conv_bf16_pad: the %d x %d map at (%d, %d), dilation %d, does not fit %d x %d", h, w, top, left, dilate, hp, wp);
	BLA_REQUIRE(batch <= 65535 && hp <= 65535 && (long)left + ((long)w + 64) * dilate < (1L << 31), BLA_ERR_INVALID, "bla_conv_bf16_pad: batch %d or hp %d exceeds the grid", batch, hp);
	return BLA_OK;
}

bla_status check_kernels(const void* kern, const void* dst, int f_n, int c_n, int k) {
	BLA_REQUIRE(kern && dst, BLA_ERR_INVALID, "bla_conv_bf16_prepare_kernels: NULL pointer");
	BLA_REQUIRE(f_n > 0 && c_n > 0 && k > 0, BLA_ERR_INVALID, "bla_conv_bf16_prepare_kernels: extent <= 0 (f %d c %d k %d)", f_n, c_n, k);
	BLA_REQUIRE(aligned16(dst), BLA_ERR_INVALID, "bla_conv_bf16_prepare_kernels: the destination is not 16-byte aligned");
	return BLA_OK;
}

bla_status check_gathered_shape(int rows, int batch, int hp, int wp, int cp, int k, int stride, int ho, int wo, int ep_bias_stride) {
	BLA_REQUIRE(rows > 0 && batch > 0 && hp > 0 && wp > 0 && cp > 0 && k > 0 && ho > 0 && wo > 0, BLA_ERR_INVALID,
	            "bla_conv2d_gathered_bf16: extent <= 0 (rows %d batch %d hp %d wp %d cp %d k %d ho %d wo %d)", rows, batch, hp, wp, cp, k, ho, wo);
	BLA_REQUIRE(stride >= 1, BLA_ERR_INVALID, "bla_conv2d_gathered_bf16: stride %d", stride);
	BLA_REQUIRE(cp % 8 == 0, BLA_ERR_INVALID, "bla_conv2d_gathered_bf16: cp %d is not a multiple of 8", cp);
	BLA_REQUIRE(ep_bias_stride >= 0, BLA_ERR_INVALID, "bla_conv2d_gathered_bf16: ep_bias_stride %d", ep_bias_stride);
	// every tap of every output pixel lies inside the padded copy: the gather itself checks nothing
	BLA_REQUIRE((long)(ho - 1) * stride + k <= hp && (long)(wo - 1) * stride + k <= wp, BLA_ERR_INVALID,
	            "bla_conv2d_gathered_bf16: a %d x %d output at stride %d, k %d reads past the %d x %d padded map", ho, wo, stride, k, hp, wp);
	const long K = (long)k * k * cp, n = (long)batch * ho * wo;
	BLA_REQUIRE((long)hp * wp * cp < (1L << 31) && (K + 128) * cp < (1L << 31) && n < (1L << 31) - 128 && ((rows + 127L) / 128) * ((n + 127) / 128) < (1L << 31), BLA_ERR_INVALID,
	            "bla_conv2d_gathered_bf16: the product exceeds 32-bit indexing (padded image %ld elements, K %ld, columns %ld)", (long)hp * wp * cp, K, n);
	return BLA_OK;
}

// a map of the chained entry: the kernel forms an address for every output pixel in it and checks nothing
bla_status check_chain_map(const char* what, const bla_conv_bf16_map& m, int batch, int ho, int wo) {
	const char* who = "bla_conv2d_gathered_bf16_chained";
	BLA_REQUIRE(aligned16(m.d), BLA_ERR_INVALID, "%s: %s is not 16-byte aligned", who, what);
	BLA_REQUIRE(m.hp > 0 && m.wp > 0 && m.cp > 0 && m.cp % 8 == 0, BLA_ERR_INVALID, "%s: %s has hp %d wp %d cp %d", who, what, m.hp, m.wp, m.cp);
	BLA_REQUIRE(m.top >= 0 && m.left >= 0 && m.dilate >= 1, BLA_ERR_INVALID, "%s: %s has top %d left %d dilate %d", who, what, m.top, m.left, m.dilate);
	BLA_REQUIRE((long)m.top + (long)(ho - 1) * m.dilate < m.hp && (long)m.left + (long)(wo - 1) * m.dilate < m.wp, BLA_ERR_INVALID,
	            "%s: the %d x %d output at (%d, %d), dilation %d, does not fit %s (%d x %d)", who, ho, wo, m.top, m.left, m.dilate, what, m.hp, m.wp);
	BLA_REQUIRE((long)batch * m.hp * m.wp * m.cp < (1L << 31), BLA_ERR_INVALID, "%s: %s holds %ld elements, 2^31 or more", who, what, (long)batch * m.hp * m.wp * m.cp);
	return BLA_OK;
}

// the implicit weight gradient forms an address for every (output pixel, tap) in P and every output pixel in Q and checks nothing in the kernel
bla_status check_wgrad_implicit_shape(int hq, int wq, int fp, int top, int left, int dilate, int hp, int wp, int cp, int batch, int k, int stride, int ho, int wo, int f_n,
                                      int c_n, int splits) {
	const char* who = "bla_conv2d_weight_gradient_gathered_bf16";
	BLA_REQUIRE(splits >= 0, BLA_ERR_INVALID, "%s: splits %d", who, splits);
	BLA_REQUIRE(hq > 0 && wq > 0 && fp > 0 && hp > 0 && wp > 0 && cp > 0 && batch > 0 && k > 0 && ho > 0 && wo > 0 && f_n > 0 && c_n > 0, BLA_ERR_INVALID,
	            "%s: extent <= 0 (hq %d wq %d fp %d hp %d wp %d cp %d batch %d k %d ho %d wo %d f %d c %d)", who, hq, wq, fp, hp, wp, cp, batch, k, ho, wo, f_n, c_n);
	BLA_REQUIRE(stride >= 1 && dilate >= 1 && top >= 0 && left >= 0, BLA_ERR_INVALID, "%s: stride %d dilate %d top %d left %d", who, stride, dilate, top, left);
	BLA_REQUIRE(fp % 8 == 0 && cp % 8 == 0, BLA_ERR_INVALID, "%s: fp %d or cp %d is not a multiple of 8", who, fp, cp);
	BLA_REQUIRE(fp >= f_n && cp >= c_n, BLA_ERR_INVALID, "%s: fp %d < f_n %d or cp %d < c_n %d", who, fp, f_n, cp, c_n);
	BLA_REQUIRE((long)(ho - 1) * stride + k <= hp && (long)(wo - 1) * stride + k <= wp, BLA_ERR_INVALID,
	            "%s: a %d x %d output at stride %d, k %d reads past the %d x %d padded map", who, ho, wo, stride, k, hp, wp);
	BLA_REQUIRE((long)top + (long)(ho - 1) * dilate < hq && (long)left + (long)(wo - 1) * dilate < wq, BLA_ERR_INVALID,
	            "%s: the %d x %d gradient at (%d, %d), dilation %d, does not fit %d x %d", who, ho, wo, top, left, dilate, hq, wq);
	const long n = (long)batch * ho * wo, ncols = (long)k * k * cp;
	BLA_REQUIRE((long)batch * hq * wq * fp < (1L << 31) && (long)batch * hp * wp * cp < (1L << 31) && n < (1L << 31) - 128 && ncols < (1L << 31) - 128 &&
	            (long)f_n * c_n * k * k < (1L << 31), BLA_ERR_INVALID,
	            "%s: the product exceeds 32-bit indexing (Q %ld, P %ld elements, %ld pixels, %ld columns)", who, (long)batch * hq * wq * fp, (long)batch * hp * wp * cp, n, ncols);
	return BLA_OK;
}

bla_status check_conv(const char* who, int batch, int h, int w, int k, int c_in, int f_n, int stride) {
	BLA_REQUIRE(batch > 0 && h > 0 && w > 0 && k > 0 && c_in > 0 && f_n > 0, BLA_ERR_INVALID, "%s: extent <= 0 (batch %d h %d w %d k %d c %d f %d)", who, batch, h, w, k, c_in, f_n);
	BLA_REQUIRE(stride >= 1, BLA_ERR_INVALID, "%s: stride %d", who, stride);
	return BLA_OK;
}

// ---- launches -------------------------------------------------------------------------------------------------------------------------------------------
bla_status launch_pad(hipStream_t s, const float* src, uint16_t* dst, int batch, int c, int h, int w, int hp, int wp, int top, int left, int dilate) {
	PadArgs16 a{src, dst, c, h, w, hp, wp, round8(c), top, left, dilate, (w + 63) / 64, aligned16(src) && w % 4 == 0};
	const long gx = (long)a.xtiles * ((a.cp + 63) / 64);
	BLA_REQUIRE(gx < (1L << 31), BLA_ERR_INVALID, "bla_conv_bf16_pad: %d channels x %d columns exceed the grid", c, w);
	hipLaunchKernelGGL(conv_bf16_pad_kernel, dim3((unsigned)gx, hp, batch), dim3(256), 0, s, a);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status launch_kernels(hipStream_t s, const float* kern, uint16_t* dst, int f_n, int c_n, int k, int dgrad) {
	const long n = (long)(dgrad ? c_n : f_n) * k * k * (round8(dgrad ? f_n : c_n) / 8);
	BLA_REQUIRE((n + 255) / 256 < (1L << 31), BLA_ERR_INVALID, "bla_conv_bf16_prepare_kernels: %ld chunks exceed the grid", n);
	hipLaunchKernelGGL(conv_bf16_kernels_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, kern, dst, f_n, c_n, k, dgrad);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

GatherArgs gather_args(const uint16_t* A, int rows, const uint16_t* P, int batch, int hp, int wp, int cp, int k, int stride, int ho, int wo, float* out, const float* ep_bias,
                       int ep_bias_stride) {
	GatherArgs a{};
	a.A = A; a.P = P; a.out = out; a.zero = zero_word();
	a.rows = rows; a.n = batch * ho * wo; a.K = k * k * cp;
	a.tiles_m = (rows + BM - 1) / BM; a.tiles_n = (a.n + BN - 1) / BN;
	a.hp = hp; a.wp = wp; a.cp = cp; a.kk = k; a.stride = stride; a.wo = wo; a.howo = ho * wo;
	// floor(x / d) = (x * ceil(2^32 / d)) >> 32 whenever x * d < 2^32 (check_gathered_shape: (K + 128) cp < 2^31; taps * kk is far below)
	a.magic_cp = (uint32_t)(((1ull << 32) + cp - 1) / cp);
	a.magic_kk = k == 1 ? 0u : (uint32_t)(((1ull << 32) + k - 1) / k);
	a.bias = ep_bias; a.bias_stride = ep_bias_stride;
	return a;
}

bla_status launch_gathered(hipStream_t s, const uint16_t* A, int rows, const uint16_t* P, int batch, int hp, int wp, int cp, int k, int stride, int ho, int wo, float* out,
                           const float* ep_bias, int ep_bias_stride) {
	const GatherArgs a = gather_args(A, rows, P, batch, hp, wp, cp, k, stride, ho, wo, out, ep_bias, ep_bias_stride);
	hipLaunchKernelGGL(conv_bf16_gather_kernel, dim3((unsigned)((long)a.tiles_m * a.tiles_n)), dim3(256), 2 * SLAB_BYTES, s, a);
	BLA_HIP(hipGetLastError());
	char name[64];
	snprintf(name, sizeof name, "conv_bf16_gather128x128x64_s%d", stride);
	gemm_note_last_kernel(name);
	return BLA_OK;
}

// the channel-last store's kernel, whatever outputs the epilogue names (with out_f32 alone it is the plain product behind relu / gate)
bla_status launch_gathered_chained(hipStream_t s, const uint16_t* A, int rows, const uint16_t* P, int batch, int hp, int wp, int cp, int k, int stride, int ho, int wo,
                                   const bla_conv_bf16_epilogue& ep) {
	const ChainArgs a{gather_args(A, rows, P, batch, hp, wp, cp, k, stride, ho, wo, ep.out_f32, ep.bias, ep.bias_stride), ep.relu != 0, ep.gate, ep.dst};
	hipLaunchKernelGGL(conv_bf16_gather_cl_kernel, dim3((unsigned)((long)a.g.tiles_m * a.g.tiles_n)), dim3(256), 2 * SLAB_BYTES, s, a);
	BLA_HIP(hipGetLastError());
	char name[64];
	snprintf(name, sizeof name, ep.dst.d ? "conv_bf16_gather128x128x64_s%d_cl" : "conv_bf16_gather128x128x64_s%d", stride);
	gemm_note_last_kernel(name);
	return BLA_OK;
}

// The implicit weight gradient's K-split: DESIGN 3.20's rules on m = F, n = k k Cp, k = N for the context's CUs; the partial tiles exist with one split too
struct WgradImplicitPlan { int eff, sps, tiles_m, tiles_n; size_t partial_bytes; };
WgradImplicitPlan wgrad_implicit_plan(int f_n, int k, int cp, int n, int splits) {
	WgradImplicitPlan p{1, 1, (f_n + BM - 1) / BM, (k * k * cp + BN - 1) / BN, 0};
	bla_gemm_bf16_splitk_plan(f_n, k * k * cp, n, splits, ctx().num_cus, &p.eff, &p.sps, nullptr);
	p.partial_bytes = (size_t)p.eff * p.tiles_m * p.tiles_n * (BM * BN * sizeof(float));
	return p;
}

// arguments already checked (check_wgrad_implicit_shape); partial holds plan.partial_bytes
bla_status launch_wgrad_implicit(hipStream_t s, const uint16_t* Q, int hq, int wq, int fp, int top, int left, int dilate, const uint16_t* P, int hp, int wp, int cp, int batch,
                                 int k, int stride, int ho, int wo, int f_n, int c_n, float* del_kern, float* partial, const WgradImplicitPlan& plan) {
	WgradImplicitArgs a{};
	a.Q = Q; a.P = P; a.partial = partial; a.zero = zero_word();
	a.fp = fp; a.ncols = k * k * cp; a.n = batch * ho * wo; a.tiles_m = plan.tiles_m; a.tiles_n = plan.tiles_n; a.sps = plan.sps;
	a.hq = hq; a.wq = wq; a.top = top; a.left = left; a.dilate = dilate;
	a.hp = hp; a.wp = wp; a.cp = cp; a.kk = k; a.stride = stride;
	a.ho = ho; a.wo = wo;
	// 64 pixels on: 64 = db ho wo + di wo + dj.  The offsets are uint32 and wrap (db images on may lie past the operand: such a k-row is past n and
	// unused), so the steps are formed in 64 bits and truncated
	const long db = BK / (ho * wo), rest = BK % (ho * wo), di = rest / wo, dj = rest % wo;
	auto wrap = [](long v) { return (int)(uint32_t)(unsigned long)v; };
	a.di = (int)di; a.dj = (int)dj;
	a.q_step = wrap(((db * hq + di * dilate) * wq + dj * dilate) * fp);
	a.q_carry_j = wrap((long)(wq - wo) * dilate * fp);              // j -= wo, i += 1
	a.q_carry_i = wrap(((long)hq - (long)ho * dilate) * wq * fp);   // i -= ho, the image += 1
	a.p_step = wrap(((db * hp + di * stride) * wp + dj * stride) * cp);
	a.p_carry_j = wrap((long)(wp - wo) * stride * cp);
	a.p_carry_i = wrap(((long)hp - (long)ho * stride) * wp * cp);
	const long grid = (long)plan.tiles_m * plan.tiles_n * plan.eff, out = (long)f_n * c_n * k * k;
	BLA_REQUIRE(grid < (1L << 31), BLA_ERR_INVALID, "bla_conv2d_weight_gradient_gathered_bf16: %ld workgroups exceed the grid", grid);
	hipLaunchKernelGGL(conv_bf16_wgrad_kernel, dim3((unsigned)grid), dim3(256), 2 * SLAB_BYTES, s, a);
	BLA_HIP(hipGetLastError());
	hipLaunchKernelGGL(conv_bf16_wgrad_fold_kernel, dim3((unsigned)((out + 255) / 256)), dim3(256), 0, s, partial, del_kern, f_n, c_n, k, cp, plan.tiles_m, plan.tiles_n, plan.eff);
	BLA_HIP(hipGetLastError());
	char name[64];
	snprintf(name, sizeof name, "conv_bf16_wgrad128x128x64_s%d_splitk%d", stride, plan.eff);
	gemm_note_last_kernel(name);
	return BLA_OK;
}

template <bool IM2COL>
bla_status launch_wgrad_operand(hipStream_t s, const WgradArgs& a) {
	const long n = (long)a.rows * (a.np / 8);
	BLA_REQUIRE((n + 255) / 256 < (1L << 31), BLA_ERR_INVALID, "bla_conv2d_backward_batched_f32_as_bf16: %ld chunks exceed the grid", n);
	hipLaunchKernelGGL(conv_bf16_wgrad_operand_kernel<IM2COL>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

// The materialised weight gradient's workspace: [dY16 [F][np] | G [C k k][np] | the product's partial tiles], each part rounded up to 256 bytes
struct WgradLayout { int np, ckk; size_t dy_bytes, g_bytes; };
WgradLayout wgrad_layout(int f_n, int c_in, int k, int n) {
	const int np = round8(n), ckk = c_in * k * k;
	return {np, ckk, round_up((size_t)f_n * np * 2, 256), round_up((size_t)ckk * np * 2, 256)};
}

// ... in the workspace at `base`.  splits: gemm_bf16_launch_splitk's (1 = the unsplit product)
bla_status launch_wgrad(hipStream_t s, unsigned char* base, const float* d_del_y, const float* d_x, float* d_del_kern, int h, int w, int k, int c_in, int f_n, int stride,
                        const Geometry& g, int n, int splits) {
	const WgradLayout L = wgrad_layout(f_n, c_in, k, n);
	uint16_t* dy16 = (uint16_t*)base;
	uint16_t* G = (uint16_t*)(base + L.dy_bytes);
	WgradArgs a{d_del_y, dy16, f_n, n, L.np, c_in, h, w, k, stride, g.wo, g.ho * g.wo, g.pt, g.pl};
	bla_status st;
	if ((st = launch_wgrad_operand<false>(s, a)) != BLA_OK) return st;
	a.src = d_x; a.dst = G; a.rows = L.ckk;
	if ((st = launch_wgrad_operand<true>(s, a)) != BLA_OK) return st;
	// del_kern [F][C k k] = dY16 [F][np] . G [C k k][np]^T: rows of G in (c, p, q) order, so the result is already [F][C][k][k]
	return gemm_bf16_launch_splitk(s, 0, 1, f_n, L.ckk, L.np, dy16, L.np, G, L.np, d_del_kern, L.ckk, BLA_C_F32, nullptr, base + L.dy_bytes + L.g_bytes, splits);
}

size_t padded_bytes(int batch, int hp, int wp, int cp) { return round_up((size_t)batch * hp * wp * cp * 2, 256); }
size_t kernels_bytes(int rows, int k, int inner_p) { return round_up((size_t)rows * k * k * inner_p * 2, 256); }

}  // namespace
}  // namespace bla

using namespace bla;

extern "C" {

bla_status bla_conv_bf16_layout(int h, int w, int k, int stride, int data_gradient, int* hp, int* wp, int* top, int* left, int* dilate) {
	BLA_REQUIRE(h > 0 && w > 0 && k > 0 && stride >= 1 && hp && wp && top && left && dilate, BLA_ERR_INVALID, "bla_conv_bf16_layout: bad query (h %d w %d k %d stride %d)", h, w, k, stride);
	const Layout16 L = layout16(h, w, k, stride, data_gradient != 0);
	*hp = L.hp; *wp = L.wp; *top = L.top; *left = L.left; *dilate = L.dilate;
	return BLA_OK;
}

bla_status bla_conv_bf16_pad(void* stream, const float* d_src, uint16_t* d_dst, int batch, int c, int h, int w, int hp, int wp, int top, int left, int dilate) {
	BLA_REQUIRE(d_src && d_dst, BLA_ERR_INVALID, "bla_conv_bf16_pad: NULL pointer");
	BLA_REQUIRE(aligned16(d_dst), BLA_ERR_INVALID, "bla_conv_bf16_pad: the destination is not 16-byte aligned");
	bla_status st = check_pad_shape(batch, c, h, w, hp, wp, top, left, dilate);
	if (st != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	return launch_pad(pick_stream(stream), d_src, d_dst, batch, c, h, w, hp, wp, top, left, dilate);
}

bla_status bla_conv_bf16_prepare_kernels(void* stream, const float* d_kern, uint16_t* d_dst, int f_n, int c_n, int k, int data_gradient) {
	bla_status st = check_kernels(d_kern, d_dst, f_n, c_n, k);
	if (st != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	return launch_kernels(pick_stream(stream), d_kern, d_dst, f_n, c_n, k, data_gradient != 0);
}

bla_status bla_conv2d_gathered_bf16(void* stream, const uint16_t* d_a, int rows, const uint16_t* d_p, int batch, int hp, int wp, int cp, int k, int stride, int ho, int wo,
                                    float* d_out, const float* ep_bias, int ep_bias_stride) {
	BLA_REQUIRE(d_a && d_p && d_out, BLA_ERR_INVALID, "bla_conv2d_gathered_bf16: NULL pointer");
	BLA_REQUIRE(aligned16(d_a) && aligned16(d_p), BLA_ERR_INVALID, "bla_conv2d_gathered_bf16: an operand is not 16-byte aligned");
	bla_status st = check_gathered_shape(rows, batch, hp, wp, cp, k, stride, ho, wo, ep_bias_stride);
	if (st != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	return launch_gathered(pick_stream(stream), d_a, rows, d_p, batch, hp, wp, cp, k, stride, ho, wo, d_out, ep_bias, ep_bias_stride);
}

bla_status bla_conv2d_gathered_bf16_chained(void* stream, const uint16_t* d_a, int rows, const uint16_t* d_p, int batch, int hp, int wp, int cp, int k, int stride, int ho,
                                            int wo, const bla_conv_bf16_epilogue* ep) {
	const char* who = "bla_conv2d_gathered_bf16_chained";
	BLA_REQUIRE(ep, BLA_ERR_INVALID, "%s: NULL epilogue", who);
	BLA_REQUIRE(ep->out_f32 || ep->dst.d, BLA_ERR_INVALID, "%s: neither out_f32 nor dst", who);
	BLA_REQUIRE(d_a && d_p, BLA_ERR_INVALID, "%s: NULL pointer", who);
	BLA_REQUIRE(aligned16(d_a) && aligned16(d_p), BLA_ERR_INVALID, "%s: an operand is not 16-byte aligned", who);
	bla_status st = check_gathered_shape(rows, batch, hp, wp, cp, k, stride, ho, wo, ep->bias_stride);
	if (st != BLA_OK) return st;
	if (ep->dst.d) {
		BLA_REQUIRE(ep->dst.cp == round8(rows), BLA_ERR_INVALID, "%s: dst.cp %d is not %d rows rounded up to 8", who, ep->dst.cp, rows);
		if ((st = check_chain_map("dst", ep->dst, batch, ho, wo)) != BLA_OK) return st;
	}
	if (ep->gate.d) {
		BLA_REQUIRE(ep->gate.cp >= rows, BLA_ERR_INVALID, "%s: gate.cp %d < rows %d", who, ep->gate.cp, rows);
		if ((st = check_chain_map("gate", ep->gate, batch, ho, wo)) != BLA_OK) return st;
	}
	st = require_ready();
	if (st != BLA_OK) return st;
	return launch_gathered_chained(pick_stream(stream), d_a, rows, d_p, batch, hp, wp, cp, k, stride, ho, wo, *ep);
}

bla_status bla_conv_bf16_prepare_kernels_table(void* stream, const bla_conv_bf16_prep_job* d_jobs, int n_jobs, size_t max_chunks) {
	const char* who = "bla_conv_bf16_prepare_kernels_table";
	BLA_REQUIRE(n_jobs >= 0, BLA_ERR_INVALID, "%s: n_jobs %d", who, n_jobs);
	if (n_jobs == 0) return BLA_OK;
	BLA_REQUIRE(d_jobs, BLA_ERR_INVALID, "%s: NULL table with %d jobs", who, n_jobs);
	BLA_REQUIRE(max_chunks > 0, BLA_ERR_INVALID, "%s: max_chunks 0 with %d jobs", who, n_jobs);
	BLA_REQUIRE(n_jobs <= 65535 && (max_chunks + 255) / 256 < ((size_t)1 << 31), BLA_ERR_INVALID, "%s: %d jobs of up to %zu chunks exceed the grid", who, n_jobs, max_chunks);
	bla_status st = require_ready();
	if (st != BLA_OK) return st;
	hipLaunchKernelGGL(conv_bf16_kernels_table_kernel, dim3((unsigned)((max_chunks + 255) / 256), (unsigned)n_jobs), dim3(256), 0, pick_stream(stream), d_jobs);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_conv2d_forward_batched_f32_as_bf16(void* stream, const float* d_x, const float* d_kern, float* d_out, int batch, int h, int w, int k, int c_in, int f_n,
                                                  int stride, const float* ep_bias, int ep_bias_stride) {
	return conv2d_forward_as_bf16(stream, d_x, d_kern, d_out, batch, h, w, k, c_in, f_n, stride, ep_bias, ep_bias_stride, nullptr);
}

bla_status bla_conv2d_backward_gathered_f32_as_bf16(void* stream, const float* d_del_y, const float* d_x, const float* d_kern, float* d_del_kern, float* d_del_x, int batch,
                                                    int h, int w, int k, int c_in, int f_n, int stride, int splits) {
	return conv2d_backward_gathered_as_bf16(stream, d_del_y, d_x, d_kern, d_del_kern, d_del_x, batch, h, w, k, c_in, f_n, stride, splits, nullptr);
}

bla_status bla_resnet_forward_batched_bf16(void* stream, int batch, const float* d_x, const float* d_temb, const bla_resnet_params* p, const unsigned char* d_drop,
                                           const bla_resnet_ws* ws, float* d_result, int h, int w, int cin, int cout, int k, int tdim, int group_size,
                                           const bla_resnet_bf16_maps* maps) {
	return resnet_forward_bf16(stream, batch, d_x, d_temb, p, d_drop, ws, d_result, h, w, cin, cout, k, tdim, group_size, maps, 0, nullptr);
}

bla_status bla_resnet_backward_batched_bf16(void* stream, int batch, const float* d_del_out, const float* d_x, const float* d_temb, const bla_resnet_params* p,
                                            const bla_resnet_ws* ws, const bla_resnet_grads* g, const bla_resnet_scratch* sc, float* d_dtb, float* d_del_x, int h, int w,
                                            int cin, int cout, int k, int tdim, int group_size, const bla_resnet_bf16_maps* maps, int splits) {
	return resnet_backward_bf16(stream, batch, d_del_out, d_x, d_temb, p, ws, g, sc, d_dtb, d_del_x, h, w, cin, cout, k, tdim, group_size, maps, splits, 0, nullptr);
}

}  // extern "C"

// ---- the internal forms (bla_internal.h): the public compositions above with an optional prepared kernel matrix; NULL = prepare it here, as always -------
bla_status bla::conv2d_forward_as_bf16(void* stream, const float* d_x, const float* d_kern, float* d_out, int batch, int h, int w, int k, int c_in, int f_n, int stride,
                                       const float* ep_bias, int ep_bias_stride, const uint16_t* prepared) {
	const char* who = "bla_conv2d_forward_batched_f32_as_bf16";
	BLA_REQUIRE(d_x && d_kern && d_out, BLA_ERR_INVALID, "%s: NULL pointer", who);
	BLA_REQUIRE(aligned16(prepared), BLA_ERR_INVALID, "%s: the prepared matrix is not 16-byte aligned", who);
	bla_status st = check_conv(who, batch, h, w, k, c_in, f_n, stride);
	if (st != BLA_OK) return st;
	const Geometry g = same_geometry(h, w, k, stride);
	const Layout16 L = layout16(h, w, k, stride, false);
	const int cp = round8(c_in);
	const size_t p_bytes = padded_bytes(batch, L.hp, L.wp, cp);
	// the composition's own shape checks (grid and 32-bit index limits), still before the device is asked for
	if ((st = check_pad_shape(batch, c_in, h, w, L.hp, L.wp, L.top, L.left, 1)) != BLA_OK) return st;
	if ((st = check_gathered_shape(f_n, batch, L.hp, L.wp, cp, k, stride, g.ho, g.wo, ep_bias_stride)) != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	void* ws = nullptr;
	st = ensure_workspace(p_bytes + kernels_bytes(f_n, k, cp), &ws);
	if (st != BLA_OK) return st;
	unsigned char* base = (unsigned char*)ws;
	uint16_t* P = (uint16_t*)base;
	uint16_t* A = (uint16_t*)(base + p_bytes);
	hipStream_t s = pick_stream(stream);
	if ((st = launch_pad(s, d_x, P, batch, c_in, h, w, L.hp, L.wp, L.top, L.left, 1)) != BLA_OK) return st;
	if (!prepared && (st = launch_kernels(s, d_kern, A, f_n, c_in, k, 0)) != BLA_OK) return st;
	return launch_gathered(s, prepared ? prepared : A, f_n, P, batch, L.hp, L.wp, cp, k, stride, g.ho, g.wo, d_out, ep_bias, ep_bias_stride);
}

extern "C" {

bla_status bla_conv2d_backward_batched_f32_as_bf16(void* stream, const float* d_del_y, const float* d_x, const float* d_kern, float* d_del_kern, float* d_del_x, int batch,
                                                   int h, int w, int k, int c_in, int f_n, int stride) {
	const char* who = "bla_conv2d_backward_batched_f32_as_bf16";
	BLA_REQUIRE(d_del_y, BLA_ERR_INVALID, "%s: NULL del_y", who);
	BLA_REQUIRE(!d_del_kern || d_x, BLA_ERR_INVALID, "%s: the weight gradient needs the forward input", who);
	BLA_REQUIRE(!d_del_x || d_kern, BLA_ERR_INVALID, "%s: the data gradient needs the kernels", who);
	bla_status st = check_conv(who, batch, h, w, k, c_in, f_n, stride);
	if (st != BLA_OK) return st;
	if (d_del_x && stride != 1 && strict_reference()) {
		set_error("the data gradient is undefined in the reference for stride %d (_col2im, lib/conv.c:80-135)", stride);
		return BLA_ERR_UNDEFINED;
	}
	const Geometry g = same_geometry(h, w, k, stride);
	const Layout16 L = layout16(h, w, k, stride, true);
	const int fp = round8(f_n);
	const long n = (long)batch * g.ho * g.wo;
	BLA_REQUIRE(n < (1L << 31) - 128 && (long)c_in * k * k < (1L << 31), BLA_ERR_INVALID, "%s: %ld output pixels exceed 32-bit indexing", who, n);
	if (d_del_x) {
		if ((st = check_pad_shape(batch, f_n, g.ho, g.wo, L.hp, L.wp, L.top, L.left, L.dilate)) != BLA_OK) return st;
		if ((st = check_gathered_shape(c_in, batch, L.hp, L.wp, fp, k, 1, h, w, 0)) != BLA_OK) return st;
	}
	st = require_ready();
	if (st != BLA_OK) return st;
	// one workspace for both gradients, one behind the other on the stream: [dY16 | G] for the weight gradient, then [P | A] for the data gradient
	const WgradLayout W = wgrad_layout(f_n, c_in, k, (int)n);
	const size_t p_bytes = padded_bytes(batch, L.hp, L.wp, fp);
	const size_t need_w = d_del_kern ? W.dy_bytes + W.g_bytes : 0, need_d = d_del_x ? p_bytes + kernels_bytes(c_in, k, fp) : 0;
	if (!need_w && !need_d) return BLA_OK;
	void* ws = nullptr;
	st = ensure_workspace(need_w > need_d ? need_w : need_d, &ws);
	if (st != BLA_OK) return st;
	unsigned char* base = (unsigned char*)ws;
	hipStream_t s = pick_stream(stream);
	if (d_del_kern && (st = launch_wgrad(s, base, d_del_y, d_x, d_del_kern, h, w, k, c_in, f_n, stride, g, (int)n, 1)) != BLA_OK) return st;
	if (d_del_x) {
		uint16_t* P = (uint16_t*)base;
		uint16_t* A = (uint16_t*)(base + p_bytes);
		if ((st = launch_pad(s, d_del_y, P, batch, f_n, g.ho, g.wo, L.hp, L.wp, L.top, L.left, L.dilate)) != BLA_OK) return st;
		if ((st = launch_kernels(s, d_kern, A, f_n, c_in, k, 1)) != BLA_OK) return st;
		if ((st = launch_gathered(s, A, c_in, P, batch, L.hp, L.wp, fp, k, 1, h, w, d_del_x, nullptr, 0)) != BLA_OK) return st;
	}
	return BLA_OK;
}

bla_status bla_conv2d_weight_gradient_batched_f32_as_bf16(void* stream, const float* d_del_y, const float* d_x, float* d_del_kern, int batch, int h, int w, int k, int c_in,
                                                          int f_n, int stride, int splits) {
	const char* who = "bla_conv2d_weight_gradient_batched_f32_as_bf16";
	BLA_REQUIRE(d_del_y && d_x && d_del_kern, BLA_ERR_INVALID, "%s: NULL pointer", who);
	BLA_REQUIRE(splits >= 0, BLA_ERR_INVALID, "%s: splits %d", who, splits);
	bla_status st = check_conv(who, batch, h, w, k, c_in, f_n, stride);
	if (st != BLA_OK) return st;
	const Geometry g = same_geometry(h, w, k, stride);
	const long n = (long)batch * g.ho * g.wo;
	BLA_REQUIRE(n < (1L << 31) - 128 && (long)c_in * k * k < (1L << 31), BLA_ERR_INVALID, "%s: %ld output pixels exceed 32-bit indexing", who, n);
	st = require_ready();
	if (st != BLA_OK) return st;
	const WgradLayout W = wgrad_layout(f_n, c_in, k, (int)n);
	void* ws = nullptr;
	st = ensure_workspace(W.dy_bytes + W.g_bytes + gemm_bf16_splitk_partial_bytes(f_n, W.ckk, W.np, splits), &ws);
	if (st != BLA_OK) return st;
	return launch_wgrad(pick_stream(stream), (unsigned char*)ws, d_del_y, d_x, d_del_kern, h, w, k, c_in, f_n, stride, g, (int)n, splits);
}

bla_status bla_conv2d_weight_gradient_gathered_bf16(void* stream, const uint16_t* d_q, int hq, int wq, int fp, int top, int left, int dilate, const uint16_t* d_p, int hp, int wp,
                                                    int cp, int batch, int k, int stride, int ho, int wo, int f_n, int c_n, float* d_del_kern, int splits) {
	BLA_REQUIRE(d_q && d_p && d_del_kern, BLA_ERR_INVALID, "bla_conv2d_weight_gradient_gathered_bf16: NULL pointer");
	BLA_REQUIRE(aligned16(d_q) && aligned16(d_p), BLA_ERR_INVALID, "bla_conv2d_weight_gradient_gathered_bf16: an operand is not 16-byte aligned");
	bla_status st = check_wgrad_implicit_shape(hq, wq, fp, top, left, dilate, hp, wp, cp, batch, k, stride, ho, wo, f_n, c_n, splits);
	if (st != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	const WgradImplicitPlan plan = wgrad_implicit_plan(f_n, k, cp, batch * ho * wo, splits);
	void* ws = nullptr;
	st = ensure_workspace(plan.partial_bytes, &ws);
	if (st != BLA_OK) return st;
	return launch_wgrad_implicit(pick_stream(stream), d_q, hq, wq, fp, top, left, dilate, d_p, hp, wp, cp, batch, k, stride, ho, wo, f_n, c_n, d_del_kern, (float*)ws, plan);
}

}  // extern "C"

// prepared: the DATA-GRADIENT matrix (bla_conv_bf16_prepare_kernels(.., 1))
bla_status bla::conv2d_backward_gathered_as_bf16(void* stream, const float* d_del_y, const float* d_x, const float* d_kern, float* d_del_kern, float* d_del_x, int batch,
                                                 int h, int w, int k, int c_in, int f_n, int stride, int splits, const uint16_t* prepared) {
	const char* who = "bla_conv2d_backward_gathered_f32_as_bf16";
	BLA_REQUIRE(d_del_y, BLA_ERR_INVALID, "%s: NULL del_y", who);
	BLA_REQUIRE(aligned16(prepared), BLA_ERR_INVALID, "%s: the prepared matrix is not 16-byte aligned", who);
	BLA_REQUIRE(!d_del_kern || d_x, BLA_ERR_INVALID, "%s: the weight gradient needs the forward input", who);
	BLA_REQUIRE(!d_del_x || d_kern, BLA_ERR_INVALID, "%s: the data gradient needs the kernels", who);
	BLA_REQUIRE(splits >= 0, BLA_ERR_INVALID, "%s: splits %d", who, splits);
	bla_status st = check_conv(who, batch, h, w, k, c_in, f_n, stride);
	if (st != BLA_OK) return st;
	if (d_del_x && stride != 1 && strict_reference()) {
		set_error("the data gradient is undefined in the reference for stride %d (_col2im, lib/conv.c:80-135)", stride);
		return BLA_ERR_UNDEFINED;
	}
	if (!d_del_kern && !d_del_x) return BLA_OK;
	const Geometry g = same_geometry(h, w, k, stride);
	const Layout16 Lp = layout16(h, w, k, stride, false), Lq = layout16(h, w, k, stride, true);
	const int cp = round8(c_in), fp = round8(f_n);
	// the composition's own shape checks, still before the device is asked for
	if ((st = check_pad_shape(batch, f_n, g.ho, g.wo, Lq.hp, Lq.wp, Lq.top, Lq.left, Lq.dilate)) != BLA_OK) return st;
	if (d_del_kern) {
		if ((st = check_pad_shape(batch, c_in, h, w, Lp.hp, Lp.wp, Lp.top, Lp.left, 1)) != BLA_OK) return st;
		if ((st = check_wgrad_implicit_shape(Lq.hp, Lq.wp, fp, Lq.top, Lq.left, Lq.dilate, Lp.hp, Lp.wp, cp, batch, k, stride, g.ho, g.wo, f_n, c_in, splits)) != BLA_OK) return st;
	}
	if (d_del_x && (st = check_gathered_shape(c_in, batch, Lq.hp, Lq.wp, fp, k, 1, h, w, 0)) != BLA_OK) return st;
	st = require_ready();
	if (st != BLA_OK) return st;
	// one workspace: [P | Q | A | partials]
	WgradImplicitPlan plan{};
	if (d_del_kern) plan = wgrad_implicit_plan(f_n, k, cp, batch * g.ho * g.wo, splits);
	const size_t p_bytes = d_del_kern ? padded_bytes(batch, Lp.hp, Lp.wp, cp) : 0, q_bytes = padded_bytes(batch, Lq.hp, Lq.wp, fp);
	const size_t a_bytes = d_del_x ? kernels_bytes(c_in, k, fp) : 0;
	void* ws = nullptr;
	st = ensure_workspace(p_bytes + q_bytes + a_bytes + plan.partial_bytes, &ws);
	if (st != BLA_OK) return st;
	unsigned char* base = (unsigned char*)ws;
	uint16_t* P = (uint16_t*)base;
	uint16_t* Q = (uint16_t*)(base + p_bytes);
	uint16_t* A = (uint16_t*)(base + p_bytes + q_bytes);
	float* partial = (float*)(base + p_bytes + q_bytes + a_bytes);
	hipStream_t s = pick_stream(stream);
	if (d_del_kern && (st = launch_pad(s, d_x, P, batch, c_in, h, w, Lp.hp, Lp.wp, Lp.top, Lp.left, 1)) != BLA_OK) return st;
	if ((st = launch_pad(s, d_del_y, Q, batch, f_n, g.ho, g.wo, Lq.hp, Lq.wp, Lq.top, Lq.left, Lq.dilate)) != BLA_OK) return st;   // once, for both gradients
	if (d_del_kern && (st = launch_wgrad_implicit(s, Q, Lq.hp, Lq.wp, fp, Lq.top, Lq.left, Lq.dilate, P, Lp.hp, Lp.wp, cp, batch, k, stride, g.ho, g.wo, f_n, c_in, d_del_kern,
	                                              partial, plan)) != BLA_OK) return st;
	if (d_del_x) {
		if (!prepared && (st = launch_kernels(s, d_kern, A, f_n, c_in, k, 1)) != BLA_OK) return st;
		if ((st = launch_gathered(s, prepared ? prepared : A, c_in, Q, batch, Lq.hp, Lq.wp, fp, k, 1, h, w, d_del_x, nullptr, 0)) != BLA_OK) return st;
	}
	return BLA_OK;
}

// ---- the batched ResNet block on the bf16 products (include/bla.h): a composition of the entries above and of bla_norm_bf16.hip -------------
// Everything in the context workspace is consumed by a launch that is already on the stream before the next step writes there, so the steps share it from
// its base: forward [A]; backward [Q2 | A | partials].  The two 1 x 1 residual entries size and lay out the workspace themselves (they may grow it, which
// waits for the device first); nothing of the block's is live in it across those calls, and the base is asked for again behind them.
// The internal form (bla_internal.h): the fp32 internal block's two flags -- RESNET_TDENSE_READY: ws->tdense is already filled; RESNET_DEFER_TIME_GRADS: d_dtb
// receives the per-image channel sums and the caller forms the time gradients -- and optional prepared kernel matrices (prep NULL, or a NULL field: the
// block prepares that matrix itself in the workspace).  The public entries pass no flags and no matrices.
bla_status bla::resnet_forward_bf16(void* stream, int batch, const float* d_x, const float* d_temb, const bla_resnet_params* p, const unsigned char* d_drop,
                                    const bla_resnet_ws* ws, float* d_result, int h, int w, int cin, int cout, int k, int tdim, int group_size,
                                    const bla_resnet_bf16_maps* maps, int flags, const ResnetBf16Prep* prep) {
	const char* who = "bla_resnet_forward_batched_bf16";
	const ResnetBf16Prep none = {};
	const ResnetBf16Prep& pr = prep ? *prep : none;
	BLA_REQUIRE(batch > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && k > 0 && tdim > 0 && group_size > 0, BLA_ERR_INVALID, "%s: extent <= 0", who);
	BLA_REQUIRE(d_x && d_temb && p && d_drop && ws && d_result && maps && p->conv1 && p->conv2 && p->time_w && p->time_b, BLA_ERR_INVALID, "%s: NULL operand", who);
	BLA_REQUIRE(ws->mu1 && ws->sd1 && ws->c1 && ws->tdense && ws->mu2 && ws->sd2 && ws->c2, BLA_ERR_INVALID, "%s: NULL workspace field", who);
	BLA_REQUIRE(maps->p1 && maps->p2 && aligned16(maps->p1) && aligned16(maps->p2), BLA_ERR_INVALID, "%s: a map is NULL or off 16-byte alignment", who);
	BLA_REQUIRE(cin == cout || (p->res && ws->res), BLA_ERR_INVALID, "%s: Cin != Cout needs the residual 1x1 kernels and workspace", who);
	const Layout16 L = layout16(h, w, k, 1, false);
	const int cpi = round8(cin), cpo = round8(cout);
	const bla_conv_bf16_map p1{maps->p1, L.hp, L.wp, cpi, L.top, L.left, 1}, p2{maps->p2, L.hp, L.wp, cpo, L.top, L.left, 1};
	bla_status st;
	if ((st = check_chain_map("p1", p1, batch, h, w)) != BLA_OK || (st = check_chain_map("p2", p2, batch, h, w)) != BLA_OK) return st;
	if ((st = check_gathered_shape(cout, batch, L.hp, L.wp, cpi, k, 1, h, w, cout)) != BLA_OK || (st = check_gathered_shape(cout, batch, L.hp, L.wp, cpo, k, 1, h, w, 0)) != BLA_OK) return st;
	if ((st = require_ready()) != BLA_OK) return st;
	if ((st = bla_group_norm_relu_bf16_map(stream, batch, d_x, cin, group_size, h, w, nullptr, ws->sd1, ws->mu1, nullptr, &p1)) != BLA_OK) return st;
	if (!(flags & RESNET_TDENSE_READY)) {
		bla_gemm_epilogue tep = {};
		tep.alpha = 1.f; tep.bias_col = p->time_b;
		if ((st = bla_gemm_f32(stream, 0, 0, batch, cout, tdim, d_temb, tdim, p->time_w, cout, ws->tdense, cout, &tep)) != BLA_OK) return st;
	}
	void* base = nullptr;
	if ((st = ensure_workspace(kernels_bytes(cout, k, cpi > cpo ? cpi : cpo), &base)) != BLA_OK) return st;
	uint16_t* A = (uint16_t*)base;
	if (!pr.k1_fwd && (st = bla_conv_bf16_prepare_kernels(stream, p->conv1, A, cout, cin, k, 0)) != BLA_OK) return st;
	if ((st = bla_conv2d_gathered_bf16(stream, pr.k1_fwd ? pr.k1_fwd : A, cout, p1.d, batch, L.hp, L.wp, cpi, k, 1, h, w, ws->c1, ws->tdense, cout)) != BLA_OK) return st;
	if ((st = bla_group_norm_relu_bf16_map(stream, batch, ws->c1, cout, group_size, h, w, d_drop, ws->sd2, ws->mu2, nullptr, &p2)) != BLA_OK) return st;
	if (!pr.k2_fwd && (st = bla_conv_bf16_prepare_kernels(stream, p->conv2, A, cout, cout, k, 0)) != BLA_OK) return st;
	if ((st = bla_conv2d_gathered_bf16(stream, pr.k2_fwd ? pr.k2_fwd : A, cout, p2.d, batch, L.hp, L.wp, cpo, k, 1, h, w, ws->c2, nullptr, 0)) != BLA_OK) return st;
	const float* r = d_x;
	if (cin != cout) {
		if ((st = conv2d_forward_as_bf16(stream, d_x, p->res, ws->res, batch, h, w, 1, cin, cout, 1, nullptr, 0, pr.res_fwd)) != BLA_OK) return st;
		r = ws->res;
	}
	return bla_sum_f32(stream, d_result, ws->c2, r, (size_t)batch * cout * h * w);
}

bla_status bla::resnet_backward_bf16(void* stream, int batch, const float* d_del_out, const float* d_x, const float* d_temb, const bla_resnet_params* p,
                                     const bla_resnet_ws* ws, const bla_resnet_grads* g, const bla_resnet_scratch* sc, float* d_dtb, float* d_del_x, int h, int w,
                                     int cin, int cout, int k, int tdim, int group_size, const bla_resnet_bf16_maps* maps, int splits, int flags,
                                     const ResnetBf16Prep* prep) {
	const char* who = "bla_resnet_backward_batched_bf16";
	const ResnetBf16Prep none = {};
	const ResnetBf16Prep& pr = prep ? *prep : none;
	BLA_REQUIRE(batch > 0 && h > 0 && w > 0 && cin > 0 && cout > 0 && k > 0 && tdim > 0 && group_size > 0, BLA_ERR_INVALID, "%s: extent <= 0", who);
	BLA_REQUIRE(splits >= 0, BLA_ERR_INVALID, "%s: splits %d", who, splits);
	BLA_REQUIRE(d_del_out && d_x && d_temb && p && ws && g && sc && d_dtb && maps && p->conv1 && p->conv2 && g->conv1 && g->conv2 && g->time_w && g->time_b && sc->g_out_a &&
	            sc->g_out_b && sc->g_in, BLA_ERR_INVALID, "%s: NULL operand", who);
	BLA_REQUIRE(ws->mu1 && ws->sd1 && ws->c1 && ws->mu2 && ws->sd2, BLA_ERR_INVALID, "%s: NULL workspace field", who);
	BLA_REQUIRE(maps->p1 && maps->p2 && maps->q1 && aligned16(maps->p1) && aligned16(maps->p2) && aligned16(maps->q1), BLA_ERR_INVALID,
	            "%s: a map is NULL or off 16-byte alignment", who);
	BLA_REQUIRE(cin == cout || (p->res && g->res), BLA_ERR_INVALID, "%s: Cin != Cout needs the residual 1x1 kernels and their gradient", who);
	const Layout16 Lp = layout16(h, w, k, 1, false), Lq = layout16(h, w, k, 1, true);
	const int cpi = round8(cin), cpo = round8(cout), hw = h * w;
	const bla_conv_bf16_map p1{maps->p1, Lp.hp, Lp.wp, cpi, Lp.top, Lp.left, 1}, p2{maps->p2, Lp.hp, Lp.wp, cpo, Lp.top, Lp.left, 1};
	const bla_conv_bf16_map q1{maps->q1, Lq.hp, Lq.wp, cpo, Lq.top, Lq.left, Lq.dilate};
	bla_status st;
	if ((st = check_pad_shape(batch, cout, h, w, Lq.hp, Lq.wp, Lq.top, Lq.left, Lq.dilate)) != BLA_OK) return st;
	if ((st = check_wgrad_implicit_shape(Lq.hp, Lq.wp, cpo, Lq.top, Lq.left, Lq.dilate, Lp.hp, Lp.wp, cpo, batch, k, 1, h, w, cout, cout, splits)) != BLA_OK) return st;
	if ((st = check_wgrad_implicit_shape(Lq.hp, Lq.wp, cpo, Lq.top, Lq.left, Lq.dilate, Lp.hp, Lp.wp, cpi, batch, k, 1, h, w, cout, cin, splits)) != BLA_OK) return st;
	if ((st = check_gathered_shape(cout, batch, Lq.hp, Lq.wp, cpo, k, 1, h, w, 0)) != BLA_OK || (st = check_gathered_shape(cin, batch, Lq.hp, Lq.wp, cpo, k, 1, h, w, 0)) != BLA_OK) return st;
	if ((st = check_chain_map("p1", p1, batch, h, w)) != BLA_OK || (st = check_chain_map("p2", p2, batch, h, w)) != BLA_OK || (st = check_chain_map("q1", q1, batch, h, w)) != BLA_OK) return st;
	if ((st = require_ready()) != BLA_OK) return st;
	const WgradImplicitPlan plan2 = wgrad_implicit_plan(cout, k, cpo, batch * hw, splits), plan1 = wgrad_implicit_plan(cout, k, cpi, batch * hw, splits);
	const size_t q_bytes = padded_bytes(batch, Lq.hp, Lq.wp, cpo), a_bytes = kernels_bytes(cout > cin ? cout : cin, k, cpo);
	const size_t need = q_bytes + a_bytes + (plan2.partial_bytes > plan1.partial_bytes ? plan2.partial_bytes : plan1.partial_bytes);
	uint16_t *Q2 = nullptr, *A = nullptr;
	float* partial = nullptr;
	auto slots = [&]() -> bla_status {   // asked for again behind every call that lays the workspace out itself (it may have grown, and so moved)
		void* base = nullptr;
		const bla_status s2 = ensure_workspace(need, &base);
		Q2 = (uint16_t*)base;
		A = (uint16_t*)((unsigned char*)base + q_bytes);
		partial = (float*)((unsigned char*)base + q_bytes + a_bytes);
		return s2;
	};
	if ((st = slots()) != BLA_OK) return st;
	hipStream_t s = pick_stream(stream);
	// second chunk: del_out -> Q2, conv2's weight gradient, its data gradient gated by p2 (dropout mask and ReLU's derivative at once: p2 is zero wherever dp was)
	if ((st = bla_conv_bf16_pad(stream, d_del_out, Q2, batch, cout, h, w, Lq.hp, Lq.wp, Lq.top, Lq.left, Lq.dilate)) != BLA_OK) return st;
	if ((st = launch_wgrad_implicit(s, Q2, Lq.hp, Lq.wp, cpo, Lq.top, Lq.left, Lq.dilate, p2.d, Lp.hp, Lp.wp, cpo, batch, k, 1, h, w, cout, cout, g->conv2, partial, plan2)) != BLA_OK)
		return st;
	if (!pr.k2_bwd && (st = bla_conv_bf16_prepare_kernels(stream, p->conv2, A, cout, cout, k, 1)) != BLA_OK) return st;
	bla_conv_bf16_epilogue ep = {};
	ep.gate = p2; ep.out_f32 = sc->g_out_a;
	if ((st = bla_conv2d_gathered_bf16_chained(stream, pr.k2_bwd ? pr.k2_bwd : A, cout, Q2, batch, Lq.hp, Lq.wp, cpo, k, 1, h, w, &ep)) != BLA_OK) return st;
	// (its A / B scratch is the workspace's first bytes: Q2 is consumed by then)
	if ((st = bla_group_norm_ddx_bf16_map(stream, batch, sc->g_out_a, ws->c1, ws->mu2, ws->sd2, cout, group_size, h, w, sc->g_out_b, &q1)) != BLA_OK) return st;
	// time-embedding projection, as the fp32 block forms it: per image the channel sums, their sum over the images, temb^T . dtb
	if ((st = bla_col_sum_f32(stream, sc->g_out_b, batch * cout, hw, d_dtb, BLA_COLSUM_INTENDED)) != BLA_OK) return st;
	if (!(flags & RESNET_DEFER_TIME_GRADS)) {
		if ((st = batch_sum(stream, d_dtb, g->time_b, batch, (size_t)cout)) != BLA_OK) return st;
		if ((st = bla_gemm_f32(stream, 1, 0, tdim, cout, batch, d_temb, tdim, d_dtb, cout, g->time_w, cout, nullptr)) != BLA_OK) return st;
	}
	// first chunk
	if ((st = slots()) != BLA_OK) return st;
	if ((st = launch_wgrad_implicit(s, q1.d, Lq.hp, Lq.wp, cpo, Lq.top, Lq.left, Lq.dilate, p1.d, Lp.hp, Lp.wp, cpi, batch, k, 1, h, w, cout, cin, g->conv1, partial, plan1)) != BLA_OK)
		return st;
	const float* addend = d_del_out;
	if (cin != cout) {   // the residual 1 x 1: its weight gradient always, its data gradient (the last norm gradient's addend) when del_x is wanted
		void* g_res = nullptr;
		if (d_del_x && (st = ensure_workspace2((size_t)batch * cin * hw * sizeof(float), &g_res)) != BLA_OK) return st;
		if ((st = conv2d_backward_gathered_as_bf16(stream, d_del_out, d_x, p->res, g->res, (float*)g_res, batch, h, w, 1, cin, cout, 1, splits, pr.res_bwd)) != BLA_OK) return st;
		addend = (const float*)g_res;
	}
	if (!d_del_x) return BLA_OK;
	if ((st = slots()) != BLA_OK) return st;
	if (!pr.k1_bwd && (st = bla_conv_bf16_prepare_kernels(stream, p->conv1, A, cout, cin, k, 1)) != BLA_OK) return st;
	ep.gate = p1; ep.out_f32 = sc->g_in;
	if ((st = bla_conv2d_gathered_bf16_chained(stream, pr.k1_bwd ? pr.k1_bwd : A, cin, q1.d, batch, Lq.hp, Lq.wp, cpo, k, 1, h, w, &ep)) != BLA_OK) return st;
	return bla_group_norm_ddx_gated_batched_f32(stream, batch, sc->g_in, d_del_x, d_x, ws->mu1, ws->sd1, cin, group_size, hw, nullptr, addend);
}
