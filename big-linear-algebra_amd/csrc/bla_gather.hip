// bla_gather.hip -- implicit-GEMM convolution on the direct-to-LDS GEMM pipeline: the gathered-operand kernels (bla_gather_kernel.h; gather modes in
// GatherArgs) and their host side -- tile / split planning and the launches.  Called from bla_conv.hip.
#include "bla_gather_kernel.h"

namespace bla {

// K splits of a gathered weight-gradient product (contraction over (image, pixel), K = batch * HWo, few output tiles).  The tiles are MFMA-bound
// and equally long, so what matters is that every CU gets the SAME number of workgroups: tiles * splits is rounded DOWN to a whole number of
// workgroups per CU (two) -- 9 tiles x 32 splits on 256 CUs
// left 32 CUs with two workgroups and took twice the time of 9 x 28.  A split is a whole number of 16-deep slabs, not of images.
static bool gather_hs(int mode, int M, int N) {
	static const bool use_hs = [] { const char* e = getenv("BLA_CONV_HS"); return !(e && e[0] == '0'); }();
	// mode 3 (forward / data gradient): the half-slab form (172 vs 198 us at 128->128 @32x32 x64).  Mode 4 (weight gradient): also, with its K cut for
	// TWO workgroups per CU (they fit: 32 KB of LDS, under half the registers) -- 183 against 191 us on the older form; cut for one per CU it
	// measured slower (208).  BLA_CONV_HS=1 keeps the weight gradient on the older form, BLA_CONV_HS=0 everything.
	static const bool hs4 = [] { const char* e = getenv("BLA_CONV_HS"); return !(e && e[0] == '1'); }();
	return use_hs && M % 128 == 0 && N % 128 == 0 && (mode == 3 || (mode == 4 && hs4));
}
// mode 4 on the half-slab kernel: a slab's 16 output pixels must sit at the same places relative to its first pixel whatever the slab (bla_gather_kernel.h)
static bool gather4_fixed_offsets(int wo) { return wo == 4 || wo == 8 || (wo >= 16 && wo % 16 == 0); }
static int gather_k_per_split(int mode, int batch, int M, int N, int HWo) {
	const long K = (long)batch * HWo;
	if (mode != 2 && mode != 4) return (int)K;
	const int cus = ctx().num_cus > 0 ? ctx().num_cus : 256;
	const long tiles = (long)((M + 127) / 128) * ((N + 127) / 128);
	// two workgroups per CU on either form.  On the side lane (the U-Net's weight gradients beside the main chain's kernels) ONE: the half-slab weight-gradient
	// kernel takes 108 registers, so one of its workgroups fits a CU BESIDE two of the main chain's gather kernels (188 / 172 registers each) and fills the matrix
	// pipe's bubbles instead of taking one of their two places -- batch-64 backward 9.83 -> 9.33 ms, batch 128 18.7 -> 16.9 (BLA_LANE_SLOTS=2: the old split)
	static const long lane_slots = [] { const char* e = getenv("BLA_LANE_SLOTS"); return e && *e ? atol(e) : 1L; }();
	const long slots = (ctx().side_lane && mode == 4 ? lane_slots : 2L) * cus;
	long splits = slots / tiles;
	const long slabs = K / 16;
	if (splits > slabs / 8) splits = slabs / 8;      // at least 8 slabs per split
	if (splits >= 32) splits &= ~7L;                 // a multiple of 8 where that costs little: the kernel then keeps the tiles of a split on one XCD (shared L2 fetch of del_y)
	if (splits < 1) splits = 1;
	return (int)((slabs + splits - 1) / splits) * 16;
}
// Forward / data gradient on small feature maps (8x8, 4x4: fewer 128x128 tiles than CUs): the contraction over the taps is cut so that about
// one workgroup sits on every CU, at least 8 slabs each; the slabs have the shape of the output and are summed flat.
int gather3_splits(int M, int N, int K) {
	if (!gather_hs(3, M, N)) return 1;
	const int cus = ctx().num_cus > 0 ? ctx().num_cus : 256;
	const long tiles = (long)(M / 128) * (N / 128), slabs = K / 16;
	long splits = cus / tiles;
	if (splits > slabs / 8) splits = slabs / 8;
	if (splits < 1) splits = 1;
	const long per = (slabs + splits - 1) / splits;
	return (int)((slabs + per - 1) / per);
}
// one pass over K: where the tile is stored; taps cut over workgroups (small maps): in the fold of the slabs (gather_fold_epilogue_kernel)
bool gather3_fuses_epilogue(int M, int N, int K) { (void)K; return gather_hs(3, M, N); }

// The fold of a mode-3 product whose taps were cut over workgroups, with the adds the U-Net puts behind the convolution: slabs [split][image][M][HWo]
// summed in split order, + bias[image * stride + row], second output = that + add.  16 bytes per thread.
__global__ void __launch_bounds__(256) gather_fold_epilogue_kernel(const float4* __restrict__ slab, float4* __restrict__ out, int splits, size_t total4, const float* __restrict__ bias,
                                                                    int bias_stride, const float4* __restrict__ add, float4* __restrict__ out2, int M, int hwo4) {
	for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total4; i += (size_t)gridDim.x * 256) {
		float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
		for (int z = 0; z < splits; z++) { const float4 v = slab[(size_t)z * total4 + i]; s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
		if (bias) {
			const size_t row = i / hwo4;
			const int image = (int)(row / M), ch = (int)(row - (size_t)image * M);
			const float b = bias[(size_t)image * bias_stride + ch];
			s.x += b; s.y += b; s.z += b; s.w += b;
		}
		out[i] = s;
		if (out2) { const float4 a = add[i]; out2[i] = make_float4(s.x + a.x, s.y + a.y, s.z + a.z, s.w + a.w); }
	}
}
// LDS of the image-window kernel (mode 7)
static size_t window_lds_bytes(int W) { return W == 32 ? Window<32>::LDS_BYTES : Window<16>::LDS_BYTES; }

// Everything a launch of one gathered product needs but the slab address (a.slab: set by whoever owns the workspace, where slab_floats > 0).
// hs: the half-slab instantiation of modes 3 and 4; window: mode 7's image row width (16 or 32; 0 for the other modes).
namespace { struct GatherPlan { GatherArgs a; dim3 grid; size_t lds, slab_floats; bool hs; int window, mode; }; }

// the part of a plan token (bla_conv_last_plan) a gathered product knows: mode, half-slab ("hs") or older form, window width, K splits, and the site of a
// fused epilogue -- the tile store or the fold of the slabs
static void note_product(const GatherProduct& g, const GatherPlan& p) {
	if (g.mode == 7) conv_plan_note("m7w%d", p.window);
	else if (g.mode == 1) conv_plan_note("m1");
	else conv_plan_note("m%d%s/s%d", g.mode, p.hs ? "hs" : "", p.a.splits);
	if (g.ep.bias || g.ep.out2) conv_plan_note(p.a.splits == 1 ? "/ep=tile" : "/ep=fold");
}

// the fields of a gathered product's GatherArgs that every form shares (gather_plan, gather_gemm_classes)
static GatherArgs gather_args(const GatherProduct& g) {
	GatherArgs a = {};
	a.C = g.C; a.M = g.M; a.N = g.N; a.K = g.K; a.ldc = g.ldc;
	if (g.mode == 4) { a.B = g.A; a.ldb = g.lda; }      // the dense operand (del_y) is the K-contiguous B
	else { a.A = g.A; a.lda = g.lda; }
	a.alpha = 1.f; a.beta = 0.f; a.act = BLA_ACT_NONE;
	a.g_img = g.img; a.g_zero = zero_word(); a.g_ktab = g.ktab; a.g_ntab = g.ntab; a.g_H = g.H; a.g_W = g.W; a.g_HWo = g.HWo; a.g_img_stride = g.img_stride;
	a.g_wo = g.wo;
	a.tiles_m = (g.M + 127) / 128; a.tiles_n = (g.N + 127) / 128;
	return a;
}

// Several forward-shaped products over ONE padded image in one launch (mode 3, half-slab pipeline, whole tiles): the four parity classes of a stride-2
// data gradient.  blockIdx.y = class.  The classes differ in contraction length (4F, 2F, 2F, F for 3x3 kernels); all 4 x tiles workgroups are resident
// at once (two per CU), so the ORDER decides which classes share a CU: longest with shortest, the two middle ones together (cls[] as given: the
// caller sorts).  Needs about two workgroups per CU in total; otherwise the caller runs the classes one by one with their taps cut over workgroups.
bool gather_classes_fit(int ncls, int M, int N) {
	const int cus = ctx().num_cus > 0 ? ctx().num_cus : 256;
	return ncls >= 2 && ncls <= 4 && gather_hs(3, M, N) && (long)ncls * (M / 128) * (N / 128) >= 2L * cus - cus / 2;
}
bla_status gather_gemm_classes(hipStream_t s, const GatherProduct& g, int batch, const GatherClass* cls, const GatherClass* d_cls, int ncls) {
	BLA_REQUIRE(gather_classes_fit(ncls, g.M, g.N) && g.N % 4 == 0 && g.HWo % 4 == 0 && (long)batch * g.img_stride < (1L << 29), BLA_ERR_INVALID, "class launch: M=%d N=%d classes=%d",
	            g.M, g.N, ncls);
	for (int i = 0; i < ncls; i++)
		BLA_REQUIRE(cls[i].K > 0 && cls[i].K % 16 == 0 && (uintptr_t)cls[i].A % 16 == 0, BLA_ERR_INVALID, "class %d: K = %d", i, cls[i].K);
	GatherProduct first = g;
	first.mode = 3; first.A = cls[0].A; first.K = first.lda = cls[0].K; first.ktab = cls[0].ktab; first.C = cls[0].C;
	GatherArgs a = gather_args(first);
	a.splits = 1; a.k_per_split = 1 << 30;
	a.g_ncls = ncls; a.g_cls = d_cls;       // d_cls: the same entries in device memory (the caller's launch wrote them)
	const dim3 grid((unsigned)(a.tiles_m * a.tiles_n), (unsigned)ncls, 1), block(256);
	hipLaunchKernelGGL((gather_kernel<3, true>), grid, block, 2 * (128 + 128) * 16 * sizeof(float), s, a);
	BLA_HIP(hipGetLastError());
	conv_plan_note("m3hs/x%d", ncls);
	return BLA_OK;
}

static bla_status gather_plan(const GatherProduct& g, int batch, GatherPlan* p) {
	const int mode = g.mode, M = g.M, N = g.N, K = g.K, HWo = g.HWo;
	BLA_REQUIRE((mode >= 1 && mode <= 4) || mode == 7, BLA_ERR_INVALID, "gather mode %d", mode);
	if (mode == 7) {   // the image window in LDS (3x3, stride 1): whole 128-pixel tiles inside one image, one pass over K, A = kernels re-ordered [M][(group, tap, channel)]
		const int ch = HWo > 0 ? g.img_stride / HWo : 0;
		BLA_REQUIRE(M % 128 == 0 && N % 128 == 0 && HWo == g.H * g.W && HWo % 128 == 0 && (g.W == 16 || g.W == 32) && ch % 16 == 0 && ch > 0 && K == 9 * ch && g.lda == K &&
		            (uintptr_t)g.A % 16 == 0 && (long)batch * g.img_stride < (1L << 29) && (long)N * M < (1L << 31), BLA_ERR_INVALID,
		            "mode 7 shape (M=%d N=%d K=%d H=%d W=%d C=%d)", M, N, K, g.H, g.W, ch);
	} else {
		BLA_REQUIRE(mode != 3 || (N % 4 == 0 && HWo % 4 == 0 && N >= 4), BLA_ERR_INVALID, "mode 3 needs pixel counts that are multiples of 4");
		BLA_REQUIRE(mode != 4 || M % 4 == 0, BLA_ERR_INVALID, "mode 4 needs a tap count that is a multiple of 4");
		BLA_REQUIRE(M > 0 && N > 0 && K > 0 && K % 16 == 0 && g.lda % 4 == 0 && (uintptr_t)g.A % 16 == 0 && ((mode != 2 && mode != 4) || HWo % 16 == 0), BLA_ERR_INVALID,
		            "gathered product needs K %% 16 == 0 and a 16-byte aligned dense operand (M=%d N=%d K=%d lda=%d)", M, N, K, g.lda);
		BLA_REQUIRE((long)batch * g.img_stride < (mode >= 3 ? (1L << 29) : (1L << 31)) && (long)N < (1L << 31), BLA_ERR_INVALID, "batch too large for 32-bit gather offsets");
	}
	// whole tiles: the half-slab pipeline (fragment sets per k-half, every LDS read and DMA dealt out between MFMAs) -- BLA_CONV_HS=0 keeps the older form
	p->hs = gather_hs(mode, M, N) && (mode != 4 || gather4_fixed_offsets(g.wo));
	p->window = mode == 7 ? g.W : 0; p->mode = mode;
	BLA_REQUIRE(!(g.ep.bias || g.ep.out2) || mode == 7 || (mode == 3 && p->hs), BLA_ERR_INVALID,
	            "the fused convolution epilogue needs the half-slab forward kernel (gather3_fuses_epilogue)");
	GatherArgs& a = p->a;
	a = gather_args(g);
	int splits = 1;
	a.k_per_split = K;
	if (mode == 2 || mode == 4) {
		a.k_per_split = gather_k_per_split(mode, batch, M, N, HWo);
		splits = (int)(((long)batch * HWo + a.k_per_split - 1) / a.k_per_split);
	} else if (mode == 3) {
		splits = gather3_splits(M, N, K);
		a.k_per_split = (K / 16 + splits - 1) / splits * 16;
	}
	a.splits = splits;
	// the epilogue goes into the tile store where there is one pass over K, else into the fold of the slabs (gather_fold)
	if (splits == 1) { a.g_bias = g.ep.bias; a.g_bias_stride = g.ep.bias_stride; a.g_add = g.ep.add; a.g_out2 = g.ep.out2; }
	p->grid = dim3((unsigned)(a.tiles_m * a.tiles_n), 1, (unsigned)splits);
	p->lds = mode == 7 ? window_lds_bytes(g.W) : 2 * (128 + 128) * 16 * sizeof(float);
	p->slab_floats = splits > 1 ? (size_t)splits * M * N : 0;
	return BLA_OK;
}

// The fold behind a product whose contraction was cut over workgroups: the slabs summed in split order into C, with the epilogue where the tile store
// could not apply it
static bla_status gather_fold(hipStream_t s, const GatherPlan& p, const GatherEpilogue& ep) {
	const GatherArgs& a = p.a;
	if (a.splits <= 1) return BLA_OK;
	if (ep.bias || ep.out2) {
		const size_t total4 = (size_t)a.M * a.N / 4, blocks = (total4 + 255) / 256;
		BLA_REQUIRE((uintptr_t)a.C % 16 == 0 && (!ep.out2 || ((uintptr_t)ep.out2 % 16 == 0 && (uintptr_t)ep.add % 16 == 0)), BLA_ERR_INVALID, "unaligned convolution output");
		hipLaunchKernelGGL(gather_fold_epilogue_kernel, dim3((unsigned)(blocks > 4096 ? 4096 : blocks)), dim3(256), 0, s, (const float4*)a.slab, (float4*)a.C, a.splits, total4,
		                   ep.bias, ep.bias_stride, (const float4*)ep.add, (float4*)ep.out2, a.M, a.g_HWo / 4);
		BLA_HIP(hipGetLastError());
		return BLA_OK;
	}
	GemmArgs r = a;
	if (p.mode == 4) { r.M = a.N; r.N = a.M; }   // the slabs hold the transposed tile: [split][N][M] -> C [N][M]
	if (p.mode == 3) r.ldc = r.N;                // C-shaped slabs ([image][M][HWo]): a flat sum
	BLA_HIP(launch_splitk_reduce(r, s));
	return BLA_OK;
}

size_t gather_product_slab_floats(const GatherProduct& g, int batch) {
	GatherPlan p;
	return gather_plan(g, batch, &p) == BLA_OK ? p.slab_floats : 0;
}

bla_status gather_gemm(hipStream_t s, const GatherProduct& g, int batch) {
	GatherPlan p;
	bla_status st = gather_plan(g, batch, &p);
	if (st) return st;
	if (p.slab_floats) {
		void* ws;
		st = ensure_workspace(p.slab_floats * sizeof(float), &ws);
		if (st) return st;
		p.a.slab = (float*)ws;
	}
	const dim3 block(256);
	if (p.window == 32) hipLaunchKernelGGL((gather_kernel<7, true, 32>), p.grid, block, p.lds, s, p.a);
	else if (p.window) hipLaunchKernelGGL((gather_kernel<7, true, 16>), p.grid, block, p.lds, s, p.a);
	else if (p.hs && g.mode == 3) hipLaunchKernelGGL((gather_kernel<3, true>), p.grid, block, p.lds, s, p.a);
	else if (p.hs) hipLaunchKernelGGL((gather_kernel<4, true>), p.grid, block, p.lds, s, p.a);
	else if (g.mode == 1) hipLaunchKernelGGL((gather_kernel<1, false>), p.grid, block, p.lds, s, p.a);
	else if (g.mode == 2) hipLaunchKernelGGL((gather_kernel<2, false>), p.grid, block, p.lds, s, p.a);
	else if (g.mode == 3) hipLaunchKernelGGL((gather_kernel<3, false>), p.grid, block, p.lds, s, p.a);
	else hipLaunchKernelGGL((gather_kernel<4, false>), p.grid, block, p.lds, s, p.a);
	BLA_HIP(hipGetLastError());
	note_product(g, p);
	return gather_fold(s, p, g.ep);
}

// ---- both gradients of one convolution in one launch (gather_pair_kernel) -----------------------------------------------------------------------------
// The weight gradient on the half-slab mode 4, the data gradient on mode 7 or on the half-slab mode 3 (whole 128 x 128 tiles).  The slabs are the caller's:
// it lays both products' slabs out in one workspace.
bool gather_pair_fits(int mode, int M, int N) { return mode == 7 || gather_hs(mode, M, N); }
static bla_status pair_plan(const GatherProduct& g, int batch, float* slab, GatherPlan* p) {
	BLA_REQUIRE(g.mode != 4 || gather4_fixed_offsets(g.wo), BLA_ERR_INVALID, "gather pair: the weight gradient's map is %d pixels wide (4, 8 or a multiple of 16)", g.wo);
	BLA_REQUIRE((g.mode == 3 || g.mode == 4 || g.mode == 7) && gather_pair_fits(g.mode, g.M, g.N), BLA_ERR_INVALID, "gather_plan: mode %d M=%d N=%d", g.mode, g.M, g.N);
	const bla_status st = gather_plan(g, batch, p);
	p->a.slab = p->slab_floats ? slab : nullptr;
	return st;
}
bla_status gather_pair_products(hipStream_t s, int batch, const GatherProduct& w, float* w_slab, const GatherProduct& d, float* d_slab) {
	GatherPlan pw, pd;
	bla_status st = pair_plan(w, batch, w_slab, &pw);
	if (st) return st;
	st = pair_plan(d, batch, d_slab, &pd);
	if (st) return st;
	BLA_REQUIRE(w.mode == 4 && (d.mode == 3 || d.mode == 7) && (pw.slab_floats == 0 || w_slab) && (pd.slab_floats == 0 || d_slab), BLA_ERR_INVALID, "gather_pair: bad plans");
	const int wx = (int)pw.grid.x, wz = (int)pw.grid.z, dx = (int)pd.grid.x, dz = (int)pd.grid.z, blocks_w = wx * wz;
	const dim3 grid((unsigned)(blocks_w + dx * dz)), block(256);
	const size_t lds = pw.lds > pd.lds ? pw.lds : pd.lds;
	if (pd.window == 32) hipLaunchKernelGGL((gather_pair_kernel<7, 32>), grid, block, lds, s, pw.a, pd.a, blocks_w, wx, wz, dx, dz);
	else if (pd.window) hipLaunchKernelGGL((gather_pair_kernel<7, 16>), grid, block, lds, s, pw.a, pd.a, blocks_w, wx, wz, dx, dz);
	else hipLaunchKernelGGL((gather_pair_kernel<3, 0>), grid, block, lds, s, pw.a, pd.a, blocks_w, wx, wz, dx, dz);
	BLA_HIP(hipGetLastError());
	note_product(w, pw); conv_plan_note("+"); note_product(d, pd);
	st = gather_fold(s, pw, w.ep);
	if (st) return st;
	return gather_fold(s, pd, d.ep);
}

}  // namespace bla
