// bla_group_norm.hip -- lib/norm.c's group norm in fp32 and its gradient: the eight kernels, their two launchers and every entry of the family:
// plain, fused for the ResNet block (ReLU, dropout, gate, addend) and over a batch.  Four paths, chosen by gn_route from n_max = the elements of a full group
// and vec = "hw a multiple of 4 and every tensor pointer on 16 bytes" (each launcher forms its own: the forward one also wants `drop` on 4 bytes):
//   one workgroup, 16-byte / scalar   n_max <= kGnThreads * (kGnRegs / 2) = kGnThreads * kGnVec * 4 = 16,384: the group is read once, into registers
//   sliced, 16-byte / scalar          beyond: slices of kGnSlice = 2,048 elements over blockIdx.x; a stats kernel (fp64 partials in the workspace), then an apply kernel
// pad (PadOut, optional): the result once more, inside the zero-padded copy the convolution behind the norm gathers from -- the 16-byte kernels write it in the same
// pass (pad_store4), launch_pad_split follows the scalar ones.  out == NULL (forward): only the dropped form is kept; the 16-byte kernels take that, the scalar ones cannot.
#include "bla_internal.h"

namespace bla {
// ---- group norm, lib/norm.c (quirk Q3 kept: epsilon is integer 0 and "stdev" is the variance) --------------
// One 1024-thread workgroup per group.  Groups of up to 1024*32 elements (the U-Net's 32 channels x 32x32) are read
// ONCE into registers and the mean / variance-about-the-mean / normalise passes of lib/norm.c:14-47 run on the
// register copy; larger groups re-read global memory per pass.  Sums are fp64.
constexpr int kGnThreads = 1024, kGnRegs = 32;

__device__ __forceinline__ double gn_block_sum(double v) {
	__shared__ double sh[kGnThreads / 64];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
	__syncthreads();  // protect sh against the previous call's readers
	if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
	__syncthreads();
	double t = 0;
	for (int i = 0; i < kGnThreads / 64; i++) t += sh[i];
	return t;  // every thread gets the same total (same summation order)
}

template <bool RELU>   // RELU: multi_channel_relu fused behind the normalisation (model/cifar_unet.c:1046-1047,1056-1057)
__global__ void __launch_bounds__(kGnThreads) group_norm_kernel(const float* __restrict__ in, float* __restrict__ out, float* __restrict__ stdevs,
                                                                 float* __restrict__ means, int channels, int group_size, int hw,
                                                                 const unsigned char* __restrict__ drop = nullptr, float* __restrict__ dropped = nullptr) {
	// drop / dropped: _dropout (model/cifar_unet.c:1032-1042, :1058) in the same pass -- dropped = drop ? 0 : out
	int g = blockIdx.x;
	int nch = min(group_size, channels - g * group_size);
	size_t off = (size_t)g * group_size * hw;
	int n = nch * hw;
	const int t = threadIdx.x;
	if (n <= kGnThreads * kGnRegs) {
		float v[kGnRegs];
		double s = 0;
#pragma unroll
		for (int i = 0; i < kGnRegs; i++) { int j = t + i * kGnThreads; v[i] = j < n ? in[off + j] : 0.f; s += v[i]; }
		float mean = (float)(gn_block_sum(s) / (double)n);
		double q = 0;
#pragma unroll
		for (int i = 0; i < kGnRegs; i++) { float d = t + i * kGnThreads < n ? v[i] - mean : 0.f; q += (double)d * d; }
		float var = (float)(gn_block_sum(q) / (double)n);
		if (t == 0) { means[g] = mean; stdevs[g] = var; }
#pragma unroll
		for (int i = 0; i < kGnRegs; i++) {   // (x - mean) / (stdev + 0), lib/norm.c:44
			int j = t + i * kGnThreads;
			float y = (v[i] - mean) / var;
			y = RELU && y < 0.f ? 0.f : y;
			if (j < n) { out[off + j] = y; if (dropped) dropped[off + j] = drop[off + j] ? 0.f : y; }
		}
		return;
	}
	double s = 0;
#pragma unroll 8
	for (int i = t; i < n; i += kGnThreads) s += in[off + i];
	float mean = (float)(gn_block_sum(s) / (double)n);
	double q = 0;
#pragma unroll 8
	for (int i = t; i < n; i += kGnThreads) { float v = in[off + i] - mean; q += (double)v * v; }
	float var = (float)(gn_block_sum(q) / (double)n);
	if (t == 0) { means[g] = mean; stdevs[g] = var; }
#pragma unroll 8
	for (int i = t; i < n; i += kGnThreads) {
		float y = (in[off + i] - mean) / var;
		y = RELU && y < 0.f ? 0.f : y;
		out[off + i] = y;
		if (dropped) dropped[off + i] = drop[off + i] ? 0.f : y;
	}
}

// The register path of the kernel above at 16 bytes per thread: groups of up to 16,384 elements (a multiple of 4, 16-byte aligned), four float4 per
// thread.  The U-Net's 16x16 / 8x8 / 4x4 maps at batch 64 are all of this kind (512 groups of 8,192 elements moved 3.7 TB/s in the scalar form).
constexpr int kGnVec = 4;
// a norm kernel's by-product: the four values it just stored, again at their place inside the zero-padded copy the convolution behind it gathers from
// (PadOut, bla_internal.h; e = flat element index, a multiple of 4; rows are multiples of four pixels, so the four stay in one row)
struct PadArgs { float* dst; int hw, w, wh, plane, ptl; };
__device__ __forceinline__ void pad_store4(const PadArgs& pa, size_t e, float a, float b, float c, float d) {
	const size_t pl = e / (unsigned)pa.hw;
	const int pix = (int)(e - pl * (unsigned)pa.hw), y = pix / pa.w, x = pix - y * pa.w;
	float* q = pa.dst + pl * (size_t)pa.plane + (size_t)y * pa.wh + x + pa.ptl;
	q[0] = a; q[3] = d;
	if (((uintptr_t)(q + 1) & 7) == 0) *reinterpret_cast<float2*>(q + 1) = make_float2(b, c);   // a one-pixel halo puts the middle pair on 8 bytes
	else { q[1] = b; q[2] = c; }
}
template <bool RELU>
__global__ void __launch_bounds__(kGnThreads) group_norm_vec_kernel(const float* __restrict__ in, float* __restrict__ out, float* __restrict__ stdevs,
                                                                     float* __restrict__ means, int channels, int group_size, int hw,
                                                                     const unsigned char* __restrict__ drop, float* __restrict__ dropped, PadArgs pa) {
	const int g = blockIdx.x, t = threadIdx.x;
	const int nch = min(group_size, channels - g * group_size);
	const size_t off = (size_t)g * group_size * hw;
	const int n = nch * hw, n4 = n >> 2;
	const float4* in4 = reinterpret_cast<const float4*>(in + off);
	float4 v[kGnVec];
	double s = 0;
#pragma unroll
	for (int i = 0; i < kGnVec; i++) {
		const int j = t + i * kGnThreads;
		v[i] = j < n4 ? in4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
		s += (double)v[i].x; s += (double)v[i].y; s += (double)v[i].z; s += (double)v[i].w;
	}
	const float mean = (float)(gn_block_sum(s) / (double)n);
	double q = 0;
#pragma unroll
	for (int i = 0; i < kGnVec; i++)
		if (t + i * kGnThreads < n4) {
			const float d0 = v[i].x - mean, d1 = v[i].y - mean, d2 = v[i].z - mean, d3 = v[i].w - mean;
			q += (double)d0 * d0; q += (double)d1 * d1; q += (double)d2 * d2; q += (double)d3 * d3;
		}
	const float var = (float)(gn_block_sum(q) / (double)n);
	if (t == 0) { means[g] = mean; stdevs[g] = var; }
#pragma unroll
	for (int i = 0; i < kGnVec; i++) {
		const int j = t + i * kGnThreads;
		if (j >= n4) continue;
		float y[4] = {(v[i].x - mean) / var, (v[i].y - mean) / var, (v[i].z - mean) / var, (v[i].w - mean) / var};   // (x - mean) / (stdev + 0), lib/norm.c:44
#pragma unroll
		for (int e = 0; e < 4; e++) y[e] = RELU && y[e] < 0.f ? 0.f : y[e];
		if (out) reinterpret_cast<float4*>(out + off)[j] = make_float4(y[0], y[1], y[2], y[3]);   // (out == NULL: only the dropped form is kept)
		if (dropped) {
			const uchar4 d = reinterpret_cast<const uchar4*>(drop + off)[j];
			if (d.x) y[0] = 0.f;
			if (d.y) y[1] = 0.f;
			if (d.z) y[2] = 0.f;
			if (d.w) y[3] = 0.f;
			reinterpret_cast<float4*>(dropped + off)[j] = make_float4(y[0], y[1], y[2], y[3]);
		}
		if (pa.dst) pad_store4(pa, off + 4 * (size_t)j, y[0], y[1], y[2], y[3]);
	}
}
__global__ void __launch_bounds__(kGnThreads) group_norm_ddx_vec_kernel(const float* __restrict__ source, float* __restrict__ dest, const float* __restrict__ data,
                                                                         const float* __restrict__ means, const float* __restrict__ stdevs, int channels,
                                                                         int group_size, int hw, const float* __restrict__ relu_gate, const float* __restrict__ addend, PadArgs pa) {
	const int g = blockIdx.x, t = threadIdx.x;
	const int nch = min(group_size, channels - g * group_size);
	const size_t off = (size_t)g * group_size * hw;
	const int n = nch * hw, n4 = n >> 2;
	const float mean = means[g], sd = stdevs[g];
	float sv[kGnVec][4], nv[kGnVec][4];
	double gs = 0, gws = 0;
#pragma unroll
	for (int i = 0; i < kGnVec; i++) {
		const int j = t + i * kGnThreads;
		const bool live = j < n4;
		const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
		const float4 s4 = live ? reinterpret_cast<const float4*>(source + off)[j] : z, d4 = live ? reinterpret_cast<const float4*>(data + off)[j] : z;
		const float4 g4 = live && relu_gate ? reinterpret_cast<const float4*>(relu_gate + off)[j] : make_float4(1.f, 1.f, 1.f, 1.f);
		const float ss[4] = {s4.x, s4.y, s4.z, s4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w}, gg[4] = {g4.x, g4.y, g4.z, g4.w};
#pragma unroll
		for (int e = 0; e < 4; e++) {
			sv[i][e] = live && !(relu_gate && gg[e] <= 0.f) ? ss[e] : 0.f;
			nv[i][e] = live ? (dd[e] - mean) / sd : 0.f;
			gs += sv[i][e]; gws += (double)nv[i][e] * sv[i][e];
		}
	}
	const float fgs = (float)(gn_block_sum(gs) / (double)n);
	const float fgws = (float)(gn_block_sum(gws) / (double)n);
#pragma unroll
	for (int i = 0; i < kGnVec; i++) {
		const int j = t + i * kGnThreads;
		if (j >= n4) continue;
		float r[4];
#pragma unroll
		for (int e = 0; e < 4; e++) r[e] = (sv[i][e] - fgs - nv[i][e] * fgws) / sd;
		if (addend) { const float4 a = reinterpret_cast<const float4*>(addend + off)[j]; r[0] += a.x; r[1] += a.y; r[2] += a.z; r[3] += a.w; }
		reinterpret_cast<float4*>(dest + off)[j] = make_float4(r[0], r[1], r[2], r[3]);
		if (pa.dst) pad_store4(pa, off + 4 * (size_t)j, r[0], r[1], r[2], r[3]);
	}
}

// lib/norm.c:52-93
__global__ void __launch_bounds__(kGnThreads) group_norm_ddx_kernel(const float* __restrict__ source, float* __restrict__ dest, const float* __restrict__ data,
                                                                     const float* __restrict__ means, const float* __restrict__ stdevs, int channels,
                                                                     int group_size, int hw, const float* __restrict__ relu_gate = nullptr,
                                                                     const float* __restrict__ addend = nullptr) {
	// relu_gate: multi_channel_relu_ddx on the way in (source counts as 0 where the forward ReLU output was <= 0, model/cifar_unet.c:1204);
	// addend: the residual branch's gradient on the way out (dest = group_norm_ddx(...) + addend, :1219)
	int g = blockIdx.x;
	int nch = min(group_size, channels - g * group_size);
	size_t off = (size_t)g * group_size * hw;
	int n = nch * hw;
	const int t = threadIdx.x;
	float mean = means[g], sd = stdevs[g];
	if (n <= kGnThreads * (kGnRegs / 2)) {   // two register copies (source, normalised data): 16 each (32 each spills)
		float sv[kGnRegs / 2], nv[kGnRegs / 2];
		double gs = 0, gws = 0;
#pragma unroll
		for (int i = 0; i < kGnRegs / 2; i++) {
			int j = t + i * kGnThreads;
			sv[i] = j < n ? source[off + j] : 0.f;
			if (relu_gate && j < n && relu_gate[off + j] <= 0.f) sv[i] = 0.f;
			nv[i] = j < n ? (data[off + j] - mean) / sd : 0.f;
			gs += sv[i]; gws += (double)nv[i] * sv[i];
		}
		float fgs = (float)(gn_block_sum(gs) / (double)n);
		float fgws = (float)(gn_block_sum(gws) / (double)n);
#pragma unroll
		for (int i = 0; i < kGnRegs / 2; i++) {
			int j = t + i * kGnThreads;
			if (j < n) { float d = (sv[i] - fgs - nv[i] * fgws) / sd; dest[off + j] = addend ? d + addend[off + j] : d; }
		}
		return;
	}
	double gs = 0, gws = 0;
	// (unrolled: one workgroup walks a whole group, so the loads of several iterations must be in flight together)
#pragma unroll 8
	for (int i = t; i < n; i += kGnThreads) {
		float wgt = (data[off + i] - mean) / sd;
		float sv = relu_gate && relu_gate[off + i] <= 0.f ? 0.f : source[off + i];
		gs += sv;
		gws += (double)wgt * sv;
	}
	float fgs = (float)(gn_block_sum(gs) / (double)n);
	float fgws = (float)(gn_block_sum(gws) / (double)n);
#pragma unroll 8
	for (int i = t; i < n; i += kGnThreads) {
		float nv = (data[off + i] - mean) / sd;
		float sv = relu_gate && relu_gate[off + i] <= 0.f ? 0.f : source[off + i];
		float d = (sv - fgs - nv * fgws) / sd;
		dest[off + i] = addend ? d + addend[off + i] : d;
	}
}

// Groups too large for the one-pass path: one workgroup per group is bound by a single CU's instruction rate (24 us for 32 channels x 32x32),
// so the group is cut into slices of kGnSlice elements over blockIdx.x -- partial sums (fp64) per slice, then every slice's workgroup adds the
// partials in slice order (identical totals everywhere, deterministic) and writes its part.  Same gate / addend options as the kernel above.
constexpr int kGnSlice = 2048, kGnSliceThreads = 256;

// forward pass of a large group, same slicing: partial sum x and sum x^2 in fp64 (x^2 is exact in fp64), then every slice forms
//   mean = (float)(sum x / n)   and   variance about that float mean = (sum x^2 - 2 mean sum x + n mean^2) / n
// -- the two passes of lib/norm.c:26-37 from one pass over memory -- and normalises its part.
template <bool VEC>   // VEC: 16-byte loads / stores (hw a multiple of 4, 16-byte aligned tensors) -- the scalar form moved 3.3 TB/s
__global__ void __launch_bounds__(kGnSliceThreads) group_norm_stats_kernel(const float* __restrict__ in, int channels, int group_size, int hw, double2* partials) {
	const int g = blockIdx.y, slice = blockIdx.x;
	const int nch = min(group_size, channels - g * group_size);
	const size_t off = (size_t)g * group_size * hw;
	const int n = nch * hw, lo = slice * kGnSlice, hi = min(n, lo + kGnSlice);
	double a = 0, b = 0;
	if (VEC) {
		for (int i = lo + 4 * (int)threadIdx.x; i < hi; i += 4 * kGnSliceThreads) {
			const float4 v = *reinterpret_cast<const float4*>(in + off + i);
			const double x0 = v.x, x1 = v.y, x2 = v.z, x3 = v.w;
			a += x0; b += x0 * x0; a += x1; b += x1 * x1; a += x2; b += x2 * x2; a += x3; b += x3 * x3;
		}
	} else
		for (int i = lo + (int)threadIdx.x; i < hi; i += kGnSliceThreads) { double x = in[off + i]; a += x; b += x * x; }
	__shared__ double sh[2][kGnSliceThreads / 64];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) { a += __shfl_down(a, o, 64); b += __shfl_down(b, o, 64); }
	if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = a; sh[1][threadIdx.x >> 6] = b; }
	__syncthreads();
	if (threadIdx.x == 0) {
		double ta = 0, tb = 0;
		for (int i = 0; i < kGnSliceThreads / 64; i++) { ta += sh[0][i]; tb += sh[1][i]; }
		partials[(size_t)g * gridDim.x + slice] = make_double2(ta, tb);
	}
}

template <bool RELU, bool VEC>
__global__ void __launch_bounds__(kGnSliceThreads) group_norm_apply_kernel(const float* __restrict__ in, float* __restrict__ out, float* __restrict__ stdevs,
                                                                            float* __restrict__ means, int channels, int group_size, int hw,
                                                                            const unsigned char* __restrict__ drop, float* __restrict__ dropped,
                                                                            const double2* __restrict__ partials, PadArgs pa) {
	const int g = blockIdx.y, slice = blockIdx.x;
	const int nch = min(group_size, channels - g * group_size);
	const size_t off = (size_t)g * group_size * hw;
	const int n = nch * hw, lo = slice * kGnSlice, hi = min(n, lo + kGnSlice);
	double a = 0, b = 0;
	for (unsigned i = 0; i < gridDim.x; i++) { double2 q = partials[(size_t)g * gridDim.x + i]; a += q.x; b += q.y; }   // slice order: same totals everywhere
	const float mean = (float)(a / (double)n);
	const double m = (double)mean;
	const float var = (float)((b - 2.0 * m * a + (double)n * m * m) / (double)n);
	if (slice == 0 && threadIdx.x == 0) { means[g] = mean; stdevs[g] = var; }
	if (VEC) {
		for (int i = lo + 4 * (int)threadIdx.x; i < hi; i += 4 * kGnSliceThreads) {
			const float4 v = *reinterpret_cast<const float4*>(in + off + i);
			float y[4] = {(v.x - mean) / var, (v.y - mean) / var, (v.z - mean) / var, (v.w - mean) / var};
#pragma unroll
			for (int e = 0; e < 4; e++) y[e] = RELU && y[e] < 0.f ? 0.f : y[e];
			if (out) *reinterpret_cast<float4*>(out + off + i) = make_float4(y[0], y[1], y[2], y[3]);
			if (dropped) {
				const uchar4 d = *reinterpret_cast<const uchar4*>(drop + off + i);
				if (d.x) y[0] = 0.f;
				if (d.y) y[1] = 0.f;
				if (d.z) y[2] = 0.f;
				if (d.w) y[3] = 0.f;
				*reinterpret_cast<float4*>(dropped + off + i) = make_float4(y[0], y[1], y[2], y[3]);
			}
			if (pa.dst) pad_store4(pa, off + (size_t)i, y[0], y[1], y[2], y[3]);
		}
		return;
	}
	for (int i = lo + (int)threadIdx.x; i < hi; i += kGnSliceThreads) {
		float y = (in[off + i] - mean) / var;
		y = RELU && y < 0.f ? 0.f : y;
		out[off + i] = y;
		if (dropped) dropped[off + i] = drop[off + i] ? 0.f : y;
	}
}

template <bool VEC>
__global__ void __launch_bounds__(kGnSliceThreads) group_norm_ddx_stats_kernel(const float* __restrict__ source, const float* __restrict__ data,
                                                                                const float* __restrict__ means, const float* __restrict__ stdevs, int channels,
                                                                                int group_size, int hw, const float* __restrict__ relu_gate, double2* partials) {
	const int g = blockIdx.y, slice = blockIdx.x;
	const int nch = min(group_size, channels - g * group_size);
	const size_t off = (size_t)g * group_size * hw;
	const int n = nch * hw, lo = slice * kGnSlice, hi = min(n, lo + kGnSlice);
	const float mean = means[g], sd = stdevs[g];
	double gs = 0, gws = 0;
	if (VEC) {
		for (int i = lo + 4 * (int)threadIdx.x; i < hi; i += 4 * kGnSliceThreads) {
			const float4 dv = *reinterpret_cast<const float4*>(data + off + i), sv4 = *reinterpret_cast<const float4*>(source + off + i);
			float4 gt = make_float4(1.f, 1.f, 1.f, 1.f);
			if (relu_gate) gt = *reinterpret_cast<const float4*>(relu_gate + off + i);
			const float dd[4] = {dv.x, dv.y, dv.z, dv.w}, ss[4] = {sv4.x, sv4.y, sv4.z, sv4.w}, gg[4] = {gt.x, gt.y, gt.z, gt.w};
#pragma unroll
			for (int e = 0; e < 4; e++) {
				const float wgt = (dd[e] - mean) / sd;
				const float sv = relu_gate && gg[e] <= 0.f ? 0.f : ss[e];
				gs += sv;
				gws += (double)wgt * sv;
			}
		}
	} else
	for (int i = lo + (int)threadIdx.x; i < hi; i += kGnSliceThreads) {
		float wgt = (data[off + i] - mean) / sd;
		float sv = relu_gate && relu_gate[off + i] <= 0.f ? 0.f : source[off + i];
		gs += sv;
		gws += (double)wgt * sv;
	}
	__shared__ double sh[2][kGnSliceThreads / 64];
#pragma unroll
	for (int o = 32; o > 0; o >>= 1) { gs += __shfl_down(gs, o, 64); gws += __shfl_down(gws, o, 64); }
	if ((threadIdx.x & 63) == 0) { sh[0][threadIdx.x >> 6] = gs; sh[1][threadIdx.x >> 6] = gws; }
	__syncthreads();
	if (threadIdx.x == 0) {
		double a = 0, b = 0;
		for (int i = 0; i < kGnSliceThreads / 64; i++) { a += sh[0][i]; b += sh[1][i]; }
		partials[(size_t)g * gridDim.x + slice] = make_double2(a, b);
	}
}

template <bool VEC>
__global__ void __launch_bounds__(kGnSliceThreads) group_norm_ddx_apply_kernel(const float* __restrict__ source, float* __restrict__ dest, const float* __restrict__ data,
                                                                                const float* __restrict__ means, const float* __restrict__ stdevs, int channels,
                                                                                int group_size, int hw, const float* __restrict__ relu_gate,
                                                                                const float* __restrict__ addend, const double2* __restrict__ partials, PadArgs pa) {
	const int g = blockIdx.y, slice = blockIdx.x;
	const int nch = min(group_size, channels - g * group_size);
	const size_t off = (size_t)g * group_size * hw;
	const int n = nch * hw, lo = slice * kGnSlice, hi = min(n, lo + kGnSlice);
	const float mean = means[g], sd = stdevs[g];
	double a = 0, b = 0;
	for (unsigned i = 0; i < gridDim.x; i++) { double2 q = partials[(size_t)g * gridDim.x + i]; a += q.x; b += q.y; }   // slice order: same totals in every workgroup
	const float fgs = (float)(a / (double)n), fgws = (float)(b / (double)n);
	if (VEC) {
		for (int i = lo + 4 * (int)threadIdx.x; i < hi; i += 4 * kGnSliceThreads) {
			const float4 dv = *reinterpret_cast<const float4*>(data + off + i), sv4 = *reinterpret_cast<const float4*>(source + off + i);
			float4 gt = make_float4(1.f, 1.f, 1.f, 1.f), ad = make_float4(0.f, 0.f, 0.f, 0.f);
			if (relu_gate) gt = *reinterpret_cast<const float4*>(relu_gate + off + i);
			if (addend) ad = *reinterpret_cast<const float4*>(addend + off + i);
			const float dd[4] = {dv.x, dv.y, dv.z, dv.w}, ss[4] = {sv4.x, sv4.y, sv4.z, sv4.w}, gg[4] = {gt.x, gt.y, gt.z, gt.w}, aa[4] = {ad.x, ad.y, ad.z, ad.w};
			float r[4];
#pragma unroll
			for (int e = 0; e < 4; e++) {
				const float nv = (dd[e] - mean) / sd;
				const float sv = relu_gate && gg[e] <= 0.f ? 0.f : ss[e];
				const float d = (sv - fgs - nv * fgws) / sd;
				r[e] = addend ? d + aa[e] : d;
			}
			*reinterpret_cast<float4*>(dest + off + i) = make_float4(r[0], r[1], r[2], r[3]);
			if (pa.dst) pad_store4(pa, off + (size_t)i, r[0], r[1], r[2], r[3]);
		}
		return;
	}
	for (int i = lo + (int)threadIdx.x; i < hi; i += kGnSliceThreads) {
		float nv = (data[off + i] - mean) / sd;
		float sv = relu_gate && relu_gate[off + i] <= 0.f ? 0.f : source[off + i];
		float d = (sv - fgs - nv * fgws) / sd;
		dest[off + i] = addend ? d + addend[off + i] : d;
	}
}

// ---- the dispatch, stated once for both launchers ----------------------------------------------------------------------------------------------
enum GnRoute { GN_ONE_VEC, GN_ONE_SCALAR, GN_SLICED_VEC, GN_SLICED_SCALAR };
static GnRoute gn_route(long n_max, bool vec) {   // (the one-workgroup kernels hold up to twice 16,384 elements in registers, but at 12 us against 9 sliced)
	if (n_max > kGnThreads * (kGnRegs / 2)) return vec ? GN_SLICED_VEC : GN_SLICED_SCALAR;
	return n_max <= kGnThreads * kGnVec * 4 && vec ? GN_ONE_VEC : GN_ONE_SCALAR;
}
// PadOut as the 16-byte kernels take it (dst == NULL: no by-product)
static bla_status gn_pad_args(const PadOut* pad, int hw, PadArgs* pa) {
	*pa = PadArgs{};
	if (!pad || !pad->dst) return BLA_OK;
	BLA_REQUIRE(pad->L.plane > 0 && pad->L.w > 0 && hw % pad->L.w == 0 && pad->L.w % 4 == 0, BLA_ERR_INVALID, "padded by-product: bad layout");
	*pa = PadArgs{pad->dst, hw, pad->L.w, pad->L.wh, pad->L.plane, pad->L.pt * pad->L.wh + pad->L.pl};
	return BLA_OK;
}
// a sliced route's grid (slices, groups) and its workspace, one double2 of partial sums per (group, slice); a one-workgroup route keeps grid = (groups)
static bla_status gn_slices(GnRoute route, int groups, long n_max, dim3* grid, double2** partials) {
	if (route == GN_ONE_VEC || route == GN_ONE_SCALAR) return BLA_OK;
	const unsigned slices = (unsigned)((n_max + kGnSlice - 1) / kGnSlice);
	BLA_REQUIRE(groups <= 65535, BLA_ERR_INVALID, "too many groups (%d)", groups);
	*grid = dim3(slices, groups);
	return ensure_workspace((size_t)groups * slices * sizeof(double2), (void**)partials);
}
// behind the launches: the scalar kernels wrote no pad, so a padding pass of `result` follows them (gn_pad_args insists on rows of whole float4: unaligned pointers only)
static bla_status gn_finish(hipStream_t s, GnRoute route, const float* result, const PadOut* pad, int channels, int hw) {
	BLA_HIP(hipGetLastError());
	if (!pad || !pad->dst || route == GN_ONE_VEC || route == GN_SLICED_VEC) return BLA_OK;
	launch_pad_split(s, result, pad->dst, (unsigned)channels, hw / pad->L.w, pad->L.w, pad->L.pt, pad->L.pl, 1, (unsigned)(pad->L.plane / pad->L.wh), (unsigned)pad->L.wh);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}
template <bool RELU>
static bla_status launch_group_norm(hipStream_t s, const float* in, float* out, float* stdevs, float* means, int channels, int group_size, int hw,
                                    const unsigned char* drop, float* dropped, const PadOut* pad = nullptr) {
	const int groups = (channels + group_size - 1) / group_size;
	const long n_max = (long)(channels < group_size ? channels : group_size) * hw;
	PadArgs pa;   // the padded copy of what feeds the next convolution: the dropped output when there is one, else the ReLU output
	bla_status st = gn_pad_args(pad, hw, &pa); if (st) return st;
	const bool vec = hw % 4 == 0 && ((uintptr_t)in | (uintptr_t)out | (uintptr_t)dropped) % 16 == 0 && (uintptr_t)drop % 4 == 0;
	BLA_REQUIRE(out || (dropped && vec && (n_max > kGnThreads * (kGnRegs / 2) || n_max <= kGnThreads * kGnVec * 4)), BLA_ERR_INVALID, "group norm without its plain output needs the 16-byte kernels");
	const GnRoute route = gn_route(n_max, vec);
	dim3 grid(groups); double2* ws = nullptr;
	st = gn_slices(route, groups, n_max, &grid, &ws); if (st) return st;
	switch (route) {
	case GN_ONE_VEC: hipLaunchKernelGGL(group_norm_vec_kernel<RELU>, grid, dim3(kGnThreads), 0, s, in, out, stdevs, means, channels, group_size, hw, drop, dropped, pa); break;
	case GN_ONE_SCALAR: hipLaunchKernelGGL(group_norm_kernel<RELU>, grid, dim3(kGnThreads), 0, s, in, out, stdevs, means, channels, group_size, hw, drop, dropped); break;
	case GN_SLICED_VEC:
		hipLaunchKernelGGL(group_norm_stats_kernel<true>, grid, dim3(kGnSliceThreads), 0, s, in, channels, group_size, hw, ws);
		hipLaunchKernelGGL((group_norm_apply_kernel<RELU, true>), grid, dim3(kGnSliceThreads), 0, s, in, out, stdevs, means, channels, group_size, hw, drop, dropped, ws, pa); break;
	case GN_SLICED_SCALAR:
		hipLaunchKernelGGL(group_norm_stats_kernel<false>, grid, dim3(kGnSliceThreads), 0, s, in, channels, group_size, hw, ws);
		hipLaunchKernelGGL((group_norm_apply_kernel<RELU, false>), grid, dim3(kGnSliceThreads), 0, s, in, out, stdevs, means, channels, group_size, hw, drop, dropped, ws, PadArgs{}); break;
	}
	return gn_finish(s, route, dropped ? dropped : out, pad, channels, hw);
}
static bla_status launch_group_norm_ddx(hipStream_t s, const float* source, float* dest, const float* data, const float* means, const float* stdevs, int channels,
                                        int group_size, int hw, const float* relu_gate, const float* addend, const PadOut* pad = nullptr) {
	const int groups = (channels + group_size - 1) / group_size;
	const long n_max = (long)(channels < group_size ? channels : group_size) * hw;
	PadArgs pa;   // the gradient again, inside the zero-padded copy the data-gradient convolution behind it gathers from
	bla_status st = gn_pad_args(pad, hw, &pa); if (st) return st;
	const bool vec = hw % 4 == 0 && ((uintptr_t)source | (uintptr_t)dest | (uintptr_t)data | (uintptr_t)relu_gate | (uintptr_t)addend) % 16 == 0;
	const GnRoute route = gn_route(n_max, vec);
	dim3 grid(groups); double2* ws = nullptr;
	st = gn_slices(route, groups, n_max, &grid, &ws); if (st) return st;
	switch (route) {
	case GN_ONE_VEC: hipLaunchKernelGGL(group_norm_ddx_vec_kernel, grid, dim3(kGnThreads), 0, s, source, dest, data, means, stdevs, channels, group_size, hw, relu_gate, addend, pa); break;
	case GN_ONE_SCALAR: hipLaunchKernelGGL(group_norm_ddx_kernel, grid, dim3(kGnThreads), 0, s, source, dest, data, means, stdevs, channels, group_size, hw, relu_gate, addend); break;
	case GN_SLICED_VEC:
		hipLaunchKernelGGL(group_norm_ddx_stats_kernel<true>, grid, dim3(kGnSliceThreads), 0, s, source, data, means, stdevs, channels, group_size, hw, relu_gate, ws);
		hipLaunchKernelGGL(group_norm_ddx_apply_kernel<true>, grid, dim3(kGnSliceThreads), 0, s, source, dest, data, means, stdevs, channels, group_size, hw, relu_gate, addend, ws, pa); break;
	case GN_SLICED_SCALAR:
		hipLaunchKernelGGL(group_norm_ddx_stats_kernel<false>, grid, dim3(kGnSliceThreads), 0, s, source, data, means, stdevs, channels, group_size, hw, relu_gate, ws);
		hipLaunchKernelGGL(group_norm_ddx_apply_kernel<false>, grid, dim3(kGnSliceThreads), 0, s, source, dest, data, means, stdevs, channels, group_size, hw, relu_gate, addend, ws, PadArgs{}); break;
	}
	return gn_finish(s, route, dest, pad, channels, hw);
}

// Group norm over a batch [B][C][HW]: the groups of one image never reach into the next, so the batch folds into the channel count when the
// groups divide the channels (B*C channels, same groups) or when an image is one short group (groups of C).  false: ragged, image by image.
static bool fold_groups(int batch, int c, int group_size, int* channels, int* group) {
	if (c % group_size == 0) { *channels = batch * c; *group = group_size; return true; }
	if (c < group_size) { *channels = batch * c; *group = c; return true; }
	return batch == 1 ? (*channels = c, *group = group_size, true) : false;
}

bla_status group_norm_relu_dropout(void* stream, const float* d_in, float* d_relu, const unsigned char* d_drop, float* d_dropped, float* d_stdevs, float* d_means,
                                   int channels, int group_size, int hw, const PadOut* pad) {
	BLA_ENTER();
	BLA_REQUIRE(channels > 0 && group_size > 0 && hw > 0, BLA_ERR_INVALID, "bad group_norm shape channels=%d group=%d hw=%d", channels, group_size, hw);
	BLA_REQUIRE(d_in && (d_relu || d_dropped) && d_stdevs && d_means && (d_drop == nullptr) == (d_dropped == nullptr) && (d_drop || pad), BLA_ERR_INVALID, "null operand");
	return launch_group_norm<true>(pick_stream(stream), d_in, d_relu, d_stdevs, d_means, channels, group_size, hw, d_drop, d_dropped, pad);
}
bla_status group_norm_ddx_gated(void* stream, const float* d_source, float* d_dest, const float* d_data, const float* d_means, const float* d_stdevs,
                                int channels, int group_size, int hw, const float* d_relu_gate, const float* d_addend, const PadOut* pad) {
	BLA_ENTER();
	BLA_REQUIRE(channels > 0 && group_size > 0 && hw > 0, BLA_ERR_INVALID, "bad group_norm shape channels=%d group=%d hw=%d", channels, group_size, hw);
	BLA_REQUIRE(d_source && d_dest && d_data && d_means && d_stdevs, BLA_ERR_INVALID, "null operand");
	return launch_group_norm_ddx(pick_stream(stream), d_source, d_dest, d_data, d_means, d_stdevs, channels, group_size, hw, d_relu_gate, d_addend, pad);
}

bla_status group_norm_relu_dropout_batched(void* stream, int batch, const float* in, float* out, float* sd, float* mu, int c, int gs, int hw, const unsigned char* drop,
                                           float* dropped, const PadOut* pad, bool* pad_done) {
	int ch, grp;
	if (pad_done) *pad_done = false;
	if (fold_groups(batch, c, gs, &ch, &grp)) {
		if ((pad && pad->dst) || !out) { if (pad_done) *pad_done = pad && pad->dst; return group_norm_relu_dropout(stream, in, out, drop, dropped, sd, mu, ch, grp, hw, pad); }
		return drop ? group_norm_relu_dropout(stream, in, out, drop, dropped, sd, mu, ch, grp, hw) : bla_group_norm_relu_f32(stream, in, out, sd, mu, ch, grp, hw);
	}
	const int groups = (c + gs - 1) / gs;
	for (int b = 0; b < batch; b++) {
		const size_t o = (size_t)b * c * hw;
		bla_status st = drop ? group_norm_relu_dropout(stream, in + o, out + o, drop + o, dropped + o, sd + (size_t)b * groups, mu + (size_t)b * groups, c, gs, hw)
		                     : bla_group_norm_relu_f32(stream, in + o, out + o, sd + (size_t)b * groups, mu + (size_t)b * groups, c, gs, hw);
		if (st) return st;
	}
	return BLA_OK;
}
bla_status group_norm_ddx_gated_batched(void* stream, int batch, const float* src, float* dst, const float* data, const float* mu, const float* sd, int c, int gs, int hw,
                                        const float* gate, const float* addend, const PadOut* pad, bool* pad_done) {
	int ch, grp;
	if (pad_done) *pad_done = false;
	if (fold_groups(batch, c, gs, &ch, &grp)) {
		if (pad && pad->dst && pad_done) *pad_done = true;
		return group_norm_ddx_gated(stream, src, dst, data, mu, sd, ch, grp, hw, gate, addend, pad);
	}
	const int groups = (c + gs - 1) / gs;
	for (int b = 0; b < batch; b++) {
		const size_t o = (size_t)b * c * hw;
		bla_status st = group_norm_ddx_gated(stream, src + o, dst + o, data + o, mu + (size_t)b * groups, sd + (size_t)b * groups, c, gs, hw, gate ? gate + o : nullptr,
		                                     addend ? addend + o : nullptr);
		if (st) return st;
	}
	return BLA_OK;
}

}  // namespace bla

using namespace bla;

extern "C" {

bla_status bla_group_norm_f32(void* stream, const float* d_in, float* d_out, float* d_stdevs, float* d_means, int channels, int group_size, int hw) {
	BLA_ENTER();
	BLA_REQUIRE(channels > 0 && group_size > 0 && hw > 0, BLA_ERR_INVALID, "bad group_norm shape channels=%d group=%d hw=%d", channels, group_size, hw);
	BLA_REQUIRE(d_in && d_out && d_stdevs && d_means, BLA_ERR_INVALID, "null operand");
	return launch_group_norm<false>(pick_stream(stream), d_in, d_out, d_stdevs, d_means, channels, group_size, hw, nullptr, nullptr);
}

bla_status bla_group_norm_relu_f32(void* stream, const float* d_in, float* d_out, float* d_stdevs, float* d_means, int channels, int group_size, int hw) {
	BLA_ENTER();
	BLA_REQUIRE(channels > 0 && group_size > 0 && hw > 0, BLA_ERR_INVALID, "bad group_norm shape channels=%d group=%d hw=%d", channels, group_size, hw);
	BLA_REQUIRE(d_in && d_out && d_stdevs && d_means, BLA_ERR_INVALID, "null operand");
	return launch_group_norm<true>(pick_stream(stream), d_in, d_out, d_stdevs, d_means, channels, group_size, hw, nullptr, nullptr);
}

bla_status bla_group_norm_ddx_f32(void* stream, const float* d_source, float* d_dest, const float* d_data, const float* d_means, const float* d_stdevs, int channels, int group_size, int hw) {
	return group_norm_ddx_gated(stream, d_source, d_dest, d_data, d_means, d_stdevs, channels, group_size, hw, nullptr, nullptr);   // (the same checks, no gate, no addend)
}

bla_status bla_group_norm_relu_batched_f32(void* stream, int batch, const float* d_in, float* d_out, float* d_stdevs, float* d_means, int channels, int group_size, int hw) {
	return group_norm_relu_dropout_batched(stream, batch, d_in, d_out, d_stdevs, d_means, channels, group_size, hw, nullptr, nullptr);
}
bla_status bla_group_norm_ddx_gated_batched_f32(void* stream, int batch, const float* d_source, float* d_dest, const float* d_data, const float* d_means,
                                                const float* d_stdevs, int channels, int group_size, int hw, const float* d_relu_gate, const float* d_addend) {
	return group_norm_ddx_gated_batched(stream, batch, d_source, d_dest, d_data, d_means, d_stdevs, channels, group_size, hw, d_relu_gate, d_addend);
}

}  // extern "C"
