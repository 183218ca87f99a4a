// bla_optim.hip -- fused Adam / AdamW over a flat parameter bucket, the exponential moving average of a bucket, and global-norm gradient clipping
// without a host round trip (sum of squares of the buckets, the clipping coefficient formed on the device, Adam reading its grad_scale from there).
//
// model/cifar_unet.c's train() allocates the two moment sets of Adam (:1887-1888) and never uses them; this is the update they were for.
// One pass over the data: p, g, m, v are read once and p, m, v written once (7 streams, 28 bytes per parameter, nothing to compute): the roofline
// is HBM.  The update is torch.optim.AdamW(foreach=False)'s, step for step:
//   g = grad_scale * grad;  p *= 1 - lr * wd;  m = lerp(m, g, 1 - beta1);  v = v * beta2 + (1 - beta2) * g * g;
//   p += -(lr / (1 - beta1^t)) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps)
// with the scalars formed in double on the host and rounded to fp32 once, as torch does with its Python-float scalars.  lerp is torch's CPU form,
// fma(w, g - m, m) for w < 0.5 and fma(w - 1, g - m, g) otherwise.
//
// The exponential moving average of the parameters that DDPM samples from (Ho et al. 2020) is the same shape of pass with 3 streams: e read,
// p read, e written (12 bytes per parameter):  e <- e + w (p - e),  w = 1 - decay, each operation rounded on its own.
#include "bla_internal.h"
#include <cmath>

namespace bla {
namespace {

constexpr int kThreads = 256;

struct AdamArgs { float gs, decay, w1, b2, omb2, step_size, bc2_sqrt, eps; int small_w; };

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, const AdamArgs& a) {
#pragma clang fp contract(off)   // every step rounded on its own, as torch's in-place ops: p * decay contracted into the last line's add measured
                                 // 1e-6 of max|p| away from torch after 20 steps (1.2e-7 without weight decay)
	g = a.gs * g;
	p = p * a.decay;
	m = a.small_w ? fmaf(a.w1, g - m, m) : fmaf(a.w1 - 1.0f, g - m, g);
	v = v * a.b2 + a.omb2 * g * g;
	p = p + (-a.step_size) * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}
__device__ __forceinline__ void adam4(float4& p, const float4 g, float4& m, float4& v, const AdamArgs& a) {
	adam1(p.x, g.x, m.x, v.x, a); adam1(p.y, g.y, m.y, v.y, a); adam1(p.z, g.z, m.z, v.z, a); adam1(p.w, g.w, m.w, v.w, a);
}

// Elements [head, head + 4 * n4) as float4 (16-byte aligned in all four buckets), two float4 per stream and lane per iteration (the form the
// repo's three-stream ops measured fastest, bla_elementwise.hip); the scalar elements in front and behind one per lane.
// gs (may be NULL): grad_scale read from device memory, once per lane, in place of a.gs.
__global__ void __launch_bounds__(kThreads) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                        size_t n, size_t head, size_t n4, AdamArgs a, const float* __restrict__ gs) {
	if (gs) a.gs = *gs;
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	float4* p4 = reinterpret_cast<float4*>(p + head);
	const float4* g4 = reinterpret_cast<const float4*>(g + head);
	float4* m4 = reinterpret_cast<float4*>(m + head);
	float4* v4 = reinterpret_cast<float4*>(v + head);
	const size_t n8 = n4 / 2;
	for (size_t i = tid; i < n8; i += stride) {
		float4 p0 = p4[2 * i], p1 = p4[2 * i + 1], m0 = m4[2 * i], m1 = m4[2 * i + 1], v0 = v4[2 * i], v1 = v4[2 * i + 1];
		const float4 g0 = g4[2 * i], g1 = g4[2 * i + 1];
		adam4(p0, g0, m0, v0, a); adam4(p1, g1, m1, v1, a);
		p4[2 * i] = p0; p4[2 * i + 1] = p1; m4[2 * i] = m0; m4[2 * i + 1] = m1; v4[2 * i] = v0; v4[2 * i + 1] = v1;
	}
	for (size_t i = n8 * 2 + tid; i < n4; i += stride) {
		float4 pp = p4[i], mm = m4[i], vv = v4[i];
		adam4(pp, g4[i], mm, vv, a);
		p4[i] = pp; m4[i] = mm; v4[i] = vv;
	}
	const size_t body_end = head + 4 * n4, rest = head + (n - body_end);
	for (size_t k = tid; k < rest; k += stride) {
		const size_t e = k < head ? k : body_end + (k - head);
		float pp = p[e], mm = m[e], vv = v[e];
		adam1(pp, g[e], mm, vv, a);
		p[e] = pp; m[e] = mm; v[e] = vv;
	}
}

__device__ __forceinline__ float ema1(float e, float p, float w) {
#pragma clang fp contract(off)   // e + w * (p - e) with every operation rounded: bit-equal to numpy float32
	return e + w * (p - e);
}
__device__ __forceinline__ float4 ema4(const float4 e, const float4 p, float w) {
	return make_float4(ema1(e.x, p.x, w), ema1(e.y, p.y, w), ema1(e.z, p.z, w), ema1(e.w, p.w, w));
}

// adam_kernel's split: [head, head + 4 * n4) as float4, two per stream and lane per iteration; the scalar elements in front and behind one per lane
__global__ void __launch_bounds__(kThreads) ema_kernel(float* __restrict__ e, const float* __restrict__ p, size_t n, size_t head, size_t n4, float w) {
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	float4* e4 = reinterpret_cast<float4*>(e + head);
	const float4* p4 = reinterpret_cast<const float4*>(p + head);
	const size_t n8 = n4 / 2;
	for (size_t i = tid; i < n8; i += stride) {
		const float4 e0 = e4[2 * i], e1 = e4[2 * i + 1], p0 = p4[2 * i], p1 = p4[2 * i + 1];
		e4[2 * i] = ema4(e0, p0, w); e4[2 * i + 1] = ema4(e1, p1, w);
	}
	for (size_t i = n8 * 2 + tid; i < n4; i += stride) e4[i] = ema4(e4[i], p4[i], w);
	const size_t body_end = head + 4 * n4, rest = head + (n - body_end);
	for (size_t k = tid; k < rest; k += stride) {
		const size_t i = k < head ? k : body_end + (k - head);
		e[i] = ema1(e[i], p[i], w);
	}
}

// Sum of squares of a bucket in double, bit-reproducible: workgroup k sums its grid-stride share (four float4 per lane and iteration in the body
// [head, head + 4 * n4), 16-byte aligned; the scalar elements in front and behind go to the first lanes of workgroup 0) lane by lane, then over the
// lanes of a wave by shuffles, then over its waves in order, and writes partial[k]: no atomics, every order fixed by the launch shape alone.
constexpr int kSumsqUnroll = 4;
__global__ void __launch_bounds__(kThreads) sumsq_partial_kernel(const float* __restrict__ a, size_t n, size_t head, size_t n4, double* __restrict__ partial) {
	__shared__ double part[kThreads / 64];
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	const float4* a4 = reinterpret_cast<const float4*>(a + head);
	double s = 0;
	const size_t nu = n4 / kSumsqUnroll;
	for (size_t i = tid; i < nu; i += stride) {
		float4 x[kSumsqUnroll];
#pragma unroll
		for (int k = 0; k < kSumsqUnroll; k++) x[k] = a4[kSumsqUnroll * i + k];
#pragma unroll
		for (int k = 0; k < kSumsqUnroll; k++) {
			s = fma((double)x[k].x, (double)x[k].x, s); s = fma((double)x[k].y, (double)x[k].y, s);
			s = fma((double)x[k].z, (double)x[k].z, s); s = fma((double)x[k].w, (double)x[k].w, s);
		}
	}
	for (size_t i = nu * kSumsqUnroll + tid; i < n4; i += stride) {
		const float4 x = a4[i];
		s = fma((double)x.x, (double)x.x, s); s = fma((double)x.y, (double)x.y, s); s = fma((double)x.z, (double)x.z, s); s = fma((double)x.w, (double)x.w, s);
	}
	const size_t body_end = head + 4 * n4, rest = head + (n - body_end);
	for (size_t k = tid; k < rest; k += stride) {
		const double x = a[k < head ? k : body_end + (k - head)];
		s = fma(x, x, s);
	}
	for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
	if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = s;
	__syncthreads();
	if (threadIdx.x == 0) {
		double t = 0;
		for (int w = 0; w < kThreads / 64; w++) t += part[w];
		partial[blockIdx.x] = t;
	}
}

// acc[0] += partial[0] + partial[1] + ... in index order (one lane adds; the others only stage the partials in LDS)
__global__ void __launch_bounds__(kThreads) sumsq_combine_kernel(const double* __restrict__ partial, int count, double* __restrict__ acc) {
	__shared__ double part[BLA_SUMSQ_SCRATCH_DOUBLES];
	for (int i = threadIdx.x; i < count; i += blockDim.x) part[i] = partial[i];
	__syncthreads();
	if (threadIdx.x == 0) {
		double t = 0;
		for (int i = 0; i < count; i++) t += part[i];
		acc[0] += t;
	}
}

// torch.nn.utils.clip_grad_norm_'s coefficient times grad_scale, in double, one lane
__global__ void clip_scale_kernel(const double* __restrict__ sumsq, float grad_scale, float max_norm, float* __restrict__ scale, float* __restrict__ norm_out) {
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	const double norm = fabs((double)grad_scale) * sqrt(sumsq[0]);
	const double coef = (double)max_norm / (norm + 1e-6);
	scale[0] = (float)((double)grad_scale * (coef > 1.0 ? 1.0 : coef));
	if (norm_out) norm_out[0] = (float)norm;
}

// workgroups for a pass of n4 float4 taken two per lane: two workgroups per CU at most (what Adam measured fastest)
unsigned pass_blocks(size_t n4) {
	const size_t need = (n4 / 2 + kThreads - 1) / kThreads, cap = 2 * (size_t)(ctx().num_cus > 0 ? ctx().num_cus : 256);
	return (unsigned)(need < 1 ? 1 : (need > cap ? cap : need));
}

// grad_scale by value, or from d_grad_scale (device memory) when that is not NULL
bla_status launch_adam(void* stream, float* d_params, const float* d_grads, float* d_m, float* d_v, size_t n, float lr, float beta1, float beta2, float eps,
                       float weight_decay, float grad_scale, const float* d_grad_scale, int step) {
	bla_status st = require_ready();
	if (st) return st;
	if (n == 0) return BLA_OK;
	BLA_REQUIRE(d_params && d_grads && d_m && d_v, BLA_ERR_INVALID, "null operand");
	BLA_REQUIRE(step >= 1, BLA_ERR_INVALID, "step %d (the first step is 1)", step);
	BLA_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, BLA_ERR_INVALID, "betas (%g, %g) outside [0, 1)", beta1, beta2);
	const uintptr_t mis = (uintptr_t)d_params % 16;
	BLA_REQUIRE(mis % 4 == 0, BLA_ERR_INVALID, "parameters not 4-byte aligned");
	const bool same = (uintptr_t)d_grads % 16 == mis && (uintptr_t)d_m % 16 == mis && (uintptr_t)d_v % 16 == mis;
	size_t head = same ? ((16 - mis) % 16) / 4 : n;   // buckets of different alignment: every element on the scalar path
	if (head > n) head = n;
	const size_t n4 = (n - head) / 4;
	const double bc1 = 1.0 - std::pow((double)beta1, step), bc2 = 1.0 - std::pow((double)beta2, step);
	const double w1 = 1.0 - (double)beta1;
	AdamArgs a = {grad_scale, (float)(1.0 - (double)lr * weight_decay), (float)w1, beta2, (float)(1.0 - (double)beta2), (float)((double)lr / bc1),
	              (float)std::sqrt(bc2), eps, std::fabs(w1) < 0.5 ? 1 : 0};
	hipLaunchKernelGGL(adam_kernel, dim3(pass_blocks(n4)), dim3(kThreads), 0, pick_stream(stream), d_params, d_grads, d_m, d_v, n, head, n4, a, d_grad_scale);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

}  // namespace
}  // namespace bla

using namespace bla;

extern "C" {

bla_status bla_adam_f32(void* stream, float* d_params, const float* d_grads, float* d_m, float* d_v, size_t n, float lr, float beta1, float beta2, float eps,
                        float weight_decay, float grad_scale, int step) {
	return launch_adam(stream, d_params, d_grads, d_m, d_v, n, lr, beta1, beta2, eps, weight_decay, grad_scale, nullptr, step);
}

bla_status bla_adam_scaled_f32(void* stream, float* d_params, const float* d_grads, float* d_m, float* d_v, size_t n, float lr, float beta1, float beta2, float eps,
                               float weight_decay, const float* d_grad_scale, int step) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(d_grad_scale && (uintptr_t)d_grad_scale % 4 == 0, BLA_ERR_INVALID, "grad_scale pointer null or not 4-byte aligned");
	return launch_adam(stream, d_params, d_grads, d_m, d_v, n, lr, beta1, beta2, eps, weight_decay, 0.f, d_grad_scale, step);
}

bla_status bla_sumsq_accumulate_f32(void* stream, const float* d_a, size_t n, double* d_acc, double* d_scratch) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(d_acc && d_scratch && ((uintptr_t)d_acc | (uintptr_t)d_scratch) % 8 == 0, BLA_ERR_INVALID, "accumulator or scratch null or not 8-byte aligned");
	if (n == 0) return BLA_OK;
	BLA_REQUIRE(d_a && (uintptr_t)d_a % 4 == 0, BLA_ERR_INVALID, "bucket null or not 4-byte aligned");
	size_t head = ((16 - (uintptr_t)d_a % 16) % 16) / 4;
	if (head > n) head = n;
	const size_t n4 = (n - head) / 4;
	// four workgroups per CU at most (16 waves, 64 KiB of loads in flight per CU), never more partials than the scratch holds
	const size_t need = (n4 / kSumsqUnroll + kThreads - 1) / kThreads, cus = (size_t)(ctx().num_cus > 0 ? ctx().num_cus : 256);
	const size_t cap = 4 * cus < BLA_SUMSQ_SCRATCH_DOUBLES ? 4 * cus : BLA_SUMSQ_SCRATCH_DOUBLES;
	const unsigned blocks = (unsigned)(need < 1 ? 1 : (need > cap ? cap : need));
	hipStream_t s = pick_stream(stream);
	hipLaunchKernelGGL(sumsq_partial_kernel, dim3(blocks), dim3(kThreads), 0, s, d_a, n, head, n4, d_scratch);
	BLA_HIP(hipGetLastError());
	hipLaunchKernelGGL(sumsq_combine_kernel, dim3(1), dim3(kThreads), 0, s, (const double*)d_scratch, (int)blocks, d_acc);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_clip_scale_f32(void* stream, const double* d_sumsq, float grad_scale, float max_norm, float* d_scale, float* d_norm) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(d_sumsq && d_scale, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(std::isfinite(max_norm) && max_norm > 0.f, BLA_ERR_INVALID, "max_norm %g (must be positive and finite)", max_norm);
	hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(64), 0, pick_stream(stream), d_sumsq, grad_scale, max_norm, d_scale, d_norm);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_ema_f32(void* stream, float* d_ema, const float* d_params, size_t n, float decay) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(decay >= 0.f && decay <= 1.f, BLA_ERR_INVALID, "decay %g outside [0, 1]", decay);
	if (n == 0) return BLA_OK;
	BLA_REQUIRE(d_ema && d_params, BLA_ERR_INVALID, "null operand");
	const uintptr_t mis = (uintptr_t)d_ema % 16;
	BLA_REQUIRE(mis % 4 == 0 && (uintptr_t)d_params % 4 == 0, BLA_ERR_INVALID, "buckets not 4-byte aligned");
	size_t head = (uintptr_t)d_params % 16 == mis ? ((16 - mis) % 16) / 4 : n;   // buckets of different alignment: every element on the scalar path
	if (head > n) head = n;
	const size_t n4 = (n - head) / 4;
	const float w = (float)(1.0 - (double)decay);
	hipLaunchKernelGGL(ema_kernel, dim3(pass_blocks(n4)), dim3(kThreads), 0, pick_stream(stream), d_ema, d_params, n, head, n4, w);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

}  // extern "C"
