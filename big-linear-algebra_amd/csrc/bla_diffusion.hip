// bla_diffusion.hip -- what turns the U-Net of model/cifar_unet.c into a DDPM (Ho, Jain, Abbeel 2020): the linear beta schedule, the forward noising
// of a training batch, the sinusoidal time embedding, the samplers (ancestral, DDIM, DPM-Solver++(2M), each unguided and classifier-free guided) around
// bla_unet_forward_f32, and the held-out evaluation of the trained model (the variational bound, per image).  The six samplers share one walk over the timesteps
// (sample_loop), the guided ones one set-up (guided_start); a new sampler adds a step kernel with its bla_diffusion_*_step_f32 and a choice of timesteps.
//
// The reference has the network (time embedding input, noise prediction, MSE against the noise) but never writes the embedding (:535), never noises
// an image at a timestep and leaves run() empty (:1936).  Random draws come from the Philox streams of bla_philox.h (see include/bla.h), so every
// value written here can be restated from (seed, offset) alone:
//   noise  (seed, pass):  t_b = u32(seed, pass << 32)[b] % T,  eps = normal(seed, pass << 32)[0 .. B*F),  x_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) eps
//   gather (seed, pass):  the same on the batch whose image b is record index[b], mirrored where bernoulli(0.5, seed, (pass << 32) + 2^31 + 2^30)[b] is 1
//   step   (seed, t):     z = normal(seed, (t + 1) << 32)[0 .. B*F) (0 at t = 0);  x <- (x - beta_t / sqrt(1 - abar_t) eps_hat) / sqrt(alpha_t) + sqrt(beta_t) z
//   DDIM   (seed, t):     the same z stream, drawn only when sigma > 0;  x0^ = (x - sqrt(1 - abar_t) eps_hat) / sqrt(abar_t) (clamped to [-1, 1] on request),
//                         x <- sqrt(abar_p) x0^ + sqrt(1 - abar_p - sigma^2) eps_hat + sigma z  (Song, Meng, Ermon 2021; abar_p = 1 past the last step)
//   eval   (seed, t):     eps = normal(seed, offset_base + ((t + 1) << 32))[0 .. B*F), x_t as in noise at the given t; then per image, in double, its term of
//                         the variational bound: F c_t + w_t sum (eps - eps_hat)^2 at t >= 1, the discretised decoder's -sum ln p at t = 0 (Ho et al. eq. 5)
//   DPM++  (no draws):    DPM-Solver++(2M) (Lu et al. 2022), deterministic: x0^ as in DDIM, D = w1 x0^ + w0 x0^_last (second order) or x0^,
//                         x <- (sigma_p / sigma_t) x - alpha_p expm1(-h) D with h = lambda_p - lambda_t, lambda = ln(alpha / sigma); x0^ kept for the next step
// The schedule is formed in double on the host at create time; the kernels read fp32 tables of the per-step coefficients (the evaluation: doubles).  The time embedding is
// the one examples/cifar_unet_gpu.c computes for BLA_UNET_TIMESTEP, evaluated in double: at t ~ 1000 its arguments reach 1000 rad, where an fp32
// product t * w_i alone is off by ~6e-5.
#include "bla_internal.h"
#include "bla_philox.h"
#include <algorithm>
#include <cmath>
#include <vector>

using namespace bla;

struct bla_diffusion {
	int steps = 0;
	std::vector<double> beta, alpha_bar;
	float* table = nullptr;        // device, 5 x steps: sqrt(abar), sqrt(1 - abar), beta / sqrt(1 - abar), 1 / sqrt(alpha), sqrt(beta)
	float* temb = nullptr;         // the sampler's [B][time_dim] embedding workspace (grows on first use)
	size_t temb_floats = 0;
	float* xg = nullptr;           // the guided sampler's model input [2n][C][H][W] and class rows [2n] (grow on first use)
	size_t xg_floats = 0;
	int* rows = nullptr;
	size_t rows_count = 0;
	float* hist = nullptr;         // the DPM-Solver++ samplers' previous x0 prediction, [B][C][H][W] (grows on first use)
	size_t hist_floats = 0;
	double* vlb = nullptr;         // device, 2 x steps: c_t, w_t of bla_diffusion_vlb_weights (0 at t = 0)
	float* ev = nullptr;           // the evaluation loop's eps and x_t, [2][B][C][H][W], and its embedding [B][time_dim] (grow on first use)
	size_t ev_floats = 0;
	float* ev_temb = nullptr;
	size_t ev_temb_floats = 0;
	int prediction = BLA_PREDICT_EPS;   // what the model's output is read as (bla_diffusion_set_objective)
	double min_snr_gamma = 0.0;         // 0: every timestep weighs 1
	std::vector<double> loss_w;         // the loss weights w_t in double (empty until an objective is set: all 1)
	float* loss_w_dev = nullptr;        // device, steps: loss_w rounded to fp32 once (NULL: all 1)
};

namespace {

constexpr int kThreads = 256;
enum { TAB_SQRT_AB = 0, TAB_SQRT_1MAB = 1, TAB_EPS_COEF = 2, TAB_INV_SQRT_A = 3, TAB_SIGMA = 4 };
constexpr int kMaxNoiseBatch = 4096;   // the per-image timesteps sit in LDS

// element i of the embedding of t (examples/cifar_unet_gpu.c time_embedding): w_k = exp(-ln(1e4) k / half), relu(sin(t w_k)) at k, relu(cos(t w_k)) at
// half + k; an odd time_dim leaves its last element 0
__device__ __forceinline__ float temb_value(int t, int i, int dim) {
	const int half = dim / 2;
	if (i >= 2 * half) return 0.f;
	const int k = i < half ? i : i - half;
	const double w = exp(-log(10000.0) * k / half), arg = (double)t * w;
	const double s = i < half ? sin(arg) : cos(arg);
	return (float)(s > 0 ? s : 0);
}

unsigned grid_for(size_t work, size_t cap_per_cu = 8) {
	const size_t cap = cap_per_cu * (size_t)(ctx().num_cus > 0 ? ctx().num_cus : 256);
	size_t b = (work + kThreads - 1) / kThreads;
	return (unsigned)(b < 1 ? 1 : (b > cap ? cap : b));
}

// d_t == NULL: every image at t_const
__global__ void __launch_bounds__(kThreads) time_embedding_kernel(const int* __restrict__ d_t, int t_const, int batch, int dim, float* __restrict__ out) {
	const size_t n = (size_t)batch * dim;
	for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
		out[i] = temb_value(d_t ? d_t[i / dim] : t_const, (int)(i % dim), dim);
}

// x_t = sqrt(abar_t) x0 + sqrt(1 - abar_t) z.  The float4 body has always fused the first product into the sum and the scalar path has always rounded
// both products; each form is spelled out so that neither depends on the contraction heuristics and both keep the bits they have always written.
__device__ __forceinline__ float noise1_vec(float a, float x, float c, float z) {
#pragma clang fp contract(off)
	return fmaf(a, x, c * z);
}
__device__ __forceinline__ float noise1_scalar(float a, float x, float c, float z) {
#pragma clang fp contract(off)
	return a * x + c * z;
}

constexpr int kFlipBit = 1 << 30;   // steps <= 2^24: the bit is free in the LDS copy of t_b
constexpr unsigned long long kFlipOffset = (1ull << 31) + (1ull << 30);   // the flip decisions' Philox blocks, behind the label dropout's (bla.h)

// Noises the batch whose image b is record index[b] (NULL: record b) of data [records][F], mirrored along its rows of `width` where flip is set and
// the image's Bernoulli(0.5) decision is 1.  A record outside [0, records) reads nothing: the image is zero and its label -1.  t_b, eps and the
// embedding are indexed by output position, so they depend on neither the index nor the flips.  x0_out (may be NULL) receives the assembled batch,
// labels_out (with labels) the gathered labels.
__global__ void __launch_bounds__(kThreads) noise_kernel(const float* __restrict__ data, size_t records, const unsigned int* __restrict__ index, int flip, unsigned width,
                                                         const int* __restrict__ labels, int* __restrict__ labels_out, int batch, size_t F, int dim,
                                                         unsigned long long seed, unsigned long long offset, int steps, const float* __restrict__ table,
                                                         int* __restrict__ d_t, float* __restrict__ eps, float* __restrict__ xt, float* __restrict__ temb,
                                                         float* __restrict__ x0_out, int vec) {
	__shared__ int ts[kMaxNoiseBatch];
	for (int b = threadIdx.x; b < batch; b += blockDim.x) {
		const int t = (int)(u32_at(seed, offset, (size_t)b) % (uint32_t)steps);
		ts[b] = flip && u32_at(seed, offset + kFlipOffset, (size_t)b, PHILOX_TAG_BERNOULLI) < 0x80000000u ? t | kFlipBit : t;
		if (blockIdx.x == 0) {
			d_t[b] = t;
			if (labels && labels_out) {
				const size_t r = index ? index[b] : (size_t)b;
				labels_out[b] = r < records ? labels[r] : -1;
			}
		}
	}
	__syncthreads();
	const float* sab = table + TAB_SQRT_AB * steps;
	const float* s1m = table + TAB_SQRT_1MAB * steps;
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	const size_t ne = (size_t)batch * dim;
	for (size_t i = tid; i < ne; i += stride) temb[i] = temb_value(ts[i / dim] & ~kFlipBit, (int)(i % dim), dim);
	const size_t n = (size_t)batch * F;
	if (vec) {   // F % 4 == 0 (width % 4 == 0 when flipping), every pointer 16-byte aligned: Philox block q <-> float4 q, one image per float4
		for (size_t q = tid; q < n / 4; q += stride) {
			const size_t b = (4 * q) / F, p = 4 * q - b * F;
			const int t = ts[b] & ~kFlipBit;
			const float4 z = philox_normal4(philox_block(seed, offset + q, PHILOX_TAG_NORMAL));
			const size_t r = index ? index[b] : b;
			float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
			if (r < records) {
				if (ts[b] & kFlipBit) {   // the float4 at the mirrored position, its components reversed
					const unsigned col = F >> 32 ? (unsigned)(p % width) : (unsigned)p % width;
					const float4 m = *reinterpret_cast<const float4*>(data + r * F + (p - col) + (width - 4 - col));
					x = make_float4(m.w, m.z, m.y, m.x);
				} else {
					x = *reinterpret_cast<const float4*>(data + r * F + p);
				}
			}
			const float a = sab[t], c = s1m[t];
			reinterpret_cast<float4*>(eps)[q] = z;
			reinterpret_cast<float4*>(xt)[q] = make_float4(noise1_vec(a, x.x, c, z.x), noise1_vec(a, x.y, c, z.y), noise1_vec(a, x.z, c, z.z), noise1_vec(a, x.w, c, z.w));
			if (x0_out) reinterpret_cast<float4*>(x0_out)[q] = x;
		}
	} else {
		for (size_t e = tid; e < n; e += stride) {
			const size_t b = e / F;
			size_t p = e - b * F;
			const int t = ts[b] & ~kFlipBit;
			const float z = normal_at(seed, offset, e);
			const size_t r = index ? index[b] : b;
			if (ts[b] & kFlipBit) {
				const unsigned col = F >> 32 ? (unsigned)(p % width) : (unsigned)p % width;
				p = (p - col) + (width - 1 - col);
			}
			const float x = r < records ? data[r * F + p] : 0.f;
			eps[e] = z;
			xt[e] = noise1_scalar(sab[t], x, s1m[t], z);
			if (x0_out) x0_out[e] = x;
		}
	}
}

// What the three step kernels below share.  A GUIDED instance serves the classifier-free guided samplers (Ho & Salimans 2022): the model ran on [2 batch] images, the
// conditioned ones and their null-class copies, eps_c and eps_u are the halves of its output, and x_copy (may be NULL) receives the new x too: the second half of the
// model's next input.  An unguided instance reads eps_u as eps_hat and looks at none of x_copy, eps_c, s, ctable, classes and rows.

// temb_next [(GUIDED ? 2 : 1) batch][dim] = the embedding of t, plus ctable[rows[b]] when GUIDED (nothing added where ctable is NULL or a row is outside [0, classes])
template <bool GUIDED>
__device__ __forceinline__ void next_embedding(float* __restrict__ temb_next, int t, int batch, int dim, const float* __restrict__ ctable, int classes,
                                               const int* __restrict__ rows, size_t tid, size_t stride) {
	const size_t ne = (size_t)(GUIDED ? 2 : 1) * batch * dim;
	for (size_t i = tid; i < ne; i += stride) {
		const float e = temb_value(t, (int)(i % dim), dim);
		const int r = GUIDED && ctable ? rows[i / dim] : -1;
		temb_next[i] = r >= 0 && r <= classes ? e + ctable[(size_t)r * dim + i % dim] : e;
	}
}

// eps~ = eps_u + s (eps_c - eps_u) in one explicit fmaf: at s = 0 it is eps_u bit for bit, and so is every guided step its unguided one
__device__ __forceinline__ float guided_mix(float s, float c, float u) { return fmaf(s, c - u, u); }

template <bool GUIDED>
__device__ __forceinline__ float eps_at(const float* __restrict__ eps_c, const float* __restrict__ eps_u, float s, size_t i) {
	return GUIDED ? guided_mix(s, eps_c[i], eps_u[i]) : eps_u[i];
}
template <bool GUIDED>
__device__ __forceinline__ float4 eps4_at(const float* __restrict__ eps_c, const float* __restrict__ eps_u, float s, size_t q) {
	float4 e = reinterpret_cast<const float4*>(eps_u)[q];
	if constexpr (GUIDED) {
		const float4 c = reinterpret_cast<const float4*>(eps_c)[q];
		e = make_float4(guided_mix(s, c.x, e.x), guided_mix(s, c.y, e.y), guided_mix(s, c.z, e.z), guided_mix(s, c.w, e.w));
	}
	return e;
}

// One ancestral step at t in place: x <- (x - k eps) inv + sig z with z from the stream (seed, (t + 1) << 32), 0 at t = 0.  temb_next (may be NULL) receives the
// embedding of t - 1, nothing at t = 0.
template <bool GUIDED>
__global__ void __launch_bounds__(kThreads) step_kernel(float* __restrict__ x, float* __restrict__ x_copy, const float* __restrict__ eps_c,
                                                        const float* __restrict__ eps_u, float s, size_t n, int t, int steps, unsigned long long seed,
                                                        const float* __restrict__ table, int batch, int dim, float* __restrict__ temb_next,
                                                        const float* __restrict__ ctable, int classes, const int* __restrict__ rows, int vec) {
	const float k = table[TAB_EPS_COEF * steps + t], inv = table[TAB_INV_SQRT_A * steps + t], sig = table[TAB_SIGMA * steps + t];
	const unsigned long long offset = (unsigned long long)(t + 1) << 32;
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	if (temb_next && t > 0) next_embedding<GUIDED>(temb_next, t - 1, batch, dim, ctable, classes, rows, tid, stride);
	const size_t n4 = vec ? n / 4 : 0;
	for (size_t q = tid; q < n4; q += stride) {
		const float4 z = t > 0 ? philox_normal4(philox_block(seed, offset + q, PHILOX_TAG_NORMAL)) : make_float4(0.f, 0.f, 0.f, 0.f);
		const float4 e = eps4_at<GUIDED>(eps_c, eps_u, s, q);
		float4 v = reinterpret_cast<float4*>(x)[q];
		v.x = (v.x - k * e.x) * inv + sig * z.x; v.y = (v.y - k * e.y) * inv + sig * z.y;
		v.z = (v.z - k * e.z) * inv + sig * z.z; v.w = (v.w - k * e.w) * inv + sig * z.w;
		reinterpret_cast<float4*>(x)[q] = v;
		if (GUIDED && x_copy) reinterpret_cast<float4*>(x_copy)[q] = v;
	}
	for (size_t i = 4 * n4 + tid; i < n; i += stride) {
		const float z = t > 0 ? normal_at(seed, offset, i) : 0.f;
		const float e = eps_at<GUIDED>(eps_c, eps_u, s, i);
		x[i] = (x[i] - k * e) * inv + sig * z;
		if (GUIDED && x_copy) x_copy[i] = x[i];
	}
}

// the guided sampler's start: rows[b] = labels[b] (b < n; -1 outside [0, classes]) / classes (b >= n) unless labels is NULL (rows already hold them), and
// temb [2n][dim] = the embedding of t plus table[rows[b]]
__global__ void __launch_bounds__(kThreads) guided_start_kernel(const int* __restrict__ labels, int n, int classes, int* __restrict__ rows, const float* __restrict__ ctable,
                                                                int t, int dim, float* __restrict__ temb) {
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	const size_t ne = (size_t)2 * n * dim;
	for (size_t i = tid; i < ne; i += stride) {
		const int b = (int)(i / dim);
		int r;
		if (labels) {
			r = b >= n ? classes : (labels[b] >= 0 && labels[b] <= classes ? labels[b] : -1);
			if (i % dim == 0) rows[b] = r;
		} else {
			r = rows[b];
		}
		const float e = temb_value(t, (int)(i % dim), dim);
		temb[i] = r >= 0 && r <= classes ? e + ctable[(size_t)r * dim + i % dim] : e;
	}
}

// acc[0] += sum_i (a_i - b_i)^2 in double, one workgroup in a fixed order (deterministic)
__global__ void __launch_bounds__(1024) sq_diff_sum_kernel(const float* __restrict__ a, const float* __restrict__ b, size_t n, double* __restrict__ acc) {
	__shared__ double part[16];
	double s = 0;
	for (size_t i = threadIdx.x; i < n; i += blockDim.x) { const double d = (double)a[i] - (double)b[i]; s += d * d; }
	for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
	if (threadIdx.x % 64 == 0) part[threadIdx.x / 64] = s;
	__syncthreads();
	if (threadIdx.x == 0) {
		double t = 0;
		for (int w = 0; w < (int)(blockDim.x / 64); w++) t += part[w];
		acc[0] += t;
	}
}

// ---- held-out evaluation: the variational bound of Ho et al. 2020, eq. 5 (include/bla.h) -------------------------------------------------------
// noise_kernel's job at timesteps that are given, not drawn: d_t [batch] (NULL: every image at t_const), eps = normal(seed, offset), x_t by noise1_vec /
// noise1_scalar (noise_kernel's bits on either path).  An image whose t lies outside [0, steps) gets zero rows of x_t and of the embedding.
__global__ void __launch_bounds__(kThreads) noise_at_kernel(const float* __restrict__ x0, int batch, size_t F, int dim, const int* __restrict__ d_t, int t_const,
                                                            unsigned long long seed, unsigned long long offset, int steps, const float* __restrict__ table,
                                                            float* __restrict__ eps, float* __restrict__ xt, float* __restrict__ temb, int vec) {
	__shared__ int ts[kMaxNoiseBatch];
	for (int b = threadIdx.x; b < batch; b += blockDim.x) {
		const int t = d_t ? d_t[b] : t_const;
		ts[b] = t >= 0 && t < steps ? t : -1;
	}
	__syncthreads();
	const float* sab = table + TAB_SQRT_AB * steps;
	const float* s1m = table + TAB_SQRT_1MAB * steps;
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	const size_t ne = (size_t)batch * dim;
	for (size_t i = tid; i < ne; i += stride) {
		const int t = ts[i / dim];
		temb[i] = t >= 0 ? temb_value(t, (int)(i % dim), dim) : 0.f;
	}
	const size_t n = (size_t)batch * F;
	if (vec) {   // F % 4 == 0, every pointer 16-byte aligned: Philox block q <-> float4 q, one image per float4
		for (size_t q = tid; q < n / 4; q += stride) {
			const int t = ts[(4 * q) / F];
			const float4 z = philox_normal4(philox_block(seed, offset + q, PHILOX_TAG_NORMAL));
			reinterpret_cast<float4*>(eps)[q] = z;
			float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
			if (t >= 0) {
				const float4 x = reinterpret_cast<const float4*>(x0)[q];
				const float a = sab[t], c = s1m[t];
				r = make_float4(noise1_vec(a, x.x, c, z.x), noise1_vec(a, x.y, c, z.y), noise1_vec(a, x.z, c, z.z), noise1_vec(a, x.w, c, z.w));
			}
			reinterpret_cast<float4*>(xt)[q] = r;
		}
	} else {
		for (size_t e = tid; e < n; e += stride) {
			const int t = ts[e / F];
			const float z = normal_at(seed, offset, e);
			eps[e] = z;
			xt[e] = t >= 0 ? noise1_scalar(sab[t], x0[e], s1m[t], z) : 0.f;
		}
	}
}

// The 256 per-lane partials of a workgroup summed through LDS in a fixed tree (no atomics: bit-reproducible); the total is returned to thread 0
__device__ __forceinline__ double block_sum(double v, double* part) {
	part[threadIdx.x] = v;
	__syncthreads();
	for (int s = kThreads / 2; s > 0; s >>= 1) {
		if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
		__syncthreads();
	}
	const double total = part[0];
	__syncthreads();   // part is free for the next sum
	return total;
}

// the decoder's constants at t = 0, formed in double on the host: mu = (x_t - k eps_hat) / sqrt_a, z = (x0 +- 1/255 - mu) / sigma
struct DecoderArgs { double k, sqrt_a, sigma; };

// -ln p of one element under the discretised Gaussian decoder of 8-bit data on [-1, 1] (Ho et al. 2020, section 3.3).  Phi through erfc on the side where it
// is small: Phi(z) = erfc(-z / sqrt 2) / 2, 1 - Phi(z) = erfc(z / sqrt 2) / 2; the interior difference between two tails of the same side
__device__ __forceinline__ double decoder_nll(double x0, double xt, double eh, const DecoderArgs& a) {
	const double rs2 = 0.70710678118654752440;
	const double mu = (xt - a.k * eh) / a.sqrt_a;
	const double zp = (x0 + 1.0 / 255.0 - mu) / a.sigma, zm = (x0 - 1.0 / 255.0 - mu) / a.sigma;
	double p;
	if (x0 < -0.999) p = 0.5 * erfc(-zp * rs2);
	else if (x0 > 0.999) p = 0.5 * erfc(zm * rs2);
	else if (zm > 0) p = 0.5 * (erfc(zm * rs2) - erfc(zp * rs2));
	else p = 0.5 * (erfc(-zp * rs2) - erfc(-zm * rs2));
	return -log(p > 1e-12 ? p : 1e-12);
}

// One workgroup per image: sqerr_b = sum (eps - eps_hat)^2, and the image's term of the bound -- F c_t + w_t sqerr_b at t >= 1 (vlb: c_t, w_t), the decoder's
// -sum ln p at t = 0.  The branch on t is uniform over the workgroup, so erfc and log run only in the workgroups at t = 0.  Every lane accumulates in
// double over its elements in index order.  A t outside [0, steps): term NaN, sqerr 0, nothing read.
__global__ void __launch_bounds__(kThreads) vlb_terms_kernel(const float* __restrict__ x0, const float* __restrict__ xt, const float* __restrict__ eps,
                                                             const float* __restrict__ eps_hat, const int* __restrict__ d_t, int t_const, size_t F, int steps,
                                                             const double* __restrict__ vlb, DecoderArgs dec, double* __restrict__ terms,
                                                             double* __restrict__ sqerr, int vec) {
	__shared__ double part[kThreads];
	const int b = blockIdx.x, t = d_t ? d_t[b] : t_const;
	if (t < 0 || t >= steps) {
		if (threadIdx.x == 0) { terms[b] = __longlong_as_double(0x7ff8000000000000ll); if (sqerr) sqerr[b] = 0.0; }
		return;
	}
	const size_t base = (size_t)b * F;
	double sq = 0.0, nll = 0.0;
	if (vec) {
		const float4* e4 = reinterpret_cast<const float4*>(eps + base);
		const float4* h4 = reinterpret_cast<const float4*>(eps_hat + base);
		const float4* x4 = reinterpret_cast<const float4*>(x0 + base);
		const float4* n4 = reinterpret_cast<const float4*>(xt + base);
		for (size_t q = threadIdx.x; q < F / 4; q += kThreads) {
			const float4 e = e4[q], h = h4[q];
			const double dx = (double)e.x - (double)h.x, dy = (double)e.y - (double)h.y, dz = (double)e.z - (double)h.z, dw = (double)e.w - (double)h.w;
			sq += dx * dx; sq += dy * dy; sq += dz * dz; sq += dw * dw;
			if (t == 0) {
				const float4 x = x4[q], n = n4[q];
				nll += decoder_nll(x.x, n.x, h.x, dec); nll += decoder_nll(x.y, n.y, h.y, dec);
				nll += decoder_nll(x.z, n.z, h.z, dec); nll += decoder_nll(x.w, n.w, h.w, dec);
			}
		}
	} else {
		for (size_t i = threadIdx.x; i < F; i += kThreads) {
			const double d = (double)eps[base + i] - (double)eps_hat[base + i];
			sq += d * d;
			if (t == 0) nll += decoder_nll(x0[base + i], xt[base + i], eps_hat[base + i], dec);
		}
	}
	sq = block_sum(sq, part);
	if (t == 0) nll = block_sum(nll, part);
	if (threadIdx.x == 0) {
		terms[b] = t == 0 ? nll : (double)F * vlb[t] + vlb[steps + t] * sq;
		if (sqerr) sqerr[b] = sq;
	}
}

// kl_b = (abar sum x0^2 - F abar - F ln(1 - abar)) / 2 with abar = alpha_bar of the last step: vlb_terms_kernel's reduction on one input
__global__ void __launch_bounds__(kThreads) prior_kl_kernel(const float* __restrict__ x0, size_t F, double abar, double log_1m_abar, double* __restrict__ kl, int vec) {
	__shared__ double part[kThreads];
	const size_t base = (size_t)blockIdx.x * F;
	double s = 0.0;
	if (vec) {
		const float4* x4 = reinterpret_cast<const float4*>(x0 + base);
		for (size_t q = threadIdx.x; q < F / 4; q += kThreads) {
			const float4 x = x4[q];
			s += (double)x.x * x.x; s += (double)x.y * x.y; s += (double)x.z * x.z; s += (double)x.w * x.w;
		}
	} else {
		for (size_t i = threadIdx.x; i < F; i += kThreads) { const double x = x0[base + i]; s += x * x; }
	}
	s = block_sum(s, part);
	if (threadIdx.x == 0) kl[blockIdx.x] = 0.5 * (abar * s - (double)F * abar - (double)F * log_1m_abar);
}

// c_t = (ln(beta_t / beta~_t) + beta~_t / beta_t - 1) / 2 and w_t = beta_t / (2 alpha_t (1 - abar_t)), t >= 1, in this order of operations (the tests
// restate it operation for operation)
void vlb_weights(const std::vector<double>& beta, const std::vector<double>& alpha_bar, int t, double* c, double* w) {
#pragma clang fp contract(off)
	const double b = beta[t], ab = alpha_bar[t], abp = alpha_bar[t - 1];
	const double bt = b * (1.0 - abp) / (1.0 - ab);
	*c = 0.5 * (std::log(b / bt) + bt / b - 1.0);
	*w = b / (2.0 * (1.0 - b) * (1.0 - ab));
}

// K midpoints of equal strata of 1 .. T-1 behind t = 0
std::vector<int> eval_timesteps(int T, int K) {
	std::vector<int> ts(K + 1);
	ts[0] = 0;
	for (int i = 0; i < K; i++) ts[1 + i] = 1 + (int)((long long)(T - 1) * (2 * i + 1) / (2 * K));
	return ts;
}

bla_status check_images(const bla_diffusion* d, int batch, size_t image_floats, int time_dim) {
	BLA_REQUIRE(d, BLA_ERR_INVALID, "null diffusion object");
	BLA_REQUIRE(batch >= 1 && image_floats >= 1 && time_dim >= 1, BLA_ERR_INVALID, "batch %d, image_floats %zu, time_dim %d", batch, image_floats, time_dim);
	return BLA_OK;
}

// ---- DDIM (Song, Meng, Ermon 2021) -------------------------------------------------------------------------------------------------------------
// The step's five coefficients, formed in double on the host from the schedule and passed by value (nothing is uploaded per step, so a captured
// sampler replays correctly):  x0^ = (x - s1m eps) inv_sab, clamped to [-1, 1] when clip;  x <- sab_prev x0^ + dir eps + sigma z
struct DdimArgs { float inv_sab, s1m, sab_prev, dir, sigma; int clip; };

DdimArgs ddim_args(const bla_diffusion* d, int t, int t_prev, float eta, int clip) {
	const double ab = d->alpha_bar[t], abp = t_prev >= 0 ? d->alpha_bar[t_prev] : 1.0;
	const double sigma = (double)eta * std::sqrt((1.0 - abp) / (1.0 - ab)) * std::sqrt(1.0 - ab / abp);
	const double dir2 = 1.0 - abp - sigma * sigma;
	return {(float)(1.0 / std::sqrt(ab)), (float)std::sqrt(1.0 - ab), (float)std::sqrt(abp), (float)std::sqrt(dir2 > 0 ? dir2 : 0.0), (float)sigma, clip ? 1 : 0};
}

__device__ __forceinline__ float ddim1(float x, float e, float z, const DdimArgs& a) {
#pragma clang fp contract(off)   // the fused operations spelled out: left to the contraction heuristics, the guided and the unguided instance of the
                                 // kernel below fused different products and missed bit-equality at guidance 0 (measured)
	float x0 = fmaf(-a.s1m, e, x) * a.inv_sab;
	if (a.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
	return fmaf(a.sab_prev, x0, fmaf(a.dir, e, a.sigma * z));
}

// One DDIM step from t to t_prev in place; step_kernel's structure.  z is step_kernel's stream (seed, (t + 1) << 32), drawn only when sigma > 0; temb_next (may be
// NULL) receives the embedding of t_prev, nothing at t_prev = -1.
template <bool GUIDED>
__global__ void __launch_bounds__(kThreads) ddim_step_kernel(float* __restrict__ x, float* __restrict__ x_copy, const float* __restrict__ eps_c,
                                                             const float* __restrict__ eps_u, float s, size_t n, DdimArgs a, int t, int t_prev,
                                                             unsigned long long seed, int batch, int dim, float* __restrict__ temb_next,
                                                             const float* __restrict__ ctable, int classes, const int* __restrict__ rows, int vec) {
	const unsigned long long offset = (unsigned long long)(t + 1) << 32;
	const bool noise = a.sigma > 0.f;
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	if (temb_next && t_prev >= 0) next_embedding<GUIDED>(temb_next, t_prev, batch, dim, ctable, classes, rows, tid, stride);
	const size_t n4 = vec ? n / 4 : 0;
	for (size_t q = tid; q < n4; q += stride) {
		const float4 z = noise ? philox_normal4(philox_block(seed, offset + q, PHILOX_TAG_NORMAL)) : make_float4(0.f, 0.f, 0.f, 0.f);
		const float4 e = eps4_at<GUIDED>(eps_c, eps_u, s, q);
		float4 v = reinterpret_cast<float4*>(x)[q];
		v = make_float4(ddim1(v.x, e.x, z.x, a), ddim1(v.y, e.y, z.y, a), ddim1(v.z, e.z, z.z, a), ddim1(v.w, e.w, z.w, a));
		reinterpret_cast<float4*>(x)[q] = v;
		if (GUIDED && x_copy) reinterpret_cast<float4*>(x_copy)[q] = v;
	}
	for (size_t i = 4 * n4 + tid; i < n; i += stride) {
		const float z = noise ? normal_at(seed, offset, i) : 0.f;
		const float e = eps_at<GUIDED>(eps_c, eps_u, s, i);
		const float v = ddim1(x[i], e, z, a);
		x[i] = v;
		if (GUIDED && x_copy) x_copy[i] = v;
	}
}

bla_status check_ddim(const bla_diffusion* d, int t, int t_prev, float eta) {
	BLA_REQUIRE(t >= 0 && t < d->steps, BLA_ERR_INVALID, "timestep %d outside [0, %d)", t, d->steps);
	BLA_REQUIRE(t_prev >= -1 && t_prev < t, BLA_ERR_INVALID, "t_prev %d outside [-1, %d)", t_prev, t);
	BLA_REQUIRE(eta >= 0.f && eta <= 1.f, BLA_ERR_INVALID, "eta %g outside [0, 1]", eta);
	return BLA_OK;
}

// "trailing" spacing: out[i] = floor(T (i + 1) / S) - 1, the last always T - 1
std::vector<int> ddim_timesteps(int T, int S) {
	std::vector<int> ts(S);
	for (int i = 0; i < S; i++) ts[i] = (int)((long long)T * (i + 1) / S) - 1;
	return ts;
}

// One scratch buffer of the diffusion object grown to at least `count` elements (what it held is lost).  It waits for the stream only when it has to grow, so a
// first call is not capturable and a second with the same shapes neither waits nor allocates.
template <typename T>
bla_status grow(hipStream_t s, T** buf, size_t* have, size_t count) {
	if (*have >= count) return BLA_OK;
	BLA_HIP(hipStreamSynchronize(s));
	(void)hipFree(*buf); *buf = nullptr; *have = 0;
	BLA_HIP(hipMalloc((void**)buf, count * sizeof(T)));
	*have = count;
	return BLA_OK;
}

// ---- DPM-Solver++(2M) (Lu, Zhou, Bao, Chen, Li, Zhu 2022) --------------------------------------------------------------------------------------
// The multistep second-order solver of the probability-flow ODE in the data-prediction form.  alpha = sqrt(abar), sigma = sqrt(1 - abar),
// lambda = ln(alpha / sigma) (strictly decreasing in t), alpha = 1 and sigma = 0 past the last step.

double log_snr(const bla_diffusion* d, int t) { return 0.5 * std::log(d->alpha_bar[t] / (1.0 - d->alpha_bar[t])); }

// lambda_a - lambda_b from one logarithm of one ratio: the difference of two log_snr values loses ulp(lambda) / |difference| to cancellation
// (1e-14 at neighbouring steps near t = T), the ratio does not
double log_snr_diff(const bla_diffusion* d, int a, int b) {
	const double xa = d->alpha_bar[a], xb = d->alpha_bar[b];
	return 0.5 * std::log((xa * (1.0 - xb)) / (xb * (1.0 - xa)));
}

// uniform in lambda between lambda_0 and lambda_{T-1}, each grid point taken to the nearest timestep, then made strictly increasing inside [0, T-1]
std::vector<int> logsnr_timesteps(const bla_diffusion* d, int S) {
	const int T = d->steps;
	std::vector<int> ts(S);
	if (S == 1) { ts[0] = T - 1; return ts; }
	std::vector<double> lam(T);
	for (int t = 0; t < T; t++) lam[t] = log_snr(d, t);
	int j = 0;   // the first t with lam[t] <= g; the grid falls, so j only moves up
	for (int i = 0; i < S; i++) {
		const double g = lam[0] + (lam[T - 1] - lam[0]) * i / (S - 1);
		while (j < T && lam[j] > g) j++;
		if (j == 0) ts[i] = 0;
		else if (j == T) ts[i] = T - 1;
		else ts[i] = (lam[j - 1] - g) <= (g - lam[j]) ? j - 1 : j;   // a tie takes the lower t
	}
	for (int i = 1; i < S; i++) ts[i] = std::max(ts[i], ts[i - 1] + 1);
	for (int i = S - 1; i >= 0; i--) ts[i] = std::min(ts[i], T - 1 - (S - 1 - i));
	return ts;
}

bla_status sample_timesteps(const bla_diffusion* d, int S, int spacing, std::vector<int>* out) {
	BLA_REQUIRE(S >= 1 && S <= d->steps, BLA_ERR_INVALID, "sample_steps %d outside [1, %d]", S, d->steps);
	BLA_REQUIRE(spacing == BLA_SPACING_TRAILING || spacing == BLA_SPACING_LOGSNR, BLA_ERR_INVALID, "spacing %d is neither BLA_SPACING_TRAILING nor BLA_SPACING_LOGSNR", spacing);
	*out = spacing == BLA_SPACING_LOGSNR ? logsnr_timesteps(d, S) : ddim_timesteps(d->steps, S);
	return BLA_OK;
}

bla_status check_dpmpp(const bla_diffusion* d, int t_last, int t, int t_prev) {
	BLA_REQUIRE(t >= 0 && t < d->steps, BLA_ERR_INVALID, "timestep %d outside [0, %d)", t, d->steps);
	BLA_REQUIRE(t_prev >= -1 && t_prev < t, BLA_ERR_INVALID, "t_prev %d outside [-1, %d)", t_prev, t);
	BLA_REQUIRE(t_last == -1 || (t_last > t && t_last < d->steps), BLA_ERR_INVALID, "t_last %d is neither -1 nor inside (%d, %d)", t_last, t, d->steps);
	return BLA_OK;
}

// {inv_sab, s1m, c_x, c_d, w1, w0} of bla_diffusion_dpmpp_coefficients (include/bla.h), in double; the arguments are check_dpmpp's
void dpmpp_coefficients(const bla_diffusion* d, int t_last, int t, int t_prev, double out[6]) {
	const double ab = d->alpha_bar[t];
	out[0] = 1.0 / std::sqrt(ab); out[1] = std::sqrt(1.0 - ab);
	out[2] = 0.0; out[3] = 1.0; out[4] = 1.0; out[5] = 0.0;
	if (t_prev < 0) return;   // to the data: the step returns the x0 prediction
	const double abp = d->alpha_bar[t_prev], h = log_snr_diff(d, t_prev, t);
	out[2] = std::sqrt(1.0 - abp) / std::sqrt(1.0 - ab);
	out[3] = -std::sqrt(abp) * std::expm1(-h);
	if (t_last >= 0) {
		const double r = log_snr_diff(d, t, t_last) / h;
		out[4] = 1.0 + 1.0 / (2.0 * r); out[5] = -1.0 / (2.0 * r);
	}
}

// the six coefficients rounded to fp32 once on the host and passed by value (nothing is uploaded per step, so a captured sampler replays correctly)
struct DpmppArgs { float inv_sab, s1m, c_x, c_d, w1, w0; int clip, second; };

DpmppArgs dpmpp_args(const bla_diffusion* d, int t_last, int t, int t_prev, int clip) {
	double c[6];
	dpmpp_coefficients(d, t_last, t, t_prev, c);
	return {(float)c[0], (float)c[1], (float)c[2], (float)c[3], (float)c[4], (float)c[5], clip ? 1 : 0, t_last >= 0 && t_prev >= 0 ? 1 : 0};
}

// the new x; *x0_out is the (clamped) x0 prediction, the next step's history
__device__ __forceinline__ float dpmpp1(float x, float e, float hist, const DpmppArgs& a, float* x0_out) {
#pragma clang fp contract(off)   // as in ddim1: the guided and the unguided instance must fuse the same products
	float x0 = fmaf(-a.s1m, e, x) * a.inv_sab;
	if (a.clip) x0 = fminf(fmaxf(x0, -1.f), 1.f);
	const float D = a.second ? fmaf(a.w0, hist, a.w1 * x0) : x0;
	*x0_out = x0;
	return fmaf(a.c_x, x, a.c_d * D);
}

// One DPM-Solver++(2M) step from t to t_prev in place; step_kernel's structure.
// hist [n] holds the previous step's x0 prediction: read only when a.second, always written with this step's.  No noise.
template <bool GUIDED>
__global__ void __launch_bounds__(kThreads) dpmpp_step_kernel(float* __restrict__ x, float* __restrict__ x_copy, const float* __restrict__ eps_c,
                                                              const float* __restrict__ eps_u, float s, float* __restrict__ hist, size_t n, DpmppArgs a,
                                                              int t_prev, int batch, int dim, float* __restrict__ temb_next,
                                                              const float* __restrict__ ctable, int classes, const int* __restrict__ rows, int vec) {
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	if (temb_next && t_prev >= 0) next_embedding<GUIDED>(temb_next, t_prev, batch, dim, ctable, classes, rows, tid, stride);
	const size_t n4 = vec ? n / 4 : 0;
	for (size_t q = tid; q < n4; q += stride) {
		const float4 e = eps4_at<GUIDED>(eps_c, eps_u, s, q);
		const float4 h = a.second ? reinterpret_cast<const float4*>(hist)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
		float4 v = reinterpret_cast<float4*>(x)[q], p;
		v = make_float4(dpmpp1(v.x, e.x, h.x, a, &p.x), dpmpp1(v.y, e.y, h.y, a, &p.y), dpmpp1(v.z, e.z, h.z, a, &p.z), dpmpp1(v.w, e.w, h.w, a, &p.w));
		reinterpret_cast<float4*>(x)[q] = v;
		reinterpret_cast<float4*>(hist)[q] = p;
		if (GUIDED && x_copy) reinterpret_cast<float4*>(x_copy)[q] = v;
	}
	for (size_t i = 4 * n4 + tid; i < n; i += stride) {
		const float e = eps_at<GUIDED>(eps_c, eps_u, s, i);
		float p;
		const float v = dpmpp1(x[i], e, a.second ? hist[i] : 0.f, a, &p);
		x[i] = v;
		hist[i] = p;
		if (GUIDED && x_copy) x_copy[i] = v;
	}
}

// ---- training objectives: what the network predicts and how a timestep's loss is weighted (include/bla.h) ---------------------------------------
// a = sqrt(abar_t) and c = sqrt(1 - abar_t) are the fp32 table values.  v = a eps - c x0 (Salimans & Ho 2022); back to eps given the x_t the model saw:
// eps = a v + c x_t from v, eps = (x_t - a x0) / c from x0.  Every fused operation is spelled out.
__device__ __forceinline__ float v_target1(float a, float e, float c, float x0) {
#pragma clang fp contract(off)
	return fmaf(a, e, -(c * x0));
}
__device__ __forceinline__ float v_to_eps1(float a, float v, float c, float x) {
#pragma clang fp contract(off)
	return fmaf(a, v, c * x);
}
// a true division by the table's c (correctly rounded), not a product with a reciprocal; the numerator is one fused operation
__device__ __forceinline__ float x0_to_eps1(float a, float x0, float c, float x) {
#pragma clang fp contract(off)
	return fmaf(-a, x0, x) / c;
}

// element e of [batch][F] belongs to image e / F; its timestep, -1 when outside [0, steps)
__device__ __forceinline__ int step_of(const int* __restrict__ d_t, int t_const, size_t b, int steps) {
	const int t = d_t ? d_t[b] : t_const;
	return t >= 0 && t < steps ? t : -1;
}

// target [batch][F] of the prediction type `pred` and weight[b] = w[t_b] (1 where lw is NULL).  An image whose t lies outside [0, steps): zeros, weight 0.
// x0 is read only for X0 and V, eps only for EPS and V.  The 16-byte body runs over the flat array, so a float4 may hold the end of one image and the
// start of the next: each component looks up its own image.
__global__ void __launch_bounds__(kThreads) target_kernel(const float* __restrict__ x0, const float* __restrict__ eps, const int* __restrict__ d_t, int t_const,
                                                          int batch, size_t F, int steps, int pred, const float* __restrict__ table,
                                                          const float* __restrict__ lw, float* __restrict__ target, float* __restrict__ weight, int vec) {
	const float* sab = table + TAB_SQRT_AB * steps;
	const float* s1m = table + TAB_SQRT_1MAB * steps;
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	if (weight)
		for (size_t b = tid; b < (size_t)batch; b += stride) {
			const int t = step_of(d_t, t_const, b, steps);
			weight[b] = t < 0 ? 0.f : (lw ? lw[t] : 1.f);
		}
	const size_t n = (size_t)batch * F, n4 = vec ? n / 4 : 0;
	for (size_t q = tid; q < n4; q += stride) {
		const float4 e4 = pred != BLA_PREDICT_X0 ? reinterpret_cast<const float4*>(eps)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
		const float4 x4 = pred != BLA_PREDICT_EPS ? reinterpret_cast<const float4*>(x0)[q] : make_float4(0.f, 0.f, 0.f, 0.f);
		const float e[4] = {e4.x, e4.y, e4.z, e4.w}, x[4] = {x4.x, x4.y, x4.z, x4.w};
		float r[4];
		size_t b = (4 * q) / F, p = 4 * q - b * F;
		for (int k = 0; k < 4; k++, p++) {
			while (p >= F) { p -= F; b++; }
			const int t = step_of(d_t, t_const, b, steps);
			if (t < 0) r[k] = 0.f;
			else if (pred == BLA_PREDICT_EPS) r[k] = e[k];
			else if (pred == BLA_PREDICT_X0) r[k] = x[k];
			else r[k] = v_target1(sab[t], e[k], s1m[t], x[k]);
		}
		reinterpret_cast<float4*>(target)[q] = make_float4(r[0], r[1], r[2], r[3]);
	}
	for (size_t i = 4 * n4 + tid; i < n; i += stride) {
		const int t = step_of(d_t, t_const, i / F, steps);
		float r = 0.f;
		if (t >= 0) r = pred == BLA_PREDICT_EPS ? eps[i] : (pred == BLA_PREDICT_X0 ? x0[i] : v_target1(sab[t], eps[i], s1m[t], x0[i]));
		target[i] = r;
	}
}

// pred [batch][F] <- eps_hat in place, from v (pred_type V) or from x0 (X0), given the x_t the model saw.  An image whose t lies outside [0, steps) is
// left as it is.  target_kernel's structure.
__global__ void __launch_bounds__(kThreads) to_eps_kernel(float* __restrict__ pred, const float* __restrict__ x, const int* __restrict__ d_t, int t_const, int batch,
                                                          size_t F, int steps, int pred_type, const float* __restrict__ table, int vec) {
	const float* sab = table + TAB_SQRT_AB * steps;
	const float* s1m = table + TAB_SQRT_1MAB * steps;
	const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
	const size_t n = (size_t)batch * F, n4 = vec ? n / 4 : 0;
	for (size_t q = tid; q < n4; q += stride) {
		const float4 p4 = reinterpret_cast<const float4*>(pred)[q], x4 = reinterpret_cast<const float4*>(x)[q];
		float r[4] = {p4.x, p4.y, p4.z, p4.w};
		const float xs[4] = {x4.x, x4.y, x4.z, x4.w};
		size_t b = (4 * q) / F, p = 4 * q - b * F;
		for (int k = 0; k < 4; k++, p++) {
			while (p >= F) { p -= F; b++; }
			const int t = step_of(d_t, t_const, b, steps);
			if (t >= 0) r[k] = pred_type == BLA_PREDICT_V ? v_to_eps1(sab[t], r[k], s1m[t], xs[k]) : x0_to_eps1(sab[t], r[k], s1m[t], xs[k]);
		}
		reinterpret_cast<float4*>(pred)[q] = make_float4(r[0], r[1], r[2], r[3]);
	}
	for (size_t i = 4 * n4 + tid; i < n; i += stride) {
		const int t = step_of(d_t, t_const, i / F, steps);
		if (t >= 0) pred[i] = pred_type == BLA_PREDICT_V ? v_to_eps1(sab[t], pred[i], s1m[t], x[i]) : x0_to_eps1(sab[t], pred[i], s1m[t], x[i]);
	}
}

// g = (2 w) (out - target): 2 w is exact, the difference is one rounding and the product one.  w = 1: 2 (out - target), the U-Net's own seed bit for bit.
__device__ __forceinline__ float loss_grad1(float w2, float o, float t) {
#pragma clang fp contract(off)
	return w2 * (o - t);
}

// One workgroup per image (vlb_terms_kernel's reduction): g [F] of the image (g may be NULL) and loss[b] = w_b sum_i (out_i - target_i)^2 in double (loss
// may be NULL).  Every lane sums its elements in index order, the 256 partials go through block_sum: no atomics, bit-reproducible.
__global__ void __launch_bounds__(kThreads) weighted_loss_kernel(const float* __restrict__ out, const float* __restrict__ target, const float* __restrict__ weight,
                                                                 size_t F, float* __restrict__ g, double* __restrict__ loss, int vec) {
#pragma clang fp contract(off)
	__shared__ double part[kThreads];
	const size_t b = blockIdx.x, base = b * F;
	const float w = weight ? weight[b] : 1.f, w2 = 2.f * w;
	double sq = 0.0;
	if (vec) {
		const float4* o4 = reinterpret_cast<const float4*>(out + base);
		const float4* t4 = reinterpret_cast<const float4*>(target + base);
		for (size_t q = threadIdx.x; q < F / 4; q += kThreads) {
			const float4 o = o4[q], t = t4[q];
			if (loss) {
				const double dx = (double)o.x - (double)t.x, dy = (double)o.y - (double)t.y, dz = (double)o.z - (double)t.z, dw = (double)o.w - (double)t.w;
				sq += dx * dx; sq += dy * dy; sq += dz * dz; sq += dw * dw;
			}
			if (g) reinterpret_cast<float4*>(g + base)[q] = make_float4(loss_grad1(w2, o.x, t.x), loss_grad1(w2, o.y, t.y), loss_grad1(w2, o.z, t.z), loss_grad1(w2, o.w, t.w));
		}
	} else {
		for (size_t i = threadIdx.x; i < F; i += kThreads) {
			const float o = out[base + i], t = target[base + i];
			if (loss) { const double d = (double)o - (double)t; sq += d * d; }
			if (g) g[base + i] = loss_grad1(w2, o, t);
		}
	}
	if (!loss) return;   // uniform over the workgroup
	sq = block_sum(sq, part);
	if (threadIdx.x == 0) loss[b] = (double)w * sq;
}

// w_t of bla_diffusion_set_objective in this order of operations (the tests restate it operation for operation)
double loss_weight(double alpha_bar, int prediction, double gamma) {
#pragma clang fp contract(off)
	if (gamma == 0.0) return 1.0;
	const double snr = alpha_bar / (1.0 - alpha_bar), m = snr < gamma ? snr : gamma;
	if (prediction == BLA_PREDICT_EPS) return snr > 0.0 ? m / snr : 1.0;   // alpha_bar underflown to 0 (a very long schedule): the limit of min(SNR, gamma) / SNR, not 0 / 0
	return prediction == BLA_PREDICT_X0 ? m : m / (snr + 1.0);
}

// the tail of both constructors: alpha_bar, the five fp32 tables and the VLB weights from d->beta (steps values inside (0, 1))
bla_status finish_create(bla_diffusion* d, bla_diffusion** out, const char* who) {
	const int steps = d->steps;
	d->alpha_bar.resize(steps);
	std::vector<float> tab((size_t)5 * steps);
	double ab = 1.0;
	for (int t = 0; t < steps; t++) {
		const double b = d->beta[t];
		ab *= 1.0 - b;
		d->alpha_bar[t] = ab;
		tab[TAB_SQRT_AB * steps + t] = (float)std::sqrt(ab);
		tab[TAB_SQRT_1MAB * steps + t] = (float)std::sqrt(1.0 - ab);
		tab[TAB_EPS_COEF * steps + t] = (float)(b / std::sqrt(1.0 - ab));
		tab[TAB_INV_SQRT_A * steps + t] = (float)(1.0 / std::sqrt(1.0 - b));
		tab[TAB_SIGMA * steps + t] = (float)std::sqrt(b);
	}
	hipError_t e = hipMalloc((void**)&d->table, tab.size() * sizeof(float));
	if (e == hipSuccess) e = hipMemcpy(d->table, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
	std::vector<double> vlb((size_t)2 * steps, 0.0);
	for (int t = 1; t < steps; t++) vlb_weights(d->beta, d->alpha_bar, t, &vlb[t], &vlb[steps + t]);
	if (e == hipSuccess) e = hipMalloc((void**)&d->vlb, vlb.size() * sizeof(double));
	if (e == hipSuccess) e = hipMemcpy(d->vlb, vlb.data(), vlb.size() * sizeof(double), hipMemcpyHostToDevice);
	if (e != hipSuccess) { (void)hipFree(d->table); (void)hipFree(d->vlb); delete d; return hip_fail(e, who); }
	*out = d;
	return BLA_OK;
}

// what every sampling and evaluation loop calls right behind bla_unet_forward_f32: the model's output read as d's prediction type becomes eps_hat in
// place, given the buffer the model was given (all `batch` images at timestep t).  EPS: nothing is launched, so those loops keep their bits.
bla_status output_to_eps(bla_unet* m, const bla_diffusion* d, void* stream, const float* d_x, int batch, size_t image_floats, int t) {
	if (d->prediction == BLA_PREDICT_EPS) return BLA_OK;
	return bla_diffusion_to_eps_f32(d, stream, bla_unet_output(m), d_x, nullptr, t, batch, image_floats);
}

// ---- the samplers: one walk, one guided set-up.  A sampler is a step function (one of the six bla_diffusion_*_step_f32) and a choice of timesteps -----------------

// what a sampler needs to know of its model: the batch, the embedding's width, one image's floats
struct ModelShape { int B, dim; size_t F; };

ModelShape shape_of(bla_unet* m) {
	const bla_unet_config& c = *unet_config(m);
	return {bla_unet_batch(m), c.time_dim, (size_t)c.in_channels * c.image_h * c.image_w};
}

// The walk down the timesteps ts[S-1] > ... > ts[0] (ts NULL: ts[i] = i, every timestep without a list of them): the model on x with the embedding workspace, its
// output read as eps_hat, then step(t_last, t, t_prev), which moves x to t_prev and writes the next embedding.  t_last is the timestep before t (-1 at the first),
// t_prev the one behind it (-1 at the last).
template <typename Step>
bla_status sample_loop(bla_unet* m, const bla_diffusion* d, void* stream, const float* x, const ModelShape& g, const int* ts, int S, Step step) {
	const auto at = [ts](int i) { return ts ? ts[i] : i; };
	bla_status st;
	for (int i = S - 1, t_last = -1; i >= 0; t_last = at(i), i--) {
		if ((st = bla_unet_forward_f32(m, stream, x, d->temb, nullptr))) return st;
		if ((st = output_to_eps(m, d, stream, x, g.B, g.F, at(i)))) return st;
		if ((st = step(t_last, at(i), i > 0 ? at(i - 1) : -1))) return st;
	}
	return BLA_OK;
}

// an unguided sampler's set-up: the embedding workspace and hist_floats of history grown, the embedding of the first timestep written
bla_status sample_start(const bla_diffusion* d, hipStream_t s, const ModelShape& g, int t_first, size_t hist_floats) {
	bla_diffusion* dm = const_cast<bla_diffusion*>(d);   // the workspaces are scratch, not part of the schedule
	const size_t ne = (size_t)g.B * g.dim;
	bla_status st;
	if ((st = grow(s, &dm->temb, &dm->temb_floats, ne))) return st;
	if ((st = grow(s, &dm->hist, &dm->hist_floats, hist_floats))) return st;
	hipLaunchKernelGGL(time_embedding_kernel, dim3(grid_for(ne)), dim3(kThreads), 0, s, (const int*)nullptr, t_first, g.B, g.dim, dm->temb);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

// what the three guided samplers check before their own arguments
bla_status check_guided_sampler(bla_unet* m, const bla_diffusion* d, const float* d_x, const float* d_table, int classes, const int* labels, float guidance) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(m && d && d_x && d_table && labels, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(classes >= 1, BLA_ERR_INVALID, "classes %d", classes);
	BLA_REQUIRE(std::isfinite(guidance), BLA_ERR_INVALID, "guidance %g", guidance);
	return BLA_OK;
}

// A guided sampler's set-up, n = B / 2 images: the workspaces grown, the model's input xg = [x; x], the rows [labels; classes ...] and the embedding of the first
// timestep plus the class rows.  Device labels go to guided_start_kernel with no host round trip (one outside [0, classes] gets no class row).  Host labels are
// checked here and the rows uploaded: the one wait for the stream that makes such a call not capturable.
bla_status guided_start(const bla_diffusion* d, hipStream_t s, const ModelShape& g, const float* d_x, const float* d_table, int classes, const int* labels, int t_first,
                        size_t hist_floats) {
	const int B = g.B, n = B / 2;
	BLA_REQUIRE(B % 2 == 0, BLA_ERR_INVALID, "the guided sampler needs an even model batch (n conditioned images + their n null-class copies), not %d", B);
	bla_diffusion* dm = const_cast<bla_diffusion*>(d);   // the workspaces are scratch, not part of the schedule
	const size_t ne = (size_t)B * g.dim, half = (size_t)n * g.F;
	bla_status st;
	if ((st = grow(s, &dm->temb, &dm->temb_floats, ne))) return st;
	if ((st = grow(s, &dm->xg, &dm->xg_floats, 2 * half))) return st;
	if ((st = grow(s, &dm->rows, &dm->rows_count, (size_t)B))) return st;
	if ((st = grow(s, &dm->hist, &dm->hist_floats, hist_floats))) return st;
	const int* dev_labels = labels;
	if (host_pointer(labels)) {
		std::vector<int> rows(B);
		for (int b = 0; b < n; b++) {
			BLA_REQUIRE(labels[b] >= 0 && labels[b] <= classes, BLA_ERR_INVALID, "label %d of image %d outside [0, %d]", labels[b], b, classes);
			rows[b] = labels[b]; rows[n + b] = classes;
		}
		BLA_HIP(hipMemcpyAsync(dm->rows, rows.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
		BLA_HIP(hipStreamSynchronize(s));
		dev_labels = nullptr;
	}
	BLA_HIP(hipMemcpyAsync(dm->xg, d_x, half * sizeof(float), hipMemcpyDeviceToDevice, s));
	BLA_HIP(hipMemcpyAsync(dm->xg + half, d_x, half * sizeof(float), hipMemcpyDeviceToDevice, s));
	hipLaunchKernelGGL(guided_start_kernel, dim3(grid_for(ne)), dim3(kThreads), 0, s, dev_labels, n, classes, dm->rows, d_table, t_first, g.dim, dm->temb);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

// the tear-down: the first half of xg is the sample
bla_status guided_finish(const bla_diffusion* d, hipStream_t s, const ModelShape& g, float* d_x) {
	BLA_HIP(hipMemcpyAsync(d_x, d->xg, (size_t)(g.B / 2) * g.F * sizeof(float), hipMemcpyDeviceToDevice, s));
	return BLA_OK;
}

// what the six *_step_f32 check before their own timesteps (have: the pointers each of them needs), and what the three guided ones check behind them
bla_status check_step(const bla_diffusion* d, int batch, size_t image_floats, int time_dim, bool have) {
	bla_status st = require_ready();
	if (st) return st;
	if ((st = check_images(d, batch, image_floats, time_dim))) return st;
	BLA_REQUIRE(have, BLA_ERR_INVALID, "null argument");
	return BLA_OK;
}

bla_status check_guidance(float guidance, const float* d_table, int classes, const int* d_rows) {
	BLA_REQUIRE(std::isfinite(guidance), BLA_ERR_INVALID, "guidance %g", guidance);
	BLA_REQUIRE(!d_table || (d_rows && classes >= 1), BLA_ERR_INVALID, "a class table needs the rows [2 batch] and classes >= 1");
	return BLA_OK;
}

}  // namespace

extern "C" {

bla_status bla_diffusion_create(bla_diffusion** out, int steps, float beta_start, float beta_end) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(out, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(steps >= 1 && steps <= (1 << 24), BLA_ERR_INVALID, "steps %d", steps);
	BLA_REQUIRE(beta_start > 0.f && beta_end > 0.f && beta_start < 1.f && beta_end < 1.f, BLA_ERR_INVALID, "betas (%g, %g) outside (0, 1)", beta_start, beta_end);
	bla_diffusion* d = new bla_diffusion();
	d->steps = steps;
	d->beta.resize(steps);
	for (int t = 0; t < steps; t++)
		d->beta[t] = steps == 1 ? (double)beta_start : (double)beta_start + ((double)beta_end - beta_start) * t / (steps - 1);   // linspace
	return finish_create(d, out, "bla_diffusion_create");
}

bla_status bla_diffusion_cosine_betas(int steps, double s, double max_beta, double* out) {
	BLA_REQUIRE(out, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(steps >= 1, BLA_ERR_INVALID, "steps %d", steps);
	BLA_REQUIRE(s >= 0.0 && std::isfinite(s), BLA_ERR_INVALID, "offset s %g is negative or not finite", s);
	BLA_REQUIRE(max_beta > 0.0 && max_beta < 1.0, BLA_ERR_INVALID, "max_beta %g outside (0, 1)", max_beta);
	auto f = [&](int i) { const double c = std::cos(((double)i / steps + s) / (1.0 + s) * M_PI / 2); return c * c; };
	double fi = f(0);
	for (int i = 0; i < steps; i++) {
		const double fn = f(i + 1), b = 1.0 - fn / fi;
		out[i] = b < max_beta ? b : max_beta;
		fi = fn;
	}
	return BLA_OK;
}

bla_status bla_diffusion_create_from_betas(bla_diffusion** out, int steps, const double* betas) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(out && betas, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(steps >= 1 && steps <= (1 << 24), BLA_ERR_INVALID, "steps %d", steps);
	for (int t = 0; t < steps; t++) BLA_REQUIRE(betas[t] > 0.0 && betas[t] < 1.0, BLA_ERR_INVALID, "beta %g of step %d outside (0, 1)", betas[t], t);   // NaN fails both
	bla_diffusion* d = new bla_diffusion();
	d->steps = steps;
	d->beta.assign(betas, betas + steps);
	return finish_create(d, out, "bla_diffusion_create_from_betas");
}

bla_status bla_diffusion_set_objective(bla_diffusion* d, int prediction, double min_snr_gamma) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(d, BLA_ERR_INVALID, "null diffusion object");
	BLA_REQUIRE(prediction == BLA_PREDICT_EPS || prediction == BLA_PREDICT_X0 || prediction == BLA_PREDICT_V, BLA_ERR_INVALID,
	            "prediction %d is none of BLA_PREDICT_EPS, BLA_PREDICT_X0, BLA_PREDICT_V", prediction);
	BLA_REQUIRE(min_snr_gamma >= 0.0 && std::isfinite(min_snr_gamma), BLA_ERR_INVALID, "min_snr_gamma %g is negative or not finite", min_snr_gamma);
	std::vector<double> w(d->steps);
	std::vector<float> wf(d->steps);
	for (int t = 0; t < d->steps; t++) { w[t] = loss_weight(d->alpha_bar[t], prediction, min_snr_gamma); wf[t] = (float)w[t]; }
	BLA_HIP(hipDeviceSynchronize());   // a launch in flight may still read the old table
	if (!d->loss_w_dev) BLA_HIP(hipMalloc((void**)&d->loss_w_dev, (size_t)d->steps * sizeof(float)));
	BLA_HIP(hipMemcpy(d->loss_w_dev, wf.data(), (size_t)d->steps * sizeof(float), hipMemcpyHostToDevice));
	d->loss_w.swap(w);
	d->prediction = prediction; d->min_snr_gamma = min_snr_gamma;
	return BLA_OK;
}

bla_status bla_diffusion_objective(const bla_diffusion* d, int* prediction, double* min_snr_gamma) {
	BLA_REQUIRE(d, BLA_ERR_INVALID, "null diffusion object");
	if (prediction) *prediction = d->prediction;
	if (min_snr_gamma) *min_snr_gamma = d->min_snr_gamma;
	return BLA_OK;
}

bla_status bla_diffusion_loss_weight(const bla_diffusion* d, int t, double* w) {
	BLA_REQUIRE(d && w && t >= 0 && t < d->steps, BLA_ERR_INVALID, "timestep %d outside [0, %d)", t, d ? d->steps : 0);
	*w = d->loss_w.empty() ? 1.0 : d->loss_w[t];
	return BLA_OK;
}

bla_status bla_diffusion_target_f32(const bla_diffusion* d, void* stream, const float* d_x0, const float* d_eps, const int* d_t, int t_const, int batch,
                                    size_t image_floats, float* d_target, float* d_weight) {
	bla_status st = require_ready();
	if (st) return st;
	if ((st = check_images(d, batch, image_floats, 1))) return st;
	BLA_REQUIRE(d_target, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(d->prediction == BLA_PREDICT_X0 || d_eps, BLA_ERR_INVALID, "this prediction type needs d_eps");
	BLA_REQUIRE(d->prediction == BLA_PREDICT_EPS || d_x0, BLA_ERR_INVALID, "this prediction type needs d_x0");
	BLA_REQUIRE(d_t || (t_const >= 0 && t_const < d->steps), BLA_ERR_INVALID, "timestep %d outside [0, %d)", t_const, d->steps);
	const float* x0 = d->prediction == BLA_PREDICT_EPS ? nullptr : d_x0;     // the inputs this type does not read are not looked at
	const float* eps = d->prediction == BLA_PREDICT_X0 ? nullptr : d_eps;
	const size_t n = (size_t)batch * image_floats;
	const int vec = ((uintptr_t)x0 | (uintptr_t)eps | (uintptr_t)d_target) % 16 == 0;
	hipLaunchKernelGGL(target_kernel, dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), x0, eps, d_t, t_const, batch, image_floats, d->steps,
	                   d->prediction, d->table, d->loss_w_dev, d_target, d_weight, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_diffusion_to_eps_f32(const bla_diffusion* d, void* stream, float* d_pred, const float* d_x, const int* d_t, int t_const, int batch,
                                    size_t image_floats) {
	bla_status st = require_ready();
	if (st) return st;
	if ((st = check_images(d, batch, image_floats, 1))) return st;
	BLA_REQUIRE(d_pred && d_x, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(d_t || (t_const >= 0 && t_const < d->steps), BLA_ERR_INVALID, "timestep %d outside [0, %d)", t_const, d->steps);
	if (d->prediction == BLA_PREDICT_EPS) return BLA_OK;
	const size_t n = (size_t)batch * image_floats;
	const int vec = ((uintptr_t)d_pred | (uintptr_t)d_x) % 16 == 0;
	hipLaunchKernelGGL(to_eps_kernel, dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), d_pred, d_x, d_t, t_const, batch, image_floats, d->steps,
	                   d->prediction, d->table, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_diffusion_loss_f32(void* stream, const float* d_out, const float* d_target, const float* d_weight, int batch, size_t image_floats, float* d_g,
                                  double* d_loss) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(d_out && d_target, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(batch >= 1 && image_floats >= 1, BLA_ERR_INVALID, "batch %d, image_floats %zu", batch, image_floats);
	if (!d_g && !d_loss) return BLA_OK;
	const int vec = image_floats % 4 == 0 && ((uintptr_t)d_out | (uintptr_t)d_target | (uintptr_t)d_g) % 16 == 0;
	hipLaunchKernelGGL(weighted_loss_kernel, dim3(batch), dim3(kThreads), 0, pick_stream(stream), d_out, d_target, d_weight, image_floats, d_g, d_loss, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_diffusion_destroy(bla_diffusion* d) {
	if (!d) return BLA_OK;
	(void)hipDeviceSynchronize();
	(void)hipFree(d->table); (void)hipFree(d->temb); (void)hipFree(d->xg); (void)hipFree(d->rows); (void)hipFree(d->hist);
	(void)hipFree(d->vlb); (void)hipFree(d->ev); (void)hipFree(d->ev_temb); (void)hipFree(d->loss_w_dev);
	delete d;
	return BLA_OK;
}

int bla_diffusion_steps(const bla_diffusion* d) { return d ? d->steps : 0; }

bla_status bla_diffusion_schedule(const bla_diffusion* d, int t, double* beta, double* alpha_bar) {
	BLA_REQUIRE(d && t >= 0 && t < d->steps, BLA_ERR_INVALID, "timestep %d outside [0, %d)", t, d ? d->steps : 0);
	if (beta) *beta = d->beta[t];
	if (alpha_bar) *alpha_bar = d->alpha_bar[t];
	return BLA_OK;
}

bla_status bla_time_embedding_f32(void* stream, const int* d_t, int batch, int time_dim, float* d_temb) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(d_t && d_temb, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(batch >= 1 && time_dim >= 1, BLA_ERR_INVALID, "batch %d, time_dim %d", batch, time_dim);
	hipLaunchKernelGGL(time_embedding_kernel, dim3(grid_for((size_t)batch * time_dim)), dim3(kThreads), 0, pick_stream(stream), d_t, 0, batch, time_dim, d_temb);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_diffusion_noise_gather_f32(const bla_diffusion* d, void* stream, const float* d_data, size_t records, const unsigned int* d_index, int flip, int width,
                                          const int* d_labels, int* d_labels_out, int batch, size_t image_floats, int time_dim, unsigned long long seed,
                                          unsigned long long pass, int* d_t, float* d_eps, float* d_xt, float* d_temb, float* d_x0) {
	bla_status st = require_ready();
	if (st) return st;
	if ((st = check_images(d, batch, image_floats, time_dim))) return st;
	BLA_REQUIRE(d_data && d_t && d_eps && d_xt && d_temb, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(batch <= kMaxNoiseBatch, BLA_ERR_INVALID, "batch %d > %d", batch, kMaxNoiseBatch);
	BLA_REQUIRE(pass < (1ull << 32), BLA_ERR_INVALID, "pass %llu does not fit the stream offset pass << 32", pass);
	BLA_REQUIRE(width >= 1 && image_floats % (size_t)width == 0, BLA_ERR_INVALID, "image_floats %zu is not a whole number of rows of width %d", image_floats, width);
	const int vec = image_floats % 4 == 0 && width % 4 == 0 &&
	                ((uintptr_t)d_data | (uintptr_t)d_eps | (uintptr_t)d_xt | (uintptr_t)d_x0) % 16 == 0;
	const size_t n = (size_t)batch * image_floats;
	hipLaunchKernelGGL(noise_kernel, dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), d_data, records, d_index, flip ? 1 : 0, (unsigned)width,
	                   d_labels, d_labels_out, batch, image_floats, time_dim, seed, pass << 32, d->steps, d->table, d_t, d_eps, d_xt, d_temb, d_x0, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

// the gathering launch on the batch as it stands: records 0 .. batch-1, nothing mirrored.  Rows of 4 (or, when image_floats % 4 != 0, of 1) are never
// looked at without flips and keep the float4 path open to exactly the shapes that had it before
bla_status bla_diffusion_noise_f32(const bla_diffusion* d, void* stream, const float* d_x0, int batch, size_t image_floats, int time_dim, unsigned long long seed,
                                   unsigned long long pass, int* d_t, float* d_eps, float* d_xt, float* d_temb) {
	return bla_diffusion_noise_gather_f32(d, stream, d_x0, (size_t)(batch > 0 ? batch : 0), nullptr, 0, image_floats % 4 == 0 ? 4 : 1, nullptr, nullptr, batch,
	                                      image_floats, time_dim, seed, pass, d_t, d_eps, d_xt, d_temb, nullptr);
}

bla_status bla_diffusion_step_f32(const bla_diffusion* d, void* stream, float* d_x, const float* d_eps_hat, int batch, size_t image_floats, int t,
                                  unsigned long long seed, int time_dim, float* d_temb_next) {
	bla_status st = check_step(d, batch, image_floats, time_dim, d_x && d_eps_hat);
	if (st) return st;
	BLA_REQUIRE(t >= 0 && t < d->steps, BLA_ERR_INVALID, "timestep %d outside [0, %d)", t, d->steps);
	const size_t n = (size_t)batch * image_floats;
	const int vec = ((uintptr_t)d_x | (uintptr_t)d_eps_hat) % 16 == 0;
	hipLaunchKernelGGL((step_kernel<false>), dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), d_x, (float*)nullptr, (const float*)nullptr,
	                   d_eps_hat, 0.f, n, t, d->steps, seed, d->table, batch, time_dim, d_temb_next, (const float*)nullptr, 0, (const int*)nullptr, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

// the ancestral sampler: every timestep, T - 1 down to 0
bla_status bla_unet_sample_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, unsigned long long seed) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(m && d && d_x, BLA_ERR_INVALID, "null argument");
	const ModelShape g = shape_of(m);
	if ((st = sample_start(d, pick_stream(stream), g, d->steps - 1, 0))) return st;
	return sample_loop(m, d, stream, d_x, g, nullptr, d->steps, [&](int, int t, int) {
		return bla_diffusion_step_f32(d, stream, d_x, bla_unet_output(m), g.B, g.F, t, seed, g.dim, d->temb);
	});
}

bla_status bla_diffusion_guided_step_f32(const bla_diffusion* d, void* stream, float* d_x, float* d_x_copy, const float* d_eps_cond, const float* d_eps_uncond,
                                         float guidance, int batch, size_t image_floats, int t, unsigned long long seed, int time_dim, float* d_temb_next,
                                         const float* d_table, int classes, const int* d_rows) {
	bla_status st = check_step(d, batch, image_floats, time_dim, d_x && d_eps_cond && d_eps_uncond);
	if (st) return st;
	BLA_REQUIRE(t >= 0 && t < d->steps, BLA_ERR_INVALID, "timestep %d outside [0, %d)", t, d->steps);
	if ((st = check_guidance(guidance, d_table, classes, d_rows))) return st;
	const size_t n = (size_t)batch * image_floats;
	const int vec = ((uintptr_t)d_x | (uintptr_t)d_eps_cond | (uintptr_t)d_eps_uncond | (uintptr_t)d_x_copy) % 16 == 0;
	hipLaunchKernelGGL((step_kernel<true>), dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), d_x, d_x_copy, d_eps_cond, d_eps_uncond, guidance, n,
	                   t, d->steps, seed, d->table, batch, time_dim, d_temb_next, d_table, classes, d_rows, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_unet_sample_guided_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, const float* d_table, int classes, const int* labels, float guidance,
                                      unsigned long long seed) {
	bla_status st = check_guided_sampler(m, d, d_x, d_table, classes, labels, guidance);
	if (st) return st;
	const ModelShape g = shape_of(m);
	hipStream_t s = pick_stream(stream);
	if ((st = guided_start(d, s, g, d_x, d_table, classes, labels, d->steps - 1, 0))) return st;
	const int n = g.B / 2;
	float* xg = d->xg;
	const float* out = bla_unet_output(m);
	if ((st = sample_loop(m, d, stream, xg, g, nullptr, d->steps, [&](int, int t, int) {
		    return bla_diffusion_guided_step_f32(d, stream, xg, xg + n * g.F, out, out + n * g.F, guidance, n, g.F, t, seed, g.dim, d->temb, d_table, classes, d->rows);
	    })))
		return st;
	return guided_finish(d, s, g, d_x);
}

bla_status bla_mse_accumulate_f32(void* stream, const float* d_a, const float* d_b, size_t n, double* d_acc) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(d_a && d_b && d_acc, BLA_ERR_INVALID, "null argument");
	hipLaunchKernelGGL(sq_diff_sum_kernel, dim3(1), dim3(1024), 0, pick_stream(stream), d_a, d_b, n, d_acc);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_diffusion_ddim_timesteps(const bla_diffusion* d, int sample_steps, int* out) {
	BLA_REQUIRE(d && out, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(sample_steps >= 1 && sample_steps <= d->steps, BLA_ERR_INVALID, "sample_steps %d outside [1, %d]", sample_steps, d->steps);
	const std::vector<int> ts = ddim_timesteps(d->steps, sample_steps);
	for (int i = 0; i < sample_steps; i++) out[i] = ts[i];
	return BLA_OK;
}

bla_status bla_diffusion_ddim_step_f32(const bla_diffusion* d, void* stream, float* d_x, const float* d_eps_hat, int batch, size_t image_floats, int t, int t_prev,
                                       float eta, int clip, unsigned long long seed, int time_dim, float* d_temb_next) {
	bla_status st = check_step(d, batch, image_floats, time_dim, d_x && d_eps_hat);
	if (st) return st;
	if ((st = check_ddim(d, t, t_prev, eta))) return st;
	const size_t n = (size_t)batch * image_floats;
	const int vec = ((uintptr_t)d_x | (uintptr_t)d_eps_hat) % 16 == 0;
	hipLaunchKernelGGL((ddim_step_kernel<false>), dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), d_x, (float*)nullptr,
	                   (const float*)nullptr, d_eps_hat, 0.f, n, ddim_args(d, t, t_prev, eta, clip), t, t_prev, seed, batch, time_dim, d_temb_next,
	                   (const float*)nullptr, 0, (const int*)nullptr, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_unet_sample_ddim_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, int sample_steps, float eta, int clip, unsigned long long seed) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(m && d && d_x, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(sample_steps >= 1 && sample_steps <= d->steps, BLA_ERR_INVALID, "sample_steps %d outside [1, %d]", sample_steps, d->steps);
	BLA_REQUIRE(eta >= 0.f && eta <= 1.f, BLA_ERR_INVALID, "eta %g outside [0, 1]", eta);
	const std::vector<int> ts = ddim_timesteps(d->steps, sample_steps);
	const ModelShape g = shape_of(m);
	if ((st = sample_start(d, pick_stream(stream), g, ts.back(), 0))) return st;
	return sample_loop(m, d, stream, d_x, g, ts.data(), sample_steps, [&](int, int t, int t_prev) {
		return bla_diffusion_ddim_step_f32(d, stream, d_x, bla_unet_output(m), g.B, g.F, t, t_prev, eta, clip, seed, g.dim, d->temb);
	});
}

bla_status bla_diffusion_guided_ddim_step_f32(const bla_diffusion* d, void* stream, float* d_x, float* d_x_copy, const float* d_eps_cond, const float* d_eps_uncond,
                                              float guidance, int batch, size_t image_floats, int t, int t_prev, float eta, int clip, unsigned long long seed,
                                              int time_dim, float* d_temb_next, const float* d_table, int classes, const int* d_rows) {
	bla_status st = check_step(d, batch, image_floats, time_dim, d_x && d_eps_cond && d_eps_uncond);
	if (st) return st;
	if ((st = check_ddim(d, t, t_prev, eta))) return st;
	if ((st = check_guidance(guidance, d_table, classes, d_rows))) return st;
	const size_t n = (size_t)batch * image_floats;
	const int vec = ((uintptr_t)d_x | (uintptr_t)d_eps_cond | (uintptr_t)d_eps_uncond | (uintptr_t)d_x_copy) % 16 == 0;
	hipLaunchKernelGGL((ddim_step_kernel<true>), dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), d_x, d_x_copy, d_eps_cond, d_eps_uncond,
	                   guidance, n, ddim_args(d, t, t_prev, eta, clip), t, t_prev, seed, batch, time_dim, d_temb_next, d_table, classes, d_rows, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_unet_sample_guided_ddim_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, const float* d_table, int classes, const int* labels,
                                           float guidance, int sample_steps, float eta, int clip, unsigned long long seed) {
	bla_status st = check_guided_sampler(m, d, d_x, d_table, classes, labels, guidance);
	if (st) return st;
	BLA_REQUIRE(sample_steps >= 1 && sample_steps <= d->steps, BLA_ERR_INVALID, "sample_steps %d outside [1, %d]", sample_steps, d->steps);
	BLA_REQUIRE(eta >= 0.f && eta <= 1.f, BLA_ERR_INVALID, "eta %g outside [0, 1]", eta);
	const std::vector<int> ts = ddim_timesteps(d->steps, sample_steps);
	const ModelShape g = shape_of(m);
	hipStream_t s = pick_stream(stream);
	if ((st = guided_start(d, s, g, d_x, d_table, classes, labels, ts.back(), 0))) return st;
	const int n = g.B / 2;
	float* xg = d->xg;
	const float* out = bla_unet_output(m);
	if ((st = sample_loop(m, d, stream, xg, g, ts.data(), sample_steps, [&](int, int t, int t_prev) {
		    return bla_diffusion_guided_ddim_step_f32(d, stream, xg, xg + n * g.F, out, out + n * g.F, guidance, n, g.F, t, t_prev, eta, clip, seed, g.dim, d->temb,
		                                              d_table, classes, d->rows);
	    })))
		return st;
	return guided_finish(d, s, g, d_x);
}

// ---- DPM-Solver++(2M) ---------------------------------------------------------------------------------------------------------------------------

bla_status bla_diffusion_sample_timesteps(const bla_diffusion* d, int sample_steps, int spacing, int* out) {
	BLA_REQUIRE(d && out, BLA_ERR_INVALID, "null argument");
	std::vector<int> ts;
	bla_status st = sample_timesteps(d, sample_steps, spacing, &ts);
	if (st) return st;
	for (int i = 0; i < sample_steps; i++) out[i] = ts[i];
	return BLA_OK;
}

bla_status bla_diffusion_dpmpp_coefficients(const bla_diffusion* d, int t_last, int t, int t_prev, double out[6]) {
	BLA_REQUIRE(d && out, BLA_ERR_INVALID, "null argument");
	bla_status st = check_dpmpp(d, t_last, t, t_prev);
	if (st) return st;
	dpmpp_coefficients(d, t_last, t, t_prev, out);
	return BLA_OK;
}

bla_status bla_diffusion_dpmpp_step_f32(const bla_diffusion* d, void* stream, float* d_x, const float* d_eps_hat, float* d_x0_hist, int batch, size_t image_floats,
                                        int t_last, int t, int t_prev, int clip, int time_dim, float* d_temb_next) {
	bla_status st = check_step(d, batch, image_floats, time_dim, d_x && d_eps_hat && d_x0_hist);
	if (st) return st;
	if ((st = check_dpmpp(d, t_last, t, t_prev))) return st;
	const size_t n = (size_t)batch * image_floats;
	const int vec = ((uintptr_t)d_x | (uintptr_t)d_eps_hat | (uintptr_t)d_x0_hist) % 16 == 0;
	hipLaunchKernelGGL((dpmpp_step_kernel<false>), dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), d_x, (float*)nullptr,
	                   (const float*)nullptr, d_eps_hat, 0.f, d_x0_hist, n, dpmpp_args(d, t_last, t, t_prev, clip), t_prev, batch, time_dim, d_temb_next,
	                   (const float*)nullptr, 0, (const int*)nullptr, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_diffusion_guided_dpmpp_step_f32(const bla_diffusion* d, void* stream, float* d_x, float* d_x_copy, const float* d_eps_cond, const float* d_eps_uncond,
                                               float guidance, float* d_x0_hist, int batch, size_t image_floats, int t_last, int t, int t_prev, int clip,
                                               int time_dim, float* d_temb_next, const float* d_table, int classes, const int* d_rows) {
	bla_status st = check_step(d, batch, image_floats, time_dim, d_x && d_eps_cond && d_eps_uncond && d_x0_hist);
	if (st) return st;
	if ((st = check_dpmpp(d, t_last, t, t_prev))) return st;
	if ((st = check_guidance(guidance, d_table, classes, d_rows))) return st;
	const size_t n = (size_t)batch * image_floats;
	const int vec = ((uintptr_t)d_x | (uintptr_t)d_eps_cond | (uintptr_t)d_eps_uncond | (uintptr_t)d_x_copy | (uintptr_t)d_x0_hist) % 16 == 0;
	hipLaunchKernelGGL((dpmpp_step_kernel<true>), dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), d_x, d_x_copy, d_eps_cond, d_eps_uncond,
	                   guidance, d_x0_hist, n, dpmpp_args(d, t_last, t, t_prev, clip), t_prev, batch, time_dim, d_temb_next, d_table, classes, d_rows, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_unet_sample_dpmpp_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, int sample_steps, int spacing, int clip) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(m && d && d_x, BLA_ERR_INVALID, "null argument");
	std::vector<int> ts;
	if ((st = sample_timesteps(d, sample_steps, spacing, &ts))) return st;
	const ModelShape g = shape_of(m);
	if ((st = sample_start(d, pick_stream(stream), g, ts.back(), (size_t)g.B * g.F))) return st;
	return sample_loop(m, d, stream, d_x, g, ts.data(), sample_steps, [&](int t_last, int t, int t_prev) {
		return bla_diffusion_dpmpp_step_f32(d, stream, d_x, bla_unet_output(m), d->hist, g.B, g.F, t_last, t, t_prev, clip, g.dim, d->temb);
	});
}

bla_status bla_unet_sample_guided_dpmpp_f32(bla_unet* m, const bla_diffusion* d, void* stream, float* d_x, const float* d_table, int classes, const int* labels,
                                            float guidance, int sample_steps, int spacing, int clip) {
	bla_status st = check_guided_sampler(m, d, d_x, d_table, classes, labels, guidance);
	if (st) return st;
	std::vector<int> ts;
	if ((st = sample_timesteps(d, sample_steps, spacing, &ts))) return st;
	const ModelShape g = shape_of(m);
	hipStream_t s = pick_stream(stream);
	const int n = g.B / 2;
	if ((st = guided_start(d, s, g, d_x, d_table, classes, labels, ts.back(), n * g.F))) return st;
	float* xg = d->xg;
	const float* out = bla_unet_output(m);
	if ((st = sample_loop(m, d, stream, xg, g, ts.data(), sample_steps, [&](int t_last, int t, int t_prev) {
		    return bla_diffusion_guided_dpmpp_step_f32(d, stream, xg, xg + n * g.F, out, out + n * g.F, guidance, d->hist, n, g.F, t_last, t, t_prev, clip, g.dim,
		                                               d->temb, d_table, classes, d->rows);
	    })))
		return st;
	return guided_finish(d, s, g, d_x);
}

// ---- held-out evaluation ------------------------------------------------------------------------------------------------------------------------

bla_status bla_diffusion_noise_at_f32(const bla_diffusion* d, void* stream, const float* d_x0, int batch, size_t image_floats, int time_dim, const int* d_t, int t_const,
                                      unsigned long long seed, unsigned long long offset, float* d_eps, float* d_xt, float* d_temb) {
	bla_status st = require_ready();
	if (st) return st;
	if ((st = check_images(d, batch, image_floats, time_dim))) return st;
	BLA_REQUIRE(d_x0 && d_eps && d_xt && d_temb, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(batch <= kMaxNoiseBatch, BLA_ERR_INVALID, "batch %d > %d", batch, kMaxNoiseBatch);
	BLA_REQUIRE(d_t || (t_const >= 0 && t_const < d->steps), BLA_ERR_INVALID, "timestep %d outside [0, %d)", t_const, d->steps);
	const int vec = image_floats % 4 == 0 && ((uintptr_t)d_x0 | (uintptr_t)d_eps | (uintptr_t)d_xt) % 16 == 0;
	const size_t n = (size_t)batch * image_floats;
	hipLaunchKernelGGL(noise_at_kernel, dim3(grid_for(vec ? n / 4 : n)), dim3(kThreads), 0, pick_stream(stream), d_x0, batch, image_floats, time_dim, d_t, t_const, seed,
	                   offset, d->steps, d->table, d_eps, d_xt, d_temb, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_diffusion_vlb_terms_f32(const bla_diffusion* d, void* stream, const float* d_x0, const float* d_xt, const float* d_eps, const float* d_eps_hat,
                                       const int* d_t, int t_const, int batch, size_t image_floats, double* d_terms, double* d_sqerr) {
	bla_status st = require_ready();
	if (st) return st;
	if ((st = check_images(d, batch, image_floats, 1))) return st;
	BLA_REQUIRE(d_x0 && d_xt && d_eps && d_eps_hat && d_terms, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(d_t || (t_const >= 0 && t_const < d->steps), BLA_ERR_INVALID, "timestep %d outside [0, %d)", t_const, d->steps);
	const int vec = image_floats % 4 == 0 && ((uintptr_t)d_x0 | (uintptr_t)d_xt | (uintptr_t)d_eps | (uintptr_t)d_eps_hat) % 16 == 0;
	const double b0 = d->beta[0], ab0 = d->alpha_bar[0];
	const DecoderArgs dec = {b0 / std::sqrt(1.0 - ab0), std::sqrt(1.0 - b0), std::sqrt(b0)};
	hipLaunchKernelGGL(vlb_terms_kernel, dim3(batch), dim3(kThreads), 0, pick_stream(stream), d_x0, d_xt, d_eps, d_eps_hat, d_t, t_const, image_floats, d->steps, d->vlb,
	                   dec, d_terms, d_sqerr, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_diffusion_prior_kl_f32(const bla_diffusion* d, void* stream, const float* d_x0, int batch, size_t image_floats, double* d_kl) {
	bla_status st = require_ready();
	if (st) return st;
	if ((st = check_images(d, batch, image_floats, 1))) return st;
	BLA_REQUIRE(d_x0 && d_kl, BLA_ERR_INVALID, "null argument");
	const int vec = image_floats % 4 == 0 && (uintptr_t)d_x0 % 16 == 0;
	const double ab = d->alpha_bar[d->steps - 1];
	hipLaunchKernelGGL(prior_kl_kernel, dim3(batch), dim3(kThreads), 0, pick_stream(stream), d_x0, image_floats, ab, std::log(1.0 - ab), d_kl, vec);
	BLA_HIP(hipGetLastError());
	return BLA_OK;
}

bla_status bla_diffusion_vlb_weights(const bla_diffusion* d, int t, double* c_t, double* w_t) {
	BLA_REQUIRE(d && t >= 1 && t < d->steps, BLA_ERR_INVALID, "timestep %d outside [1, %d)", t, d ? d->steps : 0);
	double c, w;
	vlb_weights(d->beta, d->alpha_bar, t, &c, &w);
	if (c_t) *c_t = c;
	if (w_t) *w_t = w;
	return BLA_OK;
}

bla_status bla_diffusion_eval_timesteps(const bla_diffusion* d, int K, int* out) {
	BLA_REQUIRE(d && out, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(K >= 0 && K <= d->steps - 1, BLA_ERR_INVALID, "%d KL terms outside [0, %d]", K, d->steps - 1);
	const std::vector<int> ts = eval_timesteps(d->steps, K);
	for (int i = 0; i <= K; i++) out[i] = ts[i];
	return BLA_OK;
}

bla_status bla_unet_evaluate_f32(bla_unet* m, const bla_diffusion* d, void* stream, const float* d_x0, const int* timesteps, int count, unsigned long long seed,
                                 unsigned long long offset_base, const float* d_table, int classes, const int* d_rows, double* d_terms, double* d_sqerr) {
	bla_status st = require_ready();
	if (st) return st;
	BLA_REQUIRE(m && d && d_x0 && timesteps && d_terms, BLA_ERR_INVALID, "null argument");
	BLA_REQUIRE(count >= 0, BLA_ERR_INVALID, "count %d", count);
	BLA_REQUIRE(!d_table || (d_rows && classes >= 1), BLA_ERR_INVALID, "a class table needs the rows [batch] and classes >= 1");
	for (int i = 0; i < count; i++) BLA_REQUIRE(timesteps[i] >= 0 && timesteps[i] < d->steps, BLA_ERR_INVALID, "timestep %d outside [0, %d)", timesteps[i], d->steps);
	const bla_unet_config& c = *unet_config(m);
	const int B = bla_unet_batch(m);
	const size_t F = (size_t)c.in_channels * c.image_h * c.image_w, ne = (size_t)B * c.time_dim, nx = (size_t)B * F;
	hipStream_t s = pick_stream(stream);
	bla_diffusion* dm = const_cast<bla_diffusion*>(d);   // workspaces, not part of the schedule
	if ((st = grow(s, &dm->ev, &dm->ev_floats, 2 * nx))) return st;
	if ((st = grow(s, &dm->ev_temb, &dm->ev_temb_floats, ne))) return st;
	if (d_table && (st = grow(s, &dm->rows, &dm->rows_count, (size_t)B))) return st;   // the rows bla_class_embedding_f32 writes
	float *eps = dm->ev, *xt = dm->ev + nx;
	for (int i = 0; i < count; i++) {
		const int t = timesteps[i];
		if ((st = bla_diffusion_noise_at_f32(d, stream, d_x0, B, F, c.time_dim, nullptr, t, seed, offset_base + ((unsigned long long)(t + 1) << 32), eps, xt, dm->ev_temb)))
			return st;
		if (d_table && (st = bla_class_embedding_f32(stream, d_table, classes, d_rows, B, c.time_dim, 0.f, seed, 0, dm->rows, dm->ev_temb))) return st;
		if ((st = bla_unet_forward_f32(m, stream, xt, dm->ev_temb, nullptr))) return st;
		if ((st = output_to_eps(m, d, stream, xt, B, F, t))) return st;
		if ((st = bla_diffusion_vlb_terms_f32(d, stream, d_x0, xt, eps, bla_unet_output(m), nullptr, t, B, F, d_terms + (size_t)i * B,
		                                      d_sqerr ? d_sqerr + (size_t)i * B : nullptr)))
			return st;
	}
	return BLA_OK;
}

}  // extern "C"
